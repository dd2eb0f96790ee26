"""CPU checks of the encoded-audio boundary (nothing runs on a GPU): the NumPy restatement against CPython's ``audioop``, exhaustively;
its round trips and dither statistics; the entries declared, exported and bound with matching arity; what the host can see refused;
the RIFF writer and reader."""
import io
import re
import struct
import wave

import numpy as np
import pytest

from conftest import ROOT, sub
import audio_codec_restated as ar

WORDS = np.arange(-32768, 32768, dtype=np.int32)
CODES = np.arange(256, dtype=np.uint8)
N = 65536


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_companding_is_audioop_exhaustively():
    audioop = pytest.importorskip("audioop")
    raw = WORDS.astype("<i2").tobytes()
    assert np.array_equal(np.frombuffer(audioop.lin2ulaw(raw, 2), dtype=np.uint8), ar.lin2ulaw(WORDS))
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(raw, 2), dtype=np.uint8), ar.lin2alaw(WORDS))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(CODES.tobytes(), 2), dtype="<i2"), ar.ulaw2lin(CODES))
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(CODES.tobytes(), 2), dtype="<i2"), ar.alaw2lin(CODES))
    # the whole encoders, from the floats v / 32768
    x = WORDS.astype(np.float32) / np.float32(32768.0)
    assert ar.encode(x, ar.PCM16).tobytes() == raw
    assert ar.encode(x, ar.ULAW).tobytes() == audioop.lin2ulaw(raw, 2) and ar.encode(x, ar.ALAW).tobytes() == audioop.lin2alaw(raw, 2)


def test_restated_round_trips():
    x = ar.decode(WORDS.astype("<i2").view(np.uint8), ar.PCM16)
    assert np.array_equal(ar.quantise(x), WORDS)                             # decode then encode returns every int16
    assert np.array_equal(ar.encode(ar.decode(CODES, ar.ALAW), ar.ALAW), CODES)
    back = ar.encode(ar.decode(CODES, ar.ULAW), ar.ULAW)
    differ = np.nonzero(back != CODES)[0]
    assert differ.tolist() == [0x7F] and back[0x7F] == 0xFF                  # mu-law's two zeros
    # both decoders' quotients are exact: value / 32768 * 32768 is the integer
    for fmt, lin in ((ar.ULAW, ar.ulaw2lin), (ar.ALAW, ar.alaw2lin)):
        assert np.array_equal((ar.decode(CODES, fmt).astype(np.float64) * 32768.0).astype(np.int32), lin(CODES))


def test_restated_quantiser_edges():
    ties = np.array([(v + 0.5) / 32768.0 for v in range(-4, 5)], dtype=np.float32)
    assert ar.quantise(ties).tolist() == [-4, -2, -2, 0, 0, 2, 2, 4, 4]      # ties to even
    edge = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0 - 2.0 ** -24, -0.0, 1e-42], dtype=np.float32)
    assert ar.quantise(edge).tolist() == [0, 32767, -32768, 32767, -32768, 32767, 0, 0]


def test_dither_statistics():
    """Derived bounds.  TPDF dither of one LSB makes the quantiser's mean exact and its error's standard deviation 0.5 LSB
    (1/6 from d, 1/12 from the rounding): over N = 65536 samples the mean's standard deviation is 0.5 / 256 = 0.002, the bound
    0.01 is 5 sigma.  The sample correlation of two independent sequences has standard deviation 1 / sqrt(N)."""
    x = np.full(N, 0.25 / 32768.0, dtype=np.float32)
    d = ar.dither(0, 0, N)
    assert d.dtype == np.float32 and np.abs(d).max() < 1.0
    q = ar.quantise(x, d)
    print(f"dithered mean {q.mean():.5f} LSB, error std {(q - 0.25).std():.4f} LSB")
    assert abs(q.mean() - 0.25) <= 0.01
    assert ar.quantise(x).mean() == 0.0                                      # without dither the quarter LSB is lost
    other = ar.dither(0, 1, N)
    corr = np.corrcoef(d.astype(np.float64), other.astype(np.float64))[0, 1]
    print(f"correlation of two keys {corr:.5f}")
    assert abs(corr) <= 5.0 / np.sqrt(N)
    assert np.array_equal(ar.dither(0, 0, N), d) and not np.array_equal(ar.dither(1, 0, N), d)
    # u1 - u2 is exact in fp32: the fp64 difference of the same two fp32 numbers is the same number
    i = np.arange(N, dtype=np.uint64)
    u1 = (ar.dither_hash(0, 0, i, 0) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    u2 = (ar.dither_hash(0, 0, i, 1) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    assert np.array_equal(d.astype(np.float64), u1 - u2)
    # the index and the stream share one word: a sample's second stream is not its neighbour's first
    assert ar.dither_hash(5, 9, 3, 1) == ar.fmix(_row_hash(5, 9) ^ np.uint64(7))


def _row_hash(seed, key):
    h = ar.fmix(np.uint64(0x9E3779B9) ^ ar.words(seed)[0])
    h = ar.fmix(h ^ ar.words(seed)[1])
    h = ar.fmix(h ^ ar.words(key)[0])
    return ar.fmix(h ^ ar.words(key)[1])


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert re.search(r"#define MTTS_ABI_VERSION 2\b", header)    # additive entries
    for name, value in (("MTTS_PCM16", 0), ("MTTS_ULAW", 1), ("MTTS_ALAW", 2)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    ac = sub("audio_codec")
    assert (ac.PCM16, ac.ULAW, ac.ALAW) == (0, 1, 2) and ac.FORMATS == {"pcm16": 0, "ulaw": 1, "alaw": 2} == ar.NAMES
    tile = int(re.search(r"#define MTTS_CODEC_TILE (\d+)", header).group(1))
    assert lib.mtts_codec_tile() == tile == ac.TILE and tile % 1024 == 0


def test_encode_refuses_what_the_host_can_see(lib):
    # (audio, ld, lengths, formats, keys, B, dither, seed, out, out_bytes, stream): never launched, refused before
    ok = (0x100000, 1024, 0x200000, 0x300000, None, 2, 0, 0, 0x400000, 0x500000, None)
    for i in (0, 2, 3, 8, 9):                                    # every pointer but the keys, which may be null
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_pcm_encode(*bad) == -1 and b"null" in lib.mtts_last_error()
    bad = list(ok); bad[5] = 0
    assert lib.mtts_pcm_encode(*bad) == -1 and b"B must" in lib.mtts_last_error()
    for ld in (0, 1022, -4):
        bad = list(ok); bad[1] = ld
        assert lib.mtts_pcm_encode(*bad) == -1 and b"multiple of 4" in lib.mtts_last_error()
    bad = list(ok); bad[0] = 0x100004
    assert lib.mtts_pcm_encode(*bad) == -1 and b"misaligned" in lib.mtts_last_error()
    # d_out inside, and straddling the end of, d_audio (2 rows of 1024 floats = 8192 bytes)
    for out in (0x100000, 0x100000 + 8192 - 16, 0x100000 - 4096 + 16):
        bad = list(ok); bad[8] = out
        assert lib.mtts_pcm_encode(*bad) == -1 and b"overlaps" in lib.mtts_last_error(), hex(out)
    assert lib.mtts_pcm_status(None, 2, None) == -1 and lib.mtts_pcm_status(0x500000, 0, None) == -1


def test_decode_refuses_what_the_host_can_see(lib):
    # (data, ld_bytes, lengths, formats, B, out, ld, out_lengths, stream)
    ok = (0x100000, 2048, 0x200000, 0x300000, 2, 0x400000, 1024, 0x500000, None)
    for i in (0, 2, 3, 5, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_pcm_decode(*bad) == -1 and b"null" in lib.mtts_last_error()
    bad = list(ok); bad[4] = 0
    assert lib.mtts_pcm_decode(*bad) == -1 and b"B must" in lib.mtts_last_error()
    bad = list(ok); bad[6] = 1022
    assert lib.mtts_pcm_decode(*bad) == -1 and b"multiple of 4" in lib.mtts_last_error()
    for ldb in (0, 2040):
        bad = list(ok); bad[1] = ldb
        assert lib.mtts_pcm_decode(*bad) == -1 and b"multiple of 16" in lib.mtts_last_error()
    bad = list(ok); bad[5] = 0x100000 + 16
    assert lib.mtts_pcm_decode(*bad) == -1 and b"overlaps" in lib.mtts_last_error()


def test_python_entries_refuse_host_tensors_and_unknown_names():
    import torch
    ac = sub("audio_codec")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ac.encode(torch.zeros(1, 8), None, "pcm16")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ac.decode(torch.zeros(1, 16, dtype=torch.uint8), [8], "ulaw")
    for bad in ("mp3", "PCM16", 3, None, True):
        with pytest.raises(ValueError):
            ac.format_id(bad)
    with pytest.raises(ValueError):
        ac.Encoded(b"\x00\x00", "opus", 8000)
    with pytest.raises(ValueError):
        ac.formats_per_row(["ulaw"], 2)
    e = ac.Encoded(b"\x01\x02\x03", "pcm16", 8000)
    assert (e.nbytes, e.samples, e.numel()) == (3, 1, 1) and e.tensor().tolist() == [1, 2, 3]


# ------------------------------------------------------------------------------------------------ the RIFF container
def test_wav_bytes_pcm16_opens_with_the_stdlib():
    ac = sub("audio_codec")
    payload = ar.encode(np.sin(np.arange(1001) / 7.0).astype(np.float32) * 0.5, ar.PCM16).tobytes()
    blob = ac.wav_bytes(payload, "pcm16", 16000)
    with wave.open(io.BytesIO(blob), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, 1001)
        assert w.readframes(1001) == payload
    back = ac.read_wav(blob)
    assert (back.format, back.sample_rate, back.data) == ("pcm16", 16000, payload)
    import torch
    assert ac.wav_bytes(torch.frombuffer(bytearray(payload), dtype=torch.uint8), "pcm16", 16000) == blob
    with pytest.raises(ValueError):
        ac.wav_bytes(payload[:-1], "pcm16", 16000)               # half a sample


@pytest.mark.parametrize("name,tag", [("ulaw", 7), ("alaw", 6)])
def test_wav_bytes_g711_header_and_round_trip(name, tag):
    ac = sub("audio_codec")
    payload = bytes(range(256)) + bytes(range(5))                # an odd count: the data chunk is padded to a word
    blob = ac.wav_bytes(payload, name, 8000)
    assert blob[:4] == b"RIFF" and struct.unpack_from("<I", blob, 4)[0] == len(blob) - 8 and blob[8:12] == b"WAVE"
    assert blob[12:16] == b"fmt " and struct.unpack_from("<I", blob, 16)[0] == 18
    wtag, channels, rate, byte_rate, block, bits, cb = struct.unpack_from("<HHIIHHH", blob, 20)
    assert (wtag, channels, rate, byte_rate, block, bits, cb) == (tag, 1, 8000, 8000, 1, 8, 0)
    assert blob[38:42] == b"fact" and struct.unpack_from("<II", blob, 42) == (4, len(payload))
    assert blob[50:54] == b"data" and struct.unpack_from("<I", blob, 54)[0] == len(payload)
    assert blob[58:58 + len(payload)] == payload and len(blob) == 58 + len(payload) + 1 and len(blob) % 2 == 0
    with pytest.raises(wave.Error):                               # why the reader exists: the stdlib refuses the form
        wave.open(io.BytesIO(blob), "rb")
    back = ac.read_wav(blob)
    assert (back.format, back.sample_rate, back.data, back.samples) == (name, 8000, payload, len(payload))


def test_read_wav_takes_channel_0_and_a_path(tmp_path):
    ac = sub("audio_codec")
    left, right = np.arange(100, dtype="<i2"), -np.arange(100, dtype="<i2")
    path = tmp_path / "stereo.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(np.stack([left, right], 1).tobytes())
    back = ac.read_wav(path)
    assert (back.format, back.sample_rate) == ("pcm16", 44100) and back.data == left.tobytes()


def test_read_wav_refuses_truncated_and_unsupported_files():
    ac = sub("audio_codec")
    blob = ac.wav_bytes(bytes(200), "ulaw", 8000)
    for cut in (3, 11, 30, 57, len(blob) - 50):
        with pytest.raises(ValueError):
            ac.read_wav(blob[:cut])
    with pytest.raises(ValueError, match="RIFF"):
        ac.read_wav(b"RIFX" + blob[4:])
    floaty = bytearray(ac.wav_bytes(bytes(200), "pcm16", 8000))
    struct.pack_into("<H", floaty, 20, 3)                         # WAVE_FORMAT_IEEE_FLOAT
    with pytest.raises(ValueError, match="unsupported"):
        ac.read_wav(bytes(floaty))
    wide = bytearray(ac.wav_bytes(bytes(200), "pcm16", 8000))
    struct.pack_into("<H", wide, 34, 24)                          # 24-bit PCM
    with pytest.raises(ValueError, match="unsupported"):
        ac.read_wav(bytes(wide))


def test_the_enrol_tool_falls_back_for_a_g711_file(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("enroll_tool", ROOT / "tools" / "enroll.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ac = sub("audio_codec")
    payload = bytes(range(256))
    g711 = tmp_path / "leg.wav"
    g711.write_bytes(ac.wav_bytes(payload, "ulaw", 8000))
    clip, rate = tool.read_wav(g711)
    assert isinstance(clip, ac.Encoded) and (clip.format, clip.data, rate) == ("ulaw", payload, 8000)
    pcm = tmp_path / "pcm.wav"
    words = np.arange(-50, 50, dtype="<i2")
    pcm.write_bytes(ac.wav_bytes(words.tobytes(), "pcm16", 16000))
    clip, rate = tool.read_wav(pcm)                               # a file it reads today is read as today: floats
    assert rate == 16000 and clip.dtype.is_floating_point and np.array_equal(clip.numpy(), words.astype(np.float32) / 32768.0)

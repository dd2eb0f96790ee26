"""CPU checks of FLAC in (nothing runs on a GPU): the restated decoder against ``flac_restated.decode`` on the RFC's example file and on
the project's own streams; the recipe writer through the decoder on the case list; ``mtts_flac_parse_host`` -- the parser the kernels
run, on host memory -- against the decoder on every accepted stream and every refusal; the two C entries refusing what the host can
see; ``read_flac``, ``FlacClip`` and the tools' reader.  All comparisons of samples are integer-exact."""
import ctypes as C
import importlib.util
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, sub
import flac_in_cases as fc
import flac_in_restated as fi
import flac_restated as fr


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def twin(lib, data, capacity=20000, max_block=4608):
    """``mtts_flac_parse_host`` on exact-size buffers with guard words: (count, samples, rate, channels, bps)."""
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8).copy()
    out = np.full(capacity + 8, 0x5A5A5A5A, dtype=np.int32)
    rate, channels, bps = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    n = lib.mtts_flac_parse_host(buf.ctypes.data, len(data), max_block, out.ctypes.data, capacity, C.byref(rate), C.byref(channels), C.byref(bps))
    assert (out[capacity:] == 0x5A5A5A5A).all(), "words behind the capacity were written"
    return n, out[:max(n, 0)].astype(np.int64), rate.value, channels.value, bps.value


# ------------------------------------------------------------------------------------------------ the restatement
def test_decoder_agrees_with_the_subset_decoder_on_the_rfc_file_and_on_own_streams():
    for name, data in fc.own().items():
        old, new = fr.decode(data), fc.expected()[name]
        assert np.array_equal(old["samples"], new["samples"]), name
        for key in ("rate", "channels", "bps", "total", "block_sizes", "frame_sizes", "md5"):
            assert old[key] == new[key], (name, key)
        assert [{k: f[k] for k in ("n", "number", "bytes", "rate", "variable", "kinds")} for f in new["frames"]] == old["frames"], name
    rfc = fc.expected()["rfc_example1"]
    assert rfc["samples"].tolist() == [[25588], [10416]] and rfc["first"] == 42
    for at in (44, 49, 52, 55):                                  # a flipped bit is seen by one of the CRCs
        bad = bytearray(fc.own()["rfc_example1"])
        bad[at] ^= 0x10
        with pytest.raises(ValueError):
            fi.decode(bytes(bad))


def test_writer_round_trips_through_the_decoder_on_the_case_list():
    for name, data in fc.good().items():
        got, want = fc.expected()[name], fc.TRUTH[name]
        assert got["samples"].shape == want.shape and np.array_equal(got["samples"], want), name
    e = fc.expected()
    kinds = lambda name: [k for f in e[name]["frames"] for k in f["kinds"]]
    assert kinds("lpc_small") == [("LPC", 32), ("LPC", 1)] and kinds("lpc_4096") == [("LPC", 32), ("LPC", 16), ("VERBATIM", 0)]
    assert [f["assign"] for f in e["stereo"]["frames"]] == [8, 9, 10, 1] and e["eight"]["channels"] == 8
    assert [f["number"] for f in e["numbers"]["frames"]] == list(range(129)) and len(fi.coded_number(128)) == 2
    assert [(f["n"], f["number"], f["variable"]) for f in e["variable"]["frames"]] == [(16, 0, 1), (700, 16, 1), (192, 716, 1), (33, 908, 1),
                                                                                        (4096, 941, 1), (1, 5037, 1)]
    assert e["metadata"]["first"] > 42 + 37 and e["empty"]["samples"].shape == (1, 0) and e["plain_24"]["bps"] == 24
    assert {e[f"block_{bs}"]["frames"][0]["n"] for bs in (16, 192, 256, 576, 4608)} == {16, 192, 256, 576, 4608}
    assert all(e[f"block_{bs}"]["frames"][-1]["n"] == 1 for bs in (16, 192, 256, 576, 4608))
    # the wide LPC case is one a 32-bit accumulator gets wrong: its largest sum of products needs more than 32 bits
    x = fc.TRUTH["lpc_wide"][0]
    assert max(abs(int(np.dot(np.where(x[i - 32:i][::-1] < 0, -16384, 16383), x[i - 32:i][::-1]))) for i in (32,)) > 1 << 40
    for v in (0, 127, 128, 2047, 2048, (1 << 31) - 1, 1 << 31, (1 << 36) - 1):       # the coded number, 1 to 7 bytes, read back by the header rule
        frame = fi.frame_bytes({"samples": np.zeros(16), "sub": {"kind": "constant"}, "variable": True}, v, 24000, 16, 24000)
        info = {"rate": 24000, "bps": 16, "channels": 1, "block_sizes": (16, 16)}
        assert fi.header(frame, 0, info)["number"] == v and len(fi.coded_number(v)) == (1 if v < 128 else (v.bit_length() + 3) // 5)


def test_golden_streams_are_the_writers():
    files = sorted((GOLDEN / "flac_in").glob("*.flac"))
    assert len(files) >= 12
    for path in files:
        name = path.stem
        data = fc.refused()[name[len("refused_"):]][0] if name.startswith("refused_") else fc.good()[name]
        assert path.read_bytes() == data, name


# ------------------------------------------------------------------------------------------------ the host twin of the device parser
def test_host_twin_agrees_with_the_decoder_on_every_accepted_stream(lib):
    for name, data in {**fc.good(), **fc.own()}.items():
        want = fc.expected()[name]
        n, x, rate, channels, bps = twin(lib, data)
        assert n == want["samples"].shape[1], name
        assert np.array_equal(x, want["samples"][0]), name
        assert (rate, channels, bps) == (want["rate"], want["channels"], want["bps"]), name
        assert twin(lib, data, capacity=n)[0] == n and (n == 0 or twin(lib, data, capacity=n - 1)[0] == -1), name
    big = fc.good()["block_576"]
    assert twin(lib, big, max_block=576)[0] == 1153 and twin(lib, big, max_block=575)[0] == -1


def test_host_twin_refuses_exactly_where_the_decoder_raises(lib):
    assert len(fc.refused()) >= 24
    for name, (data, ld) in fc.refused().items():
        with pytest.raises(ValueError):
            fi.decode(data, ld=ld)
        n, _, rate, channels, bps = twin(lib, data, capacity=ld or 20000)
        assert (n, rate, channels, bps) == (-1, 0, 0, 0), name
        assert b"refused" in lib.mtts_last_error()
    # every single-byte mutation of a small stream: the twin and the decoder give the same verdict and the same samples
    data = fc.good()["lpc_small"]
    for at in range(len(data)):
        bad = data[:at] + bytes([data[at] ^ 0x04]) + data[at + 1:]
        try:
            want = fi.decode(bad)["samples"][0]
        except ValueError:
            want = None
        n, x = twin(lib, bad)[:2]
        assert (n == -1) if want is None else (n == len(want) and np.array_equal(x, want)), at


def test_entries_are_declared_bound_and_refuse_what_the_host_can_see(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    assert "FLAC in: recordings decoded on the device" in header and "flac_decode.hip" in sub("_hip").SOURCES
    for name in ("mtts_flac_decode_workspace_bytes", "mtts_flac_decode", "mtts_flac_parse_host"):
        assert re.search(r"\b%s\(" % name, header) and getattr(lib, name).argtypes is not None
    size = lib.mtts_flac_decode_workspace_bytes
    need = size(2, 4096, 8192, 4608)
    assert need >= 2 * ((2 * 8192 + 4608) * 4 + (8192 // 16 + 64) * 44 + 4096 // 8) and size(2, 4096, 8192, 16) < need
    for args, word in (((0, 4096, 8192, 4608), b"B must"), ((65536, 4096, 8192, 4608), b"B must"), ((2, 0, 8192, 4608), b"ld_bytes"),
                       ((2, 4090, 8192, 4608), b"ld_bytes"), ((2, 4096, 0, 4608), b"ld must"), ((2, 4096, 8190, 4608), b"ld must"),
                       ((2, 4096, 8192, 15), b"max_block"), ((2, 4096, 8192, 4609), b"max_block")):
        assert size(*args) == -1 and word in lib.mtts_last_error(), args
    # (data, ld_bytes, nbytes, B, max_block, out, ld, out_lengths, out_rates, ws, ws_bytes, stream): refused before a launch
    ok = (0x100000, 4096, 0x200000, 2, 4608, 0x400000, 8192, 0x300000, 0x310000, 0x800000, need, None)
    no = lambda changes: lib.mtts_flac_decode(*[changes.get(i, v) for i, v in enumerate(ok)])
    for i in (0, 2, 5, 7, 8, 9):
        assert no({i: None}) == -1 and b"null" in lib.mtts_last_error(), i
    for B in (0, -1, 65536):
        assert no({3: B}) == -1 and b"B must" in lib.mtts_last_error()
    for ld_bytes in (0, 4088, -16):
        assert no({1: ld_bytes}) == -1 and b"ld_bytes" in lib.mtts_last_error()
    for ld in (0, 8190, -4):
        assert no({6: ld}) == -1 and b"ld must" in lib.mtts_last_error()
    for mb in (15, 4609, 0):
        assert no({4: mb}) == -1 and b"max_block" in lib.mtts_last_error()
    for ws_bytes in (need - 1, 0, -5):
        assert no({10: ws_bytes}) == -1 and b"workspace too small" in lib.mtts_last_error()
    for i in (0, 5, 9):
        assert no({i: ok[i] + 4}) == -1 and b"misaligned" in lib.mtts_last_error(), i
    # d_out and d_ws inside, and straddling the end of, d_data (2 rows of 4096 bytes); d_ws inside d_out
    for i, at in ((5, 0x100000), (5, 0x100000 + 8192 - 16), (5, 0x100000 - 2 * 8192 * 4 + 16), (9, 0x100000 + 4096), (9, 0x100000 - need + 16),
                  (9, 0x400000 + 16)):
        assert no({i: at}) == -1 and b"overlap" in lib.mtts_last_error(), (i, hex(at))
    # the host twin's own arguments
    out, r = np.zeros(4, dtype=np.int32), C.c_int()
    for args in ((None, 42, 4608, out.ctypes.data, 4), (out.ctypes.data, -1, 4608, out.ctypes.data, 4), (out.ctypes.data, 4, 4608, None, 4),
                 (out.ctypes.data, 4, 15, out.ctypes.data, 4), (out.ctypes.data, 4, 4609, out.ctypes.data, 4)):
        assert lib.mtts_flac_parse_host(*args, C.byref(r), C.byref(r), C.byref(r)) == -1


# ------------------------------------------------------------------------------------------------ the Python layer
def test_read_flac_and_flac_clip_accounting():
    import torch
    ac = sub("audio_codec")
    for name in ("stereo", "lpc_wide", "variable", "metadata", "empty"):
        data, want = fc.good()[name], fc.expected()[name]
        clip = ac.read_flac(data)
        assert isinstance(clip, ac.FlacClip) and clip.data == data and clip.nbytes == len(data) == clip.tensor().numel()
        assert (clip.sample_rate, clip.samples, clip.channels, clip.bits_per_sample) == (want["rate"], want["total"], want["channels"], want["bps"])
        assert clip.numel() == want["total"] and clip.max_block == want["block_sizes"][1] and clip.tensor().dtype == torch.uint8
    t = torch.frombuffer(bytearray(fc.good()["stereo"]), dtype=torch.uint8)
    assert ac.FlacClip(t, 16000, 64, 2).tensor() is t and ac.FlacClip(t, 16000, 64, 2).nbytes == t.numel()
    ok = fc.good()["metadata"]
    r = fc.refused()
    for bad, word in ((b"ID3\x04" + ok, "ID3"), (b"OggS" + ok, "Ogg"), (b"RIFF" + ok, "marker"), (b"", "marker"), (ok[:41], "truncated"),
                      (r["no_streaminfo"][0], "STREAMINFO"), (r["type_127"][0], "type 127"), (r["metadata_runs_off"][0], "truncated"),
                      (r["block_above_max"][0], "block sizes"), (r["unknown_total"][0], "no length"),
                      (fi.stream_head(24000, 1, 32, 0, 4096, 4096), "32 bits"), (fi.stream_head(24000, 1, 4, 0, 4096, 4096), "4 bits"),
                      (fi.stream_head(0, 1, 16, 0, 4096, 4096), "rate"), (fi.stream_head(24000, 1, 16, 0, 8, 4096), "block sizes")):
        with pytest.raises(ValueError, match=word):
            ac.read_flac(bad)
    for kw in (dict(sample_rate=0), dict(samples=-1), dict(channels=9), dict(bits_per_sample=32), dict(max_block=4609), dict(max_block=8)):
        with pytest.raises(ValueError, match="FlacClip"):
            ac.FlacClip(**{"data": ok, "sample_rate": 24000, "samples": 80, **kw})
    with pytest.raises(ValueError, match="1-D uint8"):
        ac.FlacClip(torch.zeros(2, 2, dtype=torch.uint8), 24000, 4)
    # the name "flac" stays no format of Encoded / encode / decode, and points at both FLAC entries
    with pytest.raises(ValueError, match="encode_flac"):
        ac.Encoded(ok, "flac", 24000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ac.decode_flac(torch.zeros(1, 64, dtype=torch.uint8), [42])
    for bad in (15, 4609, True, "4608", None):
        with pytest.raises(ValueError, match="max_block"):
            ac.decode_flac(torch.zeros(1, 64, dtype=torch.uint8), [42], max_block=bad)
    assert ac.ENCODINGS == {"pcm16": 0, "ulaw": 1, "alaw": 2, "flac": 3} and "flac" not in ac.FORMATS and ac.FLAC not in ac.BYTES_PER_SAMPLE


def test_the_tools_reader_returns_a_flac_clip_and_reads_wav_files_as_before(tmp_path):
    import torch
    ac = sub("audio_codec")
    spec = importlib.util.spec_from_file_location("enroll_tool", ROOT / "tools" / "enroll.py")
    enroll = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(enroll)
    path = tmp_path / "clip.flac"
    path.write_bytes(fc.good()["stereo"])
    clip, rate = enroll.read_wav(path)
    assert isinstance(clip, ac.FlacClip) and rate == 16000 and clip.samples == 64 and clip.channels == 2
    words = np.arange(-300, 300, dtype="<i2")
    (tmp_path / "a.wav").write_bytes(ac.wav_bytes(words.tobytes(), "pcm16", 22050))
    (tmp_path / "u.wav").write_bytes(ac.wav_bytes(bytes(range(200)), "ulaw", 8000))
    wav, rate = enroll.read_wav(tmp_path / "a.wav")
    assert torch.is_tensor(wav) and rate == 22050 and torch.equal(wav, torch.from_numpy(words.astype(np.float32) / 32768.0))
    enc, rate = enroll.read_wav(tmp_path / "u.wav")
    assert isinstance(enc, ac.Encoded) and (enc.format, rate, enc.data) == ("ulaw", 8000, bytes(range(200)))
    clips, rates = enroll.read_wavs([path, tmp_path / "a.wav"])
    assert isinstance(clips[0], ac.FlacClip) and torch.is_tensor(clips[1]) and rates == [16000, 22050]
    # the corpus tool's listing takes a .flac that stands in for a missing wav
    spec = importlib.util.spec_from_file_location("prepare_corpus_tool", ROOT / "tools" / "prepare_corpus.py")
    pc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pc)
    (tmp_path / "wav").mkdir()
    (tmp_path / "wav" / "x.flac").write_bytes(fc.good()["stereo"])
    (tmp_path / "wav" / "y.wav").write_bytes((tmp_path / "a.wav").read_bytes())
    (tmp_path / "wav" / "y.flac").write_bytes(fc.good()["stereo"])
    (tmp_path / "list.txt").write_text("x|0|en|text\ny|1|en|text\nz|1|en|text\n")
    assert [p.name for _, _, p in pc.entries([tmp_path / "list.txt"])] == ["x.flac", "y.wav", "z.wav"]

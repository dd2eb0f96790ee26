"""CPU checks of the FLAC boundary (nothing runs on a GPU): the independent decoder against RFC 9639's first example file and the CRCs'
known answers; the restated encoder through that decoder over the signal and length grid, every rate-code branch and the frame-number
coding; the subframe kinds the fallbacks are there for; the entries declared, bound and refusing what the host can see; the pure-Python
plumbing of the name ``"flac"``."""
import hashlib
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, sub
import flac_restated as fr

EXAMPLE = ("66 4c 61 43 80 00 00 22 10 00 10 00 00 00 0f 00 00 0f 0a c4 42 f0 00 00 00 01 3e 84 b4 18 07 dc 69 03 07 58 6a 3d ad 1a 2e 0f "
           "ff f8 69 18 00 00 bf 03 58 fd 03 12 8b aa 9a")
RATES = (24000, 8000, 11025, 100000, 65537)
LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257)


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def tonal(n, seed=0):
    t = np.arange(n) / 24000.0
    x = (0.3 * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * 180 * t) + 0.1 * np.sin(2 * np.pi * 1900 * t)
         + 0.002 * np.random.default_rng(seed).standard_normal(n))
    return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int64)


def signals(n):
    rng, i = np.random.default_rng(n), np.arange(n)
    return {"tonal": tonal(n), "white": rng.integers(-32768, 32768, n), "constant": np.full(n, -1234), "zeros": np.zeros(n, dtype=np.int64),
            "alternating": np.where(i % 2 == 0, 32767, -32768), "step": np.where(i < 300, 100, -2000), "lsb": rng.integers(-2, 3, n),
            "half": np.where(i < n // 2, 0, rng.integers(-20000, 20001, n))}


# ------------------------------------------------------------------------------------------------ the decoder and the CRCs
def test_decoder_reads_the_rfc_example_file():
    data = bytes.fromhex(EXAMPLE)
    assert (GOLDEN / "rfc9639_example1.flac").read_bytes() == data
    got = fr.decode(data)
    assert got["samples"].tolist() == [[25588], [10416]] and (got["rate"], got["channels"], got["bps"], got["total"]) == (44100, 2, 16, 1)
    assert got["block_sizes"] == (4096, 4096) and got["frame_sizes"] == (15, 15) and got["frames"][0]["bytes"] == 15
    assert got["frames"][0]["kinds"] == [("VERBATIM", 0), ("VERBATIM", 0)]          # (each with wasted bits: 2 and 4)
    assert hashlib.md5(got["samples"].T.astype("<i2").tobytes()).hexdigest() == got["md5"] == "3e84b41807dc690307586a3dad1a2e0f"
    for at in (44, 49, 52, 55):                                                     # a flipped bit is seen by one of the CRCs
        bad = bytearray(data)
        bad[at] ^= 0x10
        with pytest.raises(ValueError):
            fr.decode(bytes(bad))


def test_crc_known_answers():
    frame = bytes.fromhex(EXAMPLE)[42:]
    assert fr.crc8(bytes.fromhex("ff f8 69 18 00 00")) == 0xBF
    assert fr.crc16(frame[:-2]) == 0xAA9A
    assert fr.crc8(b"") == 0 and fr.crc16(b"") == 0 and fr.crc16(b"\x00\x00" + frame[:-2]) == 0xAA9A      # leading zeros leave it alone


# ------------------------------------------------------------------------------------------------ the encoder through the decoder
@pytest.mark.parametrize("bs", [256, 4096])
def test_restated_encoder_round_trips_through_the_decoder(bs):
    longest = {256: (2 * 256 + 7, 4 * 256), 4096: (2 * 4096 + 700,)}[bs]
    for n in LENGTHS + longest:
        for j, (name, q) in enumerate(signals(n).items()):
            rate = RATES[(j + n) % len(RATES)]
            info = []
            data = fr.encode(q, rate, bs, info)
            got = fr.decode(data)
            assert np.array_equal(got["samples"][0], q) and got["samples"].shape[0] == 1, (name, n)
            assert (got["rate"], got["total"], got["bps"], got["block_sizes"], got["md5"]) == (rate, n, 16, (bs, bs), "00" * 16)
            sizes = [s for _, _, s in info]
            assert got["frame_sizes"] == ((min(sizes), max(sizes)) if sizes else (0, 0)) and all(s <= 2 * bs + 16 for s in sizes)
            assert [f["bytes"] for f in got["frames"]] == sizes and len(data) == 42 + sum(sizes)
            assert all(f["rate"] == rate and f["number"] == k and f["variable"] == 0 for k, f in enumerate(got["frames"]))
            assert [f["n"] for f in got["frames"]] == [min(bs, n - k * bs) for k in range(len(sizes))]
    assert len(fr.encode([], 24000, bs)) == 42


def test_every_rate_code_branch_and_every_block_size():
    q = tonal(700)
    for rate, (code, tail) in {24000: (7, b""), 8000: (4, b""), 96000: (11, b""), 11025: (13, b"\x2b\x11"), 65535: (13, b"\xff\xff"),
                               100000: (14, b"\x27\x10"), 655350: (14, b"\xff\xff"), 65537: (0, b""), 655360: (0, b""), 1048575: (0, b"")}.items():
        assert fr.rate_code(rate) == (code, tail), rate
        data = fr.encode(q, rate, 256)
        assert data[42 + 2] & 15 == code and fr.decode(data)["frames"][0]["rate"] == rate
    for bs in fr.BLOCK_SIZES:
        got = fr.decode(fr.encode(tonal(bs + 200), 16000, bs))
        assert [f["n"] for f in got["frames"]] == [bs, 200] and np.array_equal(got["samples"][0], tonal(bs + 200))
    for bad in (dict(rate=0), dict(rate=1 << 20), dict(bs=128), dict(bs=8192)):
        with pytest.raises(ValueError):
            fr.encode(q, bad.get("rate", 24000), bad.get("bs", 256))


def test_frame_number_coding():
    want = {0: "00", 127: "7f", 128: "c280", 2047: "dfbf", 2048: "e0a080", 65535: "efbfbf", 65536: "f0908080", (1 << 21) - 1: "f7bfbfbf"}
    for v, coded in want.items():
        assert fr.frame_number(v).hex() == coded
        if v < 0x110000 and not 0xD800 <= v < 0xE000:
            assert fr.frame_number(v) == chr(v).encode("utf-8")                    # it is UTF-8 where UTF-8 goes
        frame, _, _ = fr.encode_frame(tonal(256), v, 24000, 256)                   # ... and the decoder reads it back
        got = fr.decode(fr.encode([], 24000, 256)[:42] + frame)
        assert got["frames"][0]["number"] == v
    with pytest.raises(ValueError):
        fr.frame_number(1 << 21)


def test_subframe_kinds_and_the_size_of_a_speech_like_signal():
    kinds = lambda q, bs: [(k, o) for k, o, _ in (lambda info: (fr.encode(q, 24000, bs, info), info)[1])([])]
    rng = np.random.default_rng(5)
    assert set(kinds(rng.integers(-32768, 32768, 1500), 256)) == {("VERBATIM", 0)}
    assert set(kinds(np.where(np.arange(1500) % 2 == 0, 32767, -32768), 256)) == {("VERBATIM", 0)}
    assert set(kinds(np.full(700, -5), 256)) == set(kinds(np.zeros(700, dtype=np.int64), 4096)) == {("CONSTANT", 0)}
    assert kinds(np.r_[np.full(300, 100), np.full(300, -2000)], 256) == [("CONSTANT", 0), ("FIXED", 1), ("CONSTANT", 0)]
    q = tonal(48000)
    info = []
    data = fr.encode(q, 24000, 4096, info)
    assert {(k, o) for k, o, _ in info} == {("FIXED", 3)}
    ratio = len(data) / (2 * q.size)
    print(f"tonal signal, 48000 samples, block size 4096: {len(data)} bytes, {ratio:.4f} of PCM16")
    assert 0.6 < ratio < 0.75                                                      # about 0.70
    # a frame whose halves differ chooses a k per partition
    half = np.r_[np.zeros(2048, dtype=np.int64), rng.integers(-20000, 20001, 2048)]
    one_k = fr.encode(half, 24000, 4096)
    flat = fr._rice_partition(np.where(half >= 0, 2 * half, -2 * half - 1))[1].size
    assert len(one_k) * 8 < flat and np.array_equal(fr.decode(one_k)["samples"][0], half)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entries_are_declared_and_sized(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert int(re.search(r"#define MTTS_FLAC (\d+)", header).group(1)) == 3 == sub("audio_codec").FLAC
    hip = sub("_hip")
    assert "flac.hip" in hip.SOURCES
    import ctypes as C
    assert lib.mtts_flac_encode.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.mtts_flac_row_bytes.restype == lib.mtts_flac_workspace_bytes.restype == C.c_int64
    for ld, bs in ((4, 256), (256, 256), (260, 256), (8892, 4096), (48000, 4096), (48000, 1024)):
        frames = -(-ld // bs)
        assert lib.mtts_flac_row_bytes(ld, bs) == (42 + frames * (2 * bs + 16) + 15) // 16 * 16
        for B in (1, 5):
            need = lib.mtts_flac_workspace_bytes(B, ld, bs)
            assert need >= B * frames * (2 * bs + 16 + 4 + 8) and need <= B * frames * (2 * bs + 16 + 4 + 8) + 3 * 256
    for ld, bs in ((0, 256), (1022, 256), (-4, 256), ((1 << 30) + 4, 256), (1024, 128), (1024, 300), (1024, 8192), (1024, 0)):
        assert lib.mtts_flac_row_bytes(ld, bs) == -1 and lib.mtts_flac_workspace_bytes(2, ld, bs) == -1, (ld, bs)
    assert lib.mtts_flac_workspace_bytes(0, 1024, 256) == -1 and b"B must" in lib.mtts_last_error()


def test_encode_refuses_what_the_host_can_see(lib):
    # (audio, ld, lengths, rates, keys, B, block_size, dither, seed, out, out_ld, out_bytes, ws, ws_bytes, stream): refused before a launch
    stride, need = lib.mtts_flac_row_bytes(1024, 256), lib.mtts_flac_workspace_bytes(2, 1024, 256)
    ok = (0x100000, 1024, 0x200000, 0x300000, None, 2, 256, 0, 0, 0x400000, stride, 0x500000, 0x600000, need, None)
    no = lambda changes: lib.mtts_flac_encode(*[changes.get(i, v) for i, v in enumerate(ok)])
    for i in (0, 2, 3, 9, 11, 12):                               # every pointer but the keys, which may be null
        assert no({i: None}) == -1 and b"null" in lib.mtts_last_error(), i
    assert no({5: 0}) == -1 and b"B must" in lib.mtts_last_error()
    for ld in (0, 1022, -4):
        assert no({1: ld}) == -1 and b"multiple of 4" in lib.mtts_last_error()
    for bs in (0, 128, 257, 8192):
        assert no({6: bs}) == -1 and b"block_size" in lib.mtts_last_error()
    for out_ld in (stride - 16, stride + 8, 0):
        assert no({10: out_ld}) == -1 and b"out_ld" in lib.mtts_last_error()
    for ws_bytes in (need - 1, 0, -5):
        assert no({13: ws_bytes}) == -1 and b"workspace too small" in lib.mtts_last_error()
    for i in (0, 9, 12):
        assert no({i: ok[i] + 4}) == -1 and b"misaligned" in lib.mtts_last_error(), i
    # d_out and d_ws inside, and straddling the end of, d_audio (2 rows of 1024 floats = 8192 bytes); d_ws inside d_out
    for i, at in ((9, 0x100000), (9, 0x100000 + 8192 - 16), (9, 0x100000 - 2 * stride + 16), (12, 0x100000 + 4096), (12, 0x100000 - need + 16),
                  (12, 0x400000 + 16)):
        assert no({i: at}) == -1 and b"overlap" in lib.mtts_last_error(), (i, hex(at))


# ------------------------------------------------------------------------------------------------ the name through the Python layers
def test_flac_is_an_encoding_and_no_sample_format():
    import torch
    ac, wf = sub("audio_codec"), sub("waveform")
    assert ac.ENCODINGS == {"pcm16": 0, "ulaw": 1, "alaw": 2, "flac": 3} and ac.FLAC not in ac.BYTES_PER_SAMPLE and "flac" not in ac.FORMATS
    assert ac.encoding_id("flac") == ac.encoding_id(3) == 3 and ac.encoding_id("ulaw") == 1
    for bad in ("mp3", "FLAC", None, True, 4):
        with pytest.raises(ValueError):
            ac.encoding_id(bad)
    assert wf._encodings_per_row("flac", 3) == [3, 3, 3] and wf._encodings_per_row([None, "flac", "pcm16"], 3) == [None, 3, 0]
    assert wf._encodings_per_row([None, None], 2) is None
    with pytest.raises(ValueError, match="one per row"):
        wf._encodings_per_row(["flac"], 2)
    # the entries whose rows are samples of a fixed size point at encode_flac, before they look at anything else
    for call in (lambda: ac.encode(torch.zeros(1, 8), None, "flac"), lambda: ac.encode(torch.zeros(2, 8), None, ["pcm16", "flac"]),
                 lambda: ac.Encoded(b"fLaC", "flac", 24000), lambda: ac.wav_bytes(b"", "flac", 24000), lambda: ac.formats_per_row("flac", 2)):
        with pytest.raises(ValueError, match="encode_flac"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ac.encode_flac(torch.zeros(1, 8), None, 24000)
    for bad in (100, 4095, True, "4096", None):
        with pytest.raises(ValueError, match="block size"):
            ac.encode_flac(torch.zeros(1, 8), None, 24000, block_size=bad)


def test_requests_documents_and_the_service_take_the_name():
    import torch
    bt, sv = sub("batcher"), sub("serving")
    r = bt.Request(ids=[1, 2], encoding="flac", dither=True, dither_key=4)
    asked = bt.tail_options([bt.Request(ids=[3]), r])
    assert (asked["encoding"], asked["dither"], asked["dither_keys"]) == ([None, "flac"], [False, True], [0, 4])
    assert bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0.0], encoding="flac").encoding == "flac"
    with pytest.raises(ValueError):
        bt.Request(ids=[1], encoding="FLAC")
    assert sv.COMPRESSED_FORMATS == {"flac": "flac"} and "flac" not in sv.RESPONSE_FORMATS
    assert sv.response_encoding("flac", flac=True) == "flac" and sv.response_encoding("wav", flac=True) == "pcm16"
    assert sv.response_encoding(None, flac=True) is None
    with pytest.raises(ValueError, match="flac=True"):                             # a service that did not opt in answers as it always has
        sv.response_encoding("flac")
    with pytest.raises(ValueError, match="response_format"):
        sv.response_encoding("mp3", flac=True)
    stream = fr.encode(tonal(300), 8000, 256)
    res = {"audio": torch.frombuffer(bytearray(stream), dtype=torch.uint8), "encoding": "flac", "sample_rate": 8000}
    body = sv.response_body(res, "flac", 8000)
    assert isinstance(body, bytes) and body == stream                              # as it is: it already is a file
    seen = []

    def run(batch):
        seen.extend(batch)
        return [{"mel_length": len(q.ids), "audio": res["audio"], "encoding": q.encoding} for q in batch]

    q = bt.FrameBudgetBatcher(model=None, max_batch=4, max_tokens=4096, max_wait_ms=5.0, run_batch=run)
    svc = sv.SpeechService(q, phonemize=lambda text, lang: [1 + (ord(c) % 50) for c in text], flac=True)
    assert svc.levelled(-16).flac and svc.timed().flac                             # the views keep the choice
    import asyncio
    with q:
        assert asyncio.run(svc.speak("lossless", sample_rate=8000, response_format="flac")) == stream
    assert [(s.encoding, s.sample_rate) for s in seen] == [("flac", 8000)]

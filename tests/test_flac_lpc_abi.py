"""CPU checks of the LPC side of FLAC out (nothing runs on a GPU): the restated encoder (tests/flac_lpc_restated.py) through the
independent decoder of tests/flac_in_restated.py and through the project's own host parser over the whole case list; order 0 against
tests/flac_restated.py; no frame longer than its FIXED twin; every subframe kind present; the size on the speech-like signal; the
analysis steps on known answers; the entry declared, bound and refusing what the host can see; ``lpc_order`` / ``flac_lpc`` through the
Python layers."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT, sub
import flac_in_restated as fi
import flac_lpc_restated as fl
import flac_restated as fr


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


@pytest.fixture(scope="module")
def streams():
    """``{(block size, max order): [(name, n, words, rate, stream, info)]}`` over the case list, encoded once."""
    out = {}
    for bs in fl.BLOCK_SIZES:
        for mo in fl.MAX_ORDERS:
            rows = []
            for name, n, q, rate in fl.cases():
                info = []
                rows.append((name, n, q, rate, fl.encode(q, rate, bs, mo, info), info))
            out[bs, mo] = rows
    return out


def parse_host(lib, data, capacity):
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8).copy()
    out = np.full(capacity + 8, 0x5A5A5A5A, dtype=np.int32)
    rate, channels, bps = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    n = lib.mtts_flac_parse_host(buf.ctypes.data, len(data), 4608, out.ctypes.data, capacity, C.byref(rate), C.byref(channels), C.byref(bps))
    assert (out[capacity:] == 0x5A5A5A5A).all()
    return n, out[:max(n, 0)].astype(np.int64), rate.value, channels.value, bps.value


# ------------------------------------------------------------------------------------------------ the streams
def test_restated_streams_decode_to_their_words(streams):
    for (bs, mo), rows in streams.items():
        for name, n, q, rate, data, info in rows:
            got = fi.decode(data)
            assert got["samples"].shape == (1, n) and np.array_equal(got["samples"][0], q), (name, n, bs, mo)
            assert (got["rate"], got["total"], got["bps"], got["block_sizes"]) == (rate, n, 16, (bs, bs))
            assert [f["bytes"] for f in got["frames"]] == [s for _, _, s in info] and len(data) == 42 + sum(s for _, _, s in info)
            assert [f["kinds"][0] for f in got["frames"]] == [(k, o) for k, o, _ in info]       # the decoder saw the kinds the encoder names
            assert all(s <= 2 * bs + 16 for _, _, s in info)


def test_the_host_parser_reads_the_restated_streams(lib, streams):
    for (bs, mo), rows in streams.items():
        for name, n, q, rate, data, info in rows:
            got, x, r, ch, bps = parse_host(lib, data, max(n, 1))
            assert got == n and np.array_equal(x, q) and (r, ch, bps) == (rate, 1, 16), (name, n, bs, mo)


def test_order_zero_is_the_fixed_encoder():
    for bs in fl.BLOCK_SIZES:
        for name, n, q, rate in fl.cases():
            assert fl.encode(q, rate, bs, 0) == fr.encode(q, rate, bs), (name, n, bs)
    for bad in (-1, 13, True):
        with pytest.raises(ValueError):
            fl.encode(np.zeros(4, dtype=np.int64), 24000, 256, bad)


def test_no_frame_is_longer_than_its_fixed_twin(streams):
    for (bs, mo), rows in streams.items():
        for name, n, q, rate, data, info in rows:
            fixed = []
            fr.encode(q, rate, bs, fixed)
            assert len(info) == len(fixed) and all(a[2] <= b[2] for a, b in zip(info, fixed)), (name, n, bs, mo)


def test_every_kind_of_subframe_occurs(streams):
    kinds = {}
    for (bs, mo), rows in streams.items():
        for name, n, q, rate, data, info in rows:
            for k, o, _ in info:
                kinds.setdefault(k, set()).add((name, o))
    print({k: sorted(v) for k, v in kinds.items()})
    assert set(kinds) == {"LPC", "FIXED", "CONSTANT", "VERBATIM"}
    assert {o for _, o in kinds["LPC"]} >= {1, 4, 8, 12}                           # every candidate order wins somewhere
    assert ("ramp", 2) in kinds["FIXED"] and not any(name == "ramp" for name, _ in kinds["LPC"])     # an exact FIXED keeps the tie
    assert ("white", 0) in kinds["VERBATIM"] and ("constant", 0) in kinds["CONSTANT"]
    # the list is cut by order < n: 12 samples try orders 4 and 8 only, 13 try 12 too
    assert fl.candidates(12, 12) == [4, 8] and fl.candidates(12, 13) == [4, 8, 12] and fl.candidates(12, 1) == []
    assert fl.candidates(1, 4096) == [1] and fl.candidates(8, 4096) == [4, 8] and fl.candidates(6, 4096) == [4, 6] and fl.candidates(3, 3) == []


def test_speech_like_signal_is_smaller_with_lpc():
    q = fl.speech_like(81920, 7)
    fixed = len(fr.encode(q, 24000, 4096))
    lpc8, lpc12 = len(fl.encode(q, 24000, 4096, 8)), len(fl.encode(q, 24000, 4096, 12))
    print(f"speech_like(81920, seed 7), block 4096: FIXED {fixed} bytes, LPC 8 {lpc8} ({lpc8 / fixed:.4f}), LPC 12 {lpc12} ({lpc12 / fixed:.4f}); "
          f"{lpc12 / (2 * q.size):.4f} of PCM16")
    assert lpc12 < 0.90 * fixed                                                    # measured 0.8203 (0.8731 at order 8)
    assert lpc12 < lpc8 < fixed


# ------------------------------------------------------------------------------------------------ the analysis on known answers
def test_window_autocorrelation_recursion_and_quantisation():
    assert fl.window(1).tolist() == [255] and fl.window(2).tolist() == [192, 192] and fl.window(4).tolist() == [112, 240, 240, 112]
    for n in (1, 2, 12, 13, 255, 256, 257, 4095, 4096):
        w = fl.window(n)
        assert w.min() >= 1 and w.max() <= 255 and np.array_equal(w, w[::-1]) and 255 * (n - 1) ** 2 < 1 << 32
    q = np.array([3, -1, 4, 1, -5], dtype=np.int64)
    x = q * fl.window(5)
    assert fl.autocorrelation(q, 2) == [int((x * x).sum()), int((x[:-1] * x[1:]).sum()), int((x[:-2] * x[2:]).sum())]
    # an AR(1) sequence: the recursion finds its pole at order 1 and adds nothing at order 2
    R = [1.0, 0.5, 0.25, 0.125]
    a = fl.levinson(R, 3)
    assert a[1] == [0.5] and a[2] == [0.5, 0.0] and a[3] == [0.5, 0.0, 0.0]
    assert fl.levinson([0.0, 0.0], 1) == {} and fl.levinson([1.0, 1.0, 1.0], 2) == {}      # no energy; an error of exactly zero
    assert list(fl.levinson([1.0, 0.5, 2.0], 2)) == [1]                           # |k| > 1 at order 2: it stops there
    # the shift follows the exponent field: max|a| in [1, 2) -> e = 1 -> 10; in [0.5, 1) -> 11; tiny -> the cap; >= 2048 -> dropped
    assert fl.quantise([1.5, -0.25]) == (10, [1536, -256]) and fl.quantise([0.75]) == (11, [1536]) and fl.quantise([-1.0]) == (10, [-1024])
    assert fl.quantise([1e-9, 0.0]) == (15, [0, 0]) and fl.quantise([0.0]) == (15, [0])
    assert fl.quantise([2047.5]) == (0, [2047]) and fl.quantise([-2047.5]) == (0, [-2048]) and fl.quantise([2048.0]) is None       # ties to even, the clamp
    assert fl.quantise([1026.5 / 2048, 1027.5 / 2048, -1026.5 / 2048]) == (11, [1026, 1028, -1026])    # ties to even
    assert fl.quantise([float("inf")]) is None and fl.quantise([float("nan")]) is None
    # prediction with an arithmetic shift, and the range drop
    q = np.array([100, -200, 300, -400], dtype=np.int64)
    assert fl.lpc_residual(q, [-3, 1], 1).tolist() == [0, 0, 300 - ((-3 * -200 + 100) >> 1), -400 - ((-3 * 300 - 200) >> 1)]
    big = np.where(np.arange(40) % 2 == 0, 32767, -32767)
    assert fl.lpc_subframe(big, 256, 1, 0, [-2048]) is None                        # (|r| = 32767 * 2049: beyond 2^20)
    assert fl.lpc_subframe(big, 256, 1, 11, [-2048]) is not None


# ------------------------------------------------------------------------------------------------ the C boundary
def test_entry_is_declared_bound_and_refuses_what_the_host_can_see(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    assert re.search(r"\bint mtts_flac_encode_lpc\(", header) and "writing LPC subframes" not in header
    old, new = lib.mtts_flac_encode.argtypes, lib.mtts_flac_encode_lpc.argtypes
    assert new == old[:7] + [C.c_int] + old[7:] and lib.mtts_flac_encode_lpc.restype == C.c_int    # max_lpc_order behind block_size
    # (audio, ld, lengths, rates, keys, B, block_size, max_lpc_order, dither, seed, out, out_ld, out_bytes, ws, ws_bytes, stream): refused
    # before a launch; the sizes are those of the old entry
    stride, need = lib.mtts_flac_row_bytes(1024, 256), lib.mtts_flac_workspace_bytes(2, 1024, 256)
    ok = (0x100000, 1024, 0x200000, 0x300000, None, 2, 256, 12, 0, 0, 0x400000, stride, 0x500000, 0x600000, need, None)
    no = lambda changes: lib.mtts_flac_encode_lpc(*[changes.get(i, v) for i, v in enumerate(ok)])
    for bad in (-1, 13, 32, 1 << 20):
        assert no({7: bad}) == -1 and b"max_lpc_order" in lib.mtts_last_error(), bad
    for i in (0, 2, 3, 10, 12, 13):
        assert no({i: None}) == -1 and b"mtts_flac_encode_lpc: null" in lib.mtts_last_error(), i
    assert no({5: 0}) == -1 and b"B must" in lib.mtts_last_error()
    for ld in (0, 1022, -4):
        assert no({1: ld}) == -1 and b"multiple of 4" in lib.mtts_last_error()
    for bs in (0, 128, 257, 8192):
        assert no({6: bs}) == -1 and b"block_size" in lib.mtts_last_error()
    for out_ld in (stride - 16, stride + 8, 0):
        assert no({11: out_ld}) == -1 and b"out_ld" in lib.mtts_last_error()
    for ws_bytes in (need - 1, 0, -5):
        assert no({14: ws_bytes}) == -1 and b"workspace too small" in lib.mtts_last_error()
    for i in (0, 10, 13):
        assert no({i: ok[i] + 4}) == -1 and b"misaligned" in lib.mtts_last_error(), i
    for i, at in ((10, 0x100000), (10, 0x100000 + 8192 - 16), (13, 0x100000 + 4096), (13, 0x400000 + 16)):
        assert no({i: at}) == -1 and b"overlap" in lib.mtts_last_error(), (i, hex(at))
    for mo in (0, 1, 12):                                                          # a good order passes that check: the next refusal speaks
        assert no({7: mo, 5: 0}) == -1 and b"B must" in lib.mtts_last_error()


# ------------------------------------------------------------------------------------------------ the argument through the Python layers
def test_lpc_order_through_the_python_layers():
    import torch
    ac, wf, bt, sv = sub("audio_codec"), sub("waveform"), sub("batcher"), sub("serving")
    assert ac.FLAC_MAX_LPC_ORDER == fl.MAX_ORDER == 12
    assert [ac.flac_lpc_order(v) for v in (0, 1, 12, np.int64(8))] == [0, 1, 12, 8]
    for bad in (-1, 13, True, "12", None, 4.0):
        with pytest.raises(ValueError, match="LPC order"):
            ac.encode_flac(torch.zeros(1, 8), None, 24000, lpc_order=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ac.encode_flac(torch.zeros(1, 8), None, 24000, lpc_order=12)
    # requests and documents: a value needs encoding="flac"
    r = bt.Request(ids=[1, 2], encoding="flac", flac_lpc=12)
    asked = bt.tail_options([bt.Request(ids=[3], encoding="flac"), r])
    assert asked["flac_lpc"] == [0, 12] and asked["encoding"] == ["flac", "flac"]
    assert "flac_lpc" not in bt.tail_options([bt.Request(ids=[3]), bt.Request(ids=[4], encoding="flac")])
    assert bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0.0], encoding="flac", flac_lpc=8).flac_lpc == 8
    for make in (lambda: bt.Request(ids=[1], flac_lpc=12), lambda: bt.Request(ids=[1], encoding="pcm16", flac_lpc=12),
                 lambda: bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0.0], encoding="pcm16", flac_lpc=4)):
        with pytest.raises(ValueError, match="flac_lpc"):
            make()
    for bad in (13, -1, True):
        with pytest.raises(ValueError, match="LPC order"):
            bt.Request(ids=[1], encoding="flac", flac_lpc=bad)
    with pytest.raises(ValueError, match="flac_lpc"):
        wf.tail(torch.zeros(1, 4, 4), [4], None, encoding="pcm16", flac_lpc=12)
    with pytest.raises(ValueError, match="flac_lpc"):
        wf.finish_request(torch.zeros(8), encoding="pcm16", flac_lpc=12)
    # the service: the choice is made where it is built, kept by its views, and needs flac=True
    seen = []

    def run(batch):
        seen.extend(batch)
        return [{"mel_length": len(q.ids), "audio": torch.zeros(4, dtype=torch.uint8), "encoding": q.encoding} for q in batch]

    q = bt.FrameBudgetBatcher(model=None, max_batch=4, max_tokens=4096, max_wait_ms=5.0, run_batch=run)
    phon = lambda text, lang: [1 + (ord(c) % 50) for c in text]
    svc = sv.SpeechService(q, phonemize=phon, flac=True, flac_lpc=12)
    assert svc.flac_lpc == 12 and svc.levelled(-16).flac_lpc == 12 and svc.timed().flac_lpc == 12
    assert sv.SpeechService(q, phonemize=phon, flac=True).flac_lpc == 0
    with pytest.raises(ValueError, match="flac=True"):
        sv.SpeechService(q, phonemize=phon, flac_lpc=12)
    with pytest.raises(ValueError, match="LPC order"):
        sv.SpeechService(q, phonemize=phon, flac=True, flac_lpc=13)
    import asyncio
    with q:
        asyncio.run(svc.speak("lossless", response_format="flac"))
        asyncio.run(svc.speak("plain", response_format="pcm"))
    assert [(s.encoding, s.flac_lpc) for s in seen] == [("flac", 12), ("pcm16", 0)]

"""``mtts_loudness_r128`` and ``mtts_true_peak_filter`` (include/mtts.h "loudness") without a GPU: the bindings and what the host
refuses, the interpolator's table against the NumPy restatement (tests/r128_restated.py), the restatement against figures worked out
by hand and with an independent long interpolation, and the pure helpers the true-peak ceiling travels through."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest

from conftest import ROOT, sub
import loudness_restated as lr
import r128_restated as rr

FS = 24000


def am_noise(n, seed, rms=0.09, fs=24000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (rng.standard_normal(n) * rms * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t))).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


@pytest.fixture(scope="module")
def lra_inputs():
    """The two loudness-range inputs, restated once; every short-term block at least 0.01 dB from both gates."""
    a = am_noise(8 * FS, 21)
    a[4 * FS:] *= np.float32(10 ** (-12 / 20))
    b = am_noise(10 * FS, 22)
    b[3 * FS:6 * FS] *= np.float32(10 ** (-35 / 20))
    got = [rr.meter(a, FS), rr.meter(b, FS)]
    print(f"smallest distance of a short-term block from a gate: {min(m['margin'] for m in got):.4f} dB")
    assert min(m["margin"] for m in got) >= 0.01
    return got


# ------------------------------------------------------------------------------------------------ the C ABI
def test_bindings_exist_and_match_the_header(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    tile = int(re.search(r"#define MTTS_TRUE_PEAK_TILE (\d+)", header).group(1))
    taps = int(re.search(r"#define MTTS_TRUE_PEAK_TAPS (\d+)", header).group(1))
    assert lib.mtts_true_peak_tile() == tile == sub("loudness").TRUE_PEAK_TILE and taps == rr.TAPS == 12
    assert "True peak (oversampled) and loudness range are\n * not computed" not in header
    assert "not computed" not in (sub("loudness").__doc__ or "")


@pytest.mark.parametrize("fs", [8000, 24000, 48000, 96000])
def test_library_filter_is_the_restated_one(lib, fs):
    out, F = (C.c_float * 96)(), C.c_int(0)
    assert lib.mtts_true_peak_filter(fs, out, C.byref(F)) == 0
    want_F, table = rr.filter_table(fs)
    assert F.value == want_F == {8000: 8, 24000: 8, 48000: 4, 96000: 2}[fs]
    got = np.array(list(out)[:12 * want_F], dtype=np.float32).reshape(want_F, 12)
    want = table.astype(np.float32)
    # libm and NumPy may round the fp64 value to different neighbours: one fp32 unit in the last place per coefficient
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    assert np.all(np.abs(got.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6) and np.all(np.abs(table.sum(axis=1) - 1.0) <= 1e-15)
    assert got[0].tolist() == [0.0] * 5 + [1.0] + [0.0] * 6       # phase 0 is the sample itself
    h2, t2 = sub("loudness").true_peak_filter(fs)
    assert h2 == want_F and np.array_equal(t2.numpy(), got)


def test_r128_refuses_what_the_host_can_see(lib):
    # (audio, ld, lengths, B, rate, target, ceiling, tp_db, apply, lufs, gain, peak, tp, lra, mmax, smax, ws, ws_bytes, stream)
    ok = (0x100000, 1024, 0x200000, 2, 24000, None, 0.95, -1.0, 1, 0x300000, 0x400000, 0x500000, 0x700000, 0x800000, 0x900000, 0xa00000,
          0x600000, 1 << 20, None)
    for i in (0, 2, 9, 10, 11, 12, 13, 14, 15, 16):              # every pointer but the targets, which may be null
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_loudness_r128(*bad) == -1 and b"null" in lib.mtts_last_error()
    for B in (0, 65536):
        bad = list(ok); bad[3] = B
        assert lib.mtts_loudness_r128(*bad) == -1 and b"B must" in lib.mtts_last_error()
    for ld in (0, 1022, -4):
        bad = list(ok); bad[1] = ld
        assert lib.mtts_loudness_r128(*bad) == -1 and b"multiple of 4" in lib.mtts_last_error()
    bad = list(ok); bad[1] = (1 << 30) + 4
    assert lib.mtts_loudness_r128(*bad) == -1 and b"2^30" in lib.mtts_last_error()
    for rate in (7900, 24050, 192100, 0):
        bad = list(ok); bad[4] = rate
        assert lib.mtts_loudness_r128(*bad) == -1 and b"sample_rate" in lib.mtts_last_error()
        assert lib.mtts_loudness_r128_workspace_bytes(1024, 2, rate) == -1
        assert lib.mtts_true_peak_filter(rate, (C.c_float * 96)(), C.byref(C.c_int(0))) == -1 and b"sample_rate" in lib.mtts_last_error()
    for i, p in ((0, 0x100004), (16, 0x600008), (9, 0x300004), (13, 0x800004), (14, 0x900004), (15, 0xa00004)):
        bad = list(ok); bad[i] = p
        assert lib.mtts_loudness_r128(*bad) == -1 and b"misaligned" in lib.mtts_last_error()
    for ceiling in (0.0, -1.0, math.inf, math.nan):
        bad = list(ok); bad[6] = ceiling
        assert lib.mtts_loudness_r128(*bad) == -1 and b"peak_ceiling" in lib.mtts_last_error()
    for tp in (0.5, math.inf, -math.inf):                         # (NaN means none and is no refusal)
        bad = list(ok); bad[7] = tp
        assert lib.mtts_loudness_r128(*bad) == -1 and b"true_peak_ceiling_db" in lib.mtts_last_error()
    need = lib.mtts_loudness_r128_workspace_bytes(1024, 2, 24000)
    bad = list(ok); bad[17] = need - 1
    assert lib.mtts_loudness_r128(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()
    assert lib.mtts_true_peak_filter(24000, None, C.byref(C.c_int(0))) == -1 and lib.mtts_true_peak_filter(24000, (C.c_float * 96)(), None) == -1
    # the workspace holds that of mtts_loudness and grows with the row
    assert need > lib.mtts_loudness_workspace_bytes(1024, 2, 24000)
    large = lib.mtts_loudness_r128_workspace_bytes(1 << 21, 2, 24000)
    assert need < large < 64 << 20


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("fs", [8000, 24000, 48000])
def test_restated_true_peak_of_a_sine_between_the_samples(fs):
    """Amplitude 0.5 at fs / 4 with phase pi / 4: every sample is 0.5 / sqrt 2, the peaks lie half way between two of them."""
    x = (0.5 * np.sin(2.0 * np.pi * (fs / 4.0) * np.arange(4000) / fs + np.pi / 4.0)).astype(np.float32)
    got = float(rr.true_peak(x, fs))
    print(f"fs {fs}: sample peak {np.abs(x).max():.4f}, true peak {got:.5f} = {got / 0.5:.4f} x the amplitude")
    assert abs(float(np.abs(x).max()) - 0.3536) < 1e-4 and 0.5 <= got <= 0.51


def test_restated_true_peak_edges_and_nan():
    assert rr.true_peak(np.zeros(0, np.float32), FS) == 0.0
    one = rr.true_peak(np.array([0.25], np.float32), FS)
    assert one == np.float32(0.25)                                # a single sample: every phase reads less than the sample
    x = am_noise(500, 1)
    y = x.copy()
    y[100] = np.float32(np.nan)
    got = rr.true_peak(y, FS)
    assert np.isfinite(got) and 0 < got <= rr.true_peak(x, FS) * 1.5
    # the fixed order: a plain Python loop over one position gives the same bits as the vectorised form
    h = rr.filter_table(FS)[1].astype(np.float32)
    pad = np.concatenate([np.zeros(5, np.float32), x, np.zeros(6, np.float32)])
    best = np.float32(0)
    for j in range(len(x)):
        best = max(best, abs(x[j]))
        for p in range(1, 8):
            acc = np.float32(0)
            for k in range(12):
                acc = np.float32(acc + np.float32(h[p, k] * pad[j + k]))
            best = max(best, abs(acc))
    assert np.float32(best).view(np.uint32) == rr.true_peak(x, FS).view(np.uint32)


def test_percentile_indices():
    assert [rr.percentile_indices(n) for n in (1, 2, 10, 11, 21, 100)] == [(0, 0), (0, 1), (1, 9), (1, 10), (2, 19), (10, 94)]


def test_restated_loudness_range(lra_inputs):
    a, b = lra_inputs
    print(f"two levels: LRA {a['lra']:.4f} LU, {a['n']} of {len(a['short'])} blocks, margin {a['margin']:.2f} dB; "
          f"dip: LRA {b['lra']:.4f} LU, {b['n']} of {len(b['short'])} blocks, margin {b['margin']:.2f} dB")
    assert abs(a["lra"] - 12.03) < 0.005 and a["n"] == 51 == len(a["short"]) and abs(a["margin"] - 10.8) < 0.05
    assert abs(b["lra"] - 8.94) < 0.005 and b["n"] == 70 and len(b["short"]) == 71 and abs(b["margin"] - 2.08) < 0.01
    # lufs and peak are loudness_restated's; the maxima bound the integrated figure from above
    for m in (a, b):
        assert m["momentary_max"] >= m["short_term_max"] >= m["lufs"] - 3.0 and math.isfinite(m["short_term_max"])
    short = rr.meter(am_noise(int(2.9 * FS), 24), FS)
    assert short["lra"] == 0.0 and short["short_term_max"] == -math.inf and math.isfinite(short["momentary_max"])
    tiny = rr.meter(am_noise(int(0.3 * FS), 25), FS)
    assert tiny["momentary_max"] == tiny["lufs"] and tiny["lra"] == 0.0
    empty = rr.meter(np.zeros(0, np.float32), FS)
    assert empty["momentary_max"] == -math.inf and empty["lra"] == 0.0 and empty["true_peak"] == 0.0
    silent = rr.meter(np.zeros(4 * FS, np.float32), FS)
    assert silent["lra"] == 0.0 and silent["short_term_max"] == -math.inf and silent["n"] == 0


def test_restated_gain_with_two_ceilings():
    # no ceiling, or one that does not bind: loudness_restated's gain bit for bit
    for args in ((-20.0, -23.0, 0.5), (-30.0, -10.0, 0.5)):
        assert rr.gain(*args, 0.6, None) == lr.gain(*args) and rr.gain(*args, 0.1, -1.0) == lr.gain(*args)
    c = rr.ceiling_linear(-1.0)
    assert abs(float(c) - 10 ** (-1 / 20)) < 1e-7 and np.isnan(rr.ceiling_linear(None))
    g = rr.gain(-30.0, -10.0, 0.5, 0.55, -1.0)                    # the sample ceiling gives 1.9; 0.55 * 1.9 > 0.891: the second one binds
    assert g < lr.gain(-30.0, -10.0, 0.5) and np.float32(0.55) * g <= c and abs(float(g) - float(c) / 0.55) < 1e-6
    assert rr.gain(-math.inf, -23.0, 0.0, 0.0, -1.0) == 1.0 and rr.gain(-20.0, None, 0.5, 0.9, -1.0) == 1.0
    assert rr.gain(-20.0, -10.0, 0.5, 0.9, -1.0, n=0) == 1.0


# ------------------------------------------------------------------------------------------------ the pure helpers
def test_python_entries_refuse_before_anything_is_launched():
    import torch
    L = sub("loudness")
    assert L.check_true_peak(None) is None and L.check_true_peak(-1) == -1.0 and L.check_true_peak(0) == 0.0
    for bad in ("loud", True, [-1.0]):
        with pytest.raises(TypeError):
            L.check_true_peak(bad)
    for bad in (0.5, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="dBTP"):
            L.check_true_peak(bad)
    assert L.dbtp(1.0) == 0.0 and abs(L.dbtp(0.5) + 6.0206) < 1e-4 and L.dbtp(0.0) == -math.inf
    assert abs(float(L.dbtp(torch.tensor([0.5]))[0]) + 6.0206) < 1e-4
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.meter(torch.zeros(1, 8))
    with pytest.raises(ValueError, match="dBTP"):
        L.normalize(torch.zeros(1, 8), None, -23.0, true_peak=1.0)
    inf = sub("inference")
    for fn in (inf.to_waveforms, inf.pipeline):
        p = inspect.signature(fn).parameters
        assert p["true_peak"].default is None and p["true_peak"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(inf.to_waveforms).parameters["return_meter"].default is False
    # a ceiling on a row without a target: refused on the host, ahead of the vocoder (None here)
    for kw in (dict(true_peak=-1.0), dict(true_peak=-1.0, loudness=[None, None]), dict(true_peak=[-1.0, -1.0], loudness=[-23.0, None]),
               dict(true_peak=[None, -2.0], loudness=[-23.0, None]), dict(true_peak=0.5, loudness=-23.0), dict(true_peak="hot", loudness=-23.0)):
        with pytest.raises((TypeError, ValueError)):
            inf.to_waveforms(None, [1, 1], None, **kw)
    ceilings = sub("waveform")._true_peak_ceilings
    assert ceilings(-1.0, [-23.0, math.nan], 2) == [-1.0, None]          # one ceiling: it binds the rows with a target
    assert ceilings([None, -2], [-23.0, -16.0], 2) == [None, -2.0] and ceilings([None, None], None, 2) is None
    with pytest.raises(ValueError, match="one per row"):
        ceilings([-1.0], [-23.0, -23.0], 2)
    with pytest.raises(ValueError, match="target"):
        inf.pipeline(None, None, "never spoken", true_peak=-1.0)


def test_request_document_and_service_fields():
    import torch
    bt, sv = sub("batcher"), sub("serving")
    r = bt.Request(ids=[1, 2])
    true_peak_field = lambda batch: bt.tail_options(batch).get("true_peak")
    assert r.true_peak is None and true_peak_field([r, bt.Request(ids=[3], loudness=-16)]) is None
    mixed = [r, bt.Request(ids=[3], loudness=-16, true_peak=-1), bt.Request(ids=[4], loudness=-23.0)]
    assert true_peak_field(mixed) == [None, -1.0, None] and isinstance(mixed[1].true_peak, float)
    d = bt.Document(rows=[bt.Request(ids=[1]), bt.Request(ids=[2])], pauses_ms=[100, 0], loudness=-19, true_peak=-2.0)
    assert true_peak_field([d, r]) == [-2.0, None] and all(x.true_peak is None for x in d.rows)
    for make in (lambda **kw: bt.Request(ids=[1], **kw), lambda **kw: bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0], **kw)):
        with pytest.raises(ValueError, match="target"):
            make(true_peak=-1.0)                                  # a ceiling without a target
        with pytest.raises(ValueError, match="dBTP"):
            make(loudness=-23, true_peak=0.5)
        with pytest.raises(TypeError):
            make(loudness=-23, true_peak="hot")
    # what a result carries
    rep = dict(lufs=-20.5, gain=0.75, lra=4.25, momentary_max=-18.0, short_term_max=-19.0, peak=0.5, true_peak=0.53)
    def report_into(res, rep, target, ceiling=None):
        unit = bt.Request(ids=[1], loudness=target, true_peak=ceiling)
        bt.results_into([res], [unit], sub("waveform").Tail(rows=[None], report=[rep]))
        assert res.pop("audio") is None
    res = {}
    report_into(res, rep, -23.0, -1.0)
    assert res == {"loudness": -20.5, "gain": 0.75, "true_peak": 20 * math.log10(0.53), "lra": 4.25}
    res = {}
    report_into(res, rep, -23.0, None)                            # in a metered batch, a unit without a ceiling keeps today's keys
    assert res == {"loudness": -20.5, "gain": 0.75}
    res = {}
    report_into(res, (-20.5, 0.75), -23.0)
    assert res == {"loudness": -20.5, "gain": 0.75}
    report_into(res := {}, rep, None, None)
    assert res == {}
    p = inspect.signature(bt.waveforms_into).parameters
    assert "units" in p and not {"loudness", "true_peak", "sample_rates", "encodings", "dithers", "dither_keys"} & set(p)    # no per-field list to misplace
    res = [{"mel": None, "mel_length": 3}]
    bt.waveforms_into(res, None, None, None, True, [bt.Request(ids=[1, 2, 3], loudness=-23.0, true_peak=-1.0)])
    assert res == [{"mel": None, "mel_length": 3}]
    # the service: the ceiling reaches the batcher from every entry, and one without a target is refused before anything is submitted
    assert sv.checked_ceiling(None, None) is None and sv.checked_ceiling(-1, -23.0) == -1.0
    seen = []

    def run(batch):
        seen.extend(batch)
        return [{"audio": torch.zeros(5)} for _ in batch]

    q = bt.FrameBudgetBatcher(model=None, max_batch=8, max_tokens=4096, max_wait_ms=5.0, run_batch=run)
    svc = sv.SpeechService(q, phonemize=lambda text, lang: [1 + (ord(c) % 50) for c in text], loudness=-23, true_peak=-1)
    with q:
        svc.submit("with the service's").result(timeout=30)
        svc.levelled(-16, -2.0).submit("one request's own").result(timeout=30)
        svc.levelled(-16).submit("levelled, no ceiling").result(timeout=30)
        svc.submit_long("A long one. Of two.").result(timeout=30)
        svc.submit_long("A long one. Of two.", loudness=-19, true_peak=-3).result(timeout=30)
        svc.submit_long("A long one. Of two.", loudness=None).result(timeout=30)
        for bad, err in (("hot", TypeError), (0.5, ValueError)):
            with pytest.raises(err):
                svc.levelled(-16, bad)
            with pytest.raises(err):
                svc.submit_long("never submitted", true_peak=bad)
        with pytest.raises(ValueError, match="target"):
            svc.levelled(None, -1.0)
        with pytest.raises(ValueError, match="target"):
            svc.submit_long("never submitted", loudness=None, true_peak=-1.0)
    assert [(u.loudness, u.true_peak) for u in seen] == [(-23.0, -1.0), (-16.0, -2.0), (-16.0, None), (-23.0, -1.0), (-19.0, -3.0), (None, None)]
    with pytest.raises(ValueError, match="target"):
        sv.SpeechService(None, None, true_peak=-1.0)

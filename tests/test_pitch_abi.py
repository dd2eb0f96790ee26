"""Pitch (include/mtts.h "pitch") without a GPU: the entries are declared, exported and bound; every refusal the host can see; the
frame-count formula; the NumPy restatement of tests/pitch_restated.py against independent code (energies and ``np.correlate``), on
steady tones (every frame within 1 cent of the truth) and, as its fp32 twin in the header's order of operations, against its own fp64
on the signals the GPU tests judge decisions on: no decidable frame differs and d' stays inside the derived budget."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sub
import pitch_restated as pr

LLVM = "/opt/rocm/lib/llvm/bin"
PKG = ROOT / "matcha-tts-24k_amd"


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def test_entries_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (arity and types of every prototype: test_abi.py checks them for the whole header)
    assert re.search(r"#define\s+MTTS_ABI_VERSION\s+2\b", header) and lib.mtts_abi_version() == 2       # entries were only added
    assert re.search(r"#define\s+MTTS_PITCH_MAX_LAG\s+1024\b", header) and pr.MAX_LAG == sub("pitch").MAX_LAG == 1024
    assert "pitch.hip" in sub("_hip").SOURCES
    for name in ("mtts_pitch_tile", "mtts_pitch_plan", "mtts_pitch_workspace_bytes", "mtts_pitch_track", "mtts_pitch_stats", "mtts_pitch_status"):
        assert re.search(r"\b%s\s*\(" % name, header) and getattr(lib, name).argtypes is not None, name
    for word in ("de Cheveigne & Kawahara", "s = s + d * d", "v[g] = v[g] + v[g - o]", "(0.5f * (a - c)) / ((a - b) + (c - b))",
                 "(k H + (W + tmax) / 2) / fs", "v[(m - 1) / 20]"):
        assert word in header, word
    assert lib.mtts_pitch_tile() == 8


def test_python_signatures():
    pitch, corpus, inf = sub("pitch"), sub("corpus"), sub("inference")
    p = inspect.signature(pitch.track).parameters
    assert list(p) == ["audio", "lengths", "sample_rate", "hop", "fmin", "fmax", "threshold", "check"]
    assert [p[k].default for k in list(p)[1:]] == [None, 24000, None, 60.0, 500.0, 0.15, True]
    assert list(inspect.signature(pitch.frame_times).parameters) == ["n", "hop", "window", "max_lag", "sample_rate"]
    p = inspect.signature(pitch.stats).parameters
    assert list(p) == ["f0", "frames", "hop", "sample_rate", "tail"] and p["tail"].default == 0.25
    assert list(inspect.signature(corpus.measure_pitch).parameters)[:3] == ["audio", "lengths", "sample_rate"]
    assert list(inspect.signature(inf.MatchaTTSInfer.speaker_delta).parameters) == ["self", "plus", "minus"]
    assert "speaker_embeddings=(e_enc + alpha * delta_enc, e_dur + alpha * delta_dur)" in inf.MatchaTTSInfer.speaker_delta.__doc__
    assert pitch.default_hop(24000) == 128 and pitch.default_hop(8000) == 43 and pitch.default_hop(48000) == 256 and pitch.default_hop(22050) == 118


def test_plan_and_frame_count(lib):
    pitch = sub("pitch")
    assert pitch.plan() == (128, 1024, 48, 400) and pitch.plan(8000, 16, 100.0) == (16, 128, 16, 80)
    assert pitch.plan(8000, 40) == (40, 320, 16, 134) and pitch.plan(44100, None, 55.0, 880.0) == (235, 1880, 50, 802)
    for fs, hop, fmin, fmax in ((24000, 128, 60.0, 500.0), (8000, 16, 100.0, 500.0), (48000, 512, 47.0, 1000.0), (22050, 118, 60.0, 500.0)):
        assert pitch.plan(fs, hop, fmin, fmax)[1:] == pr.plan(fs, hop, fmin, fmax)
    assert pitch.plan(48000)[3] == 800
    with pytest.raises(ValueError, match="max_lag <= 1024"):
        pitch.plan(48000, None, 40.0)                            # 48000 / 40 = 1200 lags
    for hop, W, tmax in ((128, 1024, 400), (16, 128, 80)):
        need = W + tmax
        for L, want in ((0, 0), (need - 1, 0), (need, 1), (need + hop - 1, 1), (need + hop, 2), (need + 7 * hop + 3, 8)):
            assert pitch.n_frames(L, hop, W, tmax) == pr.n_frames(L, hop, tmax) == want, (hop, L)
    t = pitch.frame_times(3, 128, 1024, 400, 24000)
    assert t.dtype.is_floating_point and t.tolist() == [712 / 24000, 840 / 24000, 968 / 24000]
    assert np.array_equal(t.numpy(), pr.frame_times(3, 128, 400, 24000))


def test_track_refuses_what_the_host_can_see(lib):
    # d_audio, ld, d_lengths, B, fs, hop, fmin, fmax, thr, d_f0, d_aper, ld_frames, d_frames, d_ws, ws_bytes, stream: never launched
    ok = [0x10000, 4096, 0x20000, 2, 24000, 128, 60.0, 500.0, 0.15, 0x30000, 0x40000, 21, 0x50000, 0x60000, 1 << 24, None]
    need = lib.mtts_pitch_workspace_bytes(4096, 2, 24000, 128, 60.0, 500.0)
    assert need >= 256 + 2 * (21 + 7) * 400 * 4 + 2 * (21 + 7) * 4 and need < (1 << 24)

    def refused(i, value, word):
        bad = list(ok)
        bad[i] = value
        assert lib.mtts_pitch_track(*bad) == -1 and word in lib.mtts_last_error(), (i, value, lib.mtts_last_error())

    for i in (0, 2, 9, 10, 12, 13):
        refused(i, None, b"null")
    for b in (0, -3, 70000):
        refused(3, b, b"B must")
    for ld in (4094, 0, -4):
        refused(1, ld, b"16-byte aligned")
    refused(0, 0x10004, b"16-byte aligned")
    for hop in (7, 513):
        refused(5, hop, b"hop must lie in [8, 512]")
    for fs in (7999, 48001):
        refused(4, fs, b"sample_rate must lie in [8000, 48000]")
    refused(7, 12001.0, b"2 <= min_lag")                           # floor(24000 / 12001) = 1
    refused(6, 23.43, b"max_lag <= 1024")                          # ceil(24000 / 23.43) = 1025
    assert int(np.ceil(24000 / 23.43)) == 1025 and int(np.ceil(24000 / 23.4375)) == 1024
    assert sub("pitch").plan(24000, 128, 23.4375)[3] == 1024       # (1024 itself is inside the contract)
    assert sub("pitch").plan(24000, 128, 480.0)[2:] == (48, 50)
    refused(6, 490.0, b"min_lag + 2 <= max_lag")                   # lags [48, 50] are fine; ceil(24000 / 490) = 49 is not
    for v in (0.0, -1.0, float("nan")):
        refused(6, v, b"positive and finite")
        refused(7, v, b"positive and finite")
    for thr in (0.0, 1.0, -0.1, 1.5, float("nan")):
        refused(8, thr, b"threshold must lie in (0, 1)")
    assert pr.n_frames(4096, 128, 400) == 21
    refused(11, 20, b"ld_frames")
    refused(11, 0, b"ld_frames")
    refused(14, need - 257, b"workspace too small")                # the slack of 256 bytes is not counted on
    refused(14, 16, b"workspace too small")
    assert lib.mtts_pitch_workspace_bytes(0, 2, 24000, 128, 60.0, 500.0) == -1 and lib.mtts_pitch_workspace_bytes(4096, 0, 24000, 128, 60.0, 500.0) == -1
    assert lib.mtts_pitch_workspace_bytes(4096, 2, 24000, 7, 60.0, 500.0) == -1 and b"hop" in lib.mtts_last_error()
    assert lib.mtts_pitch_status(None, None) == -1 and b"null" in lib.mtts_last_error()
    w = ctypes.c_int()
    assert lib.mtts_pitch_plan(24000, 128, 60.0, 500.0, ctypes.byref(w), None, None) == 0 and w.value == 1024
    assert lib.mtts_pitch_plan(7999, 128, 60.0, 500.0, None, None, None) == -1


def test_stats_refuses_what_the_host_can_see(lib):
    ok = [0x10000, 21, 0x20000, 2, 47, 0x30000, 0x40000, 0x50000, 256, None]
    for i in (0, 2, 5, 6, 7):
        bad = list(ok); bad[i] = None
        assert lib.mtts_pitch_stats(*bad) == -1 and b"null" in lib.mtts_last_error()
    for b in (0, 70000):
        bad = list(ok); bad[3] = b
        assert lib.mtts_pitch_stats(*bad) == -1 and b"B must" in lib.mtts_last_error()
    bad = list(ok); bad[1] = 0
    assert lib.mtts_pitch_stats(*bad) == -1 and b"ld_frames" in lib.mtts_last_error()
    bad = list(ok); bad[4] = -1
    assert lib.mtts_pitch_stats(*bad) == -1 and b"tail_frames" in lib.mtts_last_error()
    bad = list(ok); bad[8] = 255
    assert lib.mtts_pitch_stats(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()
    bad = list(ok); bad[7] = 0x50004
    assert lib.mtts_pitch_stats(*bad) == -1 and b"misaligned" in lib.mtts_last_error()


def test_python_refuses_before_a_device_is_touched(lib):
    import torch
    pitch = sub("pitch")
    for kw, word in ((dict(hop=7), "hop must lie"), (dict(sample_rate=7999), "sample_rate must lie"), (dict(fmax=12001.0), "min_lag"),
                     (dict(fmin=23.43), "max_lag"), (dict(threshold=1.0), "threshold"), (dict(threshold=0.0), "threshold")):
        with pytest.raises(ValueError, match=word):
            pitch.track([torch.zeros(4000)], **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pitch.stats(torch.zeros(2, 5), [5, 5], 128, 24000)
    with pytest.raises(ValueError, match=r"f0 must be \[B, T\]"):
        pitch.stats(torch.zeros(5), [5], 128, 24000)


def test_kernels_are_in_the_gfx950_code_object_without_scratch(tmp_path):
    sub("_hip").build()
    obj = PKG / "build" / "pitch.o"
    assert obj.exists(), obj
    fat, co = tmp_path / "pitch.fat", tmp_path / "pitch.co"
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, flags=re.M)
        scratch = re.search(r"^    \.private_segment_fixed_size:\s+(\d+)", block, flags=re.M)
        if name and scratch:
            meta[name.group(1)] = int(scratch.group(1))
    for kernel in ("pitch_block_kernel", "pitch_frame_kernel", "pitch_stats_kernel"):
        hits = [k for k in meta if kernel in k]
        assert len(hits) == 1 and meta[hits[0]] == 0, (kernel, meta)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_difference_function_against_correlation():
    """Validates the restatement (the tests' yardstick), not the library: block sums added up against energies - 2 x correlation.
    Both are fp64 sums of W = 8 H terms of magnitude <= 4 max(x^2): the difference of the two orders is bounded by
    (W + tmax) 2^-52 x (sum of the magnitudes) <= 3 (W + tmax) 2^-52 x 2 E, E the frame's largest windowed energy."""
    rng = np.random.default_rng(5)
    for fs, hop, fmin, L in ((8000, 16, 100.0, 700), (24000, 128, 60.0, 3000), (16000, 37, 80.0, 1500)):
        x = rng.uniform(-1, 1, L).astype(np.float32)
        _, _, tmax = pr.plan(fs, hop, fmin, 500.0)
        n = pr.n_frames(L, hop, tmax)
        assert n >= 3
        got = pr.frame_sums(pr.block_sums(x, hop, tmax, n + 7, False), n)
        want = pr.difference_by_correlation(x, fs, hop, fmin)
        energy = np.convolve(x.astype(np.float64) ** 2, np.ones(8 * hop), mode="valid").max()
        assert got.shape == want.shape == (n, tmax)
        assert np.abs(got - want).max() <= 6 * (8 * hop + tmax) * 2.0 ** -52 * energy


@pytest.mark.parametrize("freq", [70.3, 110.0, 147.7, 220.5, 333.3, 440.0])
def test_steady_tones_within_one_cent(freq):
    """Two-harmonic steady tones of 0.12 s at 24 kHz with the defaults: every frame voiced and within 1 cent of the truth, in fp64 and
    in the fp32 twin.  (Measured when written: at most 0.19 cents, at 333.3 Hz.)"""
    x = pr.tone(freq)
    for twin in (False, True):
        r = pr.analyse(x, 24000, 128, twin=twin)
        assert r["n"] == 12 and r["voiced"].all()
        cents = 1200.0 * np.log2(r["f0"].astype(np.float64) / freq)
        print(f"{freq} Hz twin={twin}: worst {np.abs(cents).max():.4f} cents")
        assert np.abs(cents).max() <= 1.0
        assert np.all(np.abs(r["lag"] - 24000 / freq) <= 1.0) and np.all(r["aperiodicity"] < 0.15)


def test_walk_rules_on_handmade_curves():
    thr, zero = 0.15, np.zeros(12)
    dp = np.array([1, 1, 0.9, 0.5, 0.14, 0.10, 0.08, 0.09, 0.01, 0.5, 0.6, 0.7])       # tau = 1 .. 12
    assert pr.walk(dp, 2, 12, thr, zero)[:2] == (7, True)         # first below at 5, descends to 7, stops although 9 is lower
    assert pr.walk(dp, 8, 12, thr, zero)[:2] == (9, True)
    assert pr.walk(dp, 10, 12, thr, zero)[:2] == (10, False)      # none below: the minimum of [10, 12)
    flat = np.full(12, 0.3)
    assert pr.walk(flat, 2, 12, thr, zero)[:2] == (2, False)      # ties: the lowest index
    down = np.linspace(0.14, 0.01, 12)
    assert pr.walk(down, 2, 12, thr, zero)[:2] == (11, True)      # the descent stays below tmax
    star, voiced, margin = pr.walk(dp, 2, 12, thr, 0.02 * dp)
    assert (star, voiced) == (7, True) and margin == pytest.approx(0.09 - 0.08 - 0.02 * 0.17)   # the closest call: the step that ends the descent


def test_twin_agrees_with_fp64_on_the_decision_signals():
    """The fp32 twin in the header's order against fp64 on the glides: d' inside the derived budget at every lag of every frame, at
    most 2 % of a signal's frames undecidable, and no decidable frame with another lag or voicing; f0 inside its propagated budget."""
    total = 0
    for name, x, fs, hop in pr.decision_signals():
        a, b = pr.analysed(name), pr.analysed(name, True)
        n = a["n"]
        total += n
        assert n == b["n"] and n > 100
        err = np.abs(b["dprime"].astype(np.float64) - a["dprime"])
        print(f"{name}: {n} frames, {int(a['voiced'].sum())} voiced, worst |d' - fp64| {err.max():.3e} "
              f"(relative {np.max(err / a['dprime']):.3e}, budget {pr.rel_budget(hop):.3e}), undecidable {int((a['margin'] <= 0).sum())}")
        assert np.all(err <= pr.rel_budget(hop) * a["dprime"])
        decidable = a["margin"] > 0
        assert (~decidable).sum() <= 0.02 * n
        assert np.array_equal(a["lag"][decidable], b["lag"][decidable]) and np.array_equal(a["voiced"][decidable], b["voiced"][decidable])
        v = decidable & a["voiced"]
        assert v.sum() > 0.6 * n and (~a["voiced"]).sum() > 10                       # glide, gap and zeros are all there
        assert np.all(np.abs(b["f0"][v].astype(np.float64) - a["f0"][v]) <= a["f0_budget"][v])
        assert a["f0_budget"][v].max() < 0.01                                          # Hz: the budget is no blank cheque
    assert total > 500


def test_glides_are_tracked():
    """The yardstick follows the glides: voiced frames within 1 % of the instantaneous fundamental at the frame's centre."""
    for (f_from, f_to, seed), fs, hop in (((90.0, 250.0, 1), 24000, 128), ((220.0, 140.0, 2), 8000, 40)):
        x, f = pr.glide(f_from, f_to, fs, seed=seed)
        r = pr.analyse(x, fs, hop)
        t = pr.frame_times(r["n"], hop, r["max_lag"], fs)
        truth = f[np.round(t * fs).astype(int)]
        span = 8 * hop + r["max_lag"]
        inside = np.array([np.all(f[k * hop:k * hop + span] > 0) for k in range(r["n"])])     # frames wholly inside the voiced parts
        assert inside.sum() > 60 and r["voiced"][inside].all()
        assert np.all(np.abs(r["f0"][inside] / truth[inside] - 1.0) < 0.01)


def test_select_restatement():
    f0 = np.array([0, 100, 0, 300, 200, 0, 250, 150, 0, 0], dtype=np.float32)
    out, counts = pr.select(f0, 10, 3)
    assert counts == (10, 5, 3) and out.tolist() == [100.0, 200.0, 250.0, 200.0]      # tail: indices >= 7 - 3 -> 200, 250, 150
    out, counts = pr.select(f0, 10, 0)
    assert counts == (10, 5, 1) and np.isnan(out[3]) and out[1] == 200.0
    out, counts = pr.select(f0, 1, 3)
    assert counts == (1, 0, 0) and np.isnan(out).all()
    assert pr.select(f0, 11, 3)[1] == (-1, 0, 0) and pr.select(f0, -1, 3)[1] == (-1, 0, 0)
    v = np.arange(1, 42, dtype=np.float32)
    assert pr.select(v, 41, 100)[0].tolist() == [3.0, 21.0, 39.0, 21.0]               # ranks 40 // 20, 40 // 2, 19 * 40 // 20


def test_pitch_table_layout():
    import importlib.util
    spec = importlib.util.spec_from_file_location("prepare_corpus_pitch", ROOT / "tools" / "prepare_corpus.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = [("0", 183.25, 7.5, 2.25, True), ("0", 170.0, 6.5, -0.75, False), ("1", 110.0, 5.0, float("nan"), True), ("1", 120.0, 4.0, 0.5, False)]
    table = tool.pitch_table(rows).split("\n")
    assert table[0].startswith("Pitch per speaker") and table[1] == "=" * tool.RULE and table[3] == "-" * tool.RULE
    assert table[2].split() == ["Speaker", "Count", "Median", "Hz", "Range", "st", "Rise", "?", "st", "Rise", "rest", "st", "Difference", "st"]
    assert table[4].split() == ["0", "2", "176.6", "7.00", "2.25", "-0.75", "3.00"]
    assert table[5].split() == ["1", "2", "115.0", "4.50", "nan", "0.50", "nan"]

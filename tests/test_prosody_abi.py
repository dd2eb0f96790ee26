"""Prosody (include/mtts.h "prosody") without a GPU: the entries are declared, exported and bound and the Python signatures; every
refusal the host can see; the NumPy restatement of tests/prosody_restated.py against independent code -- its shortest path against
brute force over all paths, its fold against ``np.sort`` / ``np.sum`` --; ``pitch.compare`` on hand-made contours; and the three
signal conditions of the feature (an octave excursion smoothed, a genuine octave step kept, voicing unchanged) on the fp32 twin."""
import inspect
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import pitch_restated as pr
import prosody_restated as ps

LLVM = "/opt/rocm/lib/llvm/bin"
PKG = ROOT / "matcha-tts-24k_amd"
ENTRIES = ("mtts_pitch_candidates", "mtts_pitch_viterbi_workspace_bytes", "mtts_pitch_viterbi", "mtts_pitch_fold")


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def test_entries_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    assert re.search(r"#define\s+MTTS_ABI_VERSION\s+2\b", header) and lib.mtts_abi_version() == 2       # entries were only added
    assert re.search(r"#define\s+MTTS_PITCH_CANDS\s+8\b", header) and ps.CANDS == sub("pitch").CANDS == 8 and sub("pitch").UNVOICED == ps.U == 8
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header) and getattr(lib, name).argtypes is not None, name
    for word in ("d'(tau) < d'(tau - 1)", "F(v) = min(max(v / thr2, 0), 1)", "exactly 1.0f", "fabsf(p_s - p_r) / fminf(p_s, p_r)",
                 "the lowest index wins a tie", "D_k(s) - min_s D_k(s)", "2 start_i <= 2 k H + W + tmax < 2 end_i", "v[(m - 1) / 2]",
                 "v[l] = v[l] + v[l ^ o]"):
        assert word in header, word


def test_python_signatures():
    pitch, corpus, inf = sub("pitch"), sub("corpus"), sub("inference")
    track = list(inspect.signature(pitch.track).parameters)
    for fn in (pitch.candidates, pitch.track_viterbi):
        assert list(inspect.signature(fn).parameters)[:len(track)] == track          # the arguments of track, in its order
    p = inspect.signature(pitch.track_viterbi).parameters
    assert list(p)[len(track):] == ["jump", "switch"] and (p["jump"].default, p["switch"].default) == (2.0, 0.5)
    p = inspect.signature(pitch.viterbi).parameters
    assert list(p)[:3] == ["lattice", "jump", "switch"] and (p["jump"].default, p["switch"].default) == (2.0, 0.5)
    assert "real speech" in pitch.viterbi.__doc__
    p = inspect.signature(pitch.fold).parameters
    assert list(p)[:5] == ["tracked", "marks", "x_lengths", "audio", "lengths"] and p["audio"].default is None and p["lengths"].default is None
    assert list(inspect.signature(pitch.compare).parameters)[:2] == ["a", "b"]
    p = inspect.signature(pitch.contour).parameters
    assert p["method"].default == "yin" and set(pitch.METHODS) == {"yin", "viterbi"} and pitch.METHODS["yin"] is pitch.track
    p = inspect.signature(inf.MatchaTTSInfer.prosody).parameters
    assert list(p)[:4] == ["self", "x", "x_lengths", "audio"] and "sample_rate" in p and "silence" in p
    assert "method" in corpus.measure_pitch.__doc__
    with pytest.raises(ValueError, match="method must be one of"):
        pitch.contour([torch.zeros(4000)], method="pyin")
    with pytest.raises(ValueError, match="method must be one of"):
        corpus.measure_pitch([torch.zeros(4000)], method="pyin")


def refuser(fn, ok, lib):
    def refused(i, value, word):
        bad = list(ok)
        bad[i] = value
        assert fn(*bad) == -1 and word in lib.mtts_last_error(), (i, value, lib.mtts_last_error())
    return refused


def test_candidates_refuses_what_the_host_can_see(lib):
    # d_audio, ld, d_lengths, B, fs, hop, fmin, fmax, thr, period, mass, depth, count, unvoiced, floor, ld_frames, d_frames, ws, bytes, stream
    ok = [0x10000, 4096, 0x20000, 2, 24000, 128, 60.0, 500.0, 0.15, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 21, 0x90000,
          0xa0000, 1 << 24, None]
    refused = refuser(lib.mtts_pitch_candidates, ok, lib)
    need = lib.mtts_pitch_workspace_bytes(4096, 2, 24000, 128, 60.0, 500.0)
    for i in (0, 2, 9, 10, 11, 12, 13, 14, 16, 17):
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
    refused(7, 12001.0, b"2 <= min_lag")
    refused(6, 23.43, b"max_lag <= 1024")
    for thr in (0.0, 1.0, float("nan")):
        refused(8, thr, b"threshold must lie in (0, 1)")
    refused(15, 20, b"ld_frames")
    refused(18, need - 257, b"workspace too small")


def test_viterbi_refuses_what_the_host_can_see(lib):
    # period, mass, depth, count, unvoiced, floor, ld_frames, d_frames, B, fs, jump, switch, f0, aper, state, ws, bytes, stream
    ok = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 130, 0x70000, 3, 24000, 2.0, 0.5, 0x80000, 0x90000, 0xa0000, 0xb0000, 1 << 20, None]
    refused = refuser(lib.mtts_pitch_viterbi, ok, lib)
    need = lib.mtts_pitch_viterbi_workspace_bytes(130, 3)
    assert need >= 256 + 3 * 130 * 8 and need < (1 << 20)
    for i in (0, 1, 2, 3, 4, 5, 7, 12, 13, 14, 15):
        refused(i, None, b"null")
    for b in (0, 70000):
        refused(8, b, b"B must")
    for n in (0, -1, 1 << 30):
        refused(6, n, b"ld_frames")
    for fs in (7999, 48001):
        refused(9, fs, b"sample_rate")
    for i in (10, 11):
        for v in (-0.5, float("nan"), float("inf"), 2e6):
            refused(i, v, b"jump and switch must lie in [0, 1e6]")
    refused(15, 0xb0004, b"misaligned")
    refused(16, 256 + 3 * 130 * 8 - 1, b"workspace too small")
    assert lib.mtts_pitch_viterbi_workspace_bytes(0, 3) == -1 and lib.mtts_pitch_viterbi_workspace_bytes(130, 0) == -1


def test_fold_refuses_what_the_host_can_see(lib):
    # f0, ld_frames, d_frames, B, hop, window, max_lag, marks, Tx, x_lengths, audio, ld, lengths, counts, hz, mean_square, ws, bytes, stream
    ok = [0x10000, 130, 0x20000, 3, 128, 1024, 400, 0x30000, 12, 0x40000, 0x50000, 20000, 0x60000, 0x70000, 0x80000, 0x90000, 0xa0000, 256, None]
    refused = refuser(lib.mtts_pitch_fold, ok, lib)
    for i in (0, 2, 7, 9, 13, 14, 16):
        refused(i, None, b"null")
    for b in (0, 70000):
        refused(3, b, b"B must")
    for tx in (0, -1, (1 << 20) + 1):
        refused(8, tx, b"Tx must")
    for n in (0, 1 << 30):
        refused(1, n, b"ld_frames")
    refused(4, 7, b"a plan of mtts_pitch_plan")
    refused(5, 1000, b"a plan of mtts_pitch_plan")
    refused(6, 1025, b"a plan of mtts_pitch_plan")
    refused(10, None, b"go together")                              # a mean square without audio
    refused(15, None, b"go together")                              # audio without a place for the mean square
    refused(12, None, b"audio needs its lengths")
    refused(11, 0, b"audio needs its lengths")
    refused(16, 0xa0004, b"misaligned")
    refused(17, 255, b"workspace too small")


def test_python_refuses_before_a_device_is_touched(lib):
    pitch = sub("pitch")
    for fn in (pitch.candidates, pitch.track_viterbi):
        for kw, word in ((dict(hop=7), "hop must lie"), (dict(fmax=12001.0), "min_lag"), (dict(threshold=1.0), "threshold")):
            with pytest.raises(ValueError, match=word):
                fn([torch.zeros(4000)], **kw)
    lat = {"period": torch.zeros(1, 3, 8), "sample_rate": 24000}
    with pytest.raises(RuntimeError, match="no CPU path"):
        pitch.viterbi(lat)
    with pytest.raises(ValueError, match="jump and switch"):
        pitch.viterbi(lat, jump=-1.0)
    with pytest.raises(ValueError, match=r"must be \[B, T, 8\]"):
        pitch.viterbi({"period": torch.zeros(1, 3, 4), "sample_rate": 24000})
    with pytest.raises(RuntimeError, match="no CPU path"):
        pitch.fold({"f0": torch.zeros(1, 3)}, torch.zeros(1, 2, 2), [2])
    with pytest.raises(ValueError, match=r"f0'\] must be \[B, T\]"):
        pitch.fold({"f0": torch.zeros(3)}, torch.zeros(1, 2, 2), [2])


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
    for kernel in ("pitch_cand_kernel", "pitch_viterbi_kernel", "pitch_fold_kernel"):
        hits = [k for k in meta if kernel in k]
        assert len(hits) == 1 and meta[hits[0]] == 0, (kernel, meta)


# ------------------------------------------------------------------------------------------------ the restatement itself
def random_lattice(rng, T, max_states, ties=False):
    """A lattice of T frames with 0 .. max_states - 1 candidates each, a few bad frames; with ``ties`` every number is a small
    dyadic rational, so equal path costs are exactly equal in fp32 and fp64 alike."""
    lat = {"period": np.zeros((T, 8), np.float32), "mass": np.zeros((T, 8), np.float32), "depth": np.zeros((T, 8), np.float32),
           "count": np.zeros(T, np.int32), "unvoiced_mass": np.ones(T, np.float32), "floor": np.ones(T, np.float32)}
    for k in range(T):
        c = int(rng.integers(0, max_states))
        lat["count"][k] = -1 if rng.random() < 0.1 else c
        if ties:
            lat["period"][k, :c] = np.sort(rng.choice([64.0, 128.0, 256.0], size=c))
            lat["mass"][k, :c] = rng.integers(0, 5, size=c) / 8.0
            lat["unvoiced_mass"][k] = rng.integers(0, 5) / 8.0
        else:
            lat["period"][k, :c] = np.sort(rng.uniform(50.0, 400.0, size=c))
            m = rng.dirichlet(np.ones(c + 1))
            lat["mass"][k, :c], lat["unvoiced_mass"][k] = m[:c], m[c]
        lat["depth"][k, :c] = rng.uniform(0.0, 0.3, size=c)
        lat["floor"][k] = rng.uniform(0.3, 1.0)
    return lat


def test_restated_viterbi_against_brute_force():
    """Random lattices of up to 6 frames x 4 states (3 candidates and U): the restated path, fp64 and fp32 twin, is one of the
    cheapest of all paths; where the cheapest is unique by more than 1e-4 it is that one."""
    rng = np.random.default_rng(11)
    unique = 0
    for trial in range(150):
        T = int(rng.integers(1, 7))
        lat = random_lattice(rng, T, 4)
        jump, switch = float(rng.choice([1.0, 2.0, 4.0])), float(rng.choice([0.25, 0.5, 1.0]))
        best, paths = ps.brute_force(lat, T, jump, switch)
        for twin in (False, True):
            state, f0, ap = ps.viterbi(lat, T, 24000, jump, switch, twin=twin)
            cost = ps.path_cost(lat, T, [int(s) for s in state], jump, switch)
            assert cost <= best + (1e-4 if twin else 1e-9), (trial, twin, cost, best)
            assert np.all((f0 > 0) == (state < 8))
        if len(paths) == 1:
            second = min(ps.path_cost(lat, T, p, jump, switch) for p in _neighbours(lat, T, paths[0]))
            if second - best > 1e-4:
                unique += 1
                assert tuple(int(s) for s in ps.viterbi(lat, T, 24000, jump, switch, twin=True)[0]) == paths[0]
    assert unique > 50


def _neighbours(lat, T, path):
    out = []
    for k in range(T):
        for s in ps._states(lat["count"][k]):
            if s != path[k]:
                out.append(path[:k] + (s,) + path[k + 1:])
    return out or [path]


def test_restated_viterbi_breaks_exact_ties_by_the_lowest_index():
    """Dyadic lattices: equal costs are exactly equal.  Among the cheapest paths the restatement returns the one the header's rules
    pick: the lowest end state, and walking back the lowest predecessor at every tie."""
    rng = np.random.default_rng(12)
    tied = 0
    for trial in range(600):
        T = int(rng.integers(2, 6))
        lat = random_lattice(rng, T, 4, ties=True)
        best, paths = ps.brute_force(lat, T, 2.0, 0.5)
        state = tuple(int(s) for s in ps.viterbi(lat, T, 24000, 2.0, 0.5, twin=True)[0])
        assert state in paths, (trial, state, paths)
        if len(paths) > 1:
            tied += 1
            # the header's choice among them: lowest last state, then lowest predecessor from the back
            want = sorted(paths, key=lambda p: tuple(reversed(p)))[0]
            assert state == want, (trial, state, want)
    assert tied > 20


def test_greedy_is_not_the_path():
    """A lattice on which the frame-by-frame cheapest state is not the cheapest path."""
    lat = handmade_octave_lattice()
    greedy = [int(np.argmin([1 - lat["mass"][k, 0], 1 - lat["mass"][k, 1]])) for k in range(5)]
    state = ps.viterbi(lat, 5, 24000, 2.0, 0.5)[0]
    assert greedy == [1, 1, 0, 1, 1] and state.tolist() == [1, 1, 1, 1, 1]
    assert ps.brute_force(lat, 5, 2.0, 0.5)[1] == [(1, 1, 1, 1, 1)]
    assert ps.viterbi(lat, 5, 24000, 0.0, 0.5)[0].tolist() == greedy          # without a jump cost the path is the greedy one


def handmade_octave_lattice():
    lat = {"period": np.zeros((5, 8), np.float32), "mass": np.zeros((5, 8), np.float32), "depth": np.zeros((5, 8), np.float32),
           "count": np.full(5, 2, np.int32), "unvoiced_mass": np.full(5, 0.05, np.float32), "floor": np.full(5, 0.5, np.float32)}
    lat["period"][:, 0], lat["period"][:, 1] = 80.0, 160.0
    lat["mass"][:, 0], lat["mass"][:, 1] = 0.15, 0.8
    lat["mass"][2, 0], lat["mass"][2, 1] = 0.6, 0.35                # the middle frame prefers the octave above
    lat["depth"][:, 0], lat["depth"][:, 1] = 0.2, 0.02
    return lat


def test_restated_fold_against_sort_and_sum():
    rng = np.random.default_rng(13)
    H, W, tmax = 128, 1024, 400
    L = 30000
    n = pr.n_frames(L, H, tmax)
    f0 = np.where(rng.random(n) < 0.7, rng.uniform(80, 300, n), 0.0).astype(np.float32)
    x = rng.standard_normal(L).astype(np.float32)
    cuts = np.sort(rng.choice(np.arange(0, L + 1), size=9, replace=False))
    marks = np.stack([cuts[:-1], cuts[1:]], 1)
    marks[3] = (-1, -1)
    counts, hz, ms, why = ps.fold(f0, n, H, W, tmax, marks, 8, audio=x, length=L)
    assert why == 0
    centre = (2 * np.arange(n) * H + W + tmax)
    total = 0
    for i, (st, en) in enumerate(marks):
        if st < 0:
            assert counts[i].tolist() == [0, 0] and np.isnan(hz[i]).all() and ms[i] == 0
            continue
        inside = (centre >= 2 * st) & (centre < 2 * en)
        v = f0[inside][f0[inside] > 0]
        total += int(inside.sum())
        assert counts[i].tolist() == [int(inside.sum()), v.size]
        if v.size:
            assert hz[i].tolist() == [np.sort(v)[(v.size - 1) // 2], v[0], v[-1]]
        m = en - st
        want = np.sum(x[st:en].astype(np.float64) ** 2)
        g = m * 2.0 ** -53 / (1 - m * 2.0 ** -53)
        assert abs(ms[i] * m - want) <= g * want + 2.0 ** -52 * want      # (+ the division's own rounding)
    lo, hi = marks[0][0], marks[-1][1]
    gap = int(((centre >= 2 * marks[2][1]) & (centre < 2 * marks[4][0])).sum())
    assert total == int(((centre >= 2 * lo) & (centre < 2 * hi)).sum()) - gap
    # the frame range by two divisions: a boundary exactly on a frame centre belongs to the token that starts there
    c5 = (5 * 2 * H + W + tmax) // 2
    assert ps.first_frame(c5, H, W, tmax, n) == 5 and ps.first_frame(c5 + 1, H, W, tmax, n) == 6 and ps.first_frame(c5 - 1, H, W, tmax, n) == 5
    assert ps.first_frame(0, H, W, tmax, n) == 0 and ps.first_frame(L, H, W, tmax, n) == n
    # refusals
    for bad, why in (((5, 4), 5), ((-3, 10), 4), ((10, L + 1), 4)):
        m2 = marks.copy()
        m2[0] = bad
        assert ps.fold(f0, n, H, W, tmax, m2, 8, audio=x, length=L)[3] == why
    m2 = marks.copy()
    m2[2] = (marks[1][1] - 1, marks[2][1])
    assert ps.fold(f0, n, H, W, tmax, m2, 8, audio=x, length=L)[3] == 6
    assert ps.fold(f0, -1, H, W, tmax, marks, 8, audio=x, length=L)[3] == 1
    assert ps.fold(f0, n, H, W, tmax, marks, 9, audio=x, length=L)[3] == 2
    x2 = x.copy()
    x2[marks[1][0]] = np.inf
    assert np.isnan(ps.fold(f0, n, H, W, tmax, marks, 8, audio=x2, length=L)[2][1])


def test_compare_on_handmade_contours():
    pitch = sub("pitch")
    a = torch.tensor([[100.0, 100.0, 0.0, 200.0, 0.0, 150.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    b = torch.tensor([[100.0, 200.0, 0.0, 100.0, 120.0, 150.0], [0.0, 110.0, 0.0, 0.0, 0.0, 0.0]])
    got = pitch.compare(a, b)
    assert got["frames"].tolist() == [6, 6] and got["both_voiced"].tolist() == [4, 0]
    # row 0, voiced in both: 0, -1200, +1200, 0 cents
    assert got["rmse_cents"][0].item() == pytest.approx(math.sqrt(2 * 1200.0 ** 2 / 4))
    assert got["gross_error"][0].item() == 0.5 and got["voicing_error"][0].item() == pytest.approx(1 / 6)
    la, lb = np.log2([100.0, 100.0, 200.0, 150.0]), np.log2([100.0, 200.0, 100.0, 150.0])
    assert got["corr"][0].item() == pytest.approx(np.corrcoef(la, lb)[0, 1])
    assert math.isnan(got["rmse_cents"][1].item()) and math.isnan(got["corr"][1].item()) and math.isnan(got["gross_error"][1].item())
    assert got["voicing_error"][1].item() == pytest.approx(1 / 6)
    same = pitch.compare(a[0], a[0] * 1.01)
    assert same["rmse_cents"][0].item() == pytest.approx(1200 * math.log2(1.01)) and same["corr"][0].item() == pytest.approx(1.0)
    assert same["gross_error"][0].item() == 0.0 and same["voicing_error"][0].item() == 0.0
    short = pitch.compare(a, b, frames=[1, 0])
    assert short["both_voiced"].tolist() == [1, 0] and short["rmse_cents"][0].item() == 0.0 and math.isnan(short["voicing_error"][1].item())
    with pytest.raises(ValueError, match="one shape"):
        pitch.compare(a, b[:, :3])


def test_restated_limit_holds_the_eight_of_greatest_mass():
    """Signals that keep more dips than the lattice holds (threshold 0.95): the twin holds the 8 of greatest mass in ascending lag."""
    W, tmin, tmax = pr.plan(24000, 128, 60.0, 500.0)
    most = 0
    for amp, period in ((0.1, 8.3), (0.5, 11.7)):
        x = ps.ripple(amp, period)
        n = pr.n_frames(x.size, 128, tmax)
        dp = pr.dprime(pr.frame_sums(pr.block_sums(x, 128, tmax, n + 7, True), n), True)
        lat = ps.candidates(x, 24000, 128, thr=0.95, twin=True)
        for k in range(n):
            kept, unvoiced = ps.record_dips(dp[k], tmin, tmax, 0.95, True)
            most = max(most, len(kept))
            assert lat["count"][k] == min(len(kept), 8) and lat["unvoiced_mass"][k] == unvoiced
            masses = sorted((float(m) for _, m, _ in kept), reverse=True)
            assert sorted(lat["mass"][k, :lat["count"][k]].tolist(), reverse=True) == masses[:8]
            assert np.all(np.diff(lat["period"][k, :lat["count"][k]]) > 0)
            depths = [d for _, _, d in kept]
            assert all(b < a for a, b in zip(depths, depths[1:]))           # every kept dip set a record
    assert most > 16


# ------------------------------------------------------------------------------------------------ the three signals, on the twin
def counts_of(name, jump=2.0):
    _, x, f = next(s for s in ps.signals() if s[0] == name)
    yin, path = ps.analysed(name, jump, 0.5)
    truth = ps.truth_at_frames(f, yin["n"], yin["max_lag"])
    y = np.where(yin["voiced"], yin["f0"], 0.0)
    return y, path["f0"], truth, path


def test_dip60_is_smoothed_on_the_twin():
    y, p, truth, path = counts_of("dip60")
    print(f"dip60: {y.size} frames, YIN {ps.off_count(y, truth)} off and {int((y == 0).sum())} unvoiced, path {ps.off_count(p, truth)} off, "
          f"at most {int(path['lattice']['count'].max())} candidates")
    assert y.size == 121 and ps.off_count(y, truth) >= 1 and (y > 0).all()
    for jump in (2.0, 4.0, 8.0):
        assert ps.off_count(counts_of("dip60", jump)[1], truth) == 0, jump
    assert ps.off_count(counts_of("dip60", 1.0)[1], truth) >= 1       # too cheap a jump does not smooth the excursion


def test_step_is_kept_on_the_twin():
    y, p, truth, _ = counts_of("step")
    print(f"step: YIN {ps.off_count(y, truth)} off, {int((y == 0).sum())} unvoiced; path {ps.off_count(p, truth)} off, {int((p == 0).sum())} unvoiced")
    assert ps.off_count(p, truth) == ps.off_count(y, truth) == 0
    assert np.array_equal(p > 0, y > 0) and 0 < int((y == 0).sum()) < 20


def test_noise_tone_noise_voicing_on_the_twin():
    y, p, truth, _ = counts_of("noise_tone_noise")
    same = int(((p > 0) == (y > 0)).sum())
    print(f"noise, tone, noise: voicing equal on {same} of {y.size} frames, {int((y > 0).sum())} voiced")
    assert y.size == 158 and same == 158 and 40 < int((y > 0).sum()) < 100

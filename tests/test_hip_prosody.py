"""Prosody on the GPU (include/mtts.h "prosody"; csrc/pitch.hip) against the NumPy restatement of tests/prosody_restated.py, bit for
bit: the candidate lattice on the feature's three signals, the glides of the pitch tests and an odd hop, at the frame-count
boundaries, with non-finite samples and in any place of a batch; the shortest path on hand-made lattices that cross the staging
chunk, with ties, bad frames and refused rows; the end-to-end conditions that plain YIN fails (an octave excursion); the fold onto
token marks with every refusal; and the Python entries and tools.  Every figure is printed before it is asserted."""
import json
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import pitch_restated as pr
import prosody_restated as ps

pytestmark = pytest.mark.gpu
LATTICE = ("period", "mass", "depth", "count", "unvoiced_mass", "floor")


def words(a):
    """The 32-bit words of an array (NaN compares by its bits)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int8 if a.dtype.itemsize == 1 else np.int64)


@pytest.fixture(scope="module")
def pitch():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("pitch")


def padded(rows, extra=0):
    """Rows -> [B, ld] with NaN beyond every row's own length: a kernel that reads there shows it."""
    ld = max(4, (max(len(r) for r in rows) + extra + 3) // 4 * 4)
    x = np.full((len(rows), ld), np.nan, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).cuda()


def check_lattice(name, got, b, x, fs, hop, threshold=0.15, **kw):
    T = got["count"].shape[1]
    want = ps.candidates(x, fs, hop, thr=threshold, twin=True, T=T, **kw)
    assert int(got["frames"][b]) == want["n"], (name, int(got["frames"][b]), want["n"])
    for k in LATTICE:
        g, w = words(got[k][b]), words(want[k])
        assert np.array_equal(g, w), (name, k, np.argwhere(g != w)[:4].tolist())
    return want


# ------------------------------------------------------------------------------------------------ candidates
@pytest.mark.parametrize("case", ["three_24k", "glides_24k", "glides_8k", "odd_hop", "many_dips"])
def test_candidates_equal_the_twin(pitch, case):
    if case == "three_24k":
        rows, fs, hop, kw = [(n, x) for n, x, _ in ps.signals()], 24000, 128, {}
    elif case == "glides_24k":
        rows, fs, hop, kw = [(s[0], s[1]) for s in pr.decision_signals() if s[2] == 24000], 24000, 128, {}
    elif case == "glides_8k":
        rows, fs, hop, kw = [(s[0], s[1]) for s in pr.decision_signals() if s[2] == 8000], 8000, 40, {}
    elif case == "many_dips":                                     # more dips kept than the lattice holds: the 8 of greatest mass
        rows, fs, hop, kw = [("ripple_8.3", ps.ripple(0.1, 8.3)), ("ripple_11.7", ps.ripple(0.5, 11.7)), ("ripple_17.1", ps.ripple(0.3, 17.1))], 24000, 128, dict(threshold=0.95)
    else:
        rows, fs, hop, kw = [("up_odd", pr.glide(100.0, 260.0, 16000, seconds=0.5, seed=3)[0]), ("tone_odd", pr.tone(131.0, 16000, 0.3))], 16000, 37, dict(fmin=80.0)
    audio = padded([x for _, x in rows], extra=8)
    got = pitch.candidates(audio, [len(x) for _, x in rows], fs, hop, **kw)
    for b, (name, x) in enumerate(rows):
        want = check_lattice(name, got, b, x, fs, hop, **kw)
        c = want["count"][:want["n"]]
        print(f"{name}: {want['n']} frames, candidates per frame 0..{int(c.max())}, {int((c == 0).sum())} frames without one")
        assert want["n"] > (10 if case == "many_dips" else 20) and c.max() >= 1


def test_candidates_at_the_frame_count_boundaries(pitch):
    """fs 8000, hop 16, fmin 100: W = 128, tmax = 80.  L = W + tmax - 1, W + tmax, + H - 1, + H: 0, 1, 1, 2 frames; columns beyond hold
    the fill values; a refused row beside them."""
    fs, hop, fmin = 8000, 16, 100.0
    need = 128 + 80
    lengths = [need - 1, need, need + hop - 1, need + hop, need + 9 * hop + 5]
    rng = np.random.default_rng(4)
    t = np.arange(need + 12 * hop) / fs
    rows = [(0.4 * np.sin(2 * np.pi * (140 + 9 * i) * t[:L]) + 0.2 * np.sin(2 * np.pi * 2 * (140 + 9 * i) * t[:L] + 1) +
             0.004 * rng.standard_normal(L)).astype(np.float32) for i, L in enumerate(lengths)]
    audio = padded(rows, extra=40)
    got = pitch.candidates(audio, lengths, fs, hop, fmin)
    assert got["frames"].tolist() == [0, 1, 1, 2, 10]
    for b, x in enumerate(rows):
        check_lattice(f"L={lengths[b]}", got, b, x, fs, hop, fmin=fmin)
    refused = [lengths[0], audio.shape[1] + 1, -1, lengths[3], lengths[4]]
    bad = pitch.candidates(audio, refused, fs, hop, fmin, check=False)
    assert bad["frames"].tolist() == [0, -1, -1, 2, 10]
    for b in (1, 2):
        assert (bad["count"][b] == 0).all() and (bad["unvoiced_mass"][b] == 1).all() and (bad["floor"][b] == 1).all() and (bad["period"][b] == 0).all()
    for b in (0, 3, 4):
        for k in LATTICE:
            assert np.array_equal(words(bad[k][b]), words(got[k][b])), (b, k)
    with pytest.raises(ValueError, match="mtts_pitch_candidates: row 1 has length"):
        pitch.candidates(audio, refused, fs, hop, fmin)


def test_a_nan_sample_marks_exactly_the_frames_that_read_it(pitch):
    name, x, _ = ps.signals()[0]
    W, _, tmax = pr.plan(24000, 128, 60.0, 500.0)
    clean = pitch.candidates([torch.from_numpy(x)])
    for at, value in ((5000, np.nan), (0, np.inf), (120 * 128 + W + tmax - 1, -np.inf)):
        y = x.copy()
        y[at] = value
        got = pitch.candidates([torch.from_numpy(y)])
        n = int(got["frames"][0])
        reads = np.array([k * 128 <= at < k * 128 + W + tmax for k in range(n)])
        assert np.array_equal(got["count"][0, :n].cpu().numpy() == -1, reads), at
        check_lattice(f"{name}+{value}@{at}", got, 0, y, 24000, 128)
        for k in LATTICE:                                           # the other frames are unaffected
            assert np.array_equal(words(got[k][0, :n])[~reads], words(clean[k][0, :n])[~reads]), (at, k)


def test_a_row_alone_gives_the_bits_it_gives_in_a_batch(pitch):
    sigs = [x for _, x, _ in ps.signals()] + [s[1] for s in pr.decision_signals() if s[2] == 24000]
    alone = [pitch.candidates(padded([x]), [len(x)]) for x in sigs]
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3, 4, 1, 0, 2]):
        rows = [sigs[i] for i in order]
        got = pitch.candidates(padded(rows, extra=12), [len(r) for r in rows])
        for b, i in enumerate(order):
            n = int(alone[i]["frames"][0])
            assert int(got["frames"][b]) == n
            for k in LATTICE:
                assert np.array_equal(words(got[k][b, :n]), words(alone[i][k][0, :n])), (order, b, k)
            assert (got["count"][b, n:] == 0).all() and (got["floor"][b, n:] == 1).all()


# ------------------------------------------------------------------------------------------------ the shortest path
def lattice_batch(rows, T):
    """Host lattices (dicts of [t, 8] / [t]) -> one device lattice [B, T, ...] with the fill values beyond each."""
    B = len(rows)
    lat = {"period": np.zeros((B, T, 8), np.float32), "mass": np.zeros((B, T, 8), np.float32), "depth": np.zeros((B, T, 8), np.float32),
           "count": np.zeros((B, T), np.int32), "unvoiced_mass": np.ones((B, T), np.float32), "floor": np.ones((B, T), np.float32)}
    for b, r in enumerate(rows):
        t = r["count"].shape[0]
        for k in LATTICE:
            lat[k][b, :t] = r[k]
    return lat


def run_viterbi(pitch, rows, frames, T, jump=2.0, switch=0.5, fs=24000):
    lat = lattice_batch(rows, T)
    dev = {k: torch.from_numpy(v).cuda() for k, v in lat.items()}
    dev.update(frames=torch.tensor(frames), sample_rate=fs)
    got = pitch.viterbi(dev, jump, switch, check=False)
    for b, n in enumerate(frames):
        row = {k: lat[k][b] for k in LATTICE}
        state, f0, ap = ps.viterbi(row, n, fs, jump, switch, twin=True)
        assert np.array_equal(got["state"][b].cpu().numpy(), state), (b, n, got["state"][b].tolist(), state.tolist())
        assert np.array_equal(words(got["f0"][b]), words(f0)), (b, n)
        assert np.array_equal(words(got["aperiodicity"][b]), words(ap)), (b, n)
    return got, lat


def random_row(rng, T, max_count=9, ties=False, bad=0.08):
    """A lattice of T frames with 0 .. max_count - 1 candidates each around a slowly moving period (its multiples and fractions, so
    the voiced path has something to follow) and a few bad frames; with ``ties`` every number is a small dyadic rational, so equal
    path costs are exactly equal."""
    r = {"period": np.zeros((T, 8), np.float32), "mass": np.zeros((T, 8), np.float32), "depth": np.zeros((T, 8), np.float32),
         "count": np.zeros(T, np.int32), "unvoiced_mass": np.ones(T, np.float32), "floor": np.ones(T, np.float32)}
    base = 150.0 * np.exp(np.cumsum(0.02 * rng.standard_normal(T)))
    for k in range(T):
        c = int(rng.integers(0, max_count))
        r["count"][k] = -1 if rng.random() < bad else c
        if ties:
            r["period"][k, :c] = np.sort(rng.choice([64.0, 128.0, 256.0], size=c))
            r["mass"][k, :c] = rng.integers(4, 8, size=c) / 8.0
            r["unvoiced_mass"][k] = rng.integers(0, 3) / 8.0
        else:
            ratios = np.concatenate([[1.0], rng.choice([0.25, 0.5, 0.75, 1.5, 2.0, 3.0, 4.0], size=max(c - 1, 0), replace=False)])[:c]
            order = np.argsort(ratios)
            u = rng.uniform(0.0, 0.2) if c else 1.0
            share = np.concatenate([[0.7], 0.3 * rng.dirichlet(np.ones(c - 1))]) if c > 1 else np.ones(c)      # the period itself leads
            r["period"][k, :c] = (base[k] * ratios * (1.0 + 0.01 * rng.standard_normal(c)))[order]
            r["mass"][k, :c], r["unvoiced_mass"][k] = ((1.0 - u) * share)[order], u
        r["depth"][k, :c] = rng.uniform(0.0, 0.3, size=c)
        r["floor"][k] = rng.uniform(0.3, 1.0)
    return r


def test_viterbi_on_handmade_lattices(pitch):
    """T = 1, 2, 63, 64, 65, 130 (the staging chunk is 64 frames), counts 0 .. 8 mixed, bad frames, an all-unvoiced row, and refused
    rows (frames -1 and T + 1) next to good ones: path, f0 and aperiodicity equal the twin's bits."""
    rng = np.random.default_rng(21)
    lengths = [1, 2, 63, 64, 65, 130]
    rows = [random_row(rng, t) for t in lengths]
    silent = random_row(rng, 70)
    silent["count"][:] = 0
    silent["count"][10] = -1
    rows += [silent, random_row(rng, 130), random_row(rng, 130)]
    frames = lengths + [70, -1, 131]
    got, lat = run_viterbi(pitch, rows, frames, 130)
    assert (got["state"][6, :70] == 8).all() and (got["f0"][6] == 0).all() and torch.isnan(got["aperiodicity"][6, 10])
    for b in (7, 8):                                               # refused: the fill values in every column
        assert (got["state"][b] == -1).all() and (got["f0"][b] == 0).all() and (got["aperiodicity"][b] == 1).all()
    lib, hip = sub("_hip").load(), sub("_hip")
    ws = pitch._ws.get("pitch_viterbi", 0, torch.device("cuda", torch.cuda.current_device()))
    assert lib.mtts_pitch_status(ws.data_ptr(), hip.stream_ptr()) == -1
    assert b"mtts_pitch_viterbi: row 7 has -1 frames" in lib.mtts_last_error(), lib.mtts_last_error()
    voiced = sum(int((got["state"][b, :n] < 8).sum()) for b, n in enumerate(lengths))
    print(f"hand-made lattices: {voiced} voiced states on {sum(lengths)} frames")
    assert voiced > 50
    # other costs, another sample rate
    run_viterbi(pitch, rows[:6], lengths, 130, jump=8.0, switch=1.0, fs=8000)
    run_viterbi(pitch, rows[:6], lengths, 130, jump=0.0, switch=0.0)
    with pytest.raises(ValueError, match="row 0 has 131 frames"):
        dev = {k: torch.from_numpy(v[:1]).cuda() for k, v in lat.items()}
        pitch.viterbi({**dev, "frames": torch.tensor([131]), "sample_rate": 24000})


def test_viterbi_ties_go_to_the_lowest_index(pitch):
    """Dyadic lattices, on which equal costs are exactly equal: only the lowest-index rule decides, at the end state and at every
    step of the way back."""
    rng = np.random.default_rng(22)
    lengths = [2, 3, 5, 17, 64, 65, 129, 130]
    rows = [random_row(rng, t, max_count=5, ties=True) for t in lengths]
    got, _ = run_viterbi(pitch, rows, lengths, 130)
    flat = {"period": np.tile(np.array([64.0, 64.0, 128.0, 0, 0, 0, 0, 0], np.float32), (70, 1)), "mass": np.tile(np.array([.25, .25, .25, 0, 0, 0, 0, 0], np.float32), (70, 1)),
            "depth": np.zeros((70, 8), np.float32), "count": np.full(70, 3, np.int32), "unvoiced_mass": np.full(70, 0.25, np.float32), "floor": np.ones(70, np.float32)}
    got, _ = run_viterbi(pitch, [flat], [70], 70)
    assert (got["state"][0] == 0).all()                            # states 0, 1 and U all cost the same: the lowest index


def test_viterbi_is_not_greedy(pitch):
    """The frame-by-frame cheapest state is not the cheapest path: the middle frame prefers the octave above, the path stays."""
    lat = {"period": np.zeros((5, 8), np.float32), "mass": np.zeros((5, 8), np.float32), "depth": np.zeros((5, 8), np.float32),
           "count": np.full(5, 2, np.int32), "unvoiced_mass": np.full(5, 0.05, np.float32), "floor": np.full(5, 0.5, np.float32)}
    lat["period"][:, 0], lat["period"][:, 1] = 80.0, 160.0
    lat["mass"][:, 0], lat["mass"][:, 1] = 0.15, 0.8
    lat["mass"][2, 0], lat["mass"][2, 1] = 0.6, 0.35
    lat["depth"][:, 0], lat["depth"][:, 1] = 0.2, 0.02
    got, _ = run_viterbi(pitch, [lat], [5], 5)
    assert got["state"][0].tolist() == [1, 1, 1, 1, 1] and got["f0"][0].tolist() == [150.0] * 5
    greedy, _ = run_viterbi(pitch, [lat], [5], 5, jump=0.0)
    assert greedy["state"][0].tolist() == [1, 1, 0, 1, 1] and greedy["f0"][0, 2].item() == 300.0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tracked(pitch):
    """The three signals through ``track`` and ``track_viterbi``, once."""
    sigs = ps.signals()
    audio, lengths = padded([x for _, x, _ in sigs], extra=4), [len(x) for _, x, _ in sigs]
    return pitch.track(audio, lengths), pitch.track_viterbi(audio, lengths)


def off(tr, b, f):
    n = int(tr["frames"][b])
    truth = ps.truth_at_frames(f, n, tr["max_lag"])
    return ps.off_count(tr["f0"][b, :n].cpu().numpy(), truth), n


def test_the_path_removes_the_octave_excursion(pitch, tracked):
    """The test plain YIN fails: on dip60 no frame of the path is more than 50 cents off the true contour; YIN has at least one."""
    yin, path = tracked
    _, x, f = ps.signals()[0]
    (y_off, n), (p_off, _) = off(yin, 0, f), off(path, 0, f)
    print(f"dip60: {n} frames; YIN {y_off} more than 50 cents off, the path {p_off}")
    assert n == 121 and p_off == 0 and y_off >= 1
    assert int((path["f0"][0, :n] > 0).sum()) == n
    assert set(path) >= set(yin) | {"state"} and path["state"].dtype == torch.int8
    # the device's path is the twin's, bit for bit
    twin = ps.analysed("dip60")[1]
    assert np.array_equal(words(path["f0"][0, :n]), words(twin["f0"][:n])) and np.array_equal(path["state"][0, :n].cpu().numpy(), twin["state"][:n])


def test_a_genuine_octave_step_is_kept(pitch, tracked):
    yin, path = tracked
    _, x, f = ps.signals()[1]
    (y_off, n), (p_off, _) = off(yin, 1, f), off(path, 1, f)
    unv = int((path["f0"][1, :n] == 0).sum())
    print(f"step: YIN {y_off} off, the path {p_off} off, {unv} unvoiced at the step")
    assert p_off == y_off
    lo, hi = path["f0"][1, :n][path["f0"][1, :n] > 0].min().item(), path["f0"][1, :n].max().item()
    assert abs(lo - 110.0) < 1.0 and abs(hi - 220.0) < 2.0


def test_voicing_equals_yins_where_the_twin_says_so(pitch, tracked):
    yin, path = tracked
    n = int(yin["frames"][2])
    y_twin, p_twin = ps.analysed("noise_tone_noise")
    agree = (y_twin["voiced"]) == (p_twin["f0"][:n] > 0)
    got = ((yin["f0"][2, :n] > 0) == (path["f0"][2, :n] > 0)).cpu().numpy()
    print(f"noise, tone, noise: the twin's voicing agrees on {int(agree.sum())} of {n} frames, the device's on {int(got.sum())}")
    assert n == 158 and got[agree].all()


def test_track_with_its_present_arguments_is_untouched(pitch, tracked):
    """``contour`` with the default method makes ``track``'s calls: the same bits."""
    sigs = ps.signals()
    audio, lengths = padded([x for _, x, _ in sigs], extra=4), [len(x) for _, x, _ in sigs]
    again = pitch.contour(audio, lengths)
    for k in ("f0", "aperiodicity", "frames"):
        assert np.array_equal(words(again[k]), words(tracked[0][k])), k
    assert "state" not in again


# ------------------------------------------------------------------------------------------------ fold
H, W, TMAX = 128, 1024, 400


def centre(k):
    return (2 * k * H + W + TMAX) // 2                              # (W + TMAX is even here: the centre is a whole sample)


def fold_case(seed=31):
    """Three rows over 400 frames: tokens with m = 1, 2, 64, 65, 130 voiced values, empty and one-frame tokens, boundaries exactly on
    a frame centre and one sample either side, marks of -1 and tokens beyond x_lengths."""
    rng = np.random.default_rng(seed)
    n, T, Tx = 400, 404, 12
    L = 399 * H + W + TMAX + 57
    f0 = np.zeros((3, T), np.float32)
    f0[:, :n] = rng.uniform(80, 300, (3, n))
    f0[2, :n][rng.random(n) < 0.3] = 0.0                            # row 2: unvoiced frames, also at the tokens' edges
    f0[1, 200:330] = np.round(f0[1, 200:330] / 40.0) * 40.0         # many equal values: ties in the rank counting
    f0[:, n:] = 0.0
    marks = np.full((3, Tx, 2), -1, np.int64)
    # row 0: frame ranges [0,1) [1,3) [3,67) [67,132) [132,262) then an empty token, a one-sample token, (-1, -1), and a last one
    edges = [0, centre(1), centre(3), centre(67), centre(132), centre(262)]
    for i in range(5):
        marks[0, i] = edges[i], edges[i + 1]
    marks[0, 5] = edges[5], edges[5]
    marks[0, 6] = edges[5], edges[5] + 1
    marks[0, 8] = edges[5] + 1, L
    # row 1: boundaries one sample either side of a centre; a token between two centres (no frame)
    marks[1, 0] = 0, centre(10) + 1
    marks[1, 1] = centre(10) + 1, centre(20) - 1
    marks[1, 2] = centre(20) - 1, centre(20) + 3
    marks[1, 3] = centre(20) + 3, centre(21) - 2
    marks[1, 4] = centre(21) - 2, centre(200)
    marks[1, 5] = centre(200), centre(330)
    marks[1, 6] = centre(330), L
    marks[1, 9] = 5, 3                                              # beyond x_lengths: never looked at
    # row 2: few tokens, frames fewer than the others
    marks[2, 0] = 100, 9000
    marks[2, 1] = 9000, 30000
    x_len = [9, 7, 2]
    frames = [n, n, 250]
    audio = (0.3 * rng.standard_normal((3, (L + 3) // 4 * 4))).astype(np.float32)
    return f0, frames, marks, x_len, audio, [L, L, 40000]


def run_fold(pitch, f0, frames, marks, x_len, audio=None, lengths=None, check=True):
    tr = {"f0": torch.from_numpy(f0).cuda(), "frames": torch.tensor(frames), "hop": H, "window": W, "max_lag": TMAX}
    return pitch.fold(tr, torch.from_numpy(marks), x_len, None if audio is None else torch.from_numpy(audio).cuda(), lengths, check=check)


def check_fold(got, b, f0, n, marks, x_len, audio=None, length=None):
    counts, hz, ms, why = ps.fold(f0, n, H, W, TMAX, marks, x_len, None if audio is None else audio[:len(audio)], length)
    assert np.array_equal(got["frames"][b].cpu().numpy(), counts[:, 0]) and np.array_equal(got["voiced"][b].cpu().numpy(), counts[:, 1]), (b, counts.tolist())
    for j, k in enumerate(("median_hz", "first_hz", "last_hz")):
        assert np.array_equal(words(got[k][b]), words(hz[:, j])), (b, k)
    if ms is not None:
        assert np.array_equal(words(got["mean_square"][b]), words(ms)), (b, got["mean_square"][b].tolist(), ms.tolist())
    return counts, ms, why


def test_fold_equals_the_restatement(pitch):
    f0, frames, marks, x_len, audio, lengths = fold_case()
    got = run_fold(pitch, f0, frames, marks, x_len, audio, lengths)
    for b in range(3):
        counts, ms, why = check_fold(got, b, f0[b], frames[b], marks[b], x_len[b], audio[b], lengths[b])
        assert why == 0
        print(f"row {b}: frames {counts[:x_len[b], 0].tolist()}, voiced {counts[:x_len[b], 1].tolist()}")
    assert got["frames"][0, :9].tolist() == got["voiced"][0, :9].tolist() == [1, 2, 64, 65, 130, 0, 1, 0, 137]
    assert got["voiced"][1, 5].item() == 130 and got["frames"][1, :5].tolist() == [11, 9, 1, 0, 179]
    assert torch.isnan(got["median_hz"][0, 5]) and got["mean_square"][0, 5].item() == 0.0 and got["mean_square"][0, 7].item() == 0.0
    assert (got["frames"][1, 7:] == 0).all() and torch.isnan(got["median_hz"][1, 7:]).all()
    # the mean square against np.sum in fp64, within gamma_n of it (u = 2^-53, n = the token's samples) and the division's rounding
    for b in range(3):
        for i in range(x_len[b]):
            st, en = marks[b, i]
            if en > st >= 0:
                m = int(en - st)
                want = np.sum(audio[b, st:en].astype(np.float64) ** 2)
                g = m * 2.0 ** -53 / (1 - m * 2.0 ** -53)
                assert abs(got["mean_square"][b, i].item() * m - want) <= (g + 2.0 ** -52) * want, (b, i)
                assert got["energy_db"][b, i].item() == pytest.approx(10 * np.log10(want / m), abs=1e-9)
    # without audio: the same counts and hz, no energy; lengths alone bound the marks
    bare = run_fold(pitch, f0, frames, marks, x_len)
    assert "mean_square" not in bare
    for k in bare:
        assert np.array_equal(words(bare[k]), words(got[k])), k
    only = run_fold(pitch, f0, frames, marks, x_len, None, lengths)
    assert np.array_equal(words(only["median_hz"]), words(got["median_hz"]))


def test_fold_refusals_leave_the_neighbours_alone(pitch):
    f0, frames, marks, x_len, audio, lengths = fold_case()
    good = run_fold(pitch, f0, frames, marks, x_len, audio, lengths)
    L = lengths[1]

    def broken(what):
        m, fr, xl, ln = marks.copy(), list(frames), list(x_len), list(lengths)
        if what == "mark above the length":
            m[1, 6, 1] = L + 1
        elif what == "mark below zero":
            m[1, 0, 0] = -2
        elif what == "start > end":
            m[1, 3] = m[1, 3, 1], m[1, 3, 0]
        elif what == "not ascending":
            m[1, 2, 0] -= 1
        elif what == "not ascending across a gap":
            m[1, 1] = -1, -1
            m[1, 2, 0] = m[1, 0, 1] - 1
        elif what == "frames":
            fr[1] = -1
        elif what == "x_length":
            xl[1] = 13
        elif what == "length":
            ln[1] = audio.shape[1] + 1
        return m, fr, xl, ln

    words_of = {"mark above the length": "a mark outside", "mark below zero": "a mark outside", "start > end": "start > end",
                "not ascending": "do not ascend", "not ascending across a gap": "do not ascend", "frames": "frame count", "x_length": "x_length",
                "length": "a length outside"}
    for what, word in words_of.items():
        m, fr, xl, ln = broken(what)
        got = run_fold(pitch, f0, fr, m, xl, audio, ln, check=False)
        assert (got["frames"][1] == -1).all() and (got["voiced"][1] == 0).all() and torch.isnan(got["median_hz"][1]).all(), what
        assert torch.isnan(got["mean_square"][1]).all(), what
        for b in (0, 2):
            for k in got:
                assert np.array_equal(words(got[k][b]), words(good[k][b])), (what, b, k)
        assert check_fold(got, 1, f0[1], fr[1], m[1], xl[1], audio[1], ln[1])[2] != 0
        with pytest.raises(ValueError, match=f"mtts_pitch_fold: row 1 .*{word}"):
            run_fold(pitch, f0, fr, m, xl, audio, ln)


# ------------------------------------------------------------------------------------------------ the Python entries and the tools
def test_measure_pitch_with_the_path(pitch):
    corpus = sub("corpus")
    clips = [torch.from_numpy(ps.signals()[0][1]), torch.from_numpy(ps.signals()[1][1][:12001]).cuda()]
    got = corpus.measure_pitch(clips, method="viterbi", jump=4.0)
    tr = pitch.track_viterbi(clips, jump=4.0)
    st = pitch.stats(tr["f0"], tr["frames"], tr["hop"], 24000)
    for k in ("f0", "aperiodicity"):
        assert np.array_equal(words(got[k]), words(tr[k])), k
    for k, v in st.items():
        assert got[k].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), k
    yin = corpus.measure_pitch(clips)
    n = int(tr["frames"][0])
    print(f"dip60 highest f0: YIN {float(yin['f0'][0, :n].max()):.1f} Hz, the path {float(got['f0'][0, :n].max()):.1f} Hz")
    assert float(got["f0"][0, :n].max()) < 175.0 < 250.0 < float(yin["f0"][0, :n].max())       # the glide ends at 170 Hz; the excursion is an octave up
    cmp = pitch.compare(tr, pitch.track(clips))
    assert cmp["gross_error"][0].item() > 0 and cmp["voicing_error"][0].item() == 0.0 and cmp["frames"].tolist() == tr["frames"].tolist()


@pytest.fixture(scope="module")
def tiny_model(hparams, synthetic):
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    inference = sub("inference")
    hp = hparams.tiny(n_spks=2)
    model = inference.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    return hp, model.to("cuda:0").eval()


def two_clips():
    return [ps.signals()[0][1], ps.signals()[1][1][:13000]]


def test_model_prosody(pitch, tiny_model, synthetic):
    """align, token_marks, track and fold in one call: the tokens' frame counts add up to the pitch frames whose centres lie inside
    the marks."""
    hp, model = tiny_model
    x, x_len, _ = synthetic.make_inputs(hp, 2, 12, seed=5)
    x, x_len = x[:, :12].cuda(), torch.tensor([12, 9]).cuda()
    clips = [torch.from_numpy(c) for c in two_clips()]
    out = model.prosody(x, x_len, audio=clips)
    marks, frames = out["marks"].cpu().numpy(), out["frames"].cpu().numpy()
    assert out["hop"] == 128 and out["marks"].shape == (2, 12, 2) and out["audio_lengths"].tolist() == [len(c) for c in clips]
    for b in range(2):
        n = int(out["pitch_frames"][b])
        c = 2 * np.arange(n) * 128 + out["window"] + out["max_lag"]
        inside = sum(int(((c >= 2 * st) & (c < 2 * en)).sum()) for st, en in marks[b, :int(x_len[b])])
        print(f"clip {b}: {n} pitch frames, {inside} inside the marks, per token {frames[b].tolist()}")
        assert frames[b, :int(x_len[b])].sum() == inside and inside > 0.8 * n
        assert (frames[b, int(x_len[b]):] == 0).all()
    assert torch.isfinite(out["energy_db"][0]).all() and (out["voiced"] <= out["frames"]).all()
    yin = model.prosody(x, x_len, audio=clips, method="yin")
    assert np.array_equal(yin["frames"].cpu().numpy(), frames)
    with pytest.raises(ValueError, match="fine-mel hop"):
        model.prosody(x, x_len, audio=clips, hop=64)


def write_wav(path, x, rate=24000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.clip(np.round(x.astype(np.float64) * 32767.0), -32768, 32767).astype("<i2").tobytes())


def test_align_tool_prints_pitch_per_token(pitch, tiny_model, synthetic, tmp_path):
    from safetensors.torch import save_file
    ck = sub("checkpoint")
    hp, model = tiny_model
    out = tmp_path / "model"
    out.mkdir()
    save_file(ck.select_path_tensors(hp, synthetic.make_state_dict(hp, seed=7)), str(out / ck.WEIGHTS),
              metadata={"format": "matcha-tts-24k_amd", "version": str(ck.FORMAT_VERSION)})
    (out / ck.HPARAMS).write_text(json.dumps(ck.hparams_to_json(hp)))
    x, _, _ = synthetic.make_inputs(hp, 2, 10, seed=5)
    (tmp_path / "ids.txt").write_text("\n".join(" ".join(str(int(t)) for t in row[:n]) for row, n in zip(x, (10, 7))) + "\n")
    for i, c in enumerate(two_clips()):
        write_wav(tmp_path / f"c{i}.wav", c)
    res = subprocess.run([sys.executable, str(ROOT / "tools" / "align.py"), "--matcha", str(out), "--ids-file", str(tmp_path / "ids.txt"), "--marks", "--pitch",
                          "--out", str(tmp_path / "a.npz"), str(tmp_path / "c0.wav"), str(tmp_path / "c1.wav")], capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in res.stdout.splitlines() if " Hz (" in ln and " dB" in ln]
    assert len(lines) == 17
    saved = np.load(tmp_path / "a.npz")
    for k in ("marks", "token_median_hz", "token_first_hz", "token_last_hz", "token_energy_db", "token_frames", "token_voiced"):
        assert saved[k].shape[:2] == (2, 10), k
    med = saved["token_median_hz"][0][saved["token_voiced"][0] > 0]
    assert med.size > 0 and np.all((med > 140) & (med < 180))       # dip60 glides 150 -> 170 Hz


def test_prepare_corpus_pitch_viterbi(pitch, tmp_path):
    tool = str(ROOT / "tools" / "prepare_corpus.py")
    res = subprocess.run([sys.executable, tool, "pitch", "--viterbi", "--synthetic", "4", "--root", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    print(res.stdout)
    assert "pitch.track_viterbi" in res.stdout and "Pitch per speaker" in res.stdout
    rows = [ln.split() for ln in res.stdout.split("Pitch per speaker")[1].splitlines()[4:6]]
    assert abs(float(rows[0][2]) - 140.0) < 1.0 and abs(float(rows[1][2]) - 160.0) < 1.0     # sines of 120 + 20 i Hz: speaker 0 has clips 0 and 2

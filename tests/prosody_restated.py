"""NumPy restatement of include/mtts.h "prosody", written from the contract there and not from the kernels: the candidates of a
frame (``candidates``), the shortest path through a lattice (``viterbi``) and the fold of a contour onto token marks (``fold``),
each as the fp32 twin in the header's order of operations (``twin=True``: every word is meant to equal the device's) and in fp64
(the yardstick).  The block sums, frame sums and d' come from ``pitch_restated`` by import.  ``brute_force`` walks every path of a
small lattice; ``signals`` builds the three test signals of the prosody tests."""
from functools import lru_cache
from itertools import product

import numpy as np

import pitch_restated as pr

CANDS = 8
U = 8


def _dt(twin):
    return np.float32 if twin else np.float64


def cdf(v, thr2):
    """F(v) = min(max(v / thr2, 0), 1) in the type of its arguments."""
    dt = type(thr2)
    return min(max(dt(v) / thr2, dt(0.0)), dt(1.0))


def record_dips(dp, tmin, tmax, thr, twin):
    """One frame's record-setting dips before the limit of 8: ([(tau, mass, depth), ...] in ascending lag, unvoiced mass)."""
    dt = _dt(twin)
    dp = np.asarray(dp, dtype=dt)
    thr2 = dt(2.0) * dt(np.float32(thr))
    kept = []
    prev = None
    for tau in range(tmin + 1, tmax - 1):
        b = dp[tau - 1]
        if not (b < dp[tau - 2] and b <= dp[tau]):
            continue
        if not b < thr2 or (prev is not None and not b < prev):
            continue
        before = dt(1.0) if prev is None else cdf(prev, thr2)
        kept.append((tau, dt(before - cdf(b, thr2)), b))
        prev = b
    return kept, (dt(1.0) if prev is None else cdf(prev, thr2))


def frame_candidates(dp, tmin, tmax, thr, twin):
    """One frame's d' (column tau - 1) -> (period, mass, depth [8], count, unvoiced mass, floor)."""
    dt = _dt(twin)
    dp = np.asarray(dp, dtype=dt)
    kept, unvoiced = record_dips(dp, tmin, tmax, thr, twin)
    if len(kept) > CANDS:                                          # the 8 of greatest mass, ties to the lower lag; ascending lag
        order = sorted(range(len(kept)), key=lambda j: (-float(kept[j][1]), j))[:CANDS]
        kept = [kept[j] for j in sorted(order)]
    period, mass, depth = np.zeros(CANDS, dtype=dt), np.zeros(CANDS, dtype=dt), np.zeros(CANDS, dtype=dt)
    for j, (tau, m, b) in enumerate(kept):
        a, c = dp[tau - 2], dp[tau]
        den = (a - b) + (c - b)
        delta = (dt(0.5) * (a - c)) / den if den > 0 else dt(0.0)
        period[j], mass[j], depth[j] = dt(tau) + delta, m, b
    seg = dp[tmin - 1:tmax - 1]
    floor = seg[int(np.argmin(seg))]
    return period, mass, depth, len(kept), unvoiced, floor


def candidates(x, fs, hop, fmin=60.0, fmax=500.0, thr=0.15, twin=True, T=None):
    """The lattice of one clip: dict of ``period``, ``mass``, ``depth`` [T, 8], ``count`` int32 [T], ``unvoiced_mass``, ``floor`` [T]
    and ``n``; columns at or beyond n hold the fill values (T defaults to max(1, n))."""
    dt = _dt(twin)
    W, tmin, tmax = pr.plan(fs, hop, fmin, fmax)
    x = np.asarray(x, dtype=np.float32)
    n = pr.n_frames(x.size, hop, tmax)
    T = max(1, n) if T is None else T
    out = {"period": np.zeros((T, CANDS), dtype=dt), "mass": np.zeros((T, CANDS), dtype=dt), "depth": np.zeros((T, CANDS), dtype=dt),
           "count": np.zeros(T, dtype=np.int32), "unvoiced_mass": np.ones(T, dtype=dt), "floor": np.ones(T, dtype=dt), "n": n,
           "window": W, "min_lag": tmin, "max_lag": tmax}
    if n == 0:
        return out
    dp = pr.dprime(pr.frame_sums(pr.block_sums(x, hop, tmax, n + 7, twin), n), twin)
    fin = np.isfinite(x)
    for k in range(n):
        if not fin[k * hop:k * hop + W + tmax].all():
            out["count"][k], out["floor"][k] = -1, np.nan
            continue
        p, m, d, c, u, f = frame_candidates(dp[k], tmin, tmax, thr, twin)
        out["period"][k], out["mass"][k], out["depth"][k] = p, m, d
        out["count"][k], out["unvoiced_mass"][k], out["floor"][k] = c, u, f
    return out


def _states(count):
    c = min(max(int(count), 0), CANDS)
    return list(range(c)) + [U]


def _local(lat, k, s, dt):
    if s == U:
        return dt(0.0) if lat["count"][k] < 0 else dt(1.0) - dt(lat["unvoiced_mass"][k])
    return dt(1.0) - dt(lat["mass"][k, s])


def _trans(lat, k, r, s, jump, switch, dt):
    if r == U and s == U:
        return dt(0.0)
    if r == U or s == U:
        return switch
    pr_, ps = dt(lat["period"][k - 1, r]), dt(lat["period"][k, s])
    return jump * (abs(ps - pr_) / min(ps, pr_))


def viterbi(lat, n, fs, jump=2.0, switch=0.5, twin=True):
    """The path of one clip: (state int8 [T], f0 [T], aperiodicity [T]) with the fill values at or beyond n; n outside [0, T] is a
    refused row: fill values everywhere."""
    dt = _dt(twin)
    T = lat["count"].shape[0]
    state, f0, ap = np.full(T, -1, dtype=np.int8), np.zeros(T, dtype=dt), np.ones(T, dtype=dt)
    if n <= 0 or n > T:
        return state, f0, ap
    jump, switch = dt(np.float32(jump)), dt(np.float32(switch))
    inf = dt(np.inf)
    D = np.full(9, inf, dtype=dt)
    back = np.zeros((n, 9), dtype=np.int64)
    for k in range(n):
        Dn = np.full(9, inf, dtype=dt)
        for s in _states(lat["count"][k]):
            if k == 0:
                best = dt(0.0)
            else:
                best = inf
                for r in range(9):                                 # ascending, strict <: the lowest index wins a tie
                    if D[r] < inf:
                        c = D[r] + _trans(lat, k, r, s, jump, switch, dt)
                        if c < best:
                            best, back[k, s] = c, r
            Dn[s] = best + _local(lat, k, s, dt)
        D = Dn - Dn.min()
    s = int(np.argmin(D))                                          # (argmin: the lowest index of the minimum)
    for k in range(n - 1, -1, -1):
        state[k] = s
        if s == U:
            f0[k], ap[k] = 0.0, (np.nan if lat["count"][k] < 0 else lat["floor"][k])
        else:
            f0[k], ap[k] = dt(np.float32(fs)) / dt(lat["period"][k, s]), lat["depth"][k, s]
        s = int(back[k, s])
    return state, f0, ap


def path_cost(lat, n, path, jump, switch):
    """Plain fp64 cost of a path (no normalisation): what ``brute_force`` minimises."""
    dt = np.float64
    cost = _local(lat, 0, path[0], dt)
    for k in range(1, n):
        cost += _trans(lat, k, path[k - 1], path[k], dt(jump), dt(switch), dt) + _local(lat, k, path[k], dt)
    return cost


def brute_force(lat, n, jump, switch):
    """(the lowest cost, every path that reaches it within 1e-12) over all paths of the first n frames."""
    best, paths = np.inf, []
    for path in product(*[_states(lat["count"][k]) for k in range(n)]):
        c = path_cost(lat, n, path, jump, switch)
        if c < best - 1e-12:
            best, paths = c, [path]
        elif abs(c - best) <= 1e-12:
            paths.append(path)
    return best, paths


def track(x, fs, hop, jump=2.0, switch=0.5, twin=True, **kw):
    """``candidates`` then ``viterbi`` on one clip: dict with ``state``, ``f0``, ``aperiodicity``, ``n`` and the lattice."""
    lat = candidates(x, fs, hop, twin=twin, **kw)
    state, f0, ap = viterbi(lat, lat["n"], fs, jump, switch, twin)
    return {"state": state, "f0": f0, "aperiodicity": ap, "n": lat["n"], "lattice": lat}


# ------------------------------------------------------------------------------------------------ fold
def first_frame(mark, H, W, tmax, n):
    """The first k with 2 k H + W + tmax >= 2 mark, inside [0, n]."""
    num = 2 * mark - W - tmax
    return 0 if num <= 0 else min(n, (num + 2 * H - 1) // (2 * H))


def mean_square(x, start, end):
    """The header's order: 64 lane-strided fp64 partial sums ascending, then v[l] = v[l] + v[l ^ o], o = 32 .. 1."""
    if end <= start:
        return 0.0
    seg = np.asarray(x[start:end], dtype=np.float32)
    if not np.isfinite(seg).all():
        return np.nan
    seg = seg.astype(np.float64)
    v = np.zeros(64)
    for j in range(0, seg.size, 64):
        part = seg[j:j + 64]
        v[:part.size] = v[:part.size] + part * part
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    return v[0] / float(end - start)


def fold_refusal(n, T, marks, x_len, Tx, length=None, ld=None):
    """0 when the row is accepted, else the first reason in the header's list (1 frames .. 6 not ascending)."""
    if n < 0 or n > T:
        return 1
    if x_len < 0 or x_len > Tx:
        return 2
    L = np.iinfo(np.int64).max
    if length is not None:
        L = length
        if L < 0 or (ld is not None and L > ld):
            return 3
    why, prev_end = 0, None
    for i in range(x_len):
        st, en = int(marks[i][0]), int(marks[i][1])
        if st == -1 and en == -1:
            continue
        w = 0
        if st < 0 or en < 0 or st > L or en > L:
            w = 4
        elif st > en:
            w = 5
        elif prev_end is not None and st < prev_end:
            w = 6
        prev_end = en
        if w and (not why or w < why):
            why = w
    return why


def fold(f0, n, H, W, tmax, marks, x_len, audio=None, length=None):
    """One row: (counts int32 [Tx, 2], hz float32 [Tx, 3], mean_square float64 [Tx] or None, reason).  ``np.sort`` for the median."""
    f0 = np.asarray(f0, dtype=np.float32)
    marks = np.asarray(marks, dtype=np.int64)
    Tx = marks.shape[0]
    counts, hz = np.zeros((Tx, 2), dtype=np.int32), np.full((Tx, 3), np.nan, dtype=np.float32)
    ms = None if audio is None else np.zeros(Tx)
    why = fold_refusal(n, f0.size, marks, x_len, Tx, length, None if audio is None else np.asarray(audio).size)
    if why:
        counts[:, 0] = -1
        if ms is not None:
            ms[:] = np.nan
        return counts, hz, ms, why
    for i in range(x_len):
        st, en = int(marks[i, 0]), int(marks[i, 1])
        if st < 0:
            continue
        lo, hi = first_frame(st, H, W, tmax, n), first_frame(en, H, W, tmax, n)
        seg = f0[lo:hi]
        v = seg[seg > 0]
        counts[i] = hi - lo, v.size
        if v.size:
            hz[i] = np.sort(v)[(v.size - 1) // 2], v[0], v[-1]
        if ms is not None:
            ms[i] = mean_square(audio, st, en)
    return counts, hz, ms, 0


# ------------------------------------------------------------------------------------------------ the signals of the tests
FS, HOP = 24000, 128


def _hann_smooth(a, taps=241):
    w = np.hanning(taps)
    return np.convolve(a, w / w.sum(), mode="same")


def dip60(seed=0):
    """A glide 150 -> 170 Hz whose odd harmonics dip to 0.1 for 60 ms; returns (samples, instantaneous fundamental)."""
    rng = np.random.default_rng(seed)
    n = int(0.7 * FS)
    t = np.arange(n) / FS
    f = 150.0 + (170.0 - 150.0) * t / 0.7
    ph = 2 * np.pi * np.cumsum(f) / FS
    a = np.ones(n)
    a[(t >= 0.30) & (t < 0.36)] = 0.1
    a = _hann_smooth(a)
    x = 0.3 * (a * np.sin(ph) + 0.8 * np.sin(2 * ph) + 0.3 * a * np.sin(3 * ph) + 0.01 * rng.standard_normal(n))
    return x.astype(np.float32), f


def step(seed=1):
    """110 Hz, then 220 Hz from 0.35 s, harmonics 1 : 0.5 : 0.25, noise 0.003: a genuine octave step."""
    rng = np.random.default_rng(seed)
    n = int(0.7 * FS)
    t = np.arange(n) / FS
    f = np.where(t < 0.35, 110.0, 220.0)
    ph = 2 * np.pi * np.cumsum(f) / FS
    x = 0.3 * (np.sin(ph) + 0.5 * np.sin(2 * ph) + 0.25 * np.sin(3 * ph)) + 0.003 * rng.standard_normal(n)
    return x.astype(np.float32), f


def noise_tone_noise(seed=2):
    """0.25 s of 0.05 white noise, 0.4 s of the dip-free glide, 0.25 s of noise."""
    rng = np.random.default_rng(seed)
    n = int(0.4 * FS)
    t = np.arange(n) / FS
    f = 150.0 + (170.0 - 150.0) * t / 0.4
    ph = 2 * np.pi * np.cumsum(f) / FS
    tone = 0.3 * (np.sin(ph) + 0.8 * np.sin(2 * ph) + 0.3 * np.sin(3 * ph) + 0.01 * rng.standard_normal(n))
    m = int(0.25 * FS)
    x = np.concatenate([0.05 * rng.standard_normal(m), tone, 0.05 * rng.standard_normal(m)])
    return x.astype(np.float32), np.concatenate([np.zeros(m), f, np.zeros(m)])


def ripple(amp, period, n=3000, seed=7):
    """A slow sine (period 390.3 samples) with a fast ripple on it: on the falling half of d' every ripple is a dip deeper than the
    last, so with a threshold near 1 a frame keeps many more than 8 (amp 0.1, period 8.3: 23 or 24) or just about 8 (0.5, 11.7)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.5 * np.sin(2 * np.pi * t / 390.3) + amp * np.sin(2 * np.pi * t / period) + 0.0005 * rng.standard_normal(n)).astype(np.float32)


@lru_cache(maxsize=None)
def signals():
    """(name, samples, true fundamental per sample), built once."""
    return tuple((name, *fn()) for name, fn in (("dip60", dip60), ("step", step), ("noise_tone_noise", noise_tone_noise)))


def truth_at_frames(f, n, tmax, hop=HOP, fs=FS):
    t = pr.frame_times(n, hop, tmax, fs)
    return f[np.minimum(np.round(t * fs).astype(int), f.size - 1)]


def off_count(f0, truth, cents=50.0):
    """Voiced frames more than ``cents`` off the truth, among the frames whose truth is voiced."""
    f0 = np.asarray(f0, dtype=np.float64)
    both = (f0 > 0) & (truth > 0)
    return int(np.sum(np.abs(1200.0 * np.log2(f0[both] / truth[both])) > cents))


@lru_cache(maxsize=None)
def analysed(name, jump=2.0, switch=0.5):
    """(YIN twin analysis, path twin analysis) of a signal, computed once and shared by the tests."""
    for nm, x, _ in signals():
        if nm == name:
            return pr.analyse(x, FS, HOP, twin=True), track(x, FS, HOP, jump, switch, twin=True)
    raise KeyError(name)

"""NumPy restatement of include/mtts.h "pitch", written from the contract there and not from the kernels: ``analyse`` in fp64 (plain
sums: the yardstick) and, with ``twin=True``, in fp32 in exactly the header's order of operations (block sums ascending in j without
fused multiply-adds, eight blocks ascending, the grouped prefix with its six scan steps).  Both return, per frame, the chosen lag,
d', aperiodicity, f0 and the smallest MARGIN of any comparison the walk made, so a test can tell the frames whose decisions fp32
rounding cannot flip ("decidable") from the few where it can; ``select`` restates ``mtts_pitch_stats`` with ``np.sort``.

The error budget (``rel_budget``), derived -- not measured.  u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., Lemma 3.1); every quantity summed is non-negative, so a bound on each term's relative error is a bound
on the sum's.
  * a term (x - y)^2 as fl(fl(x - y) * fl(x - y)) carries 3 roundings; in the block sum term j then passes through at most H - 1
    additions (the first, 0.0f + t, is exact), in the frame sum through 7 more: d^(tau) = d(tau) (1 + theta), |theta| <= gamma_{H+9};
  * c(tau) adds such d's through at most 15 additions inside a group, 6 scan steps and the final P + r: 22 more,
    c^(tau) = c(tau) (1 + theta'), |theta'| <= gamma_{H+31};
  * d'^ = fl(fl(d^ * tau) / c^) ((float)tau is exact): numerator (1 + theta_{H+11}), denominator (1 + theta_{H+31}); by Lemma 3.3 the
    quotient is (1 + theta_n) with n = (H + 11) + 2 (H + 31) = 3 H + 73.
So |d'^ - d'| <= gamma_{3H+73} d' for every lag: 2.7e-5 d' at H = 128, 1.2e-5 d' at H = 40, 7.2e-6 d' at H = 16.  (The fp64 yardstick's
own error, gamma_n with u = 2^-53, is nine orders below and is covered by the factor 1 + 2^-20 applied in ``rel_budget``; underflow
does not occur: a non-zero squared difference of an audio signal is far above 2^-126, and where every difference is zero both sides
give exactly c = 0 and d' = 1.)  A comparison of two values is decided when their distance exceeds the sum of their budgets.

f0 (``f0_budget``).  With e_a, e_b, e_c the budgets of a = d'(tau* - 1), b = d'(tau*), c = d'(tau* + 1), N = a - c and
D = (a - b) + (c - b): |N^ - N| <= e_a + e_c + u |N|, |D^ - D| <= e_a + 2 e_b + e_c + u (|a - b| + |c - b| + |D|) =: E_D (each fp32
subtraction or addition rounds its own result once).  For E_D < D,
    |N^/D^ - N/D| = |N^ D - N D^| / (D D^) <= (E_N D + |N| E_D) / (D (D - E_D)),
delta = 0.5 N / D adds one rounding (the division; the product with 0.5 is exact): E_delta = 0.5 (...) + 2 u |delta|.  Then
t = fl(tau + delta) and f0 = fl(fs / t): |f0^ - f0| <= f0 (E_delta / (t - E_delta) + 4 u).  "D > 0" is a comparison like the others:
its margin is D - E_D.
"""
from functools import lru_cache

import numpy as np

U32 = 2.0 ** -24
MAX_LAG = 1024


def plan(fs, hop, fmin, fmax):
    """(window, min_lag, max_lag), or ValueError where the contract refuses the parameters."""
    if not 8000 <= fs <= 48000 or not 8 <= hop <= 512:
        raise ValueError("sample_rate or hop out of range")
    tmax, tmin = int(np.ceil(fs / fmin)), int(np.floor(fs / fmax))
    if tmin < 2 or tmin + 2 > tmax or tmax > MAX_LAG:
        raise ValueError("lags out of range")
    return 8 * hop, tmin, tmax


def n_frames(L, hop, tmax):
    return 0 if L < 8 * hop + tmax else (L - 8 * hop - tmax) // hop + 1


def frame_times(n, hop, tmax, fs):
    return (np.arange(n) * hop + (8 * hop + tmax) / 2.0) / fs


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def rel_budget(hop):
    """|d'^(tau) - d'(tau)| <= rel_budget(hop) * d'(tau): the derivation is the module's docstring."""
    return gamma(3 * hop + 73) * (1.0 + 2.0 ** -20)


def block_sums(x, hop, tmax, nblk, twin):
    """s_b(tau) [nblk, tmax] (column tau - 1).  twin: fp32, ascending j from 0.0f, d = x - y; s = s + d * d."""
    dt = np.float32 if twin else np.float64
    x = np.asarray(x, dtype=dt)
    base = (np.arange(nblk) * hop)[:, None]
    lag = np.arange(1, tmax + 1)[None, :]
    s = np.zeros((nblk, tmax), dtype=dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(hop):
            d = x[base + j] - x[base + j + lag]
            s = s + d * d
    return s


def frame_sums(s, n):
    """d_k(tau) = ((s_k + s_k+1) + ...) + s_k+7 in ascending block order [n, tmax]."""
    d = s[0:n].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(1, 8):
            d = d + s[b:b + n]
    return d


def dprime(d, twin):
    """d'(tau) [n, tmax].  fp64: c is a plain cumulative sum.  twin: the header's grouped prefix in fp32."""
    n, tmax = d.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if not twin:
            c = np.cumsum(d, axis=1)
            tau = np.arange(1, tmax + 1, dtype=np.float64)[None, :]
            return np.where(c > 0, d * tau / np.where(c > 0, c, 1.0), 1.0)
        pad = np.zeros((n, MAX_LAG), dtype=np.float32)
        pad[:, :tmax] = d
        g = pad.reshape(n, 64, 16)
        r = np.zeros_like(g)
        acc = np.zeros((n, 64), dtype=np.float32)
        for i in range(16):
            acc = acc + g[:, :, i]
            r[:, :, i] = acc
        v = acc.copy()
        for o in (1, 2, 4, 8, 16, 32):
            nxt = v.copy()
            nxt[:, o:] = v[:, o:] + v[:, :-o]
            v = nxt
        P = np.zeros((n, 64), dtype=np.float32)
        P[:, 1:] = v[:, :-1]
        c = (P[:, :, None] + r).reshape(n, MAX_LAG)[:, :tmax]
        tau = np.arange(1, tmax + 1).astype(np.float32)[None, :]
        q = (d.astype(np.float32) * tau) / np.where(c > 0, c, np.float32(1.0))
        out = np.where(c > 0, q, np.float32(1.0))
        assert out.dtype == np.float32
        return out


def walk(dp, tmin, tmax, thr, e):
    """One frame's walk over d' (column tau - 1): (tau*, voiced, margin).  ``margin``: the smallest (distance - budget) over the
    comparisons made -- the threshold tests up to the chosen lag (all of them for an unvoiced frame), the descent steps and the one
    that ended the descent, and for an unvoiced frame the minimum against every other lag.  ``e``: the absolute budget of every lag
    (zeros for the twin; zero where d' is the exact constant 1 of c = 0, which both arithmetics produce without rounding: a tie of
    two such values is decided by the lowest-index rule and is no loss of margin)."""
    v = dp.astype(np.float64)
    margin = np.inf
    first = None
    for tau in range(tmin, tmax):
        margin = min(margin, abs(v[tau - 1] - thr) - e[tau - 1])
        if dp[tau - 1] < thr:
            first = tau
            break
    if first is None:
        seg = dp[tmin - 1:tmax - 1]
        star = tmin + int(np.argmin(seg))                          # (argmin: the lowest index of the minimum)
        others = np.delete(np.arange(tmin, tmax), star - tmin)
        others = others[~((others > star) & (e[others - 1] == 0) & (e[star - 1] == 0) & (v[others - 1] == v[star - 1]))]
        if others.size:
            margin = min(margin, float(np.min(v[others - 1] - v[star - 1] - e[others - 1] - e[star - 1])))
        return star, False, margin
    star = first
    while star + 1 < tmax:
        margin = min(margin, abs(v[star] - v[star - 1]) - e[star] - e[star - 1])
        if not dp[star] < dp[star - 1]:
            break
        star += 1
    return star, True, margin


def parabola(dp, star, tmin, tmax, fs, budget, twin):
    """(f0, f0 budget, margin of the denominator test) of a voiced frame at lag ``star``."""
    dt = np.float32 if twin else np.float64
    a, b, c = (dt(dp[star - 2]), dt(dp[star - 1]), dt(dp[star]))
    delta, e_delta, margin = dt(0.0), 0.0, np.inf
    if tmin < star < tmax - 1:
        den = (a - b) + (c - b)
        A, B, C_ = float(a), float(b), float(c)
        ea, eb, ec = budget * abs(A), budget * abs(B), budget * abs(C_)
        N, D = A - C_, (A - B) + (C_ - B)
        E_N = ea + ec + U32 * abs(N)
        E_D = ea + 2 * eb + ec + U32 * (abs(A - B) + abs(C_ - B) + abs(D))
        margin = abs(D) - E_D
        if den > 0:
            delta = (dt(0.5) * (a - c)) / den
            if margin > 0:
                e_delta = 0.5 * (E_N * D + abs(N) * E_D) / (D * (D - E_D)) + 2 * U32 * abs(float(delta))
            else:
                e_delta = np.inf
    t = dt(star) + delta
    f0 = dt(fs) / t
    e_f0 = float(f0) * (e_delta / (float(t) - e_delta) + 4 * U32) if np.isfinite(e_delta) and e_delta < float(t) else np.inf
    return f0, e_f0, margin


def analyse(x, fs, hop, fmin=60.0, fmax=500.0, thr=0.15, twin=False):
    """The contract on one clip.  Returns a dict of per-frame arrays: ``lag``, ``voiced``, ``aperiodicity``, ``f0``, ``f0_budget``
    (absolute, Hz), ``margin`` (> 0: decidable), ``nonfinite`` and ``dprime`` [n, tmax].  The threshold is (float)thr, as the device
    compares it.  fp64 margins use ``rel_budget(hop)``; the twin's margins use a budget of 0 (its own decisions' distances)."""
    W, tmin, tmax = plan(fs, hop, fmin, fmax)
    x = np.asarray(x, dtype=np.float32)
    L = x.size
    n = n_frames(L, hop, tmax)
    thr32 = float(np.float32(thr))
    budget = 0.0 if twin else rel_budget(hop)
    out = {"lag": np.zeros(n, dtype=np.int64), "voiced": np.zeros(n, dtype=bool), "aperiodicity": np.zeros(n), "f0": np.zeros(n),
           "f0_budget": np.zeros(n), "margin": np.zeros(n), "nonfinite": np.zeros(n, dtype=bool), "dprime": np.zeros((n, tmax)),
           "n": n, "window": W, "min_lag": tmin, "max_lag": tmax}
    if n == 0:
        return out
    s = block_sums(x, hop, tmax, n + 7, twin)
    d = frame_sums(s, n)
    dp = dprime(d, twin)
    out["dprime"] = dp
    with np.errstate(invalid="ignore", over="ignore"):
        exact = np.cumsum(d.astype(np.float64), axis=1) == 0      # every difference up to this lag is zero: d' = 1 without rounding
        e = np.where(exact, 0.0, budget * np.abs(dp.astype(np.float64)))
    fin = np.isfinite(x)
    for k in range(n):
        if not fin[k * hop:k * hop + W + tmax].all():
            out["nonfinite"][k] = True
            out["aperiodicity"][k] = np.nan
            out["margin"][k] = np.inf
            continue
        star, voiced, margin = walk(dp[k], tmin, tmax, thr32, e[k])
        out["lag"][k], out["voiced"][k], out["aperiodicity"][k] = star, voiced, dp[k, star - 1]
        if voiced:
            f0, e_f0, m2 = parabola(dp[k], star, tmin, tmax, fs, budget, twin)
            out["f0"][k], out["f0_budget"][k] = f0, e_f0
            margin = min(margin, m2)
        out["margin"][k] = margin
    return out


def difference_by_correlation(x, fs, hop, fmin=60.0):
    """d_k(tau) [n, tmax] from energies and ``np.correlate`` -- independent code for the difference function:
    sum (x_j - x_{j+tau})^2 = sum x_j^2 + sum x_{j+tau}^2 - 2 sum x_j x_{j+tau} over the W samples of a frame."""
    tmax = int(np.ceil(fs / fmin))
    W = 8 * hop
    x = np.asarray(x, dtype=np.float64)
    n = n_frames(x.size, hop, tmax)
    sq = np.concatenate([[0.0], np.cumsum(x * x)])
    d = np.zeros((n, tmax))
    for k in range(n):
        seg = x[k * hop:k * hop + W + tmax]
        cross = np.correlate(seg, seg[:W], mode="valid")           # cross[tau] = sum_{j < W} seg[j + tau] seg[j]
        tau = np.arange(1, tmax + 1)
        e0 = sq[k * hop + W] - sq[k * hop]
        et = sq[k * hop + W + tau] - sq[k * hop + tau]
        d[k] = e0 + et - 2.0 * cross[1:tmax + 1]
    return d


def select(f0, n, tail_frames):
    """``mtts_pitch_stats`` of one row by sorting: ((p05, median, p95, tail median) float32, (frames, voiced, voiced in tail))."""
    f0 = np.asarray(f0, dtype=np.float32)
    if n < 0 or n > f0.size:
        return np.full(4, np.nan, dtype=np.float32), (-1, 0, 0)
    idx = np.flatnonzero(f0[:n] > 0)
    m = idx.size
    out = np.full(4, np.nan, dtype=np.float32)
    mt = 0
    if m:
        v = np.sort(f0[idx])
        out[:3] = v[(m - 1) // 20], v[(m - 1) // 2], v[19 * (m - 1) // 20]
        t = np.sort(f0[idx[idx >= idx[-1] - tail_frames]])
        mt = t.size
        if mt >= 3:
            out[3] = t[(mt - 1) // 2]
    return out, (n, m, mt)


# ------------------------------------------------------------------------------------------------ the signals of the tests
def tone(freq, fs=24000, seconds=0.12):
    """A steady two-harmonic tone."""
    t = np.arange(int(round(seconds * fs))) / fs
    return (0.5 * np.sin(2 * np.pi * freq * t) + 0.25 * np.sin(2 * np.pi * 2 * freq * t + 0.7)).astype(np.float32)


def glide(f_from, f_to, fs, seconds=0.9, seed=0):
    """A five-harmonic glide with noise 40 dB below it, an unvoiced noise gap in the middle and leading digital zeros; returns
    (samples float32, instantaneous fundamental per sample -- 0 in the zeros and the gap)."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * fs))
    f = f_from * (f_to / f_from) ** (np.arange(n) / n)
    phase = 2 * np.pi * np.cumsum(f) / fs
    amp = (1.0, 0.6, 0.4, 0.25, 0.15)
    x = sum(a * np.sin((h + 1) * phase + 0.3 * h) for h, a in enumerate(amp))
    x *= 0.3 / np.sqrt(np.mean(x * x))
    x += 0.3 * 10 ** (-40 / 20) * rng.standard_normal(n)
    lead = int(0.06 * fs)
    g0, g1 = int(0.42 * n), int(0.54 * n)
    x[g0:g1] = 0.05 * rng.standard_normal(g1 - g0)
    f[g0:g1] = 0.0
    x[:lead] = 0.0
    f[:lead] = 0.0
    return x.astype(np.float32), f


@lru_cache(maxsize=None)
def decision_signals():
    """The signals the decisions are judged on: (name, samples, fs, hop), each analysed once in fp64 (``analysed``)."""
    out = []
    for fs, hop in ((24000, 128), (8000, 40)):
        out.append((f"up_{fs}", glide(90.0, 250.0, fs, seed=1)[0], fs, hop))
        out.append((f"down_{fs}", glide(220.0, 140.0, fs, seed=2)[0], fs, hop))
    return tuple(out)


@lru_cache(maxsize=None)
def analysed(name, twin=False):
    for nm, x, fs, hop in decision_signals():
        if nm == name:
            return analyse(x, fs, hop, twin=twin)
    raise KeyError(name)

"""NumPy restatement of include/mtts.h "mtts_loudness_r128": the fp64 table of the true-peak interpolator, its fp32 fixed-order
evaluation, the 3 s short-term blocks, the two gates of the loudness range, its integer percentile indices, the maximum momentary
and short-term loudness and the gain with two ceilings.  The cascade and the 100 ms segments are those of loudness_restated.py.
Sums are plain left-to-right sums; the device reduces the gate's mean strided over 256 threads and then by a tree, within the
1e-7 dB the tests allow.  Not a test module: the r128 tests import it.
"""
from __future__ import annotations

import math

import numpy as np

import loudness_restated as lr

TAPS = 12


def factor(fs):
    return 8 if fs < 48000 else (4 if fs < 96000 else 2)


def filter_table(fs):
    """``(F, h float64 [F, 12])``: row p the taps of phase p, each row divided by its own sum; row 0 the unit impulse at tap 5."""
    F = factor(fs)
    h = np.zeros((F, TAPS), dtype=np.float64)
    h[0, 5] = 1.0
    for p in range(1, F):
        w = []
        for k in range(TAPS):
            d = float(k - 5) - float(p) / float(F)
            w.append(math.sin(math.pi * d) / (math.pi * d) * (0.5 * (1.0 + math.cos(math.pi * d / 6.0))))
        tot = 0.0
        for v in w:
            tot = tot + v
        h[p] = [v / tot for v in w]
    return F, h


def true_peak(x, fs, table=None):
    """The fp32 true peak of one row: ``table`` float32 [F, 12] (default: the restated one, rounded once).  Each product rounded to
    fp32, added in ascending tap order from 0; NaN samples and NaN sums are passed over (``np.fmax``)."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    if n == 0:
        return np.float32(0.0)
    h = np.asarray(filter_table(fs)[1] if table is None else table, dtype=np.float32)
    pad = np.concatenate([np.zeros(5, np.float32), x, np.zeros(6, np.float32)])
    win = np.lib.stride_tricks.sliding_window_view(pad, TAPS)         # win[j, k] = x[j - 5 + k]
    peak = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        peak = np.fmax(peak, np.fmax.reduce(np.abs(x), initial=np.float32(0.0)))
        for p in range(1, h.shape[0]):
            acc = np.zeros(n, dtype=np.float32)
            for k in range(TAPS):
                acc = acc + h[p, k] * win[:, k]
            peak = np.fmax(peak, np.fmax.reduce(np.abs(acc), initial=np.float32(0.0)))
    return np.float32(peak)


def percentile_indices(n):
    return (10 * (n - 1) + 50) // 100, (95 * (n - 1) + 50) // 100


def segments(x, fs):
    """The whole 100 ms segment energies of the K-weighted row, each a left-to-right sum, and the squares themselves."""
    y, _ = lr.cascade(np.asarray(x, dtype=np.float32), lr.coefficients(fs))
    sq = (y * y).tolist()
    seg_len = int(fs) // 10
    seg = []
    for s in range(len(sq) // seg_len):
        tot = 0.0
        for v in sq[s * seg_len:(s + 1) * seg_len]:
            tot = tot + v
        seg.append(tot)
    return seg, sq


def meter(x, fs, table=None):
    """``dict(lufs, peak, true_peak, lra, momentary_max, short_term_max, n, short, gate, margin)`` of one row: ``short`` the short-term
    loudnesses, ``n`` the blocks above both gates, ``margin`` the smallest distance in dB of a short-term block from either gate."""
    x32 = np.asarray(x, dtype=np.float32)
    n = len(x32)
    base = lr.measure(x32, fs)
    out = dict(lufs=base["lufs"], peak=base["peak"], true_peak=true_peak(x32, fs, table), lra=0.0, short_term_max=-math.inf, n=0, short=[],
               gate=-math.inf, margin=math.inf)
    out["momentary_max"] = max(base["blocks"]) if base["blocks"] else -math.inf
    seg_len = int(fs) // 10
    if n // seg_len < 30:
        return out
    seg, _ = segments(x32, fs)
    ms = []
    for k in range(len(seg) - 29):
        tot = 0.0
        for v in seg[k:k + 30]:
            tot = tot + v
        ms.append(tot / (30.0 * seg_len))
    l = [lr._db(v) for v in ms]
    out["short"] = l
    out["short_term_max"] = max(l)
    out["margin"] = min(abs(d + 70.0) for d in l)
    kept = [v for v, d in zip(ms, l) if d > -70.0]
    if not kept:
        return out
    gate = lr._db(sum(kept) / len(kept)) - 20.0
    out["gate"] = gate
    out["margin"] = min(out["margin"], min(abs(d - gate) for d in l))
    kept = sorted(v for v, d in zip(ms, l) if d > -70.0 and d > gate)
    out["n"] = len(kept)
    if kept:
        lo, hi = percentile_indices(len(kept))
        out["lra"] = lr._db(kept[hi]) - lr._db(kept[lo])
    return out


def ceiling_linear(dbtp):
    """The fp32 linear ceiling the device gets; NaN for none."""
    if dbtp is None or math.isnan(dbtp):
        return np.float32(math.nan)
    return np.float32(10.0 ** (float(np.float32(dbtp)) / 20.0))


def gain(lufs, target, peak, tp, dbtp, ceiling=0.95, n=1):
    """The fp32 gain with both ceilings: 1 when there is no target, the row is empty or ``lufs`` is not finite."""
    one = np.float32(1.0)
    if n == 0 or target is None or math.isnan(target) or not math.isfinite(lufs):
        return one
    target = float(np.float32(target))
    g = np.float32(10.0 ** ((target - lufs) / 20.0))
    for level, c in ((np.float32(peak), np.float32(ceiling)), (np.float32(tp), ceiling_linear(dbtp))):
        if not np.isnan(c) and level * g > c:
            g = c / level
            for _ in range(4):
                if level * g > c:
                    g = np.nextafter(g, np.float32(0.0))
    return g if np.isfinite(g) else one

"""NumPy / plain-Python fp64 restatement of include/mtts.h "loudness", sequential in plain sample order: the coefficients, the
two-biquad cascade, the 100 ms segments, the 400 ms blocks, the two gates and the gain.  Python floats are IEEE doubles and every
operation of the cascade is rounded once, as on the device (no FMA).  The sums are plain left-to-right sums in sample and block
order; the device adds per chunk, then chunks per segment, and reduces the block means strided over 256 threads and then by a
tree (include/mtts.h): the orders differ within the 1e-7 dB the tests allow (worst-case fp64 accumulation over 2^21 samples:
1e-9 dB).  Not a test module: the loudness tests import it.
"""
from __future__ import annotations

import math

import numpy as np


def coefficients(fs):
    """Ten words: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (bilinear transform of the analog prototype)."""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    k = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
         2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return k + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def cascade(x, k, state=(0.0, 0.0, 0.0, 0.0)):
    """The K-weighted signal of ``x`` (transposed direct form II, sample by sample) and the end state."""
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = k
    s1, s2, t1, t2 = state
    out = np.empty(len(x), dtype=np.float64)
    for i, v in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        y = b0 * v + s1
        s1 = (b1 * v - a1 * y) + s2
        s2 = b2 * v - a2 * y
        z = c0 * y + t1
        t1 = (c1 * y - d1 * z) + t2
        t2 = c2 * y - d2 * z
        out[i] = z
    return out, (s1, s2, t1, t2)


def chunk_of(fs, limit=256):
    w = int(fs) // 100
    return max(c for c in range(1, min(w, limit) + 1) if w % c == 0)


def _power(k, samples):
    """A^samples: column j is the state after ``samples`` zeros from the unit state e_j."""
    X = np.zeros((4, 4))
    for j in range(4):
        e = [0.0] * 4
        e[j] = 1.0
        X[:, j] = cascade(np.zeros(samples), k, tuple(e))[1]
    return X


def _affine(X, s, z):
    return tuple((((X[i, 0] * s[0] + X[i, 1] * s[1]) + X[i, 2] * s[2]) + X[i, 3] * s[3]) + z[i] for i in range(4))


def chunked_cascade(x, k, chunk, run=32):
    """The same signal by the device's scheme: zero-state end states z_c per chunk; the two-level scan of s[c + 1] = M s[c] + z[c]
    -- M = A^chunk, P = M^run; w_r the fold of the z_c over run r from zero, S_{r+1} = P S_r + w_r, chunk c entered with s that starts
    at S_r and becomes M s + z_c -- then every chunk again from its true entry state."""
    x = np.asarray(x, dtype=np.float64)
    M, P = _power(k, chunk), _power(k, chunk * run)
    pieces = [x[i:i + chunk] for i in range(0, len(x), chunk)]
    z = [cascade(p, k)[1] for p in pieces]
    zero = (0.0, 0.0, 0.0, 0.0)
    S, entry = zero, []
    for r in range(0, len(z), run):
        w = zero
        for i in range(run):
            w = _affine(M, w, z[r + i] if r + i < len(z) else zero)
        s = S
        for zc in z[r:r + run]:
            entry.append(s)
            s = _affine(M, s, zc)
        S = _affine(P, S, w)
    if not pieces:
        return np.zeros(0)
    return np.concatenate([cascade(p, k, st)[0] for p, st in zip(pieces, entry)])


def _db(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0.0 else (-math.inf if ms == 0.0 else math.nan)


def measure(x, fs):
    """``dict(lufs, peak, blocks, gate, margin)`` of one row: ``blocks`` the block loudnesses l_j, ``gate`` the relative gate,
    ``margin`` the smallest distance in dB of any block from either gate (inf when there is none to be near)."""
    x32 = np.asarray(x, dtype=np.float32)
    n = len(x32)
    peak = float(np.max(np.abs(x32))) if n else 0.0
    if n == 0:
        return dict(lufs=-math.inf, peak=0.0, blocks=[], gate=-math.inf, margin=math.inf)
    y, _ = cascade(x32, coefficients(fs))
    sq = (y * y).tolist()
    seg_len = int(fs) // 10
    nfull = n // seg_len
    if nfull < 4:                                    # one block of the row's own length (the documented deviation)
        tot = 0.0
        for v in sq:
            tot = tot + v
        l = _db(tot / n)
        return dict(lufs=l if l > -70.0 else -math.inf, peak=peak, blocks=[l], gate=-math.inf, margin=abs(l + 70.0))
    seg = []
    for s in range(nfull):
        tot = 0.0
        for v in sq[s * seg_len:(s + 1) * seg_len]:
            tot = tot + v
        seg.append(tot)
    ms = [(((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3]) / (4.0 * seg_len) for j in range(nfull - 3)]
    l = [_db(v) for v in ms]
    kept = [v for v, d in zip(ms, l) if d > -70.0]
    margin = min(abs(d + 70.0) for d in l)
    if not kept:
        return dict(lufs=-math.inf, peak=peak, blocks=l, gate=-math.inf, margin=margin)
    gate = _db(sum(kept) / len(kept)) - 10.0
    margin = min(margin, min(abs(d - gate) for d in l))
    kept = [v for v, d in zip(ms, l) if d > -70.0 and d > gate]
    lufs = _db(sum(kept) / len(kept)) if kept else -math.inf
    return dict(lufs=lufs, peak=peak, blocks=l, gate=gate, margin=margin)


def gain(lufs, target, peak, ceiling=0.95, n=1):
    """The fp32 gain of a row: 1 when there is no target, the row is empty or ``lufs`` is not finite."""
    one = np.float32(1.0)
    if n == 0 or target is None or math.isnan(target) or not math.isfinite(lufs):
        return one
    target = float(np.float32(target))
    g = np.float32(10.0 ** ((target - lufs) / 20.0))
    pk, c = np.float32(peak), np.float32(ceiling)
    if pk * g > c:
        g = c / pk
        for _ in range(4):
            if pk * g > c:
                g = np.nextafter(g, np.float32(0.0))
    return g if np.isfinite(g) else one

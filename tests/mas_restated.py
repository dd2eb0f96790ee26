"""NumPy restatement of Monotonic Alignment Search and its log-prior, written from the published algorithm (Kim et al. 2020,
Glow-TTS, algorithm 1) and the band / tie rule of include/mtts.h -- the yardstick of tests/test_mas_abi.py (against a brute-force
enumeration) and tests/test_hip_mas.py (against the device kernels, bit for bit)."""
import itertools

import numpy as np

NEG = np.float32(-1e9)


def maximum_path(lp, tx=None, tm=None):
    """lp [Tx, Tm] (token-major, any float dtype; computed in that dtype) -> (durations int32 [Tx], path [Tx, Tm] 0/1 float32, score).
    v[0][0] = lp[0][0]; v[x][y] = lp[x][y] + max(v[x][y-1], v[x-1][y-1]) for max(0, tx-(tm-y)) <= x <= min(y, tx-1), -1e9 outside.
    Back from (tx-1, tm-1): at frame y on token x step to x-1 iff x > 0 and (x == y or v[x-1][y-1] > v[x][y-1])."""
    lp = np.asarray(lp)
    dt = lp.dtype if lp.dtype in (np.float32, np.float64) else np.dtype(np.float32)
    lp = lp.astype(dt, copy=False)
    Tx, Tm = lp.shape
    tx = Tx if tx is None else int(tx)
    tm = Tm if tm is None else int(tm)
    assert 1 <= tx <= Tx and tx <= tm <= Tm
    neg = dt.type(-1e9)
    v = np.full((tx, tm), neg, dtype=dt)
    xs = np.arange(tx)
    for y in range(tm):
        inside = (xs >= max(0, tx - (tm - y))) & (xs <= min(y, tx - 1))
        if y == 0:
            col = np.where(xs == 0, lp[:tx, 0], neg).astype(dt)
        else:
            stay = v[:, y - 1]
            left = np.concatenate([[neg], v[:-1, y - 1]]).astype(dt)
            col = (lp[:tx, y] + np.maximum(stay, left)).astype(dt)
        v[:, y] = np.where(inside, col, neg)
    dur = np.zeros(Tx, dtype=np.int32)
    path = np.zeros((Tx, Tm), dtype=np.float32)
    x = tx - 1
    for y in range(tm - 1, -1, -1):
        path[x, y] = 1.0
        dur[x] += 1
        if y > 0 and x > 0 and (x == y or v[x - 1, y - 1] > v[x, y - 1]):
            x -= 1
    return dur, path, v[tx - 1, tm - 1]


def log_prior(mu_x, y):
    """mu_x [F, Tx], y [F, Tm] -> fp64 [Tx, Tm]: -0.5 |y|^2 + <mu, y> - 0.5 |mu|^2 (the diagonal-Gaussian log-likelihood of a
    unit-variance prior without its constant)."""
    mu = np.asarray(mu_x, dtype=np.float64)
    yy = np.asarray(y, dtype=np.float64)
    return -0.5 * (yy * yy).sum(0)[None, :] + mu.T @ yy - 0.5 * (mu * mu).sum(0)[:, None]


def brute_force(lp):
    """Every monotone path with >= 1 frame per token: (best score in the array's dtype summed in frame order, durations of the path
    the tie rule picks).  The tie rule's choice among equal-score paths: at every frame where two optimal prefixes meet, the one
    that stayed on the token wins, i.e. walking back the path leaves a token as late as it can -- among the optimal paths, the one
    whose durations are lexicographically largest read from the LAST token."""
    lp = np.asarray(lp)
    Tx, Tm = lp.shape
    best, best_d = None, None
    for cuts in itertools.combinations(range(1, Tm), Tx - 1):
        bounds = (0,) + cuts + (Tm,)
        d = [bounds[i + 1] - bounds[i] for i in range(Tx)]
        s = lp.dtype.type(0)
        for x in range(Tx):
            for yy in range(bounds[x], bounds[x + 1]):
                s = lp.dtype.type(s + lp[x, yy])
        key = tuple(reversed(d))
        if best is None or s > best or (s == best and key > tuple(reversed(best_d))):
            best, best_d = s, d
    return best, np.asarray(best_d, dtype=np.int32)


def expand(mu_x, dur):
    """mu_x [F, Tx] repeated dur[x] times along time -> [F, sum(dur)]."""
    return np.repeat(np.asarray(mu_x), np.asarray(dur, dtype=np.int64), axis=1)

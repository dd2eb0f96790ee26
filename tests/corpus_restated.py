"""NumPy restatements of the corpus-preparation entries (include/mtts.h "corpus preparation"), in the documented orders, and the
seeded clips of tests/golden/silence.npz.  Nothing here imports the library or the reference."""
import math

import numpy as np

LEAD_S, TRAIL_S = 0.2, 0.8          # the fixture's targets
CHUNK = 256                         # mtts_mel_stats_chunk()


def window(sr: int) -> int:
    return int(0.01 * sr)


def thresholds(*dbs):
    return tuple(np.float32(10.0 ** (db / 20.0)) for db in dbs)


# ---------------------------------------------------------------------------------------------------------------- clips
def clips(synthetic):
    """name -> (float32 waveform, sample rate).  Regenerated from seeds; at most 31 000 samples."""
    def noise(n, seed, amp=0.1):
        return (synthetic.portable_normal(seed, 9, n) * np.float32(amp)).astype(np.float32)

    def z(n):
        return np.zeros(n, dtype=np.float32)
    low = 3.0e-4                    # about -70 dB: between the two thresholds
    c = {
        "padded": (np.concatenate([z(2400), noise(12000, 1), z(4803)]), 24000),
        "tail_m70": (np.concatenate([noise(9600, 2), noise(4800, 3, low), z(2400)]), 24000),
        "low_both_ends": (np.concatenate([noise(2400, 4, low), noise(7200, 5), noise(3650, 6, low)]), 24000),
        "silent": (z(3000), 24000),
        "short": (noise(100, 7), 24000),
        "exact_multiple": (np.concatenate([z(1200), noise(6000, 8), z(2400)]), 24000),
        "ends_mid_window": (np.concatenate([z(1200), noise(4800 + 17, 9)]), 24000),
        "no_silence": (noise(7255, 10), 24000),
        "r44100": (np.concatenate([z(4410), noise(13230 + 100, 11), z(8827)]), 44100),
    }
    assert all(a.dtype == np.float32 and a.size <= 31000 for a, _ in c.values())
    return c


# ---------------------------------------------------------------------------------------------------------------- silence
def window_rms(x: np.ndarray, W: int) -> np.ndarray:
    """fp32 RMS of every window of x (the last partial one included) in the documented fp64 order: lane l of 64 adds the exact
    squares of samples e = VEC * (l + 64 k) + j in ascending order, then v[l] += v[l ^ o] for o = 32 .. 1."""
    x = np.asarray(x, dtype=np.float32)
    L = x.size
    n_win = -(-L // W)
    vec = 4 if W % 4 == 0 else 1
    per = 64 * vec
    rounds = -(-W // per)
    sq = np.zeros((n_win, rounds * per), dtype=np.float64)           # samples that do not exist add nothing: s + 0.0 == s
    pad = np.zeros(n_win * W, dtype=np.float64)
    pad[:L] = x.astype(np.float64)
    sq[:, :W] = (pad * pad).reshape(n_win, W)
    lanes = sq.reshape(n_win, rounds, 64, vec)
    v = np.zeros((n_win, 64), dtype=np.float64)
    for k in range(rounds):
        for j in range(vec):
            v = v + lanes[:, k, :, j]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ o]
    return np.sqrt(v[:, 0] / float(W)).astype(np.float32)


def _run(flags) -> int:
    n = 0
    for f in flags:
        if not f:
            break
        n += 1
    return n


def measure(x, sr: int, effective_db: float = -60.0, absolute_db: float = -90.0, rms=None):
    """The six columns of mtts_silence_measure, in samples."""
    W = window(sr)
    L = len(x)
    rms = window_rms(x, W) if rms is None else rms
    te, ta = thresholds(effective_db, absolute_db)
    active = np.nonzero(rms >= te)[0]
    if active.size:
        cs, ce = int(active[0]) * W, min((int(active[-1]) + 1) * W, L)
    else:
        cs, ce = 0, 0
    be, ba = rms < te, rms < ta
    return [cs, ce, _run(be) * W, _run(ba) * W, _run(be[::-1]) * W, _run(ba[::-1]) * W]


def rebuild(x, cs: int, ce: int, lead: int, trail: int):
    """mtts_silence_normalize of one clip: (row, changed).  lead / trail in samples, -1 keeps that end."""
    x = np.asarray(x, dtype=np.float32)
    L = x.size
    lead_ok = lead < 0 or cs == lead
    trail_ok = trail < 0 or (L - ce) == trail
    if lead_ok and trail_ok:
        return x.copy(), 0
    head = x[:cs] if lead < 0 else np.zeros(lead, dtype=np.float32)
    tail = x[ce:] if trail < 0 else np.zeros(trail, dtype=np.float32)
    return np.concatenate([head, x[cs:ce], tail]), 1


def samples(seconds, sr: int) -> int:
    return -1 if seconds is None else int(round(seconds * sr))


def normalize(x, sr: int, leading=LEAD_S, trailing=TRAIL_S, threshold_db: float = -60.0):
    cs, ce = measure(x, sr, threshold_db, threshold_db)[:2]
    out, changed = rebuild(x, cs, ce, samples(leading, sr), samples(trailing, sr))
    return out, changed, (cs, ce)


# ---------------------------------------------------------------------------------------------------------------- mel sums
def mel_sums(mel: np.ndarray, n: int):
    """(sum x, sum x^2, non-finite flag) of mel [F, T] over t < n in the documented order."""
    mel = np.asarray(mel, dtype=np.float32)
    F = mel.shape[0]
    s_tot, q_tot, flag = np.float64(0.0), np.float64(0.0), False
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for c in range(-(-n // CHUNK)):
            x = np.zeros((F, CHUNK), dtype=np.float64)
            hi = min(n, (c + 1) * CHUNK)
            x[:, :hi - c * CHUNK] = mel[:, c * CHUNK:hi].astype(np.float64)
            flag = flag or not np.isfinite(x).all()
            s, q = np.zeros(CHUNK), np.zeros(CHUNK)
            for f in range(F):
                s = s + x[f]
                q = q + x[f] * x[f]
            part = []
            for v in (s, q):
                v = v.reshape(4, 64)
                for o in (32, 16, 8, 4, 2, 1):
                    v = v + v[:, idx ^ o]
                part.append(((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])
            s_tot, q_tot = s_tot + part[0], q_tot + part[1]
    return float(s_tot), float(q_tot), bool(flag)


def fsum_sums(mel: np.ndarray, n: int):
    """Correctly rounded sums (math.fsum) and the sums of magnitudes, for the error bound n * 2^-53 * sum |x|."""
    v = np.asarray(mel, dtype=np.float32)[:, :n].astype(np.float64).ravel()
    return math.fsum(v), math.fsum(v * v), float(np.abs(v).sum()), float((v * v).sum()), v.size


def statistics(total_sum: float, total_sq: float, frames: int, n_mels: int):
    """generate_data_statistics.py:151-152 in fp64."""
    count = frames * n_mels
    mean = total_sum / count
    return float(mean), float(np.sqrt((total_sq / count) - (mean ** 2)))

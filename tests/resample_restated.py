"""NumPy restatement of the sample-rate conversion (include/mtts.h "sample-rate conversion"): the windowed-sinc polyphase
interpolation torchaudio.functional.resample documents as its default (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99),
written from its formulae.  Helper for tests/test_resample_abi.py and tests/test_hip_resample.py; not collected."""
import math
from math import gcd

import numpy as np


def factors(orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99):
    """(o, n, width, taps)."""
    g = gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    return o, n, width, 2 * width + o


def bank64(orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99) -> np.ndarray:
    """K [n, taps] in fp64.  Element by element with the C library's sin / cos (``math``), in the order the formula is written:
    NumPy's vectorised transcendental functions may differ from them in the last bit."""
    o, n, width, taps = factors(orig_freq, new_freq, lpw, rolloff)
    base = float(min(o, n)) * rolloff
    scale = base / float(o)
    K = np.zeros((n, taps), dtype=np.float64)
    for p in range(n):
        for k in range(taps):
            t = (-float(p) / float(n) + float(k - width) / float(o)) * base
            t = -float(lpw) if t < -lpw else (float(lpw) if t > lpw else t)
            c = math.cos(t * math.pi / float(lpw) / 2.0)
            a = t * math.pi
            sinc = 1.0 if t == 0.0 else math.sin(a) / a
            K[p, k] = sinc * (c * c) * scale
    return K


def bank32(orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99) -> np.ndarray:
    """The definition: the fp64 bank rounded once to fp32."""
    return bank64(orig_freq, new_freq, lpw, rolloff).astype(np.float32)


def band_of(K32: np.ndarray) -> int:
    """The widest first-to-last non-zero run of any phase."""
    band = 1
    for row in K32:
        nz = np.flatnonzero(row)
        if nz.size:
            band = max(band, int(nz[-1] - nz[0] + 1))
    return band


def out_length(L: int, o: int, n: int) -> int:
    return (n * int(L) + o - 1) // o


def _gather(x: np.ndarray, o: int, n: int, width: int, taps: int):
    """(q, p, X [out_len, taps]): X[j, k] = x[q_j * o + k - width], zero outside the clip."""
    L = x.shape[0]
    m = out_length(L, o, n)
    j = np.arange(m, dtype=np.int64)
    q, p = j // n, j % n
    idx = q[:, None] * o + np.arange(taps, dtype=np.int64)[None, :] - width
    ok = (idx >= 0) & (idx < L)
    X = np.where(ok, x[np.clip(idx, 0, max(L - 1, 0))] if L else 0.0, 0.0).astype(x.dtype)
    return q, p, X


def resample64(x: np.ndarray, K32: np.ndarray, o: int, n: int, width: int):
    """Dense fp64 evaluation with the fp32 bank: ``(out, mag)`` with mag[j] = sum_k |K[p][k] * x[.]| (the error bound's scale)."""
    x = np.asarray(x, dtype=np.float64)
    taps = K32.shape[1]
    if x.shape[0] == 0:
        return np.zeros(0), np.zeros(0)
    _, p, X = _gather(x, o, n, width, taps)
    prod = K32.astype(np.float64)[p] * X
    return prod.sum(1), np.abs(prod).sum(1)


def resample32(x: np.ndarray, K32: np.ndarray, o: int, n: int, width: int) -> np.ndarray:
    """The kernel's documented arithmetic: per output one serial fp32 chain, s = 0, then s = fl(s + fl(K[p][k] * x[.])) for k
    ascending.  Dense over k = 0 .. taps - 1: the terms outside a phase's band are products with an exact zero and leave s
    unchanged, so this has the bits of the banded sum the kernel runs."""
    x = np.asarray(x, dtype=np.float32)
    taps = K32.shape[1]
    if x.shape[0] == 0:
        return np.zeros(0, dtype=np.float32)
    _, p, X = _gather(x, o, n, width, taps)
    Kp = K32[p]
    s = np.zeros(X.shape[0], dtype=np.float32)
    for k in range(taps):
        s = (s + (Kp[:, k] * X[:, k]).astype(np.float32)).astype(np.float32)
    return s

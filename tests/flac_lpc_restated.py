"""The LPC side of FLAC out restated in NumPy, for the tests of ``mtts_flac_encode_lpc``: ``encode`` is the encoder to the rules of
include/mtts.h "FLAC out", "lpc" paragraphs, bit for bit what the device writes.  The stream header, the frame header, the Rice
coding and the FIXED / CONSTANT / VERBATIM subframes are those of tests/flac_restated.py, imported; the analysis (integer window,
exact autocorrelation, Levinson-Durbin in one fp64 operation order, quantisation from the exponent field, integer prediction) is
written out here.  No decoder: tests/flac_in_restated.py reads LPC subframes already.  The module also holds the signals and
shapes of the CPU and GPU tests, so that both run the same cases."""
import importlib.util
from pathlib import Path

import numpy as np

import flac_restated as fr

MAX_ORDER = 12
LIST = (4, 8, 12)                                                  # the candidate orders, before the caps
PRECISION = 12
KINDS = fr.KINDS + ("LPC",)


# ------------------------------------------------------------------------------------------------ the analysis
def candidates(max_order: int, n: int):
    """The LPC orders tried on a frame of n samples: each listed order capped at ``max_order``, once each, ascending, below n."""
    return sorted({min(o, max_order) for o in LIST if 1 <= min(o, max_order) < n})


def window(n: int):
    i = np.arange(n, dtype=np.int64)
    return 255 - (255 * (2 * i + 1 - n) ** 2) // (n * n)


def autocorrelation(q, lags: int):
    """R[0..lags] of the windowed words, exact in int64."""
    x = np.asarray(q, dtype=np.int64) * window(len(q))
    return [int(np.dot(x[:len(x) - l], x[l:])) for l in range(lags + 1)]


def levinson(R, top: int):
    """``{m: [a_1..a_m]}`` for the orders 1..top the recursion reaches: fp64, the one operation order of the contract.  It stops at the
    first order whose error is not a positive finite number; that order and those above are absent."""
    R = [np.float64(r) for r in R]
    out, a, err = {}, [], R[0]
    if not (err > 0 and np.isfinite(err)):
        return out
    with np.errstate(all="ignore"):
        for m in range(1, top + 1):
            acc = R[m]
            for j in range(1, m):
                acc = acc - a[j - 1] * R[m - j]
            k = acc / err
            a = [a[j - 1] - k * a[m - j - 1] for j in range(1, m)] + [k]
            err = err * (np.float64(1.0) - k * k)
            if not (err > 0 and np.isfinite(err)):
                break
            out[m] = a
    return out


def quantise(a):
    """``(shift, [c_0..c_{m-1}])`` of fp64 coefficients at precision 12, or None when the shift would be negative.  e, with
    max|a| < 2^e, is the biased exponent field - 1022 (so zero and subnormals give the cap, infinities and NaN a negative shift)."""
    cmax = np.float64(max(abs(v) for v in a))
    e = int((np.array([cmax]).view(np.int64)[0] >> 52) & 0x7FF) - 1022
    shift = min(15, PRECISION - 1 - e)
    if shift < 0:
        return None
    lo, hi = -(1 << (PRECISION - 1)), (1 << (PRECISION - 1)) - 1
    return shift, [int(min(max(np.rint(v * np.float64(1 << shift)), lo), hi)) for v in a]     # (rint: ties to even)


def lpc_residual(q, c, shift):
    """q[i] - ((sum_j c[j] q[i-1-j]) >> shift) for i >= len(c); zeros before.  The sum stays inside 32 bits (12 taps of 12 bits on
    16-bit words: 12 * 2^11 * 2^15 < 2^31)."""
    q = np.asarray(q, dtype=np.int64)
    m, r = len(c), np.zeros(len(q), dtype=np.int64)
    s = np.zeros(len(q) - m, dtype=np.int64)
    for j in range(m):
        s += c[j] * q[m - 1 - j:len(q) - 1 - j]
    r[m:] = q[m:] - (s >> shift)
    return r


def _residual_section(r, order, n, bs):
    """The bits of the residual of a FIXED or LPC subframe, as tests/flac_restated.py ``subframe`` writes them."""
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    po = int(np.log2(bs // 256)) if n == bs else 0
    parts = [(max(p * 256, order), (p + 1) * 256) for p in range(1 << po)] if n == bs else [(order, n)]
    pieces = [fr._bits_of([0, po], [2, 4])]
    for a, b in parts:
        k, bits = fr._rice_partition(u[a:b])
        pieces += [fr._bits_of([k], [4]), bits]
    return np.concatenate(pieces)


def lpc_subframe(q, bs, order, shift, c):
    """The bits of an LPC subframe, or None when a residual leaves (-2^20, 2^20)."""
    q = np.asarray(q, dtype=np.int64)
    r = lpc_residual(q, c, shift)
    if np.abs(r).max() >= 1 << 20:
        return None
    head = fr._bits_of([0x40 | (order - 1) << 1], [8])
    warm = fr._bits_of(q[:order] & 0xFFFF, [16] * order)
    coef = fr._bits_of(np.asarray(c) & 0xFFF, [PRECISION] * order)
    return np.concatenate([head, warm, fr._bits_of([PRECISION - 1, shift], [4, 5]), coef, _residual_section(r, order, len(q), bs)])


def subframe(q, bs, max_order):
    """``(kind, order, bits)`` of one block: CONSTANT first; the shortest of FIXED and the LPC candidates, ties to FIXED and then to
    the lower order; VERBATIM when that is not shorter."""
    q = np.asarray(q, dtype=np.int64)
    n = len(q)
    kind, order, bits = fr.subframe(q, bs)
    cands = candidates(max_order, n)
    if kind == "CONSTANT" or not cands:
        return kind, order, bits
    best = len(bits)                                               # (8 + 16 n where FIXED gave way to VERBATIM: the bound of a candidate)
    coefs = levinson(autocorrelation(q, cands[-1]), cands[-1])
    for m in cands:
        if m not in coefs:
            break
        qc = quantise(coefs[m])
        if qc is None:
            continue
        got = lpc_subframe(q, bs, m, *qc)
        if got is not None and len(got) < best:
            kind, order, bits, best = "LPC", m, got, len(got)
    return kind, order, bits


def encode_frame(q, f, rate, bs, max_order):
    head = fr.encode_frame(q, f, rate, bs)[0]
    kind, o, bits = subframe(q, bs, max_order)
    hb = 4 + len(fr.frame_number(f)) + (0 if len(q) == bs else 1 if len(q) <= 256 else 2) + len(fr.rate_code(rate)[1]) + 1
    body = head[:hb] + np.packbits(bits).tobytes()
    return body + fr.crc16(body).to_bytes(2, "big"), kind, o


def encode(q, rate, bs=4096, max_order=MAX_ORDER, info=None) -> bytes:
    """The stream of int16 words ``q`` with LPC orders up to ``max_order`` (0: ``flac_restated.encode``'s bytes).  ``info``: a list that
    receives ``(kind, order, bytes)`` per frame."""
    if isinstance(max_order, bool) or not 0 <= int(max_order) <= MAX_ORDER:
        raise ValueError("max_order lies in 0..12")
    q = np.asarray(q, dtype=np.int64)
    if bs not in fr.BLOCK_SIZES or not 1 <= rate <= 1048575 or q.ndim != 1:
        raise ValueError("bad block size, rate or samples")
    frames = []
    for f in range((len(q) + bs - 1) // bs):
        data, kind, o = encode_frame(q[f * bs:(f + 1) * bs], f, rate, bs, int(max_order))
        frames.append(data)
        if info is not None:
            info.append((kind, o, len(data)))
    sizes = [len(d) for d in frames] or [0]
    v = bs << 256 | bs << 240 | min(sizes) << 216 | max(sizes) << 192 | rate << 172 | 0 << 169 | 15 << 164 | len(q) << 128
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(34, "big") + b"".join(frames)


# ------------------------------------------------------------------------------------------------ the cases of the tests
BLOCK_SIZES = (256, 4096)
LENGTHS = (0, 1, 12, 13, 255, 256, 257, 4096 + 5, 2 * 4096)
SIGNALS = ("speech", "constant", "impulse", "alternating", "white", "sine200", "ramp", "fade")
MAX_ORDERS = (1, 8, 12)
RATES = (24000, 8000, 11025, 100000)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parent.parent / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_speech = {}


def speech_like(n, seed=7):
    """The int16 words of the first row of tools/flac_time.py's ``speech_like(1, n, seed)``."""
    if (n, seed) not in _speech:
        x = _tool("flac_time").speech_like(1, n, seed)[0].numpy().astype(np.float64)
        _speech[n, seed] = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int64)
    return _speech[n, seed]


def signal(name, n):
    """n int16 words (int64) of one of SIGNALS; every word is exact in fp32 as word / 32768."""
    i = np.arange(n)
    if name == "speech":
        return speech_like(2 * 4096)[:n].copy()
    if name == "constant":
        return np.full(n, 321, dtype=np.int64)
    if name == "impulse":
        return np.where(i == n // 3, 32767, 0).astype(np.int64)
    if name == "alternating":
        return np.where(i % 2 == 0, 32767, -32767).astype(np.int64)
    if name == "white":
        return np.clip(np.rint(0.5 * 32768 * np.random.default_rng(n).uniform(-1, 1, n)), -32768, 32767).astype(np.int64)
    if name == "sine200":
        return np.clip(np.rint(32767 * np.sin(2 * np.pi * 200 * i / 24000.0)), -32768, 32767).astype(np.int64)
    if name == "ramp":
        return (3 * i - 9000).astype(np.int64)
    if name == "fade":                                             # a sinusoid under a linear fade that reaches exact zeros at 40 % of the row
        gain = np.clip(1.0 - i / max(0.4 * n, 1.0), 0.0, 1.0)
        return np.rint(12000 * gain * np.sin(2 * np.pi * 440 * i / 24000.0)).astype(np.int64)
    raise ValueError(name)


def cases():
    """``[(signal name, n, words, rate)]``: every signal at every length, the rates in turn."""
    return [(name, n, signal(name, n), RATES[(j + k) % len(RATES)]) for j, name in enumerate(SIGNALS) for k, n in enumerate(LENGTHS)]

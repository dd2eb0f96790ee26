"""NumPy restatement of the encoded-audio arithmetic (include/mtts.h "encoded audio"), written from its definitions and not from the
kernel: the quantiser q = clamp(rint(x * 32768 [+ d])), ITU-T G.711 companding in integer operations, both decoders, and the
counter-based dither hash.  The tests hold the kernels, and this file itself (against ``audioop``), to it bit for bit."""
import numpy as np

PCM16, ULAW, ALAW = 0, 1, 2
BYTES = {PCM16: 2, ULAW: 1, ALAW: 1}
NAMES = {"pcm16": PCM16, "ulaw": ULAW, "alaw": ALAW}
M32 = np.uint64(0xFFFFFFFF)


def fmix(h):
    """murmur3's 32-bit finaliser on uint32 values (held in uint64 so that the products do not overflow NumPy's checks)."""
    h = np.asarray(h, dtype=np.uint64) & M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def words(v):
    """(low, high) 32 bits of an int64 given as a Python int."""
    u = int(v) & 0xFFFFFFFFFFFFFFFF
    return np.uint64(u & 0xFFFFFFFF), np.uint64(u >> 32)


def dither_hash(seed, key, index, stream):
    """h of (seed, key, sample index within the row, stream 0 or 1): uint32 values as a uint64 array shaped like ``index``."""
    s_lo, s_hi = words(seed)
    k_lo, k_hi = words(key)
    h = fmix(np.uint64(0x9E3779B9) ^ s_lo)
    h = fmix(h ^ s_hi)
    h = fmix(h ^ k_lo)
    h = fmix(h ^ k_hi)
    i = np.asarray(index, dtype=np.uint64)
    return fmix(h ^ ((np.uint64(2) * i + np.uint64(stream)) & M32))


def dither(seed, key, n):
    """The TPDF sequence d[0 .. n) of a row: u1 - u2 in fp32 with u = (h >> 8) * 2^-24."""
    i = np.arange(n, dtype=np.uint64)
    u1 = (dither_hash(seed, key, i, 0) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (dither_hash(seed, key, i, 1) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u1 - u2).astype(np.float32)


def quantise(x, d=None):
    """q of fp32 samples: y = x * 32768 (+ d, one fp32 add), rint with ties to even, clamp, NaN -> 0.  int32 values."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(x, dtype=np.float32) * np.float32(32768.0)
        if d is not None:
            y = (y + np.asarray(d, dtype=np.float32)).astype(np.float32)
        r = np.clip(np.rint(y), np.float32(-32768.0), np.float32(32767.0))
    return np.where(np.isnan(y), np.float32(0.0), r).astype(np.int32)


def segment(v, e0):
    """The number of i in [0, 8) with v > (e0 << i) - 1."""
    return sum((v > (e0 << i) - 1).astype(np.int32) for i in range(8))


def lin2ulaw(q):
    q = np.asarray(q, dtype=np.int32)
    v = q >> 2
    neg = v < 0
    mask = np.where(neg, 0x7F, 0xFF)
    v = np.minimum(np.where(neg, -v, v), 8159) + 33
    s = segment(v, 0x40)
    code = np.where(s == 8, 0x7F, (s << 4) | ((v >> np.minimum(s + 1, 9)) & 15))
    return ((code ^ mask) & 0xFF).astype(np.uint8)


def lin2alaw(q):
    q = np.asarray(q, dtype=np.int32)
    v = q >> 3
    neg = v < 0
    mask = np.where(neg, 0x55, 0xD5)
    v = np.where(neg, -v - 1, v)
    s = segment(v, 0x20)
    code = np.where(s == 8, 0x7F, (s << 4) | ((v >> np.where(s < 2, 1, s)) & 15))
    return ((code ^ mask) & 0xFF).astype(np.uint8)


def ulaw2lin(codes):
    c = (~np.asarray(codes, dtype=np.uint8)).astype(np.int32) & 0xFF
    t = (((c & 15) << 3) + 132) << ((c >> 4) & 7)
    return np.where(c & 0x80, 132 - t, t - 132).astype(np.int32)


def alaw2lin(codes):
    c = (np.asarray(codes, dtype=np.uint8).astype(np.int32) ^ 0x55) & 0xFF
    s = (c >> 4) & 7
    t = (c & 15) << 4
    t = np.where(s == 0, t + 8, (t + 0x108) << np.maximum(s - 1, 0))
    return np.where(c & 0x80, t, -t).astype(np.int32)


def encode(x, fmt, dither_on=False, seed=0, key=0):
    """The bytes of one row of fp32 samples (uint8 array): s16le, or one G.711 code per sample of the undithered q."""
    x = np.asarray(x, dtype=np.float32)
    if fmt == PCM16:
        q = quantise(x, dither(seed, key, x.shape[0]) if dither_on else None)
        return q.astype("<i2").view(np.uint8)
    q = quantise(x)
    return lin2ulaw(q) if fmt == ULAW else lin2alaw(q)


def decode(data, fmt):
    """fp32 samples of one row's bytes: the 16-bit value (the word, or the G.711 linear value) / 32768."""
    data = np.asarray(data, dtype=np.uint8)
    if fmt == PCM16:
        v = data[: data.shape[0] // 2 * 2].view("<i2").astype(np.int32)
    else:
        v = ulaw2lin(data) if fmt == ULAW else alaw2lin(data)
    return (v.astype(np.float32) / np.float32(32768.0)).astype(np.float32)

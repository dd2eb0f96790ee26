"""FLAC (RFC 9639) restated twice, for the tests of ``mtts_flac_encode``: ``encode`` is the project's encoder to the rules of
include/mtts.h "FLAC out" in NumPy, bit for bit what the device writes; ``decode`` is a reader of general FLAC of the subset a check
needs -- CONSTANT, VERBATIM and FIXED subframes, wasted bits, independent channels, every block-size and rate code, both Rice
methods with their escapes -- written from the RFC and anchored to its first example file.  The two share nothing but the two CRC
functions, which have known answers of their own."""
import numpy as np

BLOCK_SIZES = (256, 512, 1024, 2048, 4096)
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
KINDS = ("CONSTANT", "VERBATIM", "FIXED")


# ------------------------------------------------------------------------------------------------ the CRCs (shared)
def _crc_table(poly, width):
    top, mask, table = 1 << (width - 1), (1 << width) - 1, []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data) -> int:
    c = 0
    for b in bytes(data):
        c = _T8[c ^ b]
    return c


def crc16(data) -> int:
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


# ------------------------------------------------------------------------------------------------ the encoder (the project's rules)
def frame_number(v: int) -> bytes:
    """The RFC's UTF-8-like coding of a frame number below 2^21: 1 to 4 bytes."""
    if v < 0x80:
        return bytes([v])
    if v < 0x800:
        return bytes([0xC0 | v >> 6, 0x80 | v & 63])
    if v < 0x10000:
        return bytes([0xE0 | v >> 12, 0x80 | (v >> 6) & 63, 0x80 | v & 63])
    if v < 0x200000:
        return bytes([0xF0 | v >> 18, 0x80 | (v >> 12) & 63, 0x80 | (v >> 6) & 63, 0x80 | v & 63])
    raise ValueError("a row of more than 2^21 frames is refused")


def rate_code(rate: int):
    """``(4-bit code, tail bytes)`` of a sample rate, first match."""
    if rate in RATE_CODES:
        return RATE_CODES[rate], b""
    if rate <= 65535:
        return 13, rate.to_bytes(2, "big")
    if rate % 10 == 0 and rate // 10 <= 65535:
        return 14, (rate // 10).to_bytes(2, "big")
    return 0, b""


def _bits_of(values, widths):
    """The bits (uint8 0/1) of ``values[i]`` in ``widths[i]`` bits each, MSB first, back to back."""
    values, widths = np.asarray(values, dtype=np.int64), np.asarray(widths, dtype=np.int64)
    ends = np.cumsum(widths)
    out = np.zeros(int(ends[-1]) if len(ends) else 0, dtype=np.uint8)
    for j in range(int(widths.max()) if len(widths) else 0):       # bit j counted from the LSB, of the values that have one
        has = widths > j
        out[ends[has] - 1 - j] = (values[has] >> j) & 1
    return out


def _rice_partition(u):
    """``(k, bits)`` of one partition's folded residuals: k in 0..14 with the fewest bits, ties to the smaller."""
    u = u.astype(np.int64)
    cost = [len(u) * (k + 1) + int((u >> k).sum()) for k in range(15)]
    k = int(np.argmin(cost))                                       # (the first minimum)
    quo = u >> k
    starts = np.cumsum(quo + 1 + k) - (quo + 1 + k)
    bits = np.zeros(cost[k], dtype=np.uint8)
    bits[starts + quo] = 1
    for j in range(k):                                             # remainder bit j from its MSB
        bits[starts + quo + 1 + j] = (u >> (k - 1 - j)) & 1
    return k, bits


def subframe(q, bs):
    """``(kind, order, bits)`` of one block of int samples ``q`` (n of them) in a stream of block size ``bs``."""
    q = np.asarray(q, dtype=np.int64)
    n = len(q)
    word = lambda v: _bits_of(np.asarray(v) & 0xFFFF, [16] * np.size(v))
    if np.all(q == q[0]):
        return "CONSTANT", 0, np.concatenate([_bits_of([0], [8]), word([q[0]])])
    diffs = [q]
    for _ in range(4):
        d = np.zeros(n, dtype=np.int64)
        d[1:] = diffs[-1][1:] - diffs[-1][:-1]
        diffs.append(d)
    costs = [int(np.abs(e[4:]).sum()) for e in diffs]              # (empty for n <= 4: all 0, the tie goes to order 0)
    o = int(np.argmin(costs))
    r = diffs[o]
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    po = int(np.log2(bs // 256)) if n == bs else 0
    parts = [(max(p * 256, o), (p + 1) * 256) for p in range(1 << po)] if n == bs else [(o, n)]
    pieces = [_bits_of([0x10 | o << 1], [8]), word(q[:o]), _bits_of([0, po], [2, 4])]
    for a, b in parts:
        k, bits = _rice_partition(u[a:b])
        pieces += [_bits_of([k], [4]), bits]
    bits = np.concatenate(pieces)
    if len(bits) >= 8 + 16 * n:
        return "VERBATIM", 0, np.concatenate([_bits_of([2], [8]), word(q)])
    return "FIXED", o, bits


def encode_frame(q, f, rate, bs):
    """``(frame bytes, kind, order)`` of frame ``f`` holding the samples ``q``."""
    n = len(q)
    if n == bs:
        bcode, btail = 8 + BLOCK_SIZES.index(bs), b""
    elif n <= 256:
        bcode, btail = 6, bytes([n - 1])
    else:
        bcode, btail = 7, (n - 1).to_bytes(2, "big")
    rcode, rtail = rate_code(rate)
    head = bytes([0xFF, 0xF8, bcode << 4 | rcode, 0x08]) + frame_number(f) + btail + rtail
    head += bytes([crc8(head)])
    kind, o, bits = subframe(q, bs)
    body = head + np.packbits(bits).tobytes()                      # (packbits pads the last byte with zeros)
    return body + crc16(body).to_bytes(2, "big"), kind, o


def encode(q, rate, bs=4096, info=None) -> bytes:
    """The stream of int16 words ``q`` at ``rate`` Hz with block size ``bs``.  ``info``: a list that receives ``(kind, order, bytes)``
    per frame."""
    q = np.asarray(q, dtype=np.int64)
    if bs not in BLOCK_SIZES or not 1 <= rate <= 1048575 or q.ndim != 1:
        raise ValueError("bad block size, rate or samples")
    frames = []
    for f in range((len(q) + bs - 1) // bs):
        data, kind, o = encode_frame(q[f * bs:(f + 1) * bs], f, rate, bs)
        frames.append(data)
        if info is not None:
            info.append((kind, o, len(data)))
    sizes = [len(d) for d in frames] or [0]
    v = bs << 256 | bs << 240 | min(sizes) << 216 | max(sizes) << 192 | rate << 172 | 0 << 169 | 15 << 164 | len(q) << 128
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(34, "big") + b"".join(frames)


# ------------------------------------------------------------------------------------------------ the decoder (from the RFC)
class _Reader:
    def __init__(self, data: bytes, at: int = 0):
        self.s = bin(int.from_bytes(b"\x01" + data, "big"))[3:]    # '0' / '1' per bit, leading zeros kept
        self.p = 8 * at

    def u(self, n: int) -> int:
        if self.p + n > len(self.s):
            raise ValueError("truncated FLAC stream")
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v

    def i(self, n: int) -> int:
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self) -> int:
        e = self.s.find("1", self.p)
        if e < 0:
            raise ValueError("truncated FLAC stream (unary run)")
        v, self.p = e - self.p, e + 1
        return v


def _residual(rd, n, order):
    method = rd.u(2)
    if method > 1:
        raise ValueError("reserved residual coding method")
    pbits, po = 4 + method, rd.u(4)
    if n % (1 << po) or (n >> po) < order:
        raise ValueError("the partition order does not fit the block")
    out = []
    for p in range(1 << po):
        cnt = (n >> po) - (order if p == 0 else 0)
        k = rd.u(pbits)
        if k == (1 << pbits) - 1:                                  # escape: raw two's-complement words
            raw = rd.u(5)
            out += [rd.i(raw) for _ in range(cnt)]
        else:
            for _ in range(cnt):
                v = rd.unary() << k | rd.u(k)
                out.append(v >> 1 if not v & 1 else -(v >> 1) - 1)
    return out


def _subframe(rd, n, bps):
    if rd.u(1):
        raise ValueError("subframe padding bit set")
    kind = rd.u(6)
    wasted = rd.unary() + 1 if rd.u(1) else 0
    bps -= wasted
    if kind == 0:
        x, name, order = [rd.i(bps)] * n, "CONSTANT", 0
    elif kind == 1:
        x, name, order = [rd.i(bps) for _ in range(n)], "VERBATIM", 0
    elif 8 <= kind <= 12:
        order, name = kind - 8, "FIXED"
        x = [rd.i(bps) for _ in range(order)]
        coef = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))[order]
        for r in _residual(rd, n, order):
            x.append(r + sum(c * x[-1 - j] for j, c in enumerate(coef)))
    else:
        raise ValueError(f"subframe type {kind:06b} is outside the subset read here (LPC or reserved)")
    return [v << wasted for v in x], name, order


def decode(data: bytes) -> dict:
    """A FLAC stream -> ``{"rate", "channels", "bps", "total", "block_sizes": (min, max), "frame_sizes": (min, max), "md5",
    "samples": int64 [channels, total], "frames": [{"n", "number", "bytes", "rate", "kinds": [(kind, order) per channel]}]}``.
    Every CRC is checked, and so is the sample count against STREAMINFO's; ``ValueError`` for anything else."""
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise ValueError("no fLaC marker")
    at, info = 4, None
    while True:
        if at + 4 > len(data):
            raise ValueError("truncated metadata")
        last, kind, size = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        if kind == 0:
            if size != 34 or at + 4 + 34 > len(data):
                raise ValueError("STREAMINFO has 34 bytes")
            rd = _Reader(data, at + 4)
            info = {"block_sizes": (rd.u(16), rd.u(16)), "frame_sizes": (rd.u(24), rd.u(24)), "rate": rd.u(20), "channels": rd.u(3) + 1,
                    "bps": rd.u(5) + 1, "total": rd.u(36), "md5": data[at + 22:at + 38].hex()}
        at += 4 + size
        if last:
            break
    if info is None:
        raise ValueError("no STREAMINFO block")
    chans, frames, rd = [[] for _ in range(info["channels"])], [], _Reader(data)
    while at < len(data):
        rd.p = 8 * at
        if rd.u(15) != 0x7FFC:
            raise ValueError(f"no frame sync at byte {at}")
        variable, bcode, rcode, assign, scode = rd.u(1), rd.u(4), rd.u(4), rd.u(4), rd.u(3)
        if rd.u(1) or bcode == 0 or rcode == 15 or scode == 3 or assign > 7:
            raise ValueError("reserved frame header value, or a stereo decorrelation mode (not read here)")
        lead = rd.u(8)
        if 0x80 <= lead < 0xC0 or lead == 0xFF:
            raise ValueError("bad coded number")
        extra = 0 if lead < 0x80 else next(j for j in range(1, 7) if not lead >> (6 - j) & 1)
        number = lead if lead < 0x80 else lead & (0x3F >> extra)
        for _ in range(extra):
            cont = rd.u(8)
            if cont >> 6 != 2:
                raise ValueError("bad coded number")
            number = number << 6 | cont & 63
        n = {1: 192, 6: None, 7: None}.get(bcode, 144 << bcode if 2 <= bcode <= 5 else 1 << bcode)
        if bcode in (6, 7):
            n = rd.u(8 if bcode == 6 else 16) + 1
        rate = ([info["rate"], 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000] + [None] * 3)[rcode]
        if rcode >= 12:
            rate = rd.u(8) * 1000 if rcode == 12 else rd.u(16) * (10 if rcode == 14 else 1)
        bps = (info["bps"], 8, 12, None, 16, 20, 24, 32)[scode]
        if crc8(data[at:rd.p // 8]) != rd.u(8):
            raise ValueError(f"frame {len(frames)}: header CRC-8 mismatch")
        kinds = []
        for c in range(assign + 1):
            x, name, order = _subframe(rd, n, bps)
            chans[c] += x
            kinds.append((name, order))
        rd.p = (rd.p + 7) // 8 * 8
        end = rd.p // 8
        if crc16(data[at:end]) != rd.u(16):
            raise ValueError(f"frame {len(frames)}: CRC-16 mismatch")
        frames.append({"n": n, "number": number, "bytes": end + 2 - at, "rate": rate, "variable": variable, "kinds": kinds})
        at = end + 2
    samples = np.array(chans, dtype=np.int64).reshape(info["channels"], -1)
    if info["total"] and samples.shape[1] != info["total"]:
        raise ValueError(f"STREAMINFO names {info['total']} samples, the frames hold {samples.shape[1]}")
    return {**info, "samples": samples, "frames": frames}

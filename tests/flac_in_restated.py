"""FLAC in (include/mtts.h "FLAC in") restated for the tests of ``mtts_flac_decode`` and ``mtts_flac_parse_host``, in two halves that
share nothing but the CRC functions and the bit reader of ``flac_restated``:

``decode`` is a full RFC 9639 frame decoder written to the header's acceptance rule: the metadata walk, every frame-header code, LPC
and FIXED prediction, the three stereo modes, wasted bits, both Rice methods with their escapes, fixed and variable blocking, and the
walk that decides whether a row is accepted.  It raises ``ValueError`` exactly where the contract refuses.

``write_stream`` is a test-stream writer that takes an explicit recipe per frame, which is what makes the hard cases reachable without
an encoder library: block size, per channel the subframe kind, order, precision, shift, wasted bits and the coefficients themselves,
the stereo mode, Rice method, partition order and per-partition parameter or escape width, fixed or variable numbering, extra metadata
blocks.  It computes residuals from the prediction formula; the decoder knows nothing of it."""
import numpy as np

from flac_restated import _Reader, crc8, crc16

RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def wrap32(v: int) -> int:
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


# ------------------------------------------------------------------------------------------------ the decoder (from the contract)
def metadata(data: bytes, max_block: int = 4608) -> dict:
    """The marker and the metadata chain -> STREAMINFO's words and ``first``, the first byte behind the chain."""
    n = len(data)
    if n < 42 or data[:4] != b"fLaC":
        raise ValueError("no fLaC marker, or too short for STREAMINFO")
    at, blocks, info = 4, 0, None
    while True:
        if at + 4 > n:
            raise ValueError("the metadata chain runs off the row")
        last, kind, size = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        if kind == 127 or (blocks == 0) != (kind == 0) or at + 4 + size > n:
            raise ValueError("bad metadata block")
        if kind == 0:
            if size != 34:
                raise ValueError("STREAMINFO has 34 bytes")
            v = int.from_bytes(data[at + 4:at + 38], "big")
            info = {"block_sizes": (v >> 256, v >> 240 & 0xFFFF), "frame_sizes": (v >> 216 & 0xFFFFFF, v >> 192 & 0xFFFFFF),
                    "rate": v >> 172 & 0xFFFFF, "channels": (v >> 169 & 7) + 1, "bps": (v >> 164 & 31) + 1, "total": v >> 128 & (1 << 36) - 1,
                    "md5": data[at + 22:at + 38].hex()}
        at, blocks = at + 4 + size, blocks + 1
        if last:
            break
    lo, hi = info["block_sizes"]
    if not 8 <= info["bps"] <= 24 or info["rate"] < 1 or lo < 16 or lo > hi or hi > max_block:
        raise ValueError("STREAMINFO outside what is read: bits per sample, rate or block sizes")
    info["first"] = at
    return info


def header(data: bytes, at: int, info: dict):
    """The candidate rule at byte ``at``: the header's facts, or None."""
    n = len(data)
    if at + 6 > n or data[at] != 0xFF or data[at + 1] & 0xFE != 0xF8:
        return None
    variable, bcode, rcode, assign, scode = data[at + 1] & 1, data[at + 2] >> 4, data[at + 2] & 15, data[at + 3] >> 4, data[at + 3] >> 1 & 7
    if data[at + 3] & 1 or bcode == 0 or rcode == 15 or assign > 10 or scode == 3:
        return None
    i, lead = at + 5, data[at + 4]
    extra = 0
    if lead >= 0x80:
        if lead < 0xC0 or lead == 0xFF:
            return None
        extra = next(j for j in range(1, 7) if not lead >> (6 - j) & 1)
    number = lead & (0x7F >> (extra + 1)) if extra else lead
    if i + extra > n:
        return None
    for _ in range(extra):
        if data[i] >> 6 != 2:
            return None
        number, i = number << 6 | data[i] & 63, i + 1
    tail = {6: 1, 7: 2}.get(bcode, 0) + {12: 1, 13: 2, 14: 2}.get(rcode, 0)
    if i + tail + 1 > n:
        return None
    if bcode == 1:
        bs = 192
    elif bcode <= 5:
        bs = 144 << bcode
    elif bcode <= 7:
        bs, i = int.from_bytes(data[i:i + bcode - 5], "big") + 1, i + bcode - 5
    else:
        bs = 1 << bcode
    rate = info["rate"] if rcode == 0 else RATES.get(rcode)
    if rcode >= 12:
        w = 1 if rcode == 12 else 2
        rate, i = int.from_bytes(data[i:i + w], "big") * {12: 1000, 13: 1, 14: 10}[rcode], i + w
    bps = info["bps"] if scode == 0 else SIZES[scode]
    if crc8(data[at:i]) != data[i]:
        return None
    channels = assign + 1 if assign < 8 else 2
    if rate != info["rate"] or bps != info["bps"] or channels != info["channels"] or bs > info["block_sizes"][1]:
        return None
    return {"variable": variable, "n": bs, "assign": assign, "number": number, "rate": rate, "header_bytes": i + 1 - at}


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
        if k == (1 << pbits) - 1:
            raw = rd.u(5)
            out += [rd.i(raw) for _ in range(cnt)]
        else:
            for _ in range(cnt):
                q = rd.unary()
                low = rd.u(k)
                if q >= 1 << (32 - k) or (q << k | low) == 0xFFFFFFFF:
                    raise ValueError("a residual outside 32 bits")
                u = q << k | low
                out.append(u >> 1 if not u & 1 else -(u >> 1) - 1)
    return out


def _subframe(rd, n, bps):
    if rd.u(1):
        raise ValueError("subframe padding bit set")
    kind, wasted = rd.u(6), 0
    if rd.u(1):
        w = rd.unary()
        if w + 2 > bps:
            raise ValueError("more wasted bits than the subframe has")
        wasted = w + 1
    eff = bps - wasted
    if kind == 0:
        x, name, order = [rd.i(eff)] * n, "CONSTANT", 0
    elif kind == 1:
        x, name, order = [rd.i(eff) for _ in range(n)], "VERBATIM", 0
    elif 8 <= kind <= 12 or kind >= 32:
        lpc = kind >= 32
        order, name = (kind - 31, "LPC") if lpc else (kind - 8, "FIXED")
        if order > n:
            raise ValueError("a predictor order above the block size")
        x = [rd.i(eff) for _ in range(order)]
        coef, shift = FIXED[order] if not lpc else (), 0
        if lpc:
            prec = rd.u(4)
            if prec == 15:
                raise ValueError("LPC precision code 1111")
            shift = rd.i(5)
            if shift < 0:
                raise ValueError("negative LPC shift")
            coef = [rd.i(prec + 1) for _ in range(order)]
        for r in _residual(rd, n, order):
            x.append(wrap32(r + (sum(c * x[-1 - j] for j, c in enumerate(coef)) >> shift)))
    else:
        raise ValueError(f"reserved subframe type {kind:06b}")
    return [wrap32(v << wasted) for v in x], name, order


def decode(data: bytes, max_block: int = 4608, ld=None) -> dict:
    """A FLAC stream -> ``{"rate", "channels", "bps", "total", "block_sizes", "frame_sizes", "md5", "first", "samples": int64 [channels,
    total] with the stereo pair rebuilt, "frames": [{"n", "number", "bytes", "rate", "variable", "assign", "kinds"}]}``; ``ValueError``
    wherever include/mtts.h "FLAC in" refuses the row.  ``ld``: the capacity the sample total must fit."""
    data = bytes(data)
    info = metadata(data, max_block)
    at, n = info["first"], len(data)
    chans, frames, rd = [[] for _ in range(info["channels"])], [], _Reader(data)
    total, variable, bs0, short_seen = 0, 0, 0, False
    while at < n:
        h = header(data, at, info)
        if h is None:
            raise ValueError(f"no frame header at byte {at}")
        if not frames:
            variable, bs0 = h["variable"], h["n"]
        elif h["variable"] != variable:
            raise ValueError("the blocking strategy changes")
        if variable:
            if h["number"] != total:
                raise ValueError("a sample number that is not the sum of the blocks before")
        else:
            if h["number"] != len(frames) or short_seen or h["n"] > bs0:
                raise ValueError("frame numbers not consecutive, or a short frame that is not the last")
            short_seen = h["n"] < bs0
        total += h["n"]
        if ld is not None and total > ld:
            raise ValueError("more samples than the row holds")
        rd.p = 8 * (at + h["header_bytes"])
        a, kinds, xs = h["assign"], [], []
        for c in range(a + 1 if a < 8 else 2):
            side = (a, c) in ((8, 1), (9, 0), (10, 1))
            x, name, order = _subframe(rd, h["n"], info["bps"] + side)
            xs.append(x)
            kinds.append((name, order))
        if a == 8:
            xs[1] = [wrap32(l - s) for l, s in zip(*xs)]
        elif a == 9:
            xs[0] = [wrap32(s + r) for s, r in zip(*xs)]
        elif a == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(*xs)]
            xs = [[wrap32((m + s) >> 1) for m, s in zip(mid, xs[1])], [wrap32((m - s) >> 1) for m, s in zip(mid, xs[1])]]
        if any(not -(1 << info["bps"] - 1) <= v < 1 << info["bps"] - 1 for v in xs[0]):
            raise ValueError("a sample of channel 0 outside its bits")
        rd.p = (rd.p + 7) // 8 * 8
        end = rd.p // 8
        if end + 2 > n or crc16(data[at:end]) != int.from_bytes(data[end:end + 2], "big"):
            raise ValueError(f"frame {len(frames)}: truncated, or CRC-16 mismatch")
        for c, x in enumerate(xs):
            chans[c] += x
        frames.append({"n": h["n"], "number": h["number"], "bytes": end + 2 - at, "rate": h["rate"], "variable": h["variable"], "assign": a,
                       "kinds": kinds})
        at = end + 2
    if info["total"] == 0:
        if frames:
            raise ValueError("unknown length (STREAMINFO total 0) with frames")
    elif total != info["total"]:
        raise ValueError(f"STREAMINFO names {info['total']} samples, the frames hold {total}")
    return {**info, "samples": np.array(chans, dtype=np.int64).reshape(info["channels"], -1), "frames": frames}


# ------------------------------------------------------------------------------------------------ the writer (recipes)
def _u(v: int, n: int) -> str:
    return format(v & ((1 << n) - 1), f"0{n}b") if n else ""


def coded_number(v: int) -> bytes:
    """The UTF-8-like coding of a number below 2^36: 1 to 7 bytes."""
    if v < 0x80:
        return bytes([v])
    extra = next(e for e in range(1, 7) if v < 1 << (5 * e + 6))
    lead = (0xFF << (7 - extra)) & 0xFF | v >> (6 * extra)
    return bytes([lead] + [0x80 | v >> (6 * (extra - 1 - j)) & 63 for j in range(extra)])


def _residual_bits(res, n, order, method, po, params) -> str:
    pbits, out, i = 4 + method, [_u(method, 2), _u(po, 4)], 0
    for p in range(1 << po):
        cnt = max((n >> po) - (order if p == 0 else 0), 0)
        part, i = res[i:i + cnt], i + cnt
        k = params[p] if p < len(params) else params[-1]
        if k == "auto":                                           # the smallest parameter whose unary runs are at most one bit
            k = min(max(max([2 * r if r >= 0 else -2 * r - 1 for r in part] + [0]).bit_length() - 1, 0), (1 << pbits) - 2)
        if isinstance(k, tuple):                                  # ("esc", width)
            out += [_u((1 << pbits) - 1, pbits), _u(k[1], 5)] + [_u(r, k[1]) for r in part]
        else:
            out.append(_u(k, pbits))
            for r in part:
                u = 2 * r if r >= 0 else -2 * r - 1
                out.append("0" * (u >> k) + "1" + _u(u, k))
    return "".join(out)


def subframe_bits(x, bps: int, s: dict) -> str:
    """One subframe of the samples ``x`` in ``bps`` bits by the recipe ``s``: ``kind`` ("constant", "verbatim", "fixed", "lpc"),
    ``order`` (fixed), ``coefs`` / ``precision`` / ``shift`` (lpc; ``precision_code`` overrides the 4 bits written), ``wasted``, and for
    the residual ``method`` (0 / 1), ``po`` and ``params`` (per partition a Rice parameter, ``"auto"`` or ``("esc", width)``; the last repeats)."""
    wasted = s.get("wasted", 0)
    y, eff = [int(v) >> wasted for v in x], bps - wasted
    assert all(int(v) == w << wasted for v, w in zip(x, y)), "the samples do not have that many wasted bits"
    tail = "1" + "0" * (wasted - 1) + "1" if wasted else "0"
    kind, n = s["kind"], len(y)
    if kind == "constant":
        return "0" + _u(0, 6) + tail + _u(y[0], eff)
    if kind == "verbatim":
        return "0" + _u(1, 6) + tail + "".join(_u(v, eff) for v in y)
    if kind == "fixed":
        order, coef, shift, extra, code = s["order"], FIXED[s["order"]], 0, "", 8 + s["order"]
    else:
        coef, shift, prec = [int(c) for c in s["coefs"]], s["shift"], s["precision"]
        order, code = len(coef), 31 + len(coef)
        extra = _u(s.get("precision_code", prec - 1), 4) + _u(shift, 5) + "".join(_u(c, prec) for c in coef)
    res = [y[i] - (sum(c * y[i - 1 - j] for j, c in enumerate(coef)) >> shift) for i in range(order, n)]
    return ("0" + _u(code, 6) + tail + "".join(_u(v, eff) for v in y[:order]) + extra
            + _residual_bits(res, n, order, s.get("method", 0), s.get("po", 0), s.get("params", ["auto"])))


def frame_bytes(f: dict, number: int, rate: int, bps: int, info_rate: int) -> bytes:
    """One frame by its recipe ``f``: ``samples`` [channels, n], ``sub`` (a recipe per channel, or one for all), ``stereo`` (None,
    "ls", "sr", "ms"), ``variable``; ``bcode`` / ``rcode`` / ``scode`` override the header codes chosen from the values."""
    x = np.atleast_2d(np.asarray(f["samples"], dtype=np.int64))
    ch, n = x.shape
    stereo = f.get("stereo")
    assign = {None: ch - 1, "ls": 8, "sr": 9, "ms": 10}[stereo]
    rows, widths = [list(map(int, r)) for r in x], [bps] * ch
    if stereo:
        l, r = rows
        side = [a - b for a, b in zip(l, r)]
        rows = {"ls": [l, side], "sr": [side, r], "ms": [[(a + b) >> 1 for a, b in zip(l, r)], side]}[stereo]
        widths = {"ls": [bps, bps + 1], "sr": [bps + 1, bps], "ms": [bps, bps + 1]}[stereo]
    bcode = f.get("bcode")
    if bcode is None:
        bcode = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, **{1 << c: c for c in range(8, 16)}}.get(n, 6 if n <= 256 else 7)
    rcode = f.get("rcode", {v: k for k, v in RATES.items()}.get(rate, 13 if rate <= 65535 else 0))
    scode = f.get("scode", {v: k for k, v in SIZES.items()}.get(bps, 0))
    head = bytes([0xFF, 0xF8 | bool(f.get("variable")), bcode << 4 | rcode, assign << 4 | scode << 1]) + coded_number(number)
    head += (n - 1).to_bytes(bcode - 5, "big") if bcode in (6, 7) else b""
    head += {12: lambda: bytes([rate // 1000]), 13: lambda: rate.to_bytes(2, "big"), 14: lambda: (rate // 10).to_bytes(2, "big")}.get(rcode, bytes)()
    head += bytes([crc8(head)])
    subs = f["sub"] if isinstance(f["sub"], (list, tuple)) else [f["sub"]] * ch
    bits = "".join(subframe_bits(r, w, s) for r, w, s in zip(rows, widths, subs))
    bits += "0" * (-len(bits) % 8)
    body = head + (int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b"")
    return body + crc16(body).to_bytes(2, "big")


def stream_head(rate, channels, bps, total, min_bs, max_bs, frame_sizes=(0, 0), blocks=()) -> bytes:
    """``fLaC``, STREAMINFO and the further metadata ``blocks`` [(type, payload)]."""
    v = (min_bs << 256 | max_bs << 240 | frame_sizes[0] << 216 | frame_sizes[1] << 192 | rate << 172 | (channels - 1) << 169 | (bps - 1) << 164
         | total << 128)
    chain = [(0, v.to_bytes(34, "big"))] + list(blocks)
    return b"fLaC" + b"".join(bytes([(0x80 if j == len(chain) - 1 else 0) | t]) + len(p).to_bytes(3, "big") + p for j, (t, p) in enumerate(chain))


def write_stream(frames, rate=24000, channels=1, bps=16, blocks=(), total=None, min_bs=None, max_bs=None, numbers=None):
    """``(stream bytes, [(start, length) per frame])`` of the frame recipes (``frame_bytes``).  Frames with ``variable`` carry their
    first sample's number, the others their index; ``numbers`` overrides them.  STREAMINFO's total and block sizes come from the frames
    unless given."""
    sizes = [np.atleast_2d(np.asarray(f["samples"])).shape[1] for f in frames]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    datas = []
    for j, f in enumerate(frames):
        number = numbers[j] if numbers is not None else int(starts[j]) if f.get("variable") else j
        datas.append(frame_bytes(f, number, f.get("rate", rate), bps, rate))
    hi = max_bs if max_bs is not None else max(sizes + [16])
    fixed = not any(f.get("variable") for f in frames)
    lo = min_bs if min_bs is not None else (max(sizes[0], 16) if fixed and sizes else min(max(min(sizes + [hi]), 16), hi))
    lens = [len(d) for d in datas]
    head = stream_head(rate, channels, bps, int(starts[-1]) if total is None else total, min(lo, hi), hi,
                       (min(lens), max(lens)) if lens else (0, 0), blocks)
    at, spans = len(head), []
    for d in datas:
        spans.append((at, len(d)))
        at += len(d)
    return head + b"".join(datas), spans

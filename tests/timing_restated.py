"""NumPy restatement of include/mtts.h "token timing" and "shaped durations", written from the definitions there and not from the
kernels: shaped durations in fp32 (every operation rounded once, in the stated order) or fp64, the boundaries e_k, the break plan
(int64) and the lengthened rows, built segment by segment the way a person would splice them."""
import numpy as np

F32 = np.float32


def clamp_shaping(s, a, dtype=F32):
    """token_scale to [0, 16] (NaN: 1), token_extend to [-4096, 4096] (NaN: 0)."""
    s = np.asarray(s, dtype=dtype).copy()
    a = np.asarray(a, dtype=dtype).copy()
    s[np.isnan(s)] = 1
    a[np.isnan(a)] = 0
    return np.clip(s, dtype(0), dtype(16)), np.clip(a, dtype(-4096), dtype(4096))


def shaped_durations(exp_logw, mask, sc, ls, s=None, a=None, given=None, given_rows=None, dtype=F32):
    """(durations, cum int32, y_fine_lengths int64, v) for [B, Tx] inputs; ``exp_logw`` is exp(logw) as the caller computed it (the
    device's own fp32 expf for an integer-exact comparison).  ``v`` is the value in front of the rounding."""
    mask = np.asarray(mask, dtype=dtype)
    B, Tx = mask.shape
    s = np.ones((B, Tx)) if s is None else s
    a = np.zeros((B, Tx)) if a is None else a
    s, a = clamp_shaping(s, a, dtype)
    sc = np.asarray(sc, dtype=dtype).reshape(B, 1)
    ls = np.asarray(ls, dtype=dtype).reshape(B, 1)
    take = np.zeros(B, dtype=bool) if given is None else (np.ones(B, dtype=bool) if given_rows is None else np.asarray(given_rows) != 0)
    with np.errstate(all="ignore"):
        v = (np.asarray(exp_logw, dtype=dtype) - dtype(2)) * mask
        v = (v * sc).astype(dtype)
        v = (v * ls).astype(dtype)
        lo = np.where(s == 0, dtype(0), dtype(1)).astype(dtype)
        if given is not None:
            g = (np.asarray(given, dtype=dtype) * ls).astype(dtype)
            v = np.where(take[:, None], g, v).astype(dtype)
            lo = np.where(take[:, None], dtype(0), lo).astype(dtype)
        v = (v * s).astype(dtype)
        v = (v + a).astype(dtype)
        d = (np.maximum(np.rint(v), lo) * mask).astype(dtype)
    cum = np.cumsum(d.astype(np.int64), axis=1)
    yfl = np.maximum(cum[:, -1], 1)
    return d, cum.astype(np.int32), yfl.astype(np.int64), v


def edges(cum_row, x_len, keep, fine_hop=128):
    """e_0 .. e_{x_len} of one row (int64)."""
    e = [0]
    for k in range(1, int(x_len) + 1):
        e.append(min(max(fine_hop * int(cum_row[k - 1]) - fine_hop // 2, 0), int(keep)))
    return e


def plan_row(cum_row, x_len, keep, breaks, Tx, fine_hop=128, keep_max=1 << 40, pause_max=1 << 40, out_max=1 << 40):
    """One row: ``(reason, marks [Tx, 2], new_length, cuts)`` with ``cuts = [(position, pause)]`` of the APPLIED breaks in order.
    Reasons: 0 accepted, 1 keep outside its row, 2 a token index outside [0, x_len), 3 token indices not increasing, 4 a pause outside
    [0, pause_max], 5 x_len outside [1, Tx], 7 the lengthened row does not fit."""
    marks = np.full((Tx, 2), -1, dtype=np.int64)
    refused = lambda r: (r, marks, -1, [])
    x_len, keep = int(x_len), int(keep)
    if x_len < 1 or x_len > Tx:
        return refused(5)
    if keep < 0 or keep > keep_max:
        return refused(1)
    last = None
    for tok, pause in breaks or ():
        if tok < 0 or tok >= x_len:
            return refused(2)
        if last is not None and tok <= last:
            return refused(3)
        if pause < 0 or pause > pause_max:
            return refused(4)
        last = tok
    e = edges(cum_row, x_len, keep, fine_hop)
    cuts, before = [], np.zeros(x_len + 1, dtype=np.int64)          # before[i]: applied pauses of breaks at tokens < i
    for tok, pause in breaks or ():
        c = e[tok + 1]
        applied = 0 if (c == 0 or c >= keep) else int(pause)
        if not (c == 0 or c >= keep):
            cuts.append((c, int(pause)))
        before[tok + 1:] += applied
    new_len = keep + int(before[x_len])
    if new_len > out_max:
        return refused(7)
    for i in range(x_len):
        marks[i] = (e[i] + before[i], e[i + 1] + before[i])
    return 0, marks, new_len, cuts


def plan(cum, x_lengths, keep, breaks, **kw):
    """Every row of a batch: ``(reasons [B], marks [B, Tx, 2], new_lengths [B], cuts per row)``."""
    cum = np.asarray(cum)
    B, Tx = cum.shape
    rows = [plan_row(cum[b], x_lengths[b], keep[b], None if breaks is None else breaks[b], Tx, **kw) for b in range(B)]
    return (np.array([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int64),
            [r[3] for r in rows])


def fade_weights(n, fade):
    """(F', w) of a segment of n samples: w[i] = (float)(2 i + 1) / (float)(2 F') in fp32."""
    F = min(int(fade), n // 2)
    i = np.arange(F, dtype=np.int64)
    return F, (F32(1) * (2 * i + 1).astype(F32) / F32(2 * F)).astype(F32) if F else np.zeros(0, dtype=F32)


def spliced_row(audio_row, keep, new_len, cuts, fade, out_ld):
    """The lengthened row [out_ld] (fp32): segments between the applied cuts, ``pause`` zeros after each, faded at the cuts only;
    all zeros for a refused row (new_len < 0)."""
    out = np.zeros(out_ld, dtype=F32)
    if new_len < 0:
        return out
    x = np.asarray(audio_row, dtype=F32)
    bounds = [0] + [c for c, _ in cuts] + [int(keep)]
    pieces = []
    for k in range(len(bounds) - 1):
        seg = x[bounds[k]:bounds[k + 1]].copy()
        n = len(seg)
        F, w = fade_weights(n, fade)
        if F and k > 0:                                              # behind a cut
            seg[:F] = (seg[:F] * w).astype(F32)
        if F and k < len(bounds) - 2:                                # ahead of a cut
            seg[n - F:] = (seg[n - F:] * w[::-1]).astype(F32)
        pieces.append(seg)
        if k < len(cuts):
            pieces.append(np.zeros(cuts[k][1], dtype=F32))
    row = np.concatenate(pieces) if pieces else np.zeros(0, dtype=F32)
    assert len(row) == new_len, (len(row), new_len)
    out[:new_len] = row
    return out

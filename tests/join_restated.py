"""The document join of include/mtts.h ("long texts") restated in torch on the CPU, in fp32 and in exactly the documented order of
operations.  It has no reference counterpart (the reference refuses a long text): this file is the definition the kernels of
csrc/wave_join.hip are compared with bit for bit, and tests/test_join_abi.py checks it against an independent sample-by-sample
formulation (``join_by_samples``).

    join(audio [B, ld] fp32, lengths [B], first_row [G + 1], gaps [B], fade, scale [B] or None, out_ld, gap_max)
        -> out [G, out_ld] fp32, out_lengths int64 [G], starts int64 [B], verdict
    verdict: None, or (first refused row, its length, reason) with reason 1 length, 2 layout / gap, 3 does not fit out_ld.
"""
import numpy as np
import torch

REASONS = {1: "length", 2: "layout or a gap", 3: "does not fit"}


def default_out_ld(ld, first_row, gaps):
    need = max((b - a) * ld + sum(gaps[a:b - 1]) for a, b in zip(first_row[:-1], first_row[1:]))
    return max(4, (need + 3) // 4 * 4)


def plan(lengths, first_row, gaps, ld, out_ld, gap_max):
    """The integer half: (starts [B], out_lengths [G], verdict, standing) -- ``standing`` lists the documents that are joined."""
    B, G = len(lengths), len(first_row) - 1
    starts, out_lengths, code = [-1] * B, [-1] * G, [0] * B
    firstbad = G
    for g in range(G):
        r0, r1 = first_row[g], first_row[g + 1]
        if not (0 <= r0 < r1 <= B and (g > 0 or r0 == 0) and (g < G - 1 or r1 == B)):
            firstbad = g
            break
    fit_row, standing = B, []
    for g in range(firstbad):
        r0, r1 = first_row[g], first_row[g + 1]
        for r in range(r0, r1):
            gp = gaps[r] if r + 1 < r1 else 0
            if lengths[r] < 0 or lengths[r] > ld:
                code[r] = 1
            elif gp < 0 or gp > gap_max:
                code[r] = 2
        if any(code[r0:r1]):
            continue
        at, begin = 0, []
        for r in range(r0, r1):
            begin.append(at)
            at += lengths[r] + (gaps[r] if r + 1 < r1 else 0)
        if at > out_ld:
            fit_row = min(fit_row, r0)
            continue
        starts[r0:r1] = begin
        out_lengths[g] = at
        standing.append(g)
    layout_row = B
    if firstbad < G:
        end = first_row[firstbad] if firstbad > 0 else 0
        layout_row = min(end, B - 1)
    verdict = None
    for r in range(B):
        if code[r] or r == layout_row or r == fit_row:
            reason = 1 if code[r] == 1 else 2 if (code[r] == 2 or r == layout_row) else 3
            verdict = (r, max(min(lengths[r], 0x7fffffff), -0x7fffffff), reason)
            break
    return starts, out_lengths, verdict, standing


def _ints(v):
    return [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]


def join(audio, lengths, first_row, gaps, fade=0, scale=None, out_ld=None, gap_max=None):
    audio = torch.as_tensor(audio, dtype=torch.float32)
    B, ld = audio.shape
    lengths, first_row, gaps = _ints(lengths), _ints(first_row), _ints(gaps)
    G = len(first_row) - 1
    out_ld = default_out_ld(ld, first_row, gaps) if out_ld is None else int(out_ld)
    gap_max = max([0] + gaps) if gap_max is None else int(gap_max)
    starts, out_lengths, verdict, standing = plan(lengths, first_row, gaps, ld, out_ld, gap_max)
    out = torch.zeros(G, out_ld, dtype=torch.float32)
    one = torch.tensor(1.0, dtype=torch.float32)
    for g in standing:
        r0, r1 = first_row[g], first_row[g + 1]
        g_doc = one if scale is None else torch.as_tensor(scale, dtype=torch.float32)[r0:r1].min()
        for b in range(r0, r1):
            n = lengths[b]
            x = audio[b, :n].clone()
            r = one if scale is None else g_doc / torch.as_tensor(scale, dtype=torch.float32)[b]      # one fp32 division per row
            if float(r) != 1.0:
                x = x * r
            F = min(int(fade), n // 2)
            if F > 0:
                i = torch.arange(F)
                w = (2 * i + 1).to(torch.float32) / torch.tensor(2 * F).to(torch.float32)
                if b != r0:
                    x[:F] = x[:F] * w
                if b != r1 - 1:
                    x[n - 1 - i] = x[n - 1 - i] * w
            out[g, starts[b]:starts[b] + n] = x
    return out, torch.tensor(out_lengths, dtype=torch.long), torch.tensor(starts, dtype=torch.long), verdict


def join_by_samples(audio, lengths, first_row, gaps, fade=0, scale=None, out_ld=None):
    """The same join, formulated from the output's side, one sample at a time in NumPy fp32 scalars: output sample j of a document
    belongs to the last row that starts at or before it.  For well-formed input only (tiny sizes: it is a Python loop)."""
    a = np.asarray(audio, dtype=np.float32)
    B, ld = a.shape
    lengths, first_row, gaps = _ints(lengths), _ints(first_row), _ints(gaps)
    G = len(first_row) - 1
    out_ld = default_out_ld(ld, first_row, gaps) if out_ld is None else int(out_ld)
    sc = None if scale is None else np.asarray(scale, dtype=np.float32)
    out = np.zeros((G, out_ld), dtype=np.float32)
    out_lengths, starts = [], [0] * B
    for g in range(G):
        rows = list(range(first_row[g], first_row[g + 1]))
        for k, b in enumerate(rows):
            starts[b] = sum(lengths[r] + gaps[r] for r in rows[:k])
        total = starts[rows[-1]] + lengths[rows[-1]]
        out_lengths.append(total)
        g_doc = np.float32(1.0) if sc is None else np.float32(min(float(sc[b]) for b in rows))
        for j in range(total):
            b = max(r for r in rows if starts[r] <= j)
            i, n = j - starts[b], lengths[b]
            if i >= n:
                continue
            x = a[b, i]
            if sc is not None:
                r = np.float32(g_doc / sc[b])
                if r != np.float32(1.0):
                    x = np.float32(x * r)
            F = min(int(fade), n // 2)
            if b != rows[0] and i < F:
                x = np.float32(x * np.float32(np.float32(2 * i + 1) / np.float32(2 * F)))
            elif b != rows[-1] and n - 1 - i < F:
                x = np.float32(x * np.float32(np.float32(2 * (n - 1 - i) + 1) / np.float32(2 * F)))
            out[g, j] = x
    return out, out_lengths, starts

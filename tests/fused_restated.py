"""Restatement of the two fused P16 kernels -- tblock_chain_kernel (csrc/tblock_chain.hip) and conv_gn_kernel (csrc/resnet_conv.hip)
-- in plain fp64 PyTorch on the CPU, modelling their ROUNDING POINTS and nothing else, the yardstick of
tests/test_fused_restated.py (CPU) and tests/test_hip_kernels_fused.py (against the device).

What is modelled.  Every value a kernel keeps as a P16 image (h = fp16(x), l = fp16((x - h) * lscale); tests/p16_restated.py) is
passed through p16() at the place the kernel does it; everything between two such places is fp64.
  chain    operands att, x, W_out, W1, W2, W_qkv are split first (biases and SnakeBeta constants stay fp32);
           x1 = x + att W_out^T + b_out                        -> re-split (the x tile in LDS: the moments AND FF1 read that image)
           z  = LN(x1) W1^T + b1,  h = z + p1 sin^2(p0 z)      -> re-split (the hidden chunk image)
           x2 = x1 + h W2^T + b2                               -> re-split (the x_out image; rows times x_out_mask afterwards)
           qkv = LN(x2) W_qkv^T + b_qkv                        -> split with lscale 1 (what the attention kernel reads)
  conv_gn  input and W are split; conv + bias, GroupNorm(8) statistics over the first nrows[b] frames plus nextra[b] EXPLICIT
           copies of the bias row, Mish, mask, time row and mask again in fp64; the output is split at 2048.
LN = LayerNorm without affine, biased variance, eps 1e-5 inside the root.

The fp32 twin (dtype=torch.float32) runs the same stages in fp32 on the CPU with the same re-splits and the kernel's ALGEBRA:
LayerNorm applied after the product, rstd (x W^T - mean rowsum(W)) + b with rowsum taken from the unsplit fp32 panel as the packer
does, SnakeBeta as (z + p1/2) - (p1/2) cos(2 p0 z) with libm's cosine.  Its error against the fp64 form is the unit the device is
measured in (e_cpu32); nothing is taken from what the device returns.

Error budget B, per output element, in units of u = 2^-24 (the convention of tests/test_hip_spk_grad.py: fp32 arithmetic loses at
most u times the sum of the ABSOLUTE values of the terms a stage adds, and an input error passes through a linear stage
multiplied by the absolute weights).  Forward recursion, with |.| elementwise and X |W|^T a matrix product:
  B_x1  = |att| |W_out|^T + |b_out| + |x|                                     + 4 |x1|   (re-split: 2^-22 = 4 u)
  B_z   = LNB(x1, B_x1, W1, b1)
  B_h   = B_z (1 + p0 p1) + p1 (1 + |p0 z|) + |h|                             + 4 |h|
          (|d/dz p1 sin^2(p0 z)| <= p0 p1; the cosine's argument p0 z carries a relative error u, i.e. |p0 z| u absolute)
  B_x2  = B_x1 + |x1| + B_h |W2|^T + |h| |W2|^T + |b2|                        + 4 |x2|
  B_qkv = LNB(x2, B_x2, W_qkv, b_qkv)                                         + 4 |qkv| + 1
  LNB(v, Bv, W, b) = rstd (|v| |W|^T + 3 |mean| S + Bv |W|^T) + |b| + |y|                     [the first-order terms, S = sum_k |W|]
                   + rstd (mean_k(Bv) + 2 mean_k|v|) S                                         [a]
                   + |y - b| (rstd rms_k(Bv) + 2)                                              [b]
Corrections to the recursion as first written down (rstd (|v||W|^T + |mean| S + Bv |W|^T) + |b|):
  [a] an error of the inputs moves the row MEAN as well (by at most mean_k(Bv)), and the fp32 mean of C values is itself only good
      to u mean_k|v| per pass; either shift is multiplied by rstd S.  Without it a row with |mean| << |v| (the x100 row, whose mean
      is 0.15 std) has a budget that ignores the one quantity the post-product algebra cancels against.
  [b] the same input error moves rstd: d rstd / rstd = -cov(v - mean, dv) / (var + eps), at most rstd rms_k(dv) in magnitude, and
      the fp32 variance and the reciprocal root add two relative u; both scale the whole normalised product |y - b|.
  3 |mean| S instead of |mean| S: the kernel multiplies the SPLIT panel but subtracts mean times the row sum of the UNSPLIT one
      (csrc/unit_entries.hip plain_row_sum, as the model's packer); the two sums differ by up to 2 u S (2^-23 per weight).
  + |y|, + |h|: the last rounding of a stage, which the sums of its terms bound but do not contain when terms cancel.
  + 1 on qkv: with lscale 1 the residual of a value below 2^-4 is an fp16 subnormal (spacing 2^-24), so the image's error has an
      ABSOLUTE floor of u / 2 that 4 |qkv| does not cover in the small-magnitude columns.
conv_gn: B_y = |x| * |W| + |bias| + |y|;  n = (y - mean) rs:  B_n = rs (B_y + mean_g(B_y) + 2 mean_g|y|) + |n| (rs rms_g(B_y) + 3);
  g = n gamma + beta: B_g = |gamma| B_n + |n gamma| + |beta| + |g|;  Mish = g w / (w + 2), w = e^g (e^g + 2): |Mish'| <= 1.1, eight
  roundings and an exponent whose argument error |g| u becomes a relative error of e^g:  B_m = 1.1 B_g + (8 + 2 |g|) |m|;
  out = (m mask + cb) mask: B_o = (B_m + |cb| + |o|) mask + 4 |o|.
The hardware-cosine allowance is kept apart (cos_*): an absolute error (p1 / 2) delta_cos per hidden element, delta_cos = 1e-6
(csrc/device_utils.h), carried through |W2|^T and through LNB's input-error terms exactly as B_h is.

`operands=True, rounding=False` gives the budget of the REPRESENTATION terms alone (4 u per split operand, the re-splits, and
their propagation): what separates this restatement from independent fp64 code on the unsplit operands."""
import functools
import math

import torch
import torch.nn.functional as F

from p16_restated import p16

U = 2.0 ** -24
DELTA_COS = 1e-6
EPS = 1e-5
F16_MAX = 65504.0


def _stats(v, eps=EPS):
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def _ln_linear(v, w_split, w_raw, b, dtype):
    """LayerNorm + Linear.  fp64: the operation itself; fp32: the kernel's post-product algebra."""
    mean, rstd = _stats(v)
    if dtype == torch.float64:
        y = ((v - mean) * rstd) @ w_split.T
    else:
        wsum = w_raw.double().sum(1).to(dtype)[None]               # row sums of the fp32 panel (plain_row_sum)
        y = (v @ w_split.T) * rstd + (-(mean * rstd)) * wsum
    return mean, rstd, (y if b is None else y + b.to(dtype))


def chain(att, x, w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv=None, b_qkv=None, mask=None, dtype=torch.float64):
    """Every intermediate of the chain as a dict (x1, mean1, rstd1, z, h, x2_raw, x2, mean2, rstd2, qkv_raw, qkv, x_out)."""
    f = lambda t: None if t is None else t.to(dtype)
    s = lambda t, ls=2048.0: p16(t, ls).to(dtype)
    r = {}
    x1 = s(x)
    if att is not None:
        y = s(att) @ s(w_out).T
        x1 = (y if b_out is None else y + f(b_out)) + x1
    r["x1"] = x1 = s(x1)
    r["mean1"], r["rstd1"], z = _ln_linear(x1, s(w1), w1, b1, dtype)
    r["z"] = z
    if dtype == torch.float64:
        h = z + f(p1) * torch.sin(z * f(p0)) ** 2
    else:
        p1h = f(p1) * 0.5
        h = (z + p1h) - p1h * torch.cos(2.0 * (z * f(p0)))
    r["h"] = h = s(h)
    y = h @ s(w2).T
    r["x2_raw"] = x2 = x1 + (y if b2 is None else y + f(b2))
    r["x2"] = x2 = s(x2)
    r["x_out"] = x2 if mask is None else x2 * mask.to(dtype)[:, None]
    if w_qkv is not None:
        r["mean2"], r["rstd2"], q = _ln_linear(x2, s(w_qkv), w_qkv, b_qkv, dtype)
        r["qkv_raw"] = q
        r["qkv"] = s(q, 1.0)
    return r


def _lnb(v, Bv, w, b, mean, rstd, y, rounding):
    """LNB of the module docstring; y = the stage's output (bias included).  Bv may be None (no input error)."""
    aw = w.abs()
    S = aw.sum(1)[None]
    ylin = (y if b is None else y - b).abs()
    out = torch.zeros_like(y)
    if Bv is not None:
        out = rstd * (Bv @ aw.T) + rstd * Bv.mean(1, keepdim=True) * S + ylin * rstd * torch.sqrt((Bv ** 2).mean(1, keepdim=True))
    if rounding:
        out = out + rstd * (v.abs() @ aw.T + 3 * mean.abs() * S + 2 * v.abs().mean(1, keepdim=True) * S) + 2 * ylin + y.abs()
        if b is not None:
            out = out + b.abs()
    return out


def chain_budget(r, att, x, w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv=None, b_qkv=None, mask=None, rounding=True, operands=False):
    """Budgets in units of u for x_out and qkv (r = chain(..., dtype=float64)), and the hardware-cosine allowance in the same units.
    Masked rows of x_out are exact zeros: their budget is 0."""
    d = lambda t: None if t is None else t.double()
    s = lambda t: p16(t).double()
    rnd, op = float(rounding), 4.0 * float(operands)
    x1, z, h, x2 = r["x1"], r["z"], r["h"], r["x2"]
    p0, p1 = d(p0), d(p1)
    B = 4 * x1.abs() + op * s(x).abs()
    if att is not None:
        B = B + (rnd + 2 * op) * (s(att).abs() @ s(w_out).abs().T) + rnd * s(x).abs()
        if b_out is not None and rounding:
            B = B + d(b_out).abs()
    else:
        B = op * s(x).abs()                                          # x1 is x: splitting an image again changes nothing
    Bz = _lnb(x1, B, s(w1), d(b1), r["mean1"], r["rstd1"], z, rounding)
    n1 = (x1 - r["mean1"]) * r["rstd1"]
    Bz = Bz + op * (n1.abs() @ s(w1).abs().T)
    Bh = Bz * (1 + p0 * p1) + rnd * (p1 * (1 + (p0 * z).abs()) + h.abs()) + 4 * h.abs()
    aw2 = s(w2).abs()
    Bx2 = B + Bh @ aw2.T + (rnd + op) * (h.abs() @ aw2.T) + rnd * x1.abs() + 4 * x2.abs()
    if b2 is not None and rounding:
        Bx2 = Bx2 + d(b2).abs()
    ch = (p1 * 0.5 * DELTA_COS / U)[None].expand_as(h)
    cx2 = ch @ aw2.T
    out = {"x1": B, "z": Bz, "h": Bh, "x2": Bx2}
    keep = 1.0 if mask is None else (mask.double() != 0).double()[:, None]
    out["x_out"], out["cos_x_out"] = Bx2 * keep, cx2 * keep
    if w_qkv is not None:
        q = r["qkv_raw"]
        Bq = _lnb(x2, Bx2, s(w_qkv), d(b_qkv), r["mean2"], r["rstd2"], q, rounding)
        n2 = (x2 - r["mean2"]) * r["rstd2"]
        out["qkv"] = Bq + op * (n2.abs() @ s(w_qkv).abs().T) + 4 * q.abs() + 1
        out["cos_qkv"] = _lnb(x2, cx2, s(w_qkv), d(b_qkv), r["mean2"], r["rstd2"], q, False)
    return out


def measure(out, ref, budget):
    """max over elements of |out - ref| / (u B); an element with B == 0 must be exact."""
    err = (out.double() - ref.double()).abs()
    ratio = torch.where(budget > 0, err / (U * budget.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    return ratio.max().item()


def cos_term(cos, budget):
    """The hardware-cosine allowance of an output in the units of `measure`."""
    return torch.where(budget > 0, cos / budget.clamp_min(1e-300), torch.zeros_like(cos)).max().item()


# ------------------------------------------------------------------------------------------------ conv_gn
def _group_sets(y_b, bias, n, extra):
    """[8][values that enter the statistics of group g]: the first n frames, then `extra` copies of the bias row."""
    T = y_b.shape[1]
    sel = y_b.view(8, -1, T)[:, :, :n].reshape(8, -1)
    if extra:
        sel = torch.cat([sel, bias.view(8, -1).repeat(1, extra)], 1)
    return sel


def conv_gn(x, w, bias, gamma, beta, mask, B, T, chbias=None, nrows=None, nextra=None, dtype=torch.float64):
    """dict: y (conv + bias) [B, N, T], mean / rs [B, 8], g (normalised, affine), m (Mish), out_raw and out [B*T, N]."""
    f = lambda t: t.to(dtype)
    xs = p16(x).to(dtype).view(B, T, -1).transpose(1, 2)
    y = F.conv1d(xs, p16(w).to(dtype), f(bias), padding=1)
    N = y.shape[1]
    mean, rs = torch.zeros(B, 8, dtype=dtype), torch.zeros(B, 8, dtype=dtype)
    for b in range(B):
        n = max(0, min(T, int(nrows[b]))) if nrows is not None else T
        sel = _group_sets(y[b], f(bias), n, int(nextra[b]) if nextra is not None else 0)
        mean[b] = sel.mean(1)
        rs[b] = 1.0 / torch.sqrt(((sel - mean[b][:, None]) ** 2).mean(1) + EPS)
    rep = lambda t: t.repeat_interleave(N // 8, 1)[:, :, None]
    nrm = (y - rep(mean)) * rep(rs)
    g = nrm * f(gamma)[None, :, None] + f(beta)[None, :, None]
    m = F.mish(g)
    mk = f(mask).view(B, 1, T)
    o = m * mk
    cb = None
    if chbias is not None:
        cb = f(chbias)[None, :, None] if chbias.dim() == 1 else f(chbias)[:, :N, None]
        o = (o + cb) * mk
    flat = lambda t: t.transpose(1, 2).reshape(B * T, N)
    return {"y": y, "mean": mean, "rs": rs, "n": nrm, "g": g, "m": m, "cb": cb, "out_raw": flat(o), "out": p16(flat(o)).to(dtype)}


def conv_gn_budget(r, x, w, bias, gamma, beta, mask, B, T, chbias=None, nrows=None, nextra=None, rounding=True, operands=False):
    """Budget of conv_gn's output [B*T, N] in units of u (module docstring)."""
    d = lambda t: t.double()
    rnd, op = float(rounding), 4.0 * float(operands)
    y, N = r["y"], r["y"].shape[1]
    ax = p16(x).double().abs().view(B, T, -1).transpose(1, 2)
    prod = F.conv1d(ax, p16(w).double().abs(), None, padding=1)
    By = (rnd + 2 * op) * prod + rnd * (d(bias).abs()[None, :, None] + y.abs())
    mB, rB, mY = torch.zeros(B, 8).double(), torch.zeros(B, 8).double(), torch.zeros(B, 8).double()
    for b in range(B):
        n = max(0, min(T, int(nrows[b]))) if nrows is not None else T
        e = int(nextra[b]) if nextra is not None else 0
        sb = _group_sets(By[b], rnd * 2 * d(bias).abs(), n, e)
        mB[b], rB[b] = sb.mean(1), torch.sqrt((sb ** 2).mean(1))
        mY[b] = _group_sets(y[b].abs(), d(bias).abs(), n, e).mean(1)
    rep = lambda t: t.repeat_interleave(N // 8, 1)[:, :, None]
    rs, nrm, g, m = rep(r["rs"]), r["n"], r["g"], r["m"]
    Bn = rs * (By + rep(mB) + rnd * 2 * rep(mY)) + nrm.abs() * (rs * rep(rB) + rnd * 3)
    ga, be = d(gamma).abs()[None, :, None], d(beta).abs()[None, :, None]
    Bg = ga * Bn + rnd * ((nrm * ga).abs() + be + g.abs())
    Bm = 1.1 * Bg + rnd * (8 + 2 * g.abs()) * m.abs()
    mk = (d(mask) != 0).double().view(B, 1, T)
    o = r["out_raw"].view(B, T, N).transpose(1, 2)
    Bo = Bm + rnd * o.abs()
    if r["cb"] is not None and rounding:
        Bo = Bo + r["cb"].abs()
    Bo = Bo * mk + 4 * o.abs()
    return Bo.transpose(1, 2).reshape(B * T, N)


# ------------------------------------------------------------------------------------------------ the inputs of the two test files
# (one place, so that the CPU file proves the stated input conditions on exactly what the GPU file launches)
CHAIN_SHAPES = [(384, 64, 128), (384, 32, 128), (384, 48, 256), (384, 32, 256), (256, 64, 128), (256, 32, 128), (128, 64, 128), (128, 32, 128)]
SWEEP_SHAPES = [(384, 48, 256), (256, 64, 128), (128, 32, 128)]              # one instantiation per C takes the whole M sweep
FULL = {384: (384, 1152), 256: (256, 768), 128: (128, 384)}                # C -> (inner, n_qkv) of the production layout
POOL = 129                                                                   # rows of a plain case: 2 * 64 + 1


def sweep_ms(qb):
    return sorted({1, 15, 17, qb - 1, qb, qb + 1, 2 * qb + 1})


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _spread(n, g, zero_at):
    """row scales spread over 2^-6 .. 2^2, one all-zero row"""
    s = 2.0 ** (torch.randint(0, 9, (n,), generator=g) - 6).float()
    s[zero_at % n] = 0.0
    return s


def chain_weights(C, inner, n_qkv, seed):
    """Hard columns: every panel's rows carry scales 2^-6 .. 2^2 and one all-zero row; p0, p1 = exp(U(-1.4, 1.4)).  W1's scale is
    held to 8 / p0 per row, which keeps |p0 z| below 64 (z is a unit-variance row times the panel row, at most ~5.5 sigma)."""
    g = _gen(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    un = lambda n: torch.exp((torch.rand(n, generator=g) * 2 - 1) * 1.4)
    p0, p1 = un(4 * C), un(4 * C)
    w_out = rn(C, inner) * inner ** -0.5 * _spread(C, g, 5)[:, None] if inner else None
    b_out = 0.5 * rn(C) if inner else None
    s1 = torch.minimum(_spread(4 * C, g, 37), 8.0 / p0)
    w1, b1 = rn(4 * C, C) * C ** -0.5 * s1[:, None], 0.3 * rn(4 * C)
    w2, b2 = rn(C, 4 * C) * (4 * C) ** -0.5 * _spread(C, g, 11)[:, None], 0.5 * rn(C)
    w_qkv = rn(n_qkv, C) * C ** -0.5 * _spread(n_qkv, g, 70)[:, None] if n_qkv else None
    b_qkv = 0.5 * rn(n_qkv) if n_qkv else None
    return [w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv, b_qkv]


HARD_M = 40
HARD_CLASSES = {"m0.15": [0, 1, 2, 3], "m4": [4, 5], "m32": [6, 7], "x1e-3": [8, 9], "const": [10], "zero": [11], "x100": [13],
                "unit": list(range(14, 40)) + [12]}
HARD_MASKED = [3, 5, 7, 9, 14, 21]
HARD_KEPT = list(range(4, 15))                   # rows whose bits must not depend on their tile neighbours (the rest is replaced)


def hard_rows(C, inner, seed, loud_neighbours=False):
    """One tile with the row classes of HARD_CLASSES side by side (att is small, and zero on the rows whose x1 must be exactly x).
    loud_neighbours: every row outside HARD_KEPT becomes a x100 row."""
    g = _gen(seed)
    x = torch.randn(HARD_M, C, generator=g)
    x = (x - x.mean(1, keepdim=True)) / x.std(1, keepdim=True) + 0.15        # exact row moments: the classes below are what they say
    att = 0.1 * torch.randn(HARD_M, inner, generator=g) if inner else None
    x[4:6] += 4 - 0.15
    x[6:8] += 32 - 0.15
    x[8:10] *= 1e-3
    x[10] = 3.0
    x[11] = 0.0
    x[13] *= 100.0
    if att is not None:
        att[8:12] = 0.0
        att[13] *= 100.0
    if loud_neighbours:
        other = [i for i in range(HARD_M) if i not in HARD_KEPT]
        x[other] = 100.0 * (torch.randn(len(other), C, generator=g) + 0.15)
        if att is not None:
            att[other] = 10.0 * torch.randn(len(other), inner, generator=g)
    mask = torch.ones(HARD_M)
    mask[HARD_MASKED] = 0.0
    return att, x, mask


def plain_rows(C, inner, seed, M=POOL):
    g = _gen(seed)
    att = torch.randn(M, inner, generator=g) if inner else None
    return att, torch.randn(M, C, generator=g) * 2 + 0.3


RANGE_ROW, RANGE_COLS = 7, [3, 40, 77, 114, 121, 90, 17, 60]


def range_rows(C, inner, seed, signs):
    """plain rows (M = 40), and the same with row RANGE_ROW carrying +-65504 (the largest value an image holds) in eight channels"""
    att, x = plain_rows(C, inner, seed, M=40)
    bad = x.clone()
    bad[RANGE_ROW, RANGE_COLS] = 65504.0 * signs
    return att, x, bad


@functools.lru_cache(maxsize=None)
def chain_case(kind, C, inner, n_qkv, none=""):
    """(operands, mask, fp64 restatement, fp32 twin, budgets) of a case, computed once and never modified.  kind: plain | hard |
    loud (hard with loud neighbours); none: names of biases passed as None, e.g. "b_out,b2"."""
    seed = 1000 + C + 7 * inner + n_qkv + (0 if kind == "plain" else 50000)
    w = chain_weights(C, inner, n_qkv, seed)
    for i, name in enumerate(["w_out", "b_out", "w1", "b1", "p0", "p1", "w2", "b2", "w_qkv", "b_qkv"]):
        if name in none.split(","):
            w[i] = None
    mask = None
    if kind == "plain":
        att, x = plain_rows(C, inner, seed + 1)
    else:
        att, x, mask = hard_rows(C, inner, seed + 1, loud_neighbours=kind == "loud")
    ops = [att, x] + w
    r64 = chain(*ops, mask=mask)
    r32 = chain(*ops, mask=mask, dtype=torch.float32)
    return {"ops": ops, "mask": mask, "r64": r64, "r32": r32, "B": chain_budget(r64, *ops, mask=mask)}


def chain_case_list():
    """Every (kind, C, inner, n_qkv, none) the GPU file launches, with the shapes (qb, ch, M, pair) it launches them at."""
    out = []
    add = lambda key, qb, ch, M, pair: out.append((key, qb, ch, M, pair))
    for C, qb, ch in CHAIN_SHAPES:
        inner, n_qkv = FULL[C]
        key = ("plain", C, inner, n_qkv, "")
        ms = sweep_ms(qb) if (C, qb, ch) in SWEEP_SHAPES else [qb + qb // 2 + 3]
        for M in ms:
            add(key, qb, ch, M, False)
            add(key, qb, ch, M, True)
    # inner in {0, 128 < C}; a q|k|v width that leaves the last pass partly empty (passes of 128 C / 128 columns)
    for C, qb, ch, inner, n_qkv in [(384, 64, 128, 0, 0), (384, 32, 256, 128, 1088), (256, 32, 128, 0, 0), (256, 64, 128, 128, 576),
                                    (128, 64, 128, 0, 0), (128, 32, 128, 128, 352), (384, 48, 256, 384, 0)]:
        add(("plain", C, inner, n_qkv, ""), qb, ch, qb + 9, False)
        if inner:
            add(("plain", C, inner, n_qkv, ""), qb, ch, qb + 9, True)
    for none in ["b_out", "b1", "b2", "b_qkv", "b_out,b1,b2,b_qkv"]:
        add(("plain", 128, 128, 384, none), 64, 128, 70, False)
    for C in (384, 256, 128):                                              # hard rows: one tile; b_out None keeps x1 = x on the exact rows
        inner, n_qkv = FULL[C]
        add(("hard", C, inner, n_qkv, "b_out"), 64, 128, HARD_M, False)
        add(("hard", C, inner, n_qkv, "b_out"), 64, 128, HARD_M, True)
    add(("hard", 256, 0, 0, ""), 64, 128, HARD_M, False)                   # FeedForward alone: x1 IS x on every row
    return out


CONV_N = 384
CONV_SHAPES = [(T, C, 0) for T in (65, 66, 128, 129, 384) for C in (32, 96, 384)] + [(66, 768, 384), (384, 768, 384), (65, 96, 32), (129, 96, 32)]
CONST_GROUP, OFFSET_GROUP = 2, 5


def conv_weights(C, seed):
    """Conv panel and column constants.  Group CONST_GROUP has zero weights and one bias value (its conv output is constant:
    variance 0), group OFFSET_GROUP a bias offset that puts its mean at about 8 standard deviations."""
    g = _gen(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    w = rn(CONV_N, C, 3) / (3 * C) ** 0.5
    bias, gamma, beta = 0.2 * rn(CONV_N), 1 + 0.1 * rn(CONV_N), 0.1 * rn(CONV_N)
    w[48 * CONST_GROUP:48 * (CONST_GROUP + 1)] = 0.0
    bias[48 * CONST_GROUP:48 * (CONST_GROUP + 1)] = 0.75
    bias[48 * OFFSET_GROUP:48 * (OFFSET_GROUP + 1)] += 10.0
    return w, bias, gamma, beta, 0.3 * rn(CONV_N)


def conv_rows(B, T, C, lens, seed, scale=None):
    g = _gen(seed)
    x = torch.randn(B * T, C, generator=g) * 1.3 + 0.1
    if scale is not None:
        x = x * torch.tensor(scale).repeat_interleave(T)[:, None]
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float().reshape(-1)
    return x * mask[:, None], mask                                           # images reach the conv already masked


@functools.lru_cache(maxsize=None)
def conv_case(kind, T, C, c1=0):
    """kind: ragged (lens T, 1, T - 37; time row on even T) | loud (the middle utterance x100) | quiet (its unit twin) | extra (nextra
    closed-form rows) | rows (one time row per utterance).  Returns operands, keyword arguments, restatement, twin and budget."""
    B = 3
    w, bias, gamma, beta, cb = conv_weights(C, 77 + C + T)
    lens = [T, 1, T - 37]
    kw = {}
    if kind in ("loud", "quiet"):
        lens = [T - 5, T, T - 11]
    x, mask = conv_rows(B, T, C, lens, 5 + T + C, scale=[1.0, 100.0, 1.0] if kind == "loud" else None)
    kw["nrows"] = torch.tensor(lens, dtype=torch.int32)
    if kind == "ragged" and T % 2 == 0:
        kw["chbias"] = cb
    if kind == "rows":
        kw["chbias"] = torch.stack([cb, -cb, 2 * cb])
    if kind == "extra":
        lens = [70, 40, 1]
        x, mask = conv_rows(B, T, C, lens, 5 + T + C)
        kw["nrows"] = torch.tensor([min(T, n + 2) for n in lens], dtype=torch.int32)      # the two rows behind the end see the last frames
        kw["nextra"] = torch.tensor([30, 0, 17], dtype=torch.int32)
    ops = [x, w, bias, gamma, beta, mask]
    r64 = conv_gn(*ops, B, T, **kw)
    r32 = conv_gn(*ops, B, T, **kw, dtype=torch.float32)
    return {"ops": ops, "kw": kw, "B": B, "r64": r64, "r32": r32, "budget": conv_gn_budget(r64, *ops, B, T, **kw)}


def bias_stats(bias):
    """per group: mean of the bias row, sum of squared deviations (what the model's packer stores for the closed-form rows)"""
    gb = bias.double().view(8, -1)
    return torch.stack([gb.mean(1), ((gb - gb.mean(1, keepdim=True)) ** 2).sum(1)], 1).float().contiguous()


def conv_case_list():
    return [("ragged", T, C, c1) for T, C, c1 in CONV_SHAPES] + [("loud", 66, 96, 0), ("quiet", 66, 96, 0), ("extra", 128, 96, 0), ("rows", 129, 32, 0)]


@functools.lru_cache(maxsize=None)
def chain_range_case(C=384):
    """The range test's operands: (weights, att, x, x with the out-of-range row) and the fp64 restatement of both."""
    inner, n_qkv = FULL[C]
    w = chain_weights(C, inner, n_qkv, 4242 + C)
    signs = torch.tensor([1.0, -1.0] * 4)
    for _ in range(2):                                   # each spike takes the sign of what the FeedForward adds to it: x2 then leaves the range
        att, x, bad = range_rows(C, inner, 4243 + C, signs)
        r_bad = chain(att, bad, *w)
        d = (r_bad["x2_raw"] - r_bad["x1"])[RANGE_ROW, RANGE_COLS]
        signs = torch.where(d >= 0, 1.0, -1.0).float()
    att, x, bad = range_rows(C, inner, 4243 + C, signs)
    return {"w": w, "att": att, "x": x, "bad": bad, "r_ok": chain(att, x, *w), "r_bad": chain(att, bad, *w)}


RANGE_UTT, RANGE_CHANNELS = 1, [0, 47, 48, 200, 383]


@functools.lru_cache(maxsize=None)
def conv_range_case(T=66, C=96):
    """One time row per utterance; utterance RANGE_UTT's row holds +-70000 in five channels, so its unmasked frames leave the fp16
    range there.  Returns the operands, the two bias-row sets (in range / out of range) and both restatements."""
    base = conv_case("rows", T, C)
    ok = base["kw"]["chbias"].clone()
    bad = ok.clone()
    bad[RANGE_UTT, RANGE_CHANNELS] = torch.tensor([70000.0, -70000.0, 70000.0, -70000.0, 70000.0])
    kw = dict(base["kw"])
    run = lambda cb: conv_gn(*base["ops"], base["B"], T, **dict(kw, chbias=cb))
    return {"ops": base["ops"], "kw": kw, "B": base["B"], "ok": ok, "bad": bad, "r_ok": run(ok), "r_bad": run(bad)}

"""Restatement of the fp32-ROW kernels (fp32 rows in, fp32 rows out) -- gemm_f32_kernel at terms 0 / 2 / 6 (csrc/gemm_f32.hip,
csrc/gemm_epilogue.h), attention_f32_kernel with fp32 I/O (csrc/attention_f32.hip), gn_partial + gn_apply with the fp32 store,
layernorm_kernel and row_stats_kernel (csrc/norm_glue.hip) -- in plain PyTorch on the CPU: the yardstick of tests/test_f32_abi.py
(CPU, against independent torch code) and tests/test_hip_kernels_f32.py (against the device).

Every function takes ``dtype``: torch.float64 is the operation itself (the reference); torch.float32 is the TWIN, fp32 torch on the
same operands in the kernel's algebra (the partial-moment LayerNorm merge where one is used, Mish as x w / (w + 2), SnakeBeta as
z + p1 sin^2(p0 z)).  The twin's error against the reference (e_cpu32) is the unit the device is measured in; nothing here is taken
from what the device returns.  terms = 2 operands are passed through tests/p16_restated.py's split by the CALLER before either form
runs, so the 2^-22 representation error stays outside the bars; terms 0 / 6 operands are exact as given.

Budget ``Bud`` per output element, in units of u = 2^-24 (the convention of tests/fused_restated.py: a stage loses at most u times
the sum of the absolute values of the terms it adds, an input error passes a linear stage multiplied by the absolute weights):
  GEMM        a' = A after mask / LayerNorm;  B_z = sum_k |a'_k| |w_k| + |bias| + |z|          (z = a' . w + bias, its own rounding)
  LayerNorm   prologue from arrays: a' = (a - mean) rstd is two roundings per element: + 2 sum_k |a'_k| |w_k|.
              from partial moments (pm_j, m2_j of 64-column slices): mean = sum_j pm_j / n and var = (sum_j m2_j + 64 sum_j d_j^2) /
              (64 n), d_j = pm_j - mean, are computed by the kernel in fp32:
                dmean = 3 mean_j |pm_j|                                  (a sum of n terms about their mean, a division)
                dvar  = 4 var + 2 mean_j |d_j| (|pm_j| + |mean|)           (d_j is a difference of two numbers of size |mean|)
                drstd / rstd = dvar / (2 (var + eps)) + 2                (division, root)
              and enter as  rstd dmean S + |a' . w| drstd / rstd,  S = sum_k |w_k|.
              terms = 2 splits a' INSIDE the kernel after normalising, so there the 2^-22 = 4 u of that split cannot be moved outside:
              + 4 sum_k |a'_k| |w_k|.
  activation  through its derivative bound plus its own roundings:  relu B_z;  SiLU 1.1 B_z + (4 + |z|) |s| (expf's argument error
              |z| u is a relative error of e^-z);  SnakeBeta B_z (1 + p0 p1) + p1 (1 + |p0 z|) + |s| + (p1 / 2) delta_cos / u with
              delta_cos = 1e-6, the absolute error of the hardware cosine the kernel calls (csrc/device_utils.h sin_sq).
  then        x out_mask, x |out_scale| (+ |s out_scale| for the product's rounding when out_scale != 1), + |res| + |out|.
GroupNorm + Mish, channel LayerNorm: as conv_gn's recursion in tests/fused_restated.py (B_n, B_g, B_m), stated beside the code.
Attention is measured against A = sum_j p_j |v_j|; its allowance is derived in tests/test_hip_kernels_f32.py."""
import torch
import torch.nn.functional as F


U = 2.0 ** -24
DELTA_COS = 1e-6
EPS = 1e-5
ACT_NONE, ACT_RELU, ACT_SILU, ACT_SNAKE = 0, 1, 2, 3
FLOOR = {0: 1.0,            # the result's own rounding
         2: 1.0 + 4.0,      # + the dropped l.l product: |l| / 2^11 <= 2^-11 |h| per operand, 2^-22 = 4 u of sum |a||w| <= 4 Bud
         6: 1.0 + 0.25}     # + the three dropped products of 8-bit terms (|m| <= 2^-9 |x|, |l| <= 2^-18 |x|): m.l + l.m + l.l <=
                            #   (2 2^-27 + 2^-36) |a||w| < 2^-26 |a||w| = u / 4 of sum |a||w|


# ------------------------------------------------------------------------------------------------ GEMM
def gather_taps(a, B, T_in, T_out, tap_off, in_stride):
    """A rows [B*T_in, C] -> the GEMM's K axis [B*T_out, ntaps * C]: tap j reads row t * in_stride + tap_off[j], zero outside [0, T_in)"""
    C = a.shape[1]
    x = a.view(B, T_in, C)
    cols = []
    t = torch.arange(T_out) * in_stride
    for off in tap_off:
        ti = t + off
        ok = (ti >= 0) & (ti < T_in)
        g = x[:, ti.clamp(0, T_in - 1)] * ok.to(a.dtype)[None, :, None]
        cols.append(g)
    return torch.cat(cols, 2).reshape(B * T_out, len(tap_off) * C)


def panel(w):
    """torch weight Linear [N, C] or Conv1d [N, C, k] -> [N, k * C] in the K order of gather_taps (tap major)"""
    return w if w.dim() == 2 else w.permute(0, 2, 1).reshape(w.shape[0], -1)


def merge_parts(part, dtype, eps=EPS):
    """(mean, rstd, extra) from partial moments part [rows, n, 2] = (mean, M2) of 64-column slices: the kernel's equal-count merge"""
    pm, m2 = part[:, :, 0].to(dtype), part[:, :, 1].to(dtype)
    n = part.shape[1]
    mean = pm.sum(1, keepdim=True) / n
    d = pm - mean
    var = (m2.sum(1, keepdim=True) + 64.0 * (d * d).sum(1, keepdim=True)) / (64.0 * n)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmean = 3.0 * pm.abs().mean(1, keepdim=True)
    dvar = 4.0 * var + 2.0 * (d.abs() * (pm.abs() + mean.abs())).mean(1, keepdim=True)
    drel = dvar / (2.0 * (var + eps)) + 2.0
    return mean, rstd, (dmean.double(), drel.double())


def act_fn(z, act, p0, p1, dtype):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_SILU:
        return z / (1.0 + torch.exp(-z))
    if act == ACT_SNAKE:
        return z + p1.to(dtype) * torch.sin(z * p0.to(dtype)) ** 2
    return z


def gemm(a, w, bias=None, *, B, T_in, T_out=None, tap_off=None, in_stride=1, a_mask=None, a_mean=None, a_rstd=None, a_part=None, act=0,
         p0=None, p1=None, res=None, out_mask=None, out_scale=1.0, terms=0, dtype=torch.float64, want_budget=False):
    """a [B*T_in, C] (both channel segments side by side), w as torch stores it.  Returns out [B*T_out, N] in the launch's row order
    (the caller places rows for out_stride / out_off); with want_budget also Bud (fp64, units of u).  res / out_mask are indexed by the
    SAME row order."""
    f = lambda t: None if t is None else t.to(dtype)
    T_out = T_in if T_out is None else T_out
    ntaps = w.shape[2] if w.dim() == 3 else 1
    tap_off = list(tap_off) if tap_off is not None else [j - ntaps // 2 for j in range(ntaps)]
    x = f(a)
    extra = None
    if a_part is not None:
        mean, rstd, extra = merge_parts(a_part, dtype)
        x = (x - mean) * rstd
    elif a_mean is not None:
        x = (x - f(a_mean)[:, None]) * f(a_rstd)[:, None]
    if a_mask is not None:
        x = x * f(a_mask)[:, None]
    ak = gather_taps(x, B, T_in, T_out, tap_off, in_stride)
    wk = f(panel(w))
    lin = ak @ wk.T
    z = lin if bias is None else lin + f(bias)
    s = act_fn(z, act, p0, p1, dtype)
    o = s
    if out_mask is not None:
        o = o * f(out_mask)[:, None]
    if out_scale != 1.0:
        o = o * out_scale
    if res is not None:
        o = o + f(res)
    if not want_budget:
        return o
    assert dtype == torch.float64
    aw = wk.abs()
    prod = ak.abs() @ aw.T
    Bz = prod + z.abs() + (0 if bias is None else bias.double().abs())
    if a_mean is not None or a_part is not None:
        Bz = Bz + 2.0 * prod + (4.0 * prod if terms == 2 else 0.0)
    if extra is not None:
        dmean, drel = extra
        Bz = Bz + rstd * dmean * aw.sum(1)[None] + lin.abs() * drel
    if act == ACT_SILU:
        Bs = 1.1 * Bz + (4.0 + z.abs()) * s.abs()
    elif act == ACT_SNAKE:
        q0, q1 = p0.double(), p1.double()
        Bs = Bz * (1.0 + q0 * q1) + q1 * (1.0 + (q0 * z).abs()) + s.abs() + 0.5 * q1 * (DELTA_COS / U)
    else:
        Bs = Bz
    if out_mask is not None:
        Bs = Bs * out_mask.double()[:, None]
    if out_scale != 1.0:
        Bs = Bs * abs(out_scale) + (s * out_scale).abs()
    if res is not None:
        Bs = Bs + res.double().abs() + o.abs()
    return o, Bs


def place_rows(rows, B, T_out, out_T, out_stride, out_off):
    """indices of the output rows a launch writes, in the launch's row order"""
    b = torch.arange(B * T_out) // T_out
    t = torch.arange(B * T_out) % T_out
    return b * out_T + t * out_stride + out_off


def row_moments(o, dtype=torch.float64):
    """(mean, M2) of every 64-column slice of rows o [M, N]: what stats_out holds, two-pass"""
    M, N = o.shape
    v = o.to(dtype).view(M, N // 64, 64)
    mu = v.mean(2)
    return torch.stack([mu, ((v - mu[:, :, None]) ** 2).sum(2)], 2)


# ------------------------------------------------------------------------------------------------ attention
def attention(qkv, mask, B, T, H, D, scale, mode, klen=None, dtype=torch.float64):
    """packed q|k|v rows [B*T, 3 H D] -> (out [B*T, H D], A = sum_j p_j |v_j|, aux) with aux = dict(L, sv, sq, sk) for the allowance:
    L = sum_j exp(s_j - max_j s), sv = sum over the keys of |v|, sq = sum_d |q_d|, sk = max over the keys of sum_d |k_d|.
    mode 0: mask [B*T] float is ADDED to the logits per key; mode 1: boolean query x key mask.  klen [B]: keys [0, klen[b]).  A row
    with no key is 0."""
    q, k, v = [z.to(dtype).view(B, T, H, D).transpose(1, 2) for z in qkv.split(H * D, dim=1)]
    s = (q @ k.transpose(-1, -2)) * scale
    m = mask.view(B, T)
    allow = torch.ones(B, 1, T, T, dtype=torch.bool)
    if mode == 0:
        s = s + m.to(dtype).view(B, 1, 1, T)
    else:
        allow = (m[:, None, :, None] * m[:, None, None, :]) != 0
    if klen is not None:
        allow = allow & (torch.arange(T)[None, None, None, :] < klen.view(B, 1, 1, 1))
    s = s.masked_fill(~allow, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    L = e.sum(-1, keepdim=True)
    p = torch.where(L > 0, e / L.clamp_min(1e-38), torch.zeros_like(e))
    back = lambda t: t.transpose(1, 2).reshape(B * T, -1)
    keyed = allow.to(dtype).expand(B, H, T, T)
    aux = dict(L=back(L.expand(B, H, T, D).clamp_min(1e-38)), sv=back(keyed @ v.abs()), sq=back(q.abs().sum(-1, keepdim=True).expand(B, H, T, D)),
               sk=back((keyed * k.abs().sum(-1)[:, :, None, :]).amax(-1, keepdim=True).expand(B, H, T, D)))
    return back(p @ v), back(p @ v.abs()), aux


# ------------------------------------------------------------------------------------------------ GroupNorm + Mish
def mish(g, dtype):
    if dtype == torch.float64:
        return F.mish(g)
    n = torch.exp2(g * 1.44269504088896340736)
    w = n * (n + 2.0)
    return torch.where(g > 20.0, g, g * (w / (w + 2.0)))


def groupnorm_mish(y, gamma, beta, mask, B, T, *, G=8, chbias=None, res=None, nrows=None, nextra=None, bias_row=None, eps=EPS,
                   dtype=torch.float64, want_budget=False):
    """y [B*T, C]: statistics of utterance b over its first nrows[b] frames (None: T) plus nextra[b] copies of bias_row [C];
    out = Mish(GN(y) gamma + beta) mask; (out + chbias_b) mask when chbias ([C] or [B, >= C]); + res.  An utterance without a single
    row in its statistics is not defined (the kernel divides by the count).
    Budget: B_n = rs (|y - mu| + mean_g |y| + |mu|) + 3 |n| (the subtraction, the fp32 mean and variance of the group, the root);
    B_g = |gamma| B_n + |n gamma| + |beta| + |g|;  B_m = 1.1 B_g + (8 + 2 |g|) |m|;  B_o = (B_m + |cb| + |o|) mask + |res| + |o|."""
    C = y.shape[1]
    f = lambda t: None if t is None else t.to(dtype)
    yd = f(y).view(B, T, G, C // G)
    mu = torch.empty(B, 1, G, 1, dtype=dtype)
    var = torch.empty(B, 1, G, 1, dtype=dtype)
    for b in range(B):
        n = T if nrows is None else min(T, int(nrows[b]))
        rows = yd[b, :n]
        if nextra is not None and int(nextra[b]) > 0:
            rows = torch.cat([rows, f(bias_row).view(1, G, C // G).expand(int(nextra[b]), G, C // G)], 0)
        mu[b, 0, :, 0] = rows.mean((0, 2))
        var[b, 0, :, 0] = ((rows - mu[b, 0, :, 0][None, :, None]) ** 2).mean((0, 2))
    rs = 1.0 / torch.sqrt(var + eps)
    n_ = ((yd - mu) * rs).reshape(B * T, C)
    g = n_ * f(gamma) + f(beta)
    m = mish(g, dtype)
    mk = f(mask)[:, None]
    o = m * mk
    cb = None
    if chbias is not None:
        cb = f(chbias)[:, :C].repeat_interleave(T, 0) if chbias.dim() == 2 else f(chbias)[None]
        o = (o + cb) * mk
    if res is not None:
        o = o + f(res)
    if not want_budget:
        return o
    assert dtype == torch.float64
    gmean_abs = yd.abs().mean((1, 3), keepdim=True)
    Bn = (rs * ((yd - mu).abs() + gmean_abs + mu.abs())).reshape(B * T, C) + 3.0 * n_.abs()
    Bg = gamma.double().abs() * Bn + (n_ * gamma.double()).abs() + beta.double().abs() + g.abs()
    Bm = 1.1 * Bg + (8.0 + 2.0 * g.abs()) * m.abs()
    Bo = (Bm + (0 if cb is None else cb.abs()) + (m * mk).abs()) * mk.abs()
    if res is not None:
        Bo = Bo + res.double().abs()
    return o, Bo + o.abs()


def gn_bias_stats(bias_row, G=8):
    """per group (mean of the bias row, sum of squared deviations of ONE copy): GnApplyArgs::bias_stats, as the packer computes it"""
    bg = bias_row.double().view(G, -1)
    return torch.stack([bg.mean(1), ((bg - bg.mean(1, keepdim=True)) ** 2).sum(1)], 1).float().contiguous()


# ------------------------------------------------------------------------------------------------ channel LayerNorm, row statistics
def row_stats(x, eps=EPS, dtype=torch.float64):
    v = x.to(dtype)
    mean = v.mean(1)
    return mean, 1.0 / torch.sqrt(((v - mean[:, None]) ** 2).mean(1) + eps)


def channel_layernorm(x, B, T, gamma, beta, *, eps=EPS, act=0, film=None, mask=None, dtype=torch.float64, want_budget=False):
    """y = act(LN_C(x) gamma + beta) [* film_g[b] + film_b[b]] [* mask[row]];  film [B, 2 C] = gamma | beta.
    Budget: B_n = rs (|x - mu| + mean_c |x| + |mu|) + 3 |n|;  B_g = |gamma| B_n + |n gamma| + |beta| + |g|;  SiLU as in the GEMM;
    FiLM: B |fg| + |s fg| + |fb| + |out|;  x mask."""
    C = x.shape[1]
    f = lambda t: None if t is None else t.to(dtype)
    v = f(x)
    mu = v.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + eps)
    n_ = (v - mu) * rs
    g = n_ * f(gamma) + f(beta)
    s = act_fn(g, act, None, None, dtype)
    o = s
    if film is not None:
        fg, fb = f(film)[:, :C].repeat_interleave(T, 0), f(film)[:, C:].repeat_interleave(T, 0)
        o = o * fg + fb
    if mask is not None:
        o = o * f(mask)[:, None]
    if not want_budget:
        return o
    assert dtype == torch.float64
    Bn = rs * ((v - mu).abs() + v.abs().mean(1, keepdim=True) + mu.abs()) + 3.0 * n_.abs()
    Bg = gamma.double().abs() * Bn + (n_ * gamma.double()).abs() + beta.double().abs() + g.abs()
    Bs = 1.1 * Bg + (4.0 + g.abs()) * s.abs() if act == ACT_SILU else Bg
    if film is not None:
        Bs = Bs * fg.abs() + (s * fg).abs() + fb.abs()
    if mask is not None:
        Bs = Bs * mask.double().abs()[:, None]
    return o, Bs + o.abs()


# ------------------------------------------------------------------------------------------------ the rule
def judge(hip, cpu32, ref, bud, floor):
    """The one rule, the measure of tests/test_hip_kernels_fused.py: e = max over the elements of |value - ref| / (u Bud), each element
    in units of its OWN budget, and e_hip <= 8 e_cpu32 + floor.  An element whose budget is 0 must be exact.  Returns (ok, e_hip,
    e_cpu32, e_hip / bar)."""
    if ref.numel() == 0:
        return True, 0.0, 0.0, 0.0
    unit = U * bud
    eh, ec = (hip.double() - ref).abs(), (cpu32.double() - ref).abs()
    exact = unit == 0
    if bool((eh[exact] != 0).any()):
        return False, float("inf"), 0.0, float("inf")
    unit = unit.clamp_min(1e-300)
    e_hip, e_cpu = (eh / unit).max().item(), (ec / unit).max().item()
    bar = 8.0 * e_cpu + floor
    return e_hip <= bar, e_hip, e_cpu, e_hip / bar

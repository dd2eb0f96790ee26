"""Own-words fp64 restatements for the style encoder's parameter gradients (csrc/style_grad.hip): the encoder itself with autograd,
the plain definition of the Conv1d(k5, pad 2) weight gradient, and the backward pass GIVEN a tape of activations together with a
running bound on what fp32 arithmetic in the device's summation orders may lose against it; and integer cases on which fp32 loses
nothing, with the check that they are such cases.  Nothing here calls the library."""
import math

import torch
import torch.nn.functional as F

TAPS = 5
U = 2.0 ** -24            # unit roundoff of fp32


def fp64_bound(r, n):
    """tests/test_hip_spk_grad.py: relative to the sum of the absolute terms, n terms added with serial runs of r."""
    return 2 * (r + math.log2(max(n / r, 1.0)) + 4) * U


def chunk_rows(B, T):
    """Rows per chunk of the weight-gradient kernel's reduction over B T rows -- a function of the shape alone (include/mtts.h
    mtts_conv_wgrad): 256 up to 4096 rows, beyond that the multiple of 256 that gives at most 16 chunks."""
    return 256 * max(1, -(-(B * T) // (256 * 16)))


def wgrad_serial_run(B, T):
    """Longest serial accumulation of the weight-gradient kernel: a chunk's rows enter ONE fp32 FMA chain in row order (chunk_rows
    terms), then the chunks are added in chunk order (chunks - 1 more additions)."""
    ch = chunk_rows(B, T)
    return ch + -(-(B * T) // ch) - 1


def bias_serial_run(B, T):
    """... of the bias gradient: four phases of chunk_rows / 4 rows each, three additions to combine them, then the chunks in order."""
    ch = chunk_rows(B, T)
    return ch // 4 + 3 + -(-(B * T) // ch) - 1


def param_names(n_layers):
    names = [f"convs.{i}.{p}" for i in range(n_layers) for p in ("weight", "bias")]
    return names + [f"proj_{h}.{p}" for h in ("enc", "dur") for p in ("weight", "bias")]


def n_layers_of(sd):
    n = 0
    while f"convs.{n}.weight" in sd:
        n += 1
    return n


def prefix_mask(lengths, T, dtype=torch.float64):
    return (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).to(dtype)              # [B, T]


def style_forward(sd, mel, lengths, dtype=torch.float64):
    """StyleEncoder.forward (reference style_encoder.py:60-72) on a batch: mel [B, n_feats, T], lengths [B] -> e_enc, e_dur [B, E]."""
    mask = prefix_mask(lengths, mel.shape[-1], dtype)[:, None, :]
    x = mel.to(dtype)
    for i in range(n_layers_of(sd)):
        x = torch.relu(F.conv1d(x * mask, sd[f"convs.{i}.weight"].to(dtype), sd[f"convs.{i}.bias"].to(dtype), padding=2))
    pooled = (x * mask).sum(2) / mask.sum(2).clamp(min=1)
    return (F.linear(pooled, sd["proj_enc.weight"].to(dtype), sd["proj_enc.bias"].to(dtype)),
            F.linear(pooled, sd["proj_dur.weight"].to(dtype), sd["proj_dur.bias"].to(dtype)))


def style_param_grads(sd, mel, lengths, g_enc, g_dur, dtype=torch.float64):
    """Autograd gradient of sum_b <g_enc_b, e_enc_b> + <g_dur_b, e_dur_b> with respect to every parameter, from the inputs."""
    leaves = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in param_names(n_layers_of(sd))}
    e_enc, e_dur = style_forward(leaves, mel, lengths, dtype)
    ((e_enc * g_enc.to(dtype)).sum() + (e_dur * g_dur.to(dtype)).sum()).backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}, (e_enc.detach(), e_dur.detach())


def flat(grads, n_layers):
    return torch.cat([grads[k].reshape(-1) for k in param_names(n_layers)])


# ------------------------------------------------------------------------------------------------ the conv weight gradient
def conv_wgrad_loops(dz, x, lengths):
    """THE definition, as three plain loops: dz [B, T, cout], x [B, T, cin] fp64, lengths [B] ->
    dW[co, ci, k] = sum over b, t < len_b, k with 0 <= t + k - 2 < len_b of dz[b, t, co] x[b, t + k - 2, ci]."""
    B, T, cout = dz.shape
    dw = torch.zeros(cout, x.shape[2], TAPS, dtype=torch.float64)
    for b in range(B):
        n = max(0, min(int(lengths[b]), T))
        for t in range(n):
            for k in range(TAPS):
                tt = t + k - TAPS // 2
                if 0 <= tt < n:
                    dw[:, :, k] += torch.outer(dz[b, t], x[b, tt])
    return dw


def conv_wgrad(dz, x, lengths):
    """The same sums, one matrix product per tap, and the sums of the ABSOLUTE terms (what an error bound scales with): (dW, |dW|)."""
    B, T, _ = dz.shape
    m = prefix_mask(lengths, T)[:, :, None]
    dz = torch.nan_to_num(dz.double()) * m
    x = torch.nan_to_num(x.double()) * m
    xp = F.pad(x, (0, 0, TAPS // 2, TAPS // 2))                                                 # zero frames around every clip
    val = torch.stack([torch.einsum("bto,bti->oi", dz, xp[:, k:k + T]) for k in range(TAPS)], dim=2)
    mag = torch.stack([torch.einsum("bto,bti->oi", dz.abs(), xp[:, k:k + T].abs()) for k in range(TAPS)], dim=2)
    return val, mag


def conv_wgrad_by_chunk(dz, x, lengths, chunk):
    """conv_wgrad cut the way the device cuts it: chunk c holds the terms of the rows r = b T + t in [c chunk, (c + 1) chunk) -- the
    rows of dz; a tap may read a frame of x that lies in a neighbouring chunk.
    -> (dW [chunks, cout, cin, 5], |dW| likewise, d bias [chunks, cout], |d bias| likewise); their sums over the chunks are the whole."""
    B, T, _ = dz.shape
    m = prefix_mask(lengths, T)[:, :, None]
    dz = torch.nan_to_num(dz.double()) * m
    x = torch.nan_to_num(x.double()) * m
    xp = F.pad(x, (0, 0, TAPS // 2, TAPS // 2))
    chunks = -(-(B * T) // chunk)

    def cut(a):                                                                                 # [B, T, c] -> [chunks, chunk, c], zero rows behind the last
        return F.pad(a.reshape(B * T, -1), (0, 0, 0, chunks * chunk - B * T)).reshape(chunks, chunk, -1)
    dzc = cut(dz)
    val = torch.stack([torch.einsum("cro,cri->coi", dzc, cut(xp[:, k:k + T])) for k in range(TAPS)], dim=3)
    mag = torch.stack([torch.einsum("cro,cri->coi", dzc.abs(), cut(xp[:, k:k + T].abs())) for k in range(TAPS)], dim=3)
    return val, mag, dzc.sum(1), dzc.abs().sum(1)


# ------------------------------------------------------------------------------------------------ arithmetic in which fp32 is exact
# A sum of integers whose ABSOLUTE values add up to less than 2^24 is exact in fp32 in any order and any grouping: every partial sum
# is an integer of magnitude below 2^24, hence a float.  On such operands a device kernel has nothing to round, and must return the
# fp64 result itself: one dropped, doubled or mis-masked term changes an element by a whole number.
EXACT_BELOW = 2.0 ** 24
TAPE_LENGTHS = (0, 1, 2, 4, 8, 16, 32, 64, 128)          # 1 / max(len, 1) is a power of two: the mean pool's factor is exact as well


def is_integer(t):
    """Every element that is not NaN (the mark of what is never read as data) is a whole number."""
    t = torch.as_tensor(t)
    t = t[~torch.isnan(t)]
    return bool(torch.isfinite(t).all() and (t == t.round()).all())


def integer_wgrad_case(B, T, lengths, cin, cout, seed):
    """Operands of the weight-gradient entry with integers in [-2, 2]: dz [B, T, cout], x [B, T, cin + 4] (fp32).  NaN wherever nothing
    may be read as data: frames at t >= len_b of both, the padding columns of x."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (B, T, cin + 4), generator=g).float()
    dz = torch.randint(-2, 3, (B, T, cout), generator=g).float()
    x[:, :, cin:] = float("nan")
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")
        dz[b, n:] = float("nan")
    return dz, x


def wgrad_abs_sums(dz, x, lengths):
    """The largest sum of absolute terms of any element of dW and of d bias (conv_wgrad's second result)."""
    _, mag = conv_wgrad(dz, x, lengths)
    m = prefix_mask(lengths, dz.shape[1])[:, :, None]
    return {"dW": mag.max().item(), "d bias": (torch.nan_to_num(dz.double()) * m).abs().sum((0, 1)).max().item()}


def integer_tape_case(cfg, B, T, lengths, seed, density=0.25):
    """A state dict and a HAND-WRITTEN tape for the backward, all integers: cfg = (n_feats, hidden, n_layers, emb), lengths from
    TAPE_LENGTHS.  -> (sd, x0, hs, pooled, g_enc, g_dur), fp32:
      sd       every tensor in {-1, 0, 1}, a matrix element non-zero with probability ``density``
      x0       [B, T, n_feats] in [-2, 2], zero beyond a clip's length
      hs[l]    [B, T, hidden] in {0, 1, 2}, half of them 0 (the ReLU gates), zero beyond a clip's length
      pooled   [B, hidden] in {0 .. 3}
      g_enc, g_dur [B, emb] = max(len_b, 1) times {-1, 0, 1} (non-zero with probability ``density``): d pooled / max(len_b, 1), and
               with it every later quantity, is an integer.
    The tape is not the forward of anything; the backward takes it as given."""
    n_feats, hidden, L, E = cfg
    assert len(lengths) == B and all(n in TAPE_LENGTHS and n <= T for n in lengths), lengths
    g = torch.Generator().manual_seed(seed)

    def signs(shape, p):
        return (2.0 * torch.randint(0, 2, shape, generator=g) - 1) * (torch.rand(shape, generator=g) < p)
    sd = {}
    for i in range(L):
        sd[f"convs.{i}.weight"] = signs((hidden, n_feats if i == 0 else hidden, TAPS), density)
        sd[f"convs.{i}.bias"] = signs((hidden,), 0.5)
    for h in ("enc", "dur"):
        sd[f"proj_{h}.weight"] = signs((E, hidden), density)
        sd[f"proj_{h}.bias"] = signs((E,), 0.5)
    m = prefix_mask(lengths, T, torch.float32)[:, :, None]
    x0 = torch.randint(-2, 3, (B, T, n_feats), generator=g).float() * m
    hs = [torch.randint(1, 3, (B, T, hidden), generator=g).float() * (torch.rand(B, T, hidden, generator=g) < 0.5) * m for _ in range(L)]
    pooled = torch.randint(0, 4, (B, hidden), generator=g).float()
    n = torch.tensor(lengths).clamp(min=1).float()[:, None]
    return sd, x0, hs, pooled, n * signs((B, E), density), n * signs((B, E), density)


def tape_abs_sums(sd, x0, hs, pooled, lengths, g_enc, g_dur):
    """For every ACCUMULATED quantity of backward_from_tape's chain, the largest fp64 sum of the absolute values of the terms of any
    of its elements: the projections' gradients, d pooled, every layer's dW and d bias, every data gradient."""
    L = n_layers_of(sd)
    B, T, _ = x0.shape
    x0, pooled, g_enc, g_dur = x0.double(), pooled.double(), g_enc.double(), g_dur.double()
    hs = [h.double() for h in hs]
    mask = prefix_mask(lengths, T)
    n = torch.as_tensor(lengths).clamp(min=0, max=T).double()
    sums = {}
    for name, g in (("proj_enc", g_enc), ("proj_dur", g_dur)):
        sums[f"{name}.weight"] = (g.abs().t() @ pooled.abs()).max().item()
        sums[f"{name}.bias"] = g.abs().sum(0).max().item()
    w_all = torch.cat([sd["proj_enc.weight"], sd["proj_dur.weight"]]).double()
    g_all = torch.cat([g_enc, g_dur], dim=1)
    sums["d pooled"] = (g_all.abs() @ w_all.abs()).max().item()
    dz = (g_all @ w_all)[:, None, :] / n.clamp(min=1)[:, None, None] * (hs[L - 1] > 0).double() * mask[:, :, None]
    for l in range(L - 1, -1, -1):
        _, mag = conv_wgrad(dz, hs[l - 1] if l else x0, lengths)
        sums[f"convs.{l}.weight"] = mag.max().item()
        sums[f"convs.{l}.bias"] = dz.abs().sum((0, 1)).max().item()
        if l == 0:
            break
        w = sd[f"convs.{l}.weight"].double()
        sums[f"d h{l - 1}"] = F.conv_transpose1d(dz.abs().transpose(1, 2), w.abs(), padding=2).max().item()
        dz = F.conv_transpose1d(dz.transpose(1, 2), w, padding=2).transpose(1, 2) * (hs[l - 1] > 0).double() * mask[:, :, None]
    return sums


def fp32_is_exact_on(sums, *operands):
    """The exactness precondition: integer operands, every sum of absolute terms below 2^24."""
    return all(is_integer(t) for t in operands) and all(v < EXACT_BELOW for v in sums.values())


# The cases of tests/test_hip_style_grad.py beyond one chunk length, here so that tests/test_style_grad_abi.py can hold their
# preconditions without a device.
def ragged(B, T, seed):
    """B >= 6 lengths: T, 0, 1, 2 first, then draws from 3 .. T - 1, the last two clips full (live rows on both sides of the last clip
    boundary and in the last chunk)."""
    draws = torch.randint(3, T, (B,), generator=torch.Generator().manual_seed(seed)).tolist()
    return [T, 0, 1, 2] + draws[4:B - 2] + [T, T]


#   rows: (B, T, lengths)                                      chunk  chunks
WGRAD_ROWS = {
    4096: (8, 512, ragged(8, 512, 1)),                         # 256    16     the most chunks at the smallest chunk length
    4097: (1, 4097, [4097]),                                   # 512     9     the last chunk holds one row (one clip: one length)
    8192: (16, 512, ragged(16, 512, 2)),                       # 512    16
    8193: (3, 2731, [2731, 2, 2731]),                          # 768    11     the last chunk: 16 slabs of 32 rows and 1 row; the clip
                                                               #               boundaries 2731, 5462 are on no slab or chunk boundary
    19200: (32, 600, ragged(32, 600, 3)),                      # 1280   15     the measured training shape; 600 = 18 slabs + 24 rows
}
WGRAD_CHANNELS = {rows: [(4, 4), (20, 32)] + ([(100, 256)] if rows in (4097, 19200) else []) for rows in WGRAD_ROWS}
WGRAD_CASES = [(rows, cin, cout) for rows in WGRAD_ROWS for cin, cout in WGRAD_CHANNELS[rows]]
# clips shorter than the tap span and than the bias kernel's 4-row stride: (B, T), lengths drawn from 0 .. T
SHORT_CLIPS = [(300, 1), (200, 2), (130, 3)]
SHORT_CASES = [(B, T, cin, cout) for B, T in SHORT_CLIPS for cin, cout in ((4, 4), (20, 32))]


def short_lengths(B, T):
    return torch.randint(0, T + 1, (B,), generator=torch.Generator().manual_seed(10 * T + 7)).tolist()


#   name: (cfg, B, T, lengths) -- 4800 rows each: chunk 512, 10 chunks
TAPE_CASES = {
    "tiny": ((20, 32, 2, 16), 32, 150, [TAPE_LENGTHS[(4 * b + 8) % 9] for b in range(32)]),
    "prod": ((100, 256, 4, 96), 8, 600, [128, 0, 1, 2, 64, 4, 16, 128]),
}


# ------------------------------------------------------------------------------------------------ the backward given a tape
def backward_from_tape(sd, x0, hs, pooled, lengths, g_enc, g_dur):
    """The backward pass in fp64 with the activations as CONSTANTS: x0 [B, T, n_feats] the masked input rows, hs[l] [B, T, hidden] the
    ReLU outputs, pooled [B, hidden] (a device's tape: no gate can differ between the two sides).  Returns (grads, bounds): per
    parameter tensor the fp64 gradient and, per element, what an fp32 implementation in the device's summation orders may differ by:
    each step's fp64_bound(r, n) on the sum of its absolute terms, plus the bound carried in by its inputs (propagated through the
    absolute values of the step's factors)."""
    L = n_layers_of(sd)
    B, T, _ = x0.shape
    E = g_enc.shape[1]
    x0, pooled, g_enc, g_dur = x0.double(), pooled.double(), g_enc.double(), g_dur.double()
    hs = [h.double() for h in hs]
    mask = prefix_mask(lengths, T)
    n = torch.as_tensor(lengths).clamp(min=0, max=T).double()
    grads, bounds = {}, {}
    for name, g in (("proj_enc", g_enc), ("proj_dur", g_dur)):          # sums over the batch in batch order: r = n = B
        grads[f"{name}.weight"] = g.t() @ pooled
        bounds[f"{name}.weight"] = fp64_bound(B, B) * (g.abs().t() @ pooled.abs())
        grads[f"{name}.bias"] = g.sum(0)
        bounds[f"{name}.bias"] = fp64_bound(B, B) * g.abs().sum(0)
    w_all = torch.cat([sd["proj_enc.weight"], sd["proj_dur.weight"]]).double()
    g_all = torch.cat([g_enc, g_dur], dim=1)
    d_pooled = g_all @ w_all                                              # 2 E terms in output order: r = n = 2 E
    e_pooled = fp64_bound(2 * E, 2 * E) * (g_all.abs() @ w_all.abs())
    inv_n = 1.0 / n.clamp(min=1)
    gate = (hs[L - 1] > 0).double() * mask[:, :, None]
    dz = d_pooled[:, None, :] * inv_n[:, None, None] * gate
    ez = (e_pooled[:, None, :] * inv_n[:, None, None] + 3 * U * dz.abs()) * gate       # 1 / n rounded, the product rounded (+ 1 slack)
    r_w, r_b = wgrad_serial_run(B, T), bias_serial_run(B, T)
    for l in range(L - 1, -1, -1):
        xin = hs[l - 1] if l else x0
        val, mag = conv_wgrad(dz, xin, lengths)
        _, carried = conv_wgrad(ez, xin, lengths)
        grads[f"convs.{l}.weight"] = val
        bounds[f"convs.{l}.weight"] = fp64_bound(r_w, B * T) * mag + carried
        grads[f"convs.{l}.bias"] = dz.sum((0, 1))
        bounds[f"convs.{l}.bias"] = fp64_bound(r_b, B * T) * dz.abs().sum((0, 1)) + ez.sum((0, 1))
        if l == 0:
            break
        # data gradient: d in[b, t, ci] = sum over k, co of dz[b, t - k + 2, co] W[co, ci, k], zero frames around every clip --
        # the transposed convolution; 5 hidden terms per element in whatever order the GEMM adds them: r = n = 5 hidden
        w = sd[f"convs.{l}.weight"].double()
        K = TAPS * w.shape[0]
        d_in = F.conv_transpose1d(dz.transpose(1, 2), w, padding=2).transpose(1, 2)
        a_in = F.conv_transpose1d(dz.abs().transpose(1, 2), w.abs(), padding=2).transpose(1, 2)
        c_in = F.conv_transpose1d(ez.transpose(1, 2), w.abs(), padding=2).transpose(1, 2)
        gate = (hs[l - 1] > 0).double() * mask[:, :, None]
        dz = d_in * gate
        ez = (fp64_bound(K, K) * a_in + c_in) * gate
    return grads, bounds


# ------------------------------------------------------------------------------------------------ smooth-L1 and AdamW
def smooth_l1_sum(d, beta):
    """Sum of the reference's smooth-L1 terms (style_encoder.py:133-143): 0.5 d^2 / beta below beta, |d| - 0.5 beta from beta on."""
    a = d.abs()
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta).sum()


def smooth_l1_seed(d, beta):
    """Its derivative: clamp(d / beta, -1, 1)."""
    return (d / beta).clamp(-1.0, 1.0)


def smooth_l1_terms(d, beta):
    a = d.abs()
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta)


def match_grad(oracle, sd, hp, x, x_lengths, p_enc, p_dur, mu_ref, logw_ref, beta_mu=0.002, beta_logw=0.004, dtype=torch.float64):
    """The matching losses of the reference's style training (style_encoder.py:119-143) through the oracle's text encoder, the way
    tests/spk_grad_restated.py goes through it: its outputs under the predicted rows p_enc, p_dur [B, E] against the constants
    mu_ref [B, F, Tx], logw_ref [B, 1, Tx], smooth-L1 summed per utterance over the tokens x < len_b.
    -> g_enc = d ac_sum_b / d p_enc[b], g_dur = d rh_sum_b / d p_dur[b], ac_sum, rh_sum [B], mu_x, logw.  The reference detaches the
    duration predictor's input (text_encoder.py:404), so the rhythm loss does not reach p_enc; the oracle does not, hence the two
    gradients are taken separately.  Plain-op attention: a padded query has no allowed key."""
    B, Tx = x.shape
    sdd = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}
    p_enc = p_enc.detach().to(dtype).clone().requires_grad_(True)
    p_dur = p_dur.detach().to(dtype).clone().requires_grad_(True)
    mu_x, logw, _ = oracle.text_encoder_forward(sdd, hp, x, x_lengths, p_enc, p_dur, use_torch_sdpa=False)
    mask = prefix_mask(x_lengths, Tx, dtype)[:, None, :]
    ac = (smooth_l1_terms(mu_x - mu_ref.to(dtype), beta_mu) * mask).sum((1, 2))
    rh = (smooth_l1_terms(logw - logw_ref.to(dtype).reshape(B, 1, Tx), beta_logw) * mask).sum((1, 2))
    g_enc, = torch.autograd.grad(ac.sum(), p_enc, retain_graph=True)
    g_dur, = torch.autograd.grad(rh.sum(), p_dur)
    return {"g_enc": g_enc, "g_dur": g_dur, "ac_sum": ac.detach(), "rh_sum": rh.detach(), "mu_x": mu_x.detach(), "logw": logw.detach()}


def row_error(g, g64):
    """max|g - g64| / max|g64| per row -> [B] (float64)."""
    g, g64 = torch.as_tensor(g).double().cpu(), torch.as_tensor(g64).double().cpu()
    return (g - g64).abs().amax(1) / g64.abs().amax(1)


def adamw_step(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4):
    """One decoupled-weight-decay Adam step (Loshchilov & Hutter) on tensors of any dtype; returns the new (p, m, v).  step counts
    from 1."""
    p = p * (1 - lr * weight_decay)
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    m_hat = m / (1 - betas[0] ** step)
    v_hat = v / (1 - betas[1] ** step)
    return p - lr * m_hat / (v_hat.sqrt() + eps), m, v


def train_loop(oracle, sd, hp, style_sd, batches, dtype=torch.float64, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4,
               beta_mu=0.002, beta_logw=0.004):
    """The reference's style training (style_encoder.py:119-160) on the CPU, one AdamW step per batch of ``batches`` =
    (x, x_lengths, mel_fine, mel_fine_lengths, spks): Matcha (``sd``) frozen, the style encoder's parameters ``style_sd`` trained.
    -> (history of (acoustic_loss, rhythm_loss, emb_dist_enc, emb_dist_dur) before each step, the parameters after every step)."""
    sdd = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}
    names = param_names(n_layers_of(style_sd))
    params = {k: style_sd[k].detach().to(dtype).clone() for k in names}
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v2 = {k: torch.zeros_like(v) for k, v in params.items()}
    history, trail = [], []
    for step, (x, x_len, mel, mel_len, spks) in enumerate(batches, 1):
        B, Tx = x.shape
        leaves = {k: p.clone().requires_grad_(True) for k, p in params.items()}
        p_enc, p_dur = style_forward(leaves, mel, mel_len, dtype)
        r_enc, r_dur = sdd["speaker_embeddings_enc.weight"][spks], sdd["speaker_embeddings_dur.weight"][spks]
        with torch.no_grad():
            mu_ref, logw_ref, _ = oracle.text_encoder_forward(sdd, hp, x, x_len, r_enc, r_dur, use_torch_sdpa=False)
        mu_x, logw, _ = oracle.text_encoder_forward(sdd, hp, x, x_len, p_enc, p_dur, use_torch_sdpa=False)
        mask = prefix_mask(x_len, Tx, dtype)[:, None, :]
        tokens = mask.sum()
        ac = (smooth_l1_terms(mu_x - mu_ref, beta_mu) * mask).sum() / tokens
        rh = (smooth_l1_terms(logw - logw_ref, beta_logw) * mask).sum() / tokens
        # the reference detaches the duration predictor's input (text_encoder.py:404): the rhythm loss reaches p_dur alone
        g_enc, = torch.autograd.grad(ac, p_enc, retain_graph=True)
        g_dur, = torch.autograd.grad(rh, p_dur, retain_graph=True)
        grads = torch.autograd.grad((p_enc * g_enc.detach()).sum() + (p_dur * g_dur.detach()).sum(), [leaves[k] for k in names], allow_unused=True)
        with torch.no_grad():
            history.append((ac.item(), rh.item(), (p_enc - r_enc).pow(2).mean(1).sqrt().mean().item(),
                            (p_dur - r_dur).pow(2).mean(1).sqrt().mean().item()))
            for k, g in zip(names, grads):
                g = torch.zeros_like(params[k]) if g is None else g
                params[k], m[k], v2[k] = adamw_step(params[k], g, m[k], v2[k], step, lr, betas, eps, weight_decay)
        trail.append({k: p.clone() for k, p in params.items()})
    return history, trail

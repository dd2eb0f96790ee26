"""Yardstick of the duration predictor's parameter gradients (csrc/dp_grad.hip; include/mtts.h mtts_dp_grad): the duration loss and every
parameter gradient restated from the formulas of the header, in any dtype and in the documented summation orders, the same gradient by
torch.autograd through the oracle's predictor, the three unit reductions, and an AdamW loop around the restatement.

Layout of the flat vector (keys below ``encoder.proj_w.``): state-dict order -- spk_proj.weight, spk_proj.bias, then per layer
conv_layers.i.weight, conv_layers.i.bias, norm_layers.i.gamma, norm_layers.i.beta, then proj.weight, proj.bias.

The chunk scheme of the row reductions: M = B T rows r = b T + t in chunks of chunk_rows(M) = 256 max(1, ceil(M / 4096)) rows; inside a
chunk four phases p take the rows r0 + p, r0 + p + 4, ... in row order and are combined as ((p0 + p1) + p2) + p3; the chunks are added in
chunk order.  Rows with t >= len_b take no part."""
import math

import torch
import torch.nn.functional as F

PREFIX = "encoder.proj_w."
U = 2.0 ** -24
EPS = 1e-5


def fp64_bound(r, n):
    """tests/test_hip_spk_grad.py's bound of an fp32 sum of n terms whose longest serial chain has r additions, per unit of sum|terms|."""
    return 2 * (r + math.log2(max(n / r, 1.0)) + 4) * 2.0 ** -24


def chunk_rows(M):
    return 256 * max(1, -(-M // 4096))


def chunks_of(M):
    return -(-M // chunk_rows(M))


def serial_run(M):
    """Longest serial chain of the phased chunk scheme: a phase's rows, the three additions that combine the phases, the chunks."""
    return chunk_rows(M) // 4 + 3 + chunks_of(M) - 1


def layout(hp):
    """[(key, offset, shape)] of the flat vector."""
    e, Sd = hp.encoder, hp.spk_emb_dim
    Fd, k, Hd = e.dp_filter_channels, e.dp_kernel_size, e.n_channels + Sd
    shapes = [("spk_proj.weight", (2 * Fd, Sd)), ("spk_proj.bias", (2 * Fd,))]
    for i in range(e.dp_n_layers):
        shapes += [(f"conv_layers.{i}.weight", (Fd, Hd if i == 0 else Fd, k)), (f"conv_layers.{i}.bias", (Fd,)),
                   (f"norm_layers.{i}.gamma", (Fd,)), (f"norm_layers.{i}.beta", (Fd,))]
    shapes += [("proj.weight", (1, Fd, 1)), ("proj.bias", (1,))]
    out, off = [], 0
    for key, shape in shapes:
        out.append((key, off, shape))
        off += math.prod(shape)
    return out


def param_count(hp):
    key, off, shape = layout(hp)[-1]
    return off + math.prod(shape)


def params_of(sd, hp, dtype=torch.float64):
    """The predictor's tensors of a state dict under their short keys, in ``dtype``."""
    return {k: sd[PREFIX + k].detach().to(dtype).clone() for k, _, _ in layout(hp)}


def flatten(P, hp, dtype=None):
    return torch.cat([P[k].reshape(-1) if dtype is None else P[k].reshape(-1).to(dtype) for k, _, _ in layout(hp)])


def unflatten(flat, hp):
    return {k: flat[off:off + math.prod(shape)].reshape(shape) for k, off, shape in layout(hp)}


def mask_of(lengths, T, dtype):
    return (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).to(dtype)[:, None, :]


def huber(d, delta):
    ad = d.abs()
    return torch.where(ad < delta, 0.5 * d * d, delta * (ad - 0.5 * delta))


# ------------------------------------------------------------------------------------------------ ordered sums
def ordered_row_sum(terms):
    """terms [M, C] (rows that take no part are zero) -> [C]: the chunk scheme of the module header, every addition in terms' dtype."""
    M, C = terms.shape
    ch, n = chunk_rows(M), chunks_of(M)
    t = torch.zeros(n * ch, C, dtype=terms.dtype)
    t[:M] = terms
    t = t.reshape(n, ch // 4, 4, C)
    acc = torch.zeros(n, 4, C, dtype=terms.dtype)
    for i in range(ch // 4):
        acc = acc + t[:, i]
    comb = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    s = comb[0]
    for c in range(1, n):
        s = s + comb[c]
    return s


def rows_cl(t):
    """[B, C, T] -> channels-last rows [B T, C]"""
    return t.permute(0, 2, 1).reshape(-1, t.shape[1])


def ln_film_wgrad(x, dy, film, lengths, eps=EPS, dtype=torch.float64):
    """mtts_ln_film_wgrad: x (pre-norm rows) and dy [B, T, C], film [B, 2C] -> (d gamma [C], d beta [C], sum|terms| of each in fp64)."""
    B, T, C = x.shape
    x, dy, film = x.to(dtype), dy.to(dtype), film.to(dtype)
    live = (torch.arange(T)[None, :] < torch.as_tensor(lengths).clamp(0, T)[:, None])[:, :, None]
    x, dy = torch.where(live, x, torch.zeros((), dtype=dtype)), torch.where(live, dy, torch.zeros((), dtype=dtype))
    mu = x.mean(2, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(2, keepdim=True) + eps)
    xh = (x - mu) * rs
    g = dy * film[:, None, :C]
    tg, tb = (g * xh).reshape(B * T, C), g.reshape(B * T, C)
    return ordered_row_sum(tg), ordered_row_sum(tb), tg.double().abs().sum(0), tb.double().abs().sum(0)


def rows_wgrad(seed, h, lengths, dtype=torch.float64):
    """mtts_rows_wgrad: seed [B, T], h [B, T, C] -> (dw [C], db [1], sum|terms| of each in fp64)."""
    B, T, C = h.shape
    seed, h = seed.to(dtype), h.to(dtype)
    live = torch.arange(T)[None, :] < torch.as_tensor(lengths).clamp(0, T)[:, None]
    seed = torch.where(live, seed, torch.zeros((), dtype=dtype))
    h = torch.where(live[:, :, None], h, torch.zeros((), dtype=dtype))
    tw, tb = (seed[:, :, None] * h).reshape(B * T, C), seed.reshape(B * T, 1)
    return ordered_row_sum(tw), ordered_row_sum(tb), tw.double().abs().sum(0), tb.double().abs().sum(0)


def outer_batch_sum(g, e, dtype=torch.float64):
    """mtts_outer_batch_sum: g [B, O], e [B, J] -> (dw [O, J], db [O]) in batch order from zero."""
    g, e = g.to(dtype), e.to(dtype)
    dw, db = torch.zeros(g.shape[1], e.shape[1], dtype=dtype), torch.zeros(g.shape[1], dtype=dtype)
    for b in range(g.shape[0]):
        dw = dw + g[b][:, None] * e[b][None, :]
        db = db + g[b]
    return dw, db


def fp32_is_exact_on(*abs_sums):
    """Small-integer operands: every sum of absolute terms stays below 2^24, so fp32 has nothing to round in any order."""
    return all(float(torch.as_tensor(a).max()) < 2.0 ** 24 for a in abs_sums)


# ------------------------------------------------------------------------------------------------ the restated loss and gradient
def forward(P, hp, h, lengths, e_dur, tape=None):
    """The predictor (reference text_encoder.py:101-112) on the encoder rows h [B, Hd, T] in P's dtype -> logw [B, 1, T].  ``tape``: a
    list that receives per layer (masked input, pre-ReLU z, xhat, rstd, the affine's output a) and last (film gamma, the last FiLM
    output)."""
    e = hp.encoder
    Fd, k = e.dp_filter_channels, e.dp_kernel_size
    dtype = P["proj.weight"].dtype
    B, _, T = h.shape
    mask = mask_of(lengths, T, dtype)
    film = F.linear(e_dur.to(dtype), P["spk_proj.weight"], P["spk_proj.bias"])
    gf, bf = film[:, :Fd, None], film[:, Fd:, None]
    x = h.to(dtype)
    for i in range(e.dp_n_layers):
        xin = x * mask
        z = F.conv1d(xin, P[f"conv_layers.{i}.weight"], P[f"conv_layers.{i}.bias"], padding=k // 2)
        r = torch.relu(z)
        mu = r.mean(1, keepdim=True)
        rs = torch.rsqrt(((r - mu) ** 2).mean(1, keepdim=True) + EPS)
        xh = (r - mu) * rs
        a = xh * P[f"norm_layers.{i}.gamma"].view(1, -1, 1) + P[f"norm_layers.{i}.beta"].view(1, -1, 1)
        x = a * gf + bf
        if tape is not None:
            tape.append((xin, z, xh, rs, a))
    if tape is not None:
        tape.append((gf, x))
    return F.conv1d(x * mask, P["proj.weight"], P["proj.bias"]) * mask


def dur_sums(logw, durations, lengths, delta):
    """Per-utterance Huber sums [B] of logw [B, 1, T] against log(2 + durations) on t < len_b (matcha_tts.py:117,128 before the division)."""
    dtype = logw.dtype
    m = mask_of(lengths, logw.shape[2], dtype)[:, 0]
    d = (logw[:, 0] - torch.log(2 + torch.as_tensor(durations).to(dtype))) * m
    return (huber(d, delta) * m).sum(1), d


def param_grads(P, hp, h, lengths, e_dur, durations, delta):
    """The gradient of sum_b dur_sum_b with respect to every parameter, from the formulas of include/mtts.h, in P's dtype.
    -> (grads dict, g_dur [B, Sd], dur_sum [B], logw)."""
    e = hp.encoder
    Fd, k, L = e.dp_filter_channels, e.dp_kernel_size, e.dp_n_layers
    dtype = P["proj.weight"].dtype
    B, _, T = h.shape
    tape = []
    logw = forward(P, hp, h, lengths, e_dur, tape)
    sums, d = dur_sums(logw, durations, lengths, delta)
    mask = mask_of(lengths, T, dtype)
    seed = d.clamp(-delta, delta) * mask[:, 0]                                   # [B, T]
    gf, y_last = tape[-1]
    G = {}
    G["proj.weight"] = ordered_row_sum(seed.reshape(-1, 1) * rows_cl(y_last * mask)).reshape(1, Fd, 1)
    G["proj.bias"] = ordered_row_sum(seed.reshape(-1, 1)).reshape(1)
    dy = seed[:, None, :] * P["proj.weight"].view(1, Fd, 1)                     # gradient at the last FiLM output
    dfilm = torch.zeros(B, 2 * Fd, dtype=dtype)
    for i in range(L - 1, -1, -1):
        xin, z, xh, rs, a = tape[i]
        dfilm[:, :Fd] = dfilm[:, :Fd] + (dy * a).sum(2)
        dfilm[:, Fd:] = dfilm[:, Fd:] + dy.sum(2)
        g = dy * gf
        G[f"norm_layers.{i}.gamma"] = ordered_row_sum(rows_cl(g * xh))
        G[f"norm_layers.{i}.beta"] = ordered_row_sum(rows_cl(g))
        gx = g * P[f"norm_layers.{i}.gamma"].view(1, -1, 1)
        dr = rs * ((gx - gx.mean(1, keepdim=True)) - xh * (gx * xh).mean(1, keepdim=True))
        dz = dr * (z > 0).to(dtype)
        # dW[co, ci, j] = sum over (b, t) of dz[b, co, t] xin[b, ci, t + j - k // 2], xin zero outside [0, len_b)
        xp = F.pad(xin, (k // 2, k // 2))
        G[f"conv_layers.{i}.weight"] = torch.stack([torch.einsum("bot,bit->oi", dz, xp[:, :, j:j + T]) for j in range(k)], 2)
        G[f"conv_layers.{i}.bias"] = dz.sum((0, 2))
        if i >= 1:
            dy = F.conv_transpose1d(dz, P[f"conv_layers.{i}.weight"], padding=k // 2) * mask
    G["spk_proj.weight"], G["spk_proj.bias"] = outer_batch_sum(dfilm, e_dur, dtype)
    g_dur = dfilm @ P["spk_proj.weight"]
    return G, g_dur, sums, logw


def autograd_grads(oracle, P, hp, h, lengths, e_dur, durations, delta):
    """The same gradient by torch.autograd through the oracle's predictor -> (grads dict, g_dur [B, Sd], dur_sum [B], logw)."""
    e = hp.encoder
    dtype = P["proj.weight"].dtype
    sd = {PREFIX + k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    rows = e_dur.detach().to(dtype).clone().requires_grad_(True)
    mask = mask_of(lengths, h.shape[2], dtype)
    logw = oracle.duration_predictor_forward(sd, PREFIX, h.to(dtype), mask, rows, e.dp_n_layers, e.dp_filter_channels, e.dp_kernel_size)
    sums, _ = dur_sums(logw, durations, lengths, delta)
    keys = list(P)
    grads = torch.autograd.grad(sums.sum(), [sd[PREFIX + k] for k in keys] + [rows])
    return dict(zip(keys, grads[:-1])), grads[-1], sums.detach(), logw.detach()


def encoder_rows(oracle, sd, hp, x, x_lengths, e_enc):
    """The frozen part: the rows the predictor reads, [B, Hd, Tx], in sd's dtype (oracle text_encoder_forward up to the encoder stack)."""
    e = hp.encoder
    p = "encoder."
    h = F.embedding(x, sd[p + "emb.weight"]) * math.sqrt(e.n_channels)
    h = h.transpose(1, -1)
    x_mask = oracle.sequence_mask(x_lengths, h.shape[2]).unsqueeze(1).to(h.dtype)
    h = oracle.prenet_forward(sd, p + "prenet.", h, x_mask, e.prenet_layers, e.prenet_kernel_size)
    h = torch.cat([h, e_enc.to(h.dtype).unsqueeze(-1).expand(-1, -1, h.shape[-1])], dim=1)
    return oracle.encoder_stack_forward(sd, p + "encoder.", h, x_mask, e.n_layers, e.n_heads, e.kernel_size, False)


# ------------------------------------------------------------------------------------------------ AdamW around the restatement
def is_decayed(key):
    return key.rsplit(".", 1)[-1] not in ("bias", "gamma", "beta")


def adamw_loop(P, hp, batches, steps, lr, weight_decay, betas, eps, delta, record=None):
    """torch.optim.AdamW's update in P's dtype, two groups (weights decay; bias, gamma, beta do not), gradients from ``param_grads``
    divided by the batch's token count.  ``batches``: list of (h, lengths, e_dur, durations), cycled.  ``record``: a list that receives
    per step {key: (g, u, s)} -- the gradient, Adam's normalised update u = m^ / s and its denominator s = sqrt(v^) + eps.
    -> (parameters per step incl. the start, dur_loss before each step)."""
    P = {k: v.clone() for k, v in P.items()}
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    v2 = {k: torch.zeros_like(v) for k, v in P.items()}
    b1, b2 = betas
    trail, hist = [{k: v.clone() for k, v in P.items()}], []
    for step in range(1, steps + 1):
        h, lengths, e_dur, dur = batches[(step - 1) % len(batches)]
        G, _, sums, _ = param_grads(P, hp, h, lengths, e_dur, dur, delta)
        tokens = float(torch.as_tensor(lengths).sum())
        hist.append(float(sums.sum()) / tokens)
        rec = {}
        for k in P:
            g = G[k] / tokens
            if is_decayed(k):
                P[k] = P[k] * (1 - lr * weight_decay)
            m[k] = b1 * m[k] + (1 - b1) * g
            v2[k] = b2 * v2[k] + (1 - b2) * g * g
            s = (v2[k] / (1 - b2 ** step)).sqrt() + eps
            u = (m[k] / (1 - b1 ** step)) / s
            P[k] = P[k] - lr * u
            rec[k] = (g.clone(), u.clone(), s.clone())
        if record is not None:
            record.append(rec)
        trail.append({k: v.clone() for k, v in P.items()})
    return trail, hist


def adam_update_cap(step, betas):
    """|m^ / sqrt(v^)| <= (1 - b1) / sqrt(1 - b2) sqrt(sum_{i < k} (b1^2 / b2)^i) sqrt(1 - b2^k) / (1 - b1^k) for ANY gradient history
    (Cauchy-Schwarz on the two moving averages): what one Adam step can move a coordinate by, in units of lr."""
    b1, b2 = betas
    r = b1 * b1 / b2
    return (1 - b1) / math.sqrt(1 - b2) * math.sqrt(sum(r ** i for i in range(step))) * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)


def adam_drift_allowance(record, rel, lr, betas, p_top):
    """How far AdamW parameters may drift from the loop that produced ``record`` when every gradient of tensor t carries an absolute
    error of at most A_t^j = rel[t] max|g_t^j| at step j (``rel``: the admitted relative gradient error per tensor, in the max norm the
    whole-gradient test uses).  Per coordinate i, with m^ and sqrt(v^) the bias-corrected moving averages and s = sqrt(v^) + eps:
      |d m^| <= Am = the same moving average of the A^j;      |d s| <= Av = the moving root-mean-square of the A^j
      (sqrt(v^) is a weighted 2-norm of the gradient history: the triangle inequality)
      u' - u = (dm s - m^ ds) / (s (s + ds))   =>   |u' - u| <= (Am + |u| Av) / (s - Av)     while s > Av,
    and never more than |u| + adam_update_cap: a coordinate whose gradient lies below the gradient's error may go either way.  Summed
    over the steps and times lr; plus one fp32 rounding of the parameter per step, 2^-24 p_top[t].  For a coordinate at the gradient's
    scale (s about max|g|, |u| about 1) a step's share is 2 lr rel[t]: the factor of the admitted gradient error, once for the
    numerator and once for the denominator.  -> per step (1-based index k - 1) {key: tensor of allowances}."""
    b1, b2 = betas
    am = {k: 0.0 for k in rel}
    av = {k: 0.0 for k in rel}
    total = {k: torch.zeros_like(record[0][k][0], dtype=torch.float64) for k in rel}
    out = []
    for j, rec in enumerate(record, start=1):
        cap = adam_update_cap(j, betas)
        for k in rel:
            g, u, s = (t.double() for t in rec[k])
            A = rel[k] * float(g.abs().max())
            am[k] = b1 * am[k] + (1 - b1) * A
            av[k] = b2 * av[k] + (1 - b2) * A * A
            Am, Av = am[k] / (1 - b1 ** j), math.sqrt(av[k] / (1 - b2 ** j))
            fine = (Am + u.abs() * Av) / (s - Av).clamp(min=1e-300)
            worst = u.abs() + cap
            total[k] = total[k] + lr * torch.where(s > Av, torch.minimum(fine, worst), worst)
        out.append({k: total[k] + j * U * p_top[k] for k in rel})
    return out

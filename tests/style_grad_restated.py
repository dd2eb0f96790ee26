"""Own-words fp64 restatements for the style encoder's parameter gradients (csrc/style_grad.hip): the encoder itself with autograd,
the plain definition of the Conv1d(k5, pad 2) weight gradient, and the backward pass GIVEN a tape of activations together with a
running bound on what fp32 arithmetic in the device's summation orders may lose against it.  Nothing here calls the library."""
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

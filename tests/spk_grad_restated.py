"""Yardstick of the speaker-row gradient (tests/test_spk_grad_abi.py against finite differences, tests/test_hip_spk_grad.py against the
device): torch autograd through ``oracle.matcha_oracle.text_encoder_forward`` and the two Huber sums of tests/score_restated.py, in
float64 (the reference) or float32 (what fp32 arithmetic itself costs: the unit of the device test's bound), and an fp64 Adam
fine-tune loop around it.

What is differentiated (reference matcha/models/matcha_tts.py:108-145 with the durations held constant, :187 no_grad):
  g_enc[b] = d prior_sum_b / d e_enc[b]     g_dur[b] = d dur_sum_b / d e_dur[b]
The oracle's encoder feeds the duration predictor the encoder output itself where the reference detaches it (text_encoder.py:404);
that path only carries d dur_sum / d e_enc, which is not taken here, so both gradients are the reference's.  The attention runs in
its plain-op form (``use_torch_sdpa=False``): a padded query has no allowed key, and autograd through the fused kernel's math path
would put NaN there."""
import contextlib

import numpy as np
import torch

import score_restated as S


def cast_state_dict(sd, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


def sums(oracle, sd, hp, x, x_lengths, e_enc, e_dur, y_fine, y_fine_lengths, durations, delta_prior, delta_dur):
    """-> (prior_sum [B], dur_sum [B], mu_x, logw) in the dtype of ``sd``; autograd flows to e_enc / e_dur."""
    mu_x, logw, _ = oracle.text_encoder_forward(sd, hp, x, x_lengths, e_enc, e_dur, use_torch_sdpa=False)
    _, dur_sums, _ = S.duration_loss(logw, durations, x_lengths, delta_dur)
    _, prior_sums, _, _ = S.prior_loss(mu_x, durations, y_fine.to(mu_x.dtype), y_fine_lengths, delta_prior)
    return prior_sums, dur_sums, mu_x, logw


@contextlib.contextmanager
def relu_calls(record=None, switched=()):
    """Inside the block every ``torch.relu`` call -- the oracle's FFN ReLUs, layer by layer, then the duration predictor's -- appends
    its input to ``record`` (float64 copies) and, for every (call, flat index) of ``switched``, keeps the VALUE of its output but
    switches the DERIVATIVE of that one element (on <-> off): the gate a forward pass takes when it computes that pre-activation on
    the other side of zero."""
    real, n = torch.relu, [0]

    def relu(y):
        k, out = n[0], real(y)
        n[0] += 1
        if record is not None:
            record.append(y.detach().double().clone())
        for call, flat in switched:
            if call == k:
                m = torch.zeros(y.numel(), dtype=y.dtype)
                m[flat] = 1.0 if float(y.detach().flatten()[flat]) <= 0 else -1.0
                out = out + (y - y.detach()) * m.view_as(y)
        return out

    torch.relu = relu
    try:
        yield
    finally:
        torch.relu = real


def relu_band(rec64, rec32, x_lengths, n_calls, factor=8.0):
    """Pre-ReLU activations of valid tokens that fp32 arithmetic cannot tell from zero: |h64| < factor * max|h32 - h64| of the same
    ReLU call (the project's factor on the fp32 CPU twin's own error), among the first ``n_calls`` calls.  -> per utterance the one
    nearest zero, as (call, flat index, value), for ``relu_calls(switched=...)``; and the count per utterance."""
    B = rec64[0].shape[0]
    valid = (torch.arange(rec64[0].shape[2])[None, :] < torch.as_tensor(x_lengths)[:, None])[:, None, :]
    best, count = {}, [0] * B
    for k in range(n_calls):
        h = rec64[k]
        width = factor * float(((h - rec32[k]).abs() * valid).max())
        band = (h.abs() < width) & valid
        for b, c, t in band.nonzero().tolist():
            count[b] += 1
            v = float(h[b, c, t])
            if b not in best or abs(v) < abs(best[b][2]):
                best[b] = (k, (b * h.shape[1] + c) * h.shape[2] + t, v)
    return [best[b] for b in sorted(best)], count


def speaker_grad(oracle, sd, hp, x, x_lengths, e_enc, e_dur, y_fine, y_fine_lengths, durations, delta_prior, delta_dur,
                 dtype=torch.float64, record=None, switched=()):
    """Gradients of the per-utterance sums with given durations -> dict of g_enc, g_dur [B, E], prior_sum, dur_sum [B], mu_x, logw
    (all in ``dtype``).  One row per utterance: utterance b's sums depend on row b alone, so the gradient of the batch total IS the
    per-utterance gradient, row by row.  ``record`` / ``switched``: ``relu_calls``."""
    if record is not None or switched:
        with relu_calls(record, switched):
            return speaker_grad(oracle, sd, hp, x, x_lengths, e_enc, e_dur, y_fine, y_fine_lengths, durations, delta_prior, delta_dur, dtype)
    B = x.shape[0]
    sdd = cast_state_dict(sd, dtype)
    e_enc = e_enc.detach().to(dtype).reshape(-1, hp.spk_emb_dim).expand(B, -1).clone().requires_grad_(True)
    e_dur = e_dur.detach().to(dtype).reshape(-1, hp.spk_emb_dim).expand(B, -1).clone().requires_grad_(True)
    prior, dur, mu_x, logw = sums(oracle, sdd, hp, x, x_lengths, e_enc, e_dur, y_fine, y_fine_lengths, durations, delta_prior, delta_dur)
    g_enc, = torch.autograd.grad(prior.sum(), e_enc, retain_graph=True)
    g_dur, = torch.autograd.grad(dur.sum(), e_dur)
    return {"g_enc": g_enc, "g_dur": g_dur, "prior_sum": prior.detach(), "dur_sum": dur.detach(), "mu_x": mu_x.detach(), "logw": logw.detach()}


def row_error(g, g64):
    """max|g - g64| / max|g64| per row -> [B] (float64)."""
    g, g64 = torch.as_tensor(g).double().cpu(), torch.as_tensor(g64).double().cpu()
    return (g - g64).abs().amax(1) / g64.abs().amax(1)


def adam_step(rows, grads, m, v, step, lr, betas, eps):
    """torch.optim.Adam without weight decay, in place on the lists (any dtype)."""
    b1, b2 = betas
    for k, g in enumerate(grads):
        m[k] = b1 * m[k] + (1 - b1) * g
        v[k] = b2 * v[k] + (1 - b2) * g * g
        denom = (v[k] / (1 - b2 ** step)).sqrt() + eps
        rows[k] = rows[k] - (lr / (1 - b1 ** step)) * m[k] / denom


def finetune(oracle, sd, hp, x, x_lengths, y_fine, y_fine_lengths, e_enc, e_dur, steps, lr, betas=(0.9, 0.999), eps=1e-8,
             delta_prior=None, delta_dur=None, durations=None, dtype=torch.float64):
    """The fine-tune loop on the CPU: per step the alignment search on the current mu_x (``durations`` None; else those), the batch
    normalisation g_enc.sum(0) / sum(Tm_b), g_dur.sum(0) / sum(Tx_b), one Adam step.  -> (rows per step incl. the start: list of
    (e_enc [1, E], e_dur [1, E]), history of (dur_loss, prior_loss) before each step)."""
    dp = hp.prior_loss_threshold if delta_prior is None else delta_prior
    dd = hp.duration_loss_threshold if delta_dur is None else delta_dur
    sdd = cast_state_dict(sd, dtype)
    B = x.shape[0]
    rows = [e_enc.detach().to(dtype).reshape(1, -1).clone(), e_dur.detach().to(dtype).reshape(1, -1).clone()]
    m, v = [torch.zeros_like(r) for r in rows], [torch.zeros_like(r) for r in rows]
    n_tok, n_fine = float(torch.as_tensor(x_lengths).sum()), float(torch.as_tensor(y_fine_lengths).sum())
    trail, history = [(rows[0].clone(), rows[1].clone())], []
    for step in range(1, steps + 1):
        dur = durations
        if dur is None:
            with torch.no_grad():
                mu_x, _, _ = oracle.text_encoder_forward(sdd, hp, x, x_lengths, rows[0].expand(B, -1), rows[1].expand(B, -1), use_torch_sdpa=False)
            dur, _ = S.mas_durations(mu_x, y_fine.to(dtype), x_lengths, y_fine_lengths)
        out = speaker_grad(oracle, sd, hp, x, x_lengths, rows[0], rows[1], y_fine, y_fine_lengths, dur, dp, dd, dtype=dtype)
        history.append((float(out["dur_sum"].sum()) / n_tok, float(out["prior_sum"].sum()) / n_fine))
        adam_step(rows, [out["g_enc"].sum(0, keepdim=True) / n_fine, out["g_dur"].sum(0, keepdim=True) / n_tok], m, v, step, lr, betas, eps)
        trail.append((rows[0].clone(), rows[1].clone()))
    return trail, history


# ------------------------------------------------------------------------------------------------ kernel-level restatements
# (tests/test_spk_grad_abi.py anchors them on the CPU, tests/test_hip_kernels_grad.py holds the device to them)
U = 2.0 ** -24


def seed_verdict(durations, x_lengths, y_fine_lengths, Tx, Tm):
    """The verdict of mtts_score_prior_dur per utterance: 1 lengths outside 1 <= x_len <= Tx, x_len <= y_len <= Tm; 2 a duration of a
    valid token outside [0, Tm] or durations that do not sum to y_len; else 0.  -> list of int."""
    out = []
    for b in range(len(x_lengths)):
        xl, yl = int(x_lengths[b]), int(y_fine_lengths[b])
        if xl < 1 or xl > Tx or yl > Tm or yl < xl:
            out.append(1)
            continue
        d = np.asarray(durations[b][:xl], dtype=np.int64)
        out.append(2 if ((d < 0) | (d > Tm)).any() or int(d.sum()) != yl else 0)
    return out


def seeds(mu_x, logw, durations, y_fine, x_lengths, y_fine_lengths, w_proj, delta_prior, delta_dur, dtype=np.float64):
    """The two seeds of mtts_spk_grad from the formulas, in ``dtype`` (float64: the reference; float32: the documented order -- per token
    a serial sum over its frames in frame order, every operation rounded to fp32 -- and the CPU twin of the logw seed).

      seed_mu[(b Tx + x), f]  = - sum over the frames t of token x, in frame order, of clamp(y[b, f, t] - mu_x[b, f, x], +-delta_prior)
      seed_logw[(b Tx + x), c] = clamp(logw[b, x] - log(2 + dur[b, x]), +-delta_dur) * w_proj[c]

    for x < x_len_b of an accepted utterance (seed_verdict), zero elsewhere; the frames of token x are [cum[x-1], cum[x]).  mu_x
    [B, F, Tx], logw [B, Tx], durations [B, Tx] integers, y_fine [B, F, Tm], w_proj [Fd].  -> dict: seed_mu [B Tx, round_up(F, 4)],
    seed_logw [B Tx, Fd], abs_mu (sum of |terms| per seed_mu element, float64), n (frames per token [B Tx]), verdict,
    clamped_mu / clamped_logw (share of the live terms whose difference is at or beyond delta), log_target / diff (of the logw seed)."""
    mu_x, logw, y_fine, w_proj = (np.asarray(t, dtype=dtype) for t in (mu_x, logw, y_fine, w_proj))
    dur = np.asarray(durations, dtype=np.int64)
    B, F, Tx = mu_x.shape
    Tm, Fd, ldm = y_fine.shape[2], w_proj.shape[0], (F + 3) // 4 * 4
    dp, dd = dtype(np.float32(delta_prior)), dtype(np.float32(delta_dur))
    verdict = seed_verdict(dur, x_lengths, y_fine_lengths, Tx, Tm)
    seed_mu = np.zeros((B, Tx, ldm), dtype=dtype)
    abs_mu = np.zeros((B, Tx, ldm), dtype=np.float64)
    seed_logw = np.zeros((B, Tx, Fd), dtype=dtype)
    n_frames = np.zeros((B, Tx), dtype=np.int64)
    log_target, diff = np.zeros((B, Tx), dtype=dtype), np.zeros((B, Tx), dtype=dtype)
    n_mu = c_mu = n_lw = c_lw = 0
    for b in range(B):
        if verdict[b] != 0:
            continue
        xl = int(x_lengths[b])
        d = dur[b, :xl]
        start = np.cumsum(d) - d
        n_frames[b, :xl] = d
        acc = np.zeros((F, xl), dtype=dtype)
        mag = np.zeros((F, xl), dtype=np.float64)
        for j in range(int(d.max())):                       # the j-th frame of every token that has one: frame order per token
            live = np.nonzero(d > j)[0]
            raw = y_fine[b][:, start[live] + j] - mu_x[b][:, live]
            term = np.minimum(np.maximum(raw, -dp), dp)
            acc[:, live] = acc[:, live] + term
            mag[:, live] += np.abs(term.astype(np.float64))
            n_mu += raw.size
            c_mu += int((np.abs(raw) >= dp).sum())
        seed_mu[b, :xl, :F] = -acc.T
        abs_mu[b, :xl, :F] = mag.T
        log_target[b, :xl] = np.log((dtype(2) + d.astype(dtype)))
        diff[b, :xl] = logw[b, :xl] - log_target[b, :xl]
        s = np.minimum(np.maximum(diff[b, :xl], -dd), dd)
        seed_logw[b, :xl] = s[:, None] * w_proj[None, :]
        n_lw += xl
        c_lw += int((np.abs(diff[b, :xl]) >= dd).sum())
    return {"seed_mu": seed_mu.reshape(B * Tx, ldm), "seed_logw": seed_logw.reshape(B * Tx, Fd), "abs_mu": abs_mu.reshape(B * Tx, ldm),
            "n": n_frames.reshape(B * Tx), "verdict": verdict, "clamped_mu": c_mu / max(n_mu, 1), "clamped_logw": c_lw / max(n_lw, 1),
            "log_target": log_target.reshape(B * Tx), "diff": diff.reshape(B * Tx)}


def seed_logw_floor(ref, w_proj):
    """What fp32 may cost a seed_logw element beside the CPU twin's own error, from the roundings of clamp(logw - logf(2 + d)) * w:
    2 + d is exact (d < 2^23); logf within 1 ulp <= 2 U |L| (the documented bound of the device's logf; glibc's is tighter); the
    subtraction U |diff|; the clamp exact; the product U |seed w|.  ``ref``: the float64 result of ``seeds``.  -> [B Tx, Fd]"""
    w = np.abs(np.asarray(w_proj, dtype=np.float64))[None, :]
    return U * ((2 * np.abs(ref["log_target"]) + np.abs(ref["diff"]))[:, None] * w + np.abs(ref["seed_logw"]))


def token_sums(src, col0, C, B, T, lengths=None, verdict=None, dtype=np.float32):
    """colsum_kernel: src [B T, ld] -> [B, C] sums over t < len_b (None: T; clamped to [0, T]; a non-zero verdict: 0) of columns
    [col0, col0 + C).  float32: four phases t = p, p + 4, ... in token order, combined as ((p0 + p1) + p2) + p3, every addition rounded
    to fp32 (expected bit for bit).  float64: the plain sum.  Also -> the sum of |terms| in float64."""
    rows = np.asarray(src)[:, col0:col0 + C].reshape(B, T, C)
    out = np.zeros((B, C), dtype=dtype)
    mag = np.zeros((B, C), dtype=np.float64)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        if verdict is not None and int(verdict[b]) != 0:
            n = 0
        mag[b] = np.abs(rows[b, :n].astype(np.float64)).sum(0)
        if dtype == np.float64:
            out[b] = rows[b, :n].astype(np.float64).sum(0)
            continue
        part = np.zeros((4, C), dtype=np.float32)
        for t in range(n):
            part[t & 3] = part[t & 3] + rows[b, t].astype(np.float32)
        out[b] = ((part[0] + part[1]) + part[2]) + part[3]
    return out, mag


def relu_gate(ref, mode, mask=None):
    """The decision of gate_kernel modes 1 and 2 per element of ref [M, C] (fp32 torch tensor) -> (on, flushed), both bool [M, C].
    Mode 1: ref > 0.  Mode 2: the rule documented for the P16 image of ref times mask[row] -- head > 0, or head == 0 and residual
    > 0 -- on the restated split of tests/p16_restated.py (residual scale 2^11).  ``flushed``: positive inputs (of unmasked rows) whose
    head AND residual are zero, i.e. below what the two fp16 planes can hold (x <= 2^-36): the one place where mode 2 may differ from
    x > 0.  A row with mask 0 is off in either mode."""
    import p16_restated as P
    x = ref.float()
    live = torch.ones(x.shape[0], dtype=torch.bool) if mask is None else (mask != 0)
    if mode == 1:
        return (x > 0) & live[:, None], torch.zeros_like(x, dtype=torch.bool)
    xm = x if mask is None else x * mask.float()[:, None]
    h, l = P.split(xm, 2048.0)
    h, l = h.float(), l.float()
    on = ((h > 0) | ((h == 0) & (l > 0))) & live[:, None]
    return on, (x > 0) & live[:, None] & (h == 0) & (l == 0)


def silu_gate(g, ref, dtype=torch.float64):
    """gate_kernel mode 0: g * silu'(ref), silu'(z) = s (1 + z (1 - s)), s = 1 / (1 + exp(-z)), in ``dtype`` (float32: the CPU twin, the
    kernel's expression operation by operation)."""
    g, z = g.to(dtype), ref.to(dtype)
    s = 1 / (1 + torch.exp(-z))
    return g * (s * (1 + z * (1 - s)))


def silu_gate_floor(g, ref):
    """Roundings of the fp32 expression of mode 0, first order in U: exp within 2 ulp (4 U), 1 + e and the division U each -> s to
    6 U; t = 1 - s to 6 U s + U t; z t one more U; q = 1 + z t one more; s q carries s's 6 U and its own, g (s q) its own.  With
    |q| <= 1 + |z| t and s + t = 1 that is |err| <= U |g| s (9 + 11 |z|).  -> float64 tensor"""
    g, z = g.double().abs(), ref.double()
    s = 1 / (1 + torch.exp(-z))
    return U * g * s * (9 + 11 * z.abs())

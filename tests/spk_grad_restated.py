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


def speaker_grad(oracle, sd, hp, x, x_lengths, e_enc, e_dur, y_fine, y_fine_lengths, durations, delta_prior, delta_dur,
                 dtype=torch.float64):
    """Gradients of the per-utterance sums with given durations -> dict of g_enc, g_dur [B, E], prior_sum, dur_sum [B], mu_x, logw
    (all in ``dtype``).  One row per utterance: utterance b's sums depend on row b alone, so the gradient of the batch total IS the
    per-utterance gradient, row by row."""
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

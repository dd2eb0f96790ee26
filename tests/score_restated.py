"""Restatement of the three losses of the reference's training forward, the yardstick of tests/test_score_abi.py (against closed
forms) and tests/test_hip_score.py (against the device).  Written from the formulas, on CPU tensors, in the dtype of its inputs:

  matcha/models/matcha_tts.py:108-128   mas_durations = path.sum(-1); logw_ = log(2 + mas_durations) * x_mask;
                                         dur_loss = huber(logw, logw_, delta_dur, sum) / sum(x_lengths)
  matcha/models/matcha_tts.py:124,143-145  mu_y_fine = mu_x @ path; prior_loss = huber(y_fine * m, mu_y_fine * m, delta_prior, sum) / sum(m)
  matcha/models/matcha_tts.py:154-162   mu_y = downsample(mu_y_fine); diff_loss = compute_loss(y, y_mask, mu_y)
  matcha/models/components/flow_matching.py:84-105   x0 = noise (+ mu); y_t = (1 - (1 - sigma_min) t) x0 + t x1;
                                         u = x1 - (1 - sigma_min) x0; loss = mse(pred * mask, u * mask, sum) / (sum(mask) * n_feats)

The network comes from oracle/matcha_oracle.py, the path from tests/mas_restated.py."""
import numpy as np
import torch
import torch.nn.functional as F

import mas_restated as R


def sequence_mask(lengths, n):
    return (torch.arange(n)[None, :] < torch.as_tensor(lengths)[:, None])


def path_from_durations(durations, Tm):
    """durations [B, Tx] (integers) -> 0/1 path [B, Tx, Tm]: token x owns frames [cum[x] - d[x], cum[x])."""
    d = torch.as_tensor(durations).long()
    cum = torch.cumsum(d, 1)
    frames = torch.arange(Tm)[None, None, :]
    return ((frames < cum[:, :, None]) & (frames >= (cum - d)[:, :, None]))


def mas_durations(mu_x, y_fine, x_lengths, y_fine_lengths):
    """The search of tests/mas_restated.py on the fp64 log-prior of every utterance -> (durations int64 [B, Tx], score [B])."""
    B, _, Tx = mu_x.shape
    dur = torch.zeros(B, Tx, dtype=torch.long)
    score = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        xl, yl = int(x_lengths[b]), int(y_fine_lengths[b])
        lp = R.log_prior(mu_x[b, :, :xl].numpy(), y_fine[b, :, :yl].numpy())
        d, _, s = R.maximum_path(lp)
        dur[b, :xl] = torch.from_numpy(d.astype(np.int64))
        score[b] = float(s)
    return dur, score


def duration_loss(logw, durations, x_lengths, delta):
    """-> (batch loss, per-utterance sums [B], signed error [B, Tx]).  logw [B, 1, Tx] as the encoder returns it (masked)."""
    B, _, Tx = logw.shape
    x_mask = sequence_mask(x_lengths, Tx)[:, None, :].to(logw.dtype)
    logw_ = torch.log(2 + torch.as_tensor(durations).to(logw.dtype)[:, None, :]) * x_mask
    sums = F.huber_loss(logw, logw_, delta=delta, reduction="none").sum((1, 2))
    loss = F.huber_loss(logw, logw_, delta=delta, reduction="sum") / torch.as_tensor(x_lengths).sum()
    return loss, sums, (logw - logw_)[:, 0, :]


def prior_loss(mu_x, durations, y_fine, y_fine_lengths, delta):
    """-> (batch loss, per-utterance sums [B], per-frame sums [B, Tm], mu_y_fine [B, F, Tm])."""
    Tm = y_fine.shape[2]
    path = path_from_durations(durations, Tm).to(mu_x.dtype)
    mu_y_fine = torch.matmul(mu_x, path)
    m = sequence_mask(y_fine_lengths, Tm)[:, None, :].to(mu_x.dtype)
    per = F.huber_loss(y_fine * m, mu_y_fine * m, delta=delta, reduction="none")
    loss = F.huber_loss(y_fine * m, mu_y_fine * m, delta=delta, reduction="sum") / m.sum()
    return loss, per.sum((1, 2)), per.sum(1), mu_y_fine


def flow_target(x1, mu, t, noise, use_mu_prior, sigma_min):
    """-> (y_t, u) in the reference's operation order; t [B]."""
    t3 = torch.as_tensor(t).to(x1.dtype).reshape(-1, 1, 1)
    x0 = mu + noise if use_mu_prior else noise
    y = (1 - (1 - sigma_min) * t3) * x0 + t3 * x1
    u = x1 - (1 - sigma_min) * x0
    return y, u


def cfm_loss(estimator, x1, mask, mu, t, noise, use_mu_prior, sigma_min):
    """estimator(y, mask, mu, t[B]) -> pred.  -> (batch loss, per-utterance sums [B], pred)."""
    y, u = flow_target(x1, mu, t, noise, use_mu_prior, sigma_min)
    pred = estimator(y, mask, mu, torch.as_tensor(t).to(x1.dtype).reshape(-1))
    sums = ((pred * mask - u * mask) ** 2).sum((1, 2))
    loss = F.mse_loss(pred * mask, u * mask, reduction="sum") / (torch.sum(mask) * u.shape[1])
    return loss, sums, pred


def training_forward(oracle, sd, hp, x, x_lengths, y, y_lengths, y_fine, y_fine_lengths, e_enc, e_dur, t, noise, delta_prior, delta_dur):
    """MatchaTTS.forward restated: every figure of ``MatchaTTSInfer.score`` from the oracle's network on CPU."""
    with torch.inference_mode():
        mu_x, logw, x_mask = oracle.text_encoder_forward(sd, hp, x, x_lengths, e_enc, e_dur)
        durations, mas_score = mas_durations(mu_x, y_fine, x_lengths, y_fine_lengths)
        dur_loss, dur_sums, dur_err = duration_loss(logw, durations, x_lengths, delta_dur)
        pr_loss, pr_sums, pr_frame, mu_y_fine = prior_loss(mu_x, durations, y_fine, y_fine_lengths, delta_prior)
        mu_y = oracle.downsample(mu_y_fine)
        y_mask = sequence_mask(y_lengths, y.shape[2])[:, None, :].to(y.dtype)

        def estimator(yt, mask, mu, tt):
            return oracle.decoder_forward(sd, hp, yt, mask, mu, tt)
        t = torch.as_tensor(t, dtype=y.dtype)
        grid = t if t.dim() == 2 else t[None]
        diff = [cfm_loss(estimator, y, y_mask, mu_y, tk, noise, hp.use_mu_prior, hp.sigma_min) for tk in grid]
    n_tok, n_fine = torch.as_tensor(x_lengths).to(y.dtype), torch.as_tensor(y_fine_lengths).to(y.dtype)
    n_coarse = y_mask.sum((1, 2)) * hp.n_feats
    diff_loss = torch.stack([d[0] for d in diff])
    diff_sums = torch.stack([d[1] for d in diff])
    if t.dim() == 1:
        diff_loss, diff_sums = diff_loss[0], diff_sums[0]
    return {"dur_loss": dur_loss, "prior_loss": pr_loss, "diff_loss": diff_loss,
            "dur_loss_per_utterance": dur_sums / n_tok, "prior_loss_per_utterance": pr_sums / n_fine,
            "diff_loss_per_utterance": diff_sums / n_coarse, "durations": durations, "mas_score": mas_score,
            "prior_frame": pr_frame, "dur_err": dur_err, "mu_x": mu_x, "logw": logw, "mu_y": mu_y}

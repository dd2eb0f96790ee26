"""Plain torch restatements of the kernels that are not GEMMs (csrc/vocos.hip: depthwise k7 conv + LayerNorm, polar spectrum, iSTFT
overlap-add; csrc/norm_glue.hip: rk4 stage combinations, step tables, time sinusoid, RoPE, the four layout moves, alignment + pool).
Every function computes in the dtype of its inputs: float64 inputs give the arbiter of tests/test_hip_kernels_glue.py, float32
inputs the CPU's own fp32 result.  tests/test_glue_abi.py checks them against independent torch code (torch.istft, F.conv1d +
F.layer_norm, the oracle's rotary function, a textbook 3/8-rule step, the oracle's alignment)."""
import torch


def clamp_len(n, T):
    return max(0, min(int(n), T))


def dwconv7_ln(x, w7, bias, gamma, beta, eps=1e-6, lengths=None):
    """x [B, T, C], w7 [7, C] tap-major: out[b, t] = LayerNorm_C(bias + sum_j w7[j] * x[b, t + j - 3]) * gamma + beta, taps outside
    [0, len_b) are zero.  Applied per utterance on x[b, :len_b] alone; rows at t >= len_b are NaN (not defined)."""
    B, T, C = x.shape
    out = torch.full_like(x, float("nan"))
    for b in range(B):
        n = T if lengths is None else clamp_len(lengths[b], T)
        if n == 0:
            continue
        pad = torch.zeros(n + 6, C, dtype=x.dtype)
        pad[3:3 + n] = x[b, :n]
        acc = bias.expand(n, C).clone()
        for j in range(7):
            acc = acc + pad[j:j + n] * w7[j]
        mu = acc.mean(dim=1, keepdim=True)
        var = ((acc - mu) ** 2).mean(dim=1, keepdim=True)
        out[b, :n] = ((acc - mu) * (1.0 / torch.sqrt(var + eps))) * gamma + beta
    return out


def spec_polar(x, nbins, off, clip=1e2):
    """x [M, ld]: columns (k, off + k), k < nbins, = (log-magnitude, phase) -> min(exp(m), clip) * (cos p, sin p); the rest is kept."""
    out = x.clone()
    mag = torch.clamp(torch.exp(x[:, :nbins]), max=clip)
    p = x[:, off:off + nbins]
    out[:, :nbins] = mag * torch.cos(p)
    out[:, off:off + nbins] = mag * torch.sin(p)
    return out


def istft_ola(frames, window, hop, lengths=None):
    """frames [B, T, n_fft] (already windowed once) -> audio [B, hop * (T - 1)].  With pos = s + n_fft / 2:
    acc[s] = sum_f frames[f, pos - f * hop], env[s] = sum_f window[pos - f * hop]^2 over the frames f <= T_b - 1 with
    0 <= pos - f * hop < n_fft; audio = acc / env where env > 1e-11, else acc; zeros from hop * (T_b - 1) on.
    Returns (audio, env)."""
    B, T, n_fft = frames.shape
    L = hop * (T - 1)
    audio = torch.zeros(B, L, dtype=frames.dtype)
    envs = torch.zeros(B, L, dtype=frames.dtype)
    w2 = window * window
    j = torch.arange(n_fft)
    for b in range(B):
        Tb = T if lengths is None else clamp_len(lengths[b], T)
        Lb = hop * (Tb - 1)
        if Lb <= 0:
            continue
        acc = torch.zeros(Lb, dtype=frames.dtype)
        env = torch.zeros(Lb, dtype=frames.dtype)
        for f in range(Tb):
            s = f * hop + j - n_fft // 2
            ok = (s >= 0) & (s < Lb)
            acc.index_add_(0, s[ok], frames[b, f][ok])
            env.index_add_(0, s[ok], w2[ok])
        audio[b, :Lb] = torch.where(env > 1e-11, acc / env, acc)
        envs[b, :Lb] = env
    return audio, envs


def ode_combine(stage, dt, y, k1, k2=None, k3=None, k4=None):
    """torchdiffeq's fixed-grid rk4 (3/8 rule) in its operation order; stage 0 is the plain axpy.  dt: a 0-dim tensor or a column
    [M, 1] of the dtype of y."""
    third = torch.tensor(1.0 / 3.0, dtype=y.dtype)
    if stage == 0:
        return y + dt * k1
    if stage == 1:
        return y + (dt * k1) * third
    if stage == 2:
        return y + dt * (k2 - k1 * third)
    if stage == 3:
        return y + dt * ((k1 - k2) + k3)
    if stage == 4:
        return y + (((k1 + 3.0 * (k2 + k3)) + k4) * dt) * 0.125
    raise ValueError(stage)


def step_tables(t0, t1, mask, stages):
    """t0, t1 [B], mask [B, T] -> tv [stages * B] (stage-major), dt [B], rs_full, rs_half [B * T]."""
    dt = t1 - t0
    third = torch.tensor(1.0 / 3.0, dtype=t0.dtype)
    two_thirds = torch.tensor(2.0 / 3.0, dtype=t0.dtype)
    tv = [t0]
    if stages == 2:
        tv.append(t0 + 0.5 * dt)
    if stages == 4:
        tv += [t0 + dt * third, t0 + dt * two_thirds, t1]
    return torch.cat(tv), dt, (mask * dt[:, None]).reshape(-1), (mask * (0.5 * dt)[:, None]).reshape(-1)


def sinusoid_arg(freqs, t, scale):
    """The argument (scale * t_i) * f_j, formed in the dtype of the inputs."""
    return (scale * t)[:, None] * freqs[None, :]


def sinusoid(arg):
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)


def rope(qkv, B, T, H, D, d_rope, cos, sin):
    """qkv [B*T, 3*H*D] (q | k | v): on q and k, the first d_rope dims of each head, pairs (i, i + d_rope/2), position = row % T;
    cos / sin [>= T, d_rope]."""
    half = d_rope // 2
    x = qkv.clone().view(B, T, 3, H, D)
    c = cos[:T, None, None, :].to(qkv.dtype)
    s = sin[:T, None, None, :].to(qkv.dtype)
    a, b2 = x[:, :, :2, :, :half].clone(), x[:, :, :2, :, half:d_rope].clone()
    x[:, :, :2, :, :half] = a * c[..., :half] + (-b2) * s[..., :half]
    x[:, :, :2, :, half:d_rope] = b2 * c[..., half:] + a * s[..., half:]
    return x.view(B * T, 3 * H * D)


def cf_to_cl(src, dst, T, col_off=0, add=None, lengths=None):
    """src [B, C, T_src] -> a copy of dst [B*T, ld] with dst[b*T + t, col_off + c] = src[b, c, t] (+ add), zero rows at t >= len_b."""
    B, C, _ = src.shape
    out = dst.clone().view(B, T, -1)
    for b in range(B):
        n = T if lengths is None else clamp_len(lengths[b], T)
        out[b, :, col_off:col_off + C] = 0
        v = src[b, :, :n] if add is None else src[b, :, :n] + add[b, :, :n]
        out[b, :n, col_off:col_off + C] = v.transpose(0, 1)
    return out.view(B * T, -1)


def cl_to_cf(src, B, C, T, T_out, scale=1.0, shift=0.0):
    """src [B*T, ld] -> [B, C, T_out] = src * scale + shift."""
    return src.view(B, T, -1)[:, :T_out, :C].transpose(1, 2) * scale + shift


def slots_to_cl(pool, slots, dst, T, col_off=0):
    S, C, _ = pool.shape
    B = len(slots)
    out = dst.clone().view(B, T, -1)
    for b, sl in enumerate(slots):
        out[b, :, col_off:col_off + C] = pool[sl, :, :T].transpose(0, 1) if 0 <= sl < S else 0
    return out.view(B * T, -1)


def cl_to_slots(src, pool, slots, T):
    S, C, _ = pool.shape
    B = len(slots)
    out = pool.clone()
    for b, sl in enumerate(slots):
        if 0 <= sl < S:
            out[sl, :, :T] = src.view(B, T, -1)[b, :, :C].transpose(0, 1)
    return out


def align_pool(mu_x, durations, t_pad):
    """The one-hot alignment, zero durations allowed: fine frame f belongs to the first token whose cumulative duration exceeds f
    (frames at or beyond the total are zero), then avg_pool1d(k3, s2, p1) with the padding counted in the divisor.  mu_x [B, nf, Tx],
    durations [B, Tx] -> (mu_y [B, nf, t_pad], y_mask [B, 1, t_pad], y_lengths [B])."""
    B, nf, Tx = mu_x.shape
    cum = torch.cumsum(durations.long(), 1)
    t_fine = 2 * t_pad
    f = torch.arange(t_fine)
    start = cum - durations.long()
    path = ((f[None, None, :] >= start[:, :, None]) & (f[None, None, :] < cum[:, :, None])).to(mu_x.dtype)        # [B, Tx, t_fine]
    fine = torch.matmul(mu_x, path)
    padded = torch.cat([torch.zeros(B, nf, 1, dtype=mu_x.dtype), fine], dim=2)                                    # fine[-1] = 0
    mu_y = torch.zeros(B, nf, t_pad, dtype=mu_x.dtype)
    for k in range(3):                                              # fine[2t - 1], fine[2t], fine[2t + 1]; fine[2 t_pad] does not exist
        idx = 2 * torch.arange(t_pad) + k                           # index into `padded`
        ok = idx < t_fine + 1
        mu_y[:, :, ok] = mu_y[:, :, ok] + padded[:, :, idx[ok]]
    mu_y = mu_y / 3.0
    y_fine_len = torch.clamp_min(cum[:, -1], 1)
    y_len = torch.clamp_min((y_fine_len + 1) // 2, 1)
    y_mask = (torch.arange(t_pad)[None, :] < y_len[:, None]).to(mu_x.dtype).unsqueeze(1)
    return mu_y, y_mask, y_len

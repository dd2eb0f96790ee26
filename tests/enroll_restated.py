"""CPU restatements (fp64, plain torch / numpy) of what voice enrolment computes, from the published definitions:
torchaudio's MelSpectrogram(center=True, power=1, mel_scale="htk", norm=None) + log(clamp) and the reference's StyleEncoder.
Shared by the enrolment tests; not a test module."""
import numpy as np
import torch
import torch.nn.functional as F


def htk_fbanks(n_freqs: int, sample_rate: int, n_mels: int) -> np.ndarray:
    """[n_freqs, n_mels] triangular filters, mel(f) = 2595 log10(1 + f / 700), f in [0, sample_rate // 2], no area norm."""
    f_max = float(sample_rate // 2)
    freqs = np.linspace(0.0, f_max, n_freqs)
    m_pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + f_max / 700.0), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up))


def dft_basis(n_fft: int) -> np.ndarray:
    """[n_fft, 2 * bins]: periodic-Hann-windowed cos columns, then -sin columns."""
    n = np.arange(n_fft, dtype=np.float64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.float64)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    ang = 2.0 * np.pi * ((n * k) % n_fft) / n_fft
    return np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1)


def mel_linear(y: torch.Tensor, hop: int, n_fft: int = 1024, n_mels: int = 100, sample_rate: int = 24000) -> torch.Tensor:
    """1-D clip -> [n_mels, len // hop + 1] magnitude mel in fp64 (before log), the clip trimmed to a multiple of hop."""
    y = y.double()[: (y.numel() // hop) * hop]
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, dtype=torch.float64), center=True,
                      pad_mode="reflect", return_complex=True).abs()
    fb = torch.from_numpy(htk_fbanks(n_fft // 2 + 1, sample_rate, n_mels))
    return fb.T @ spec


def log_mel(y, hop, mean=0.0, std=1.0, **kw) -> torch.Tensor:
    return (torch.log(torch.clamp(mel_linear(y, hop, **kw), min=1e-7)) - mean) / std


def stft_frames(y: torch.Tensor, hop: int, n_fft: int, dtype=torch.float64) -> torch.Tensor:
    """1-D clip -> [len // hop + 1, n_fft]: the clip trimmed to a multiple of hop, reflect-padded by n_fft / 2 at both ends
    (center=True), one row per frame."""
    y = y.to(dtype)[: (y.numel() // hop) * hop]
    padded = F.pad(y[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    return padded.unfold(0, n_fft, hop)


def stft_mag(y: torch.Tensor, hop: int, n_fft: int, basis=None) -> torch.Tensor:
    """[len // hop + 1, bins] STFT magnitudes as a matrix product: frames times the windowed cos | -sin basis, sqrt(re^2 + im^2).
    `basis` None: fp64 throughout with dft_basis.  A given table (the library's fp32 one): everything in that table's dtype -- the
    same operation in the same form in fp32, whose error against the fp64 form is the unit of the device's error."""
    b = torch.from_numpy(dft_basis(n_fft)) if basis is None else torch.as_tensor(basis)
    z = stft_frames(y, hop, n_fft, b.dtype) @ b
    nb = n_fft // 2 + 1
    return torch.sqrt(z[:, :nb] ** 2 + z[:, nb:] ** 2)


def mel_from_mag(mag: torch.Tensor, fb, mean: float = 0.0, std: float = 1.0) -> torch.Tensor:
    """Magnitudes [T, bins] -> normalised log-mel [T, n_mels] = (log(clamp(mag @ fb, 1e-7)) - mean) / std, in fb's dtype
    (fb [bins, n_mels]: htk_fbanks for fp64, the library's fp32 table for the fp32 form)."""
    fb = torch.as_tensor(fb)
    lin = mag.to(fb.dtype) @ fb
    return (torch.log(torch.clamp(lin, min=1e-7)) - mean) / std


def style_rows(sd, mel: torch.Tensor, length: int, dtype=torch.float64):
    """StyleEncoder.forward on one clip [n_feats, T] with `length` valid frames -> (e_enc [E], e_dur [E]); fp64, or the same
    operations in another dtype (fp32: the unit of the device's error)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    T = mel.shape[-1]
    mask = (torch.arange(T) < length).to(dtype)[None, None, :]
    x = mel.to(dtype)[None]
    i = 0
    while f"convs.{i}.weight" in sd:
        x = torch.relu(F.conv1d(x * mask, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], padding=2))
        i += 1
    pooled = (x * mask).sum(2) / mask.sum(2).clamp(min=1)
    return (F.linear(pooled, sd["proj_enc.weight"], sd["proj_enc.bias"])[0], F.linear(pooled, sd["proj_dur.weight"], sd["proj_dur.bias"])[0])


def synthetic_clip(n: int, seed: int, kind: str = "voiced") -> torch.Tensor:
    """A deterministic clip in [-1, 1]: "noise" = white noise, "sweep" = a sine sweep over a low noise floor, "voiced" = a few
    harmonics with vibrato plus noise (a stand-in for speech)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 24000.0
    if kind == "noise":
        return ((torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * 0.8).float()
    if kind == "sweep":
        ph = 2 * np.pi * (100.0 * t + (9000.0 - 100.0) / (2 * max(float(t[-1]), 1e-9)) * t * t)
        return (0.5 * torch.sin(ph) + 0.01 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-1, 1).float()
    f0 = 110.0 + 15.0 * seed % 90
    y = sum((0.3 / h) * torch.sin(2 * np.pi * h * f0 * t + 0.3 * h * torch.sin(2 * np.pi * 5.0 * t)) for h in range(1, 9))
    return (y + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-1, 1).float()

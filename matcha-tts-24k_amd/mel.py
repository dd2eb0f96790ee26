"""Log-mel front end on MI355X: drop-in for the reference's ``matcha.vocos24k.mel_extractor.get_mel_extractor``
(reference matcha/vocos24k/mel_extractor.py:6-41) plus the normalised, ragged-batch form voice enrolment needs
(reference matcha/utils/precompute_mels.py:100-113: ``(log_mel - mel_mean) / mel_std`` at hop 128, the "fine" mel).

Arithmetic runs in libmtts_hip.so (``mtts_melfe_forward``: the STFT as a GEMM on the matrix pipe with the magnitude in its
epilogue, then the HTK filterbank, log and normalisation); there is no CPU path and no torchaudio dependency.
"""
from __future__ import annotations

from typing import Callable, Dict, Sequence, Tuple

import numpy as np
import torch

from . import _hip

LOG_EPS = 1e-7          # reference mel_extractor.py: log(clamp(mel, 1e-7)); fixed in the library


def n_frames(length: int, hop: int) -> int:
    """Frames of a clip of ``length`` samples: it is trimmed to a multiple of ``hop``, then ``center=True`` gives len // hop + 1."""
    return int(length) // int(hop) + 1


class MelFrontEnd:
    """One ``mtts_melfe``: the Hann-windowed DFT basis and the HTK filterbank for (sample_rate, n_fft, n_mels)."""

    def __init__(self, sample_rate: int = 24000, n_fft: int = 1024, n_mels: int = 100):
        self.lib = _hip.load()
        self.sample_rate, self.n_fft, self.n_mels = int(sample_rate), int(n_fft), int(n_mels)
        self.ctx = self.lib.mtts_melfe_create(self.sample_rate, self.n_fft, self.n_mels)
        if not self.ctx:
            raise RuntimeError("mtts_melfe_create: " + self.lib.mtts_last_error().decode())
        self.n_bins = self.lib.mtts_melfe_n_bins(self.ctx)
        self._ws = _hip.Workspaces()
        self._last: Dict[int, Tuple[int, int]] = {}      # stream -> (B, T_max) of its latest extract

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.mtts_melfe_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    def basis(self) -> np.ndarray:
        """The host table [n_fft, 2 * bins]: window[n] * cos(2 pi k n / n_fft) columns, then -window[n] * sin columns."""
        out = np.empty((self.n_fft, 2 * self.n_bins), dtype=np.float32)
        _hip.check(self.lib.mtts_melfe_basis(self.ctx, out.ctypes.data, out.size))
        return out

    def filterbank(self) -> np.ndarray:
        """The host table [bins, n_mels] (torchaudio.functional.melscale_fbanks, mel_scale="htk", norm=None)."""
        out = np.empty((self.n_bins, self.n_mels), dtype=np.float32)
        _hip.check(self.lib.mtts_melfe_filterbank(self.ctx, out.ctypes.data, out.size))
        return out

    def magnitudes(self, padded: bool = False) -> torch.Tensor:
        """|STFT| of this stream's latest ``extract`` as it lies at the start of the workspace (csrc/mel_frontend.hip: ``mag
        [B * T_max][bins padded to 32]``): a view [B, T_max, n_bins], or [B, T_max, padded bins] with ``padded``.  Rows beyond a
        clip's frames are zero.  Read-only, for the tests: the next ``extract`` on the stream overwrites it."""
        ws, shape = self._ws.latest("melfe"), self._last.get(_hip.stream_ptr())
        if ws is None or shape is None:
            raise RuntimeError("matcha-tts-24k_amd: no extract has run on this stream")
        B, t_max = shape
        nbp = (self.n_bins + 31) // 32 * 32
        mag = ws[:B * t_max * nbp * 4].view(torch.float32).view(B, t_max, nbp)
        return mag if padded else mag[:, :, :self.n_bins]

    def workspace_bytes(self, B: int, ld: int, hop: int) -> int:
        return _hip.size(self.lib.mtts_melfe_workspace_bytes(self.ctx, int(B), int(ld), int(hop)))

    @torch.inference_mode()
    def extract(self, audio: torch.Tensor, lengths, hop: int = 256, mel_mean: float = 0.0, mel_std: float = 1.0
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """audio [B, ld] (device, fp32, 24 kHz mono in [-1, 1]) + lengths [B] (samples; sequence or tensor) ->
        (mel [B, n_mels, T_max], mel_lengths [B]): row b holds ``(log_mel(audio[b, :len_b]) - mel_mean) / mel_std`` in its first
        ``len_b // hop + 1`` frames and zeros beyond; a clip's frames do not depend on the batch it is in."""
        if audio.dim() == 1:
            audio = audio[None]
        if not audio.is_cuda:
            raise RuntimeError("matcha-tts-24k_amd: audio is not on a HIP device; there is no CPU path")
        audio = audio.detach().to(torch.float32).contiguous()
        B, ld = audio.shape
        host = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(host) != B:
            raise ValueError(f"lengths must have {B} entries, got {len(host)}")
        hop = int(hop)
        if hop <= 0:
            raise ValueError("hop must be positive")
        for b, n in enumerate(host):
            if n < 0 or n > ld:
                raise ValueError(f"lengths[{b}] = {n} is outside [0, {ld}]")
            if (n // hop) * hop <= self.n_fft // 2:
                raise ValueError(f"clip {b} has {(n // hop) * hop} samples after trimming to a multiple of hop {hop}: reflect padding "
                                 f"needs more than n_fft / 2 = {self.n_fft // 2}")
        t_max = max(n_frames(n, hop) for n in host)
        d_len = torch.tensor(host, dtype=torch.int64, device=audio.device)
        mel = torch.empty(B, self.n_mels, t_max, dtype=torch.float32, device=audio.device)
        mel_len = torch.empty(B, dtype=torch.int64, device=audio.device)
        need = int(B) * t_max * ((self.n_bins + 31) // 32 * 32) * 4 + 256
        ws = self._ws.get("melfe", need, audio.device)
        self._last[_hip.stream_ptr()] = (B, t_max)
        with torch.cuda.device(audio.device):
            _hip.check(self.lib.mtts_melfe_forward(self.ctx, _hip.ptr(audio), ld, _hip.ptr(d_len), B, hop, float(mel_mean), float(mel_std),
                                                   _hip.ptr(mel), t_max, _hip.ptr(mel_len), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        return mel, mel_len


_front_ends: Dict[Tuple[int, int, int], MelFrontEnd] = {}


def front_end(sample_rate: int = 24000, n_fft: int = 1024, n_mels: int = 100) -> MelFrontEnd:
    """The process-wide front end of a shape (its tables are built once)."""
    key = (int(sample_rate), int(n_fft), int(n_mels))
    if key not in _front_ends:
        _front_ends[key] = MelFrontEnd(*key)
    return _front_ends[key]


def extract(audio: torch.Tensor, lengths: Sequence[int], hop: int, mel_mean: float = 0.0, mel_std: float = 1.0, sample_rate: int = 24000,
            n_fft: int = 1024, n_mels: int = 100) -> Tuple[torch.Tensor, torch.Tensor]:
    """Ragged batch of clips -> (normalised log-mel [B, n_mels, T_max], frames [B]); see ``MelFrontEnd.extract``."""
    return front_end(sample_rate, n_fft, n_mels).extract(audio, lengths, hop, mel_mean, mel_std)


def get_mel_extractor(*, sample_rate: int = 24000, n_fft: int = 1024, hop_length: int = 256, win_length: int = 1024, n_mels: int = 100,
                      log_eps: float = 1e-7, **_) -> Callable[[torch.Tensor], torch.Tensor]:
    """reference matcha/vocos24k/mel_extractor.py:6-41: ``extract_fn(y) -> log-mel`` (un-normalised), y [..., samples] on the device."""
    if int(win_length) != int(n_fft):
        raise ValueError("win_length must equal n_fft (the reference's only configuration)")
    if abs(float(log_eps) - LOG_EPS) > 1e-12:
        raise ValueError(f"log_eps is fixed at {LOG_EPS} in the library (the reference's value)")
    fe = front_end(sample_rate, n_fft, n_mels)

    def extract_fn(y: torch.Tensor) -> torch.Tensor:
        lead = y.shape[:-1]
        flat = y.reshape(-1, y.shape[-1])
        mel, _ = fe.extract(flat, [flat.shape[-1]] * flat.shape[0], hop_length)
        return mel.reshape(*lead, n_mels, mel.shape[-1])

    return extract_fn

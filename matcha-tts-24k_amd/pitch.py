"""Pitch on MI355X: the F0 contour of every clip of a ragged batch and its per-clip statistics -- how high a voice speaks, how wide
it ranges and whether it rises at the end, which is what the reference's documentation/pitch_raise_transfer.md needs to know about a
speaker (steps 1-2) and what a synthesised question can be checked for.

* ``track``  -- YIN (de Cheveigne & Kawahara 2002) cut into blocks (``mtts_pitch_track``): ``f0`` in Hz (0 = unvoiced) and
  ``aperiodicity`` per frame; frames step by ``hop`` samples (default: the model's fine-mel hop of 128 at 24 kHz, so pitch frames
  step with fine mel frames and with ``token_ends``), a frame reads ``8 hop + max_lag`` samples and nothing is padded.
* ``frame_times`` -- the nominal time of every frame, in seconds.
* ``stats``  -- exact order statistics of the voiced values (``mtts_pitch_stats``): median, 5 % and 95 % points, the median of the
  last ``tail`` seconds of voicing, and from them ``range_st`` and ``final_rise_st`` in semitones.

Arithmetic runs in libmtts_hip.so (include/mtts.h "pitch" states every order of summation); there is no CPU path.
Octave errors are not smoothed (no Viterbi / pYIN pass) and nothing is folded per token.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _hip

MAX_LAG = 1024            # include/mtts.h MTTS_PITCH_MAX_LAG
_ws = _hip.Workspaces()


def default_hop(sample_rate: int) -> int:
    """128 samples at 24 kHz -- the model's fine-mel hop -- and the same duration at another rate."""
    sr = int(sample_rate)
    return 128 if sr == 24000 else int(round(sr * 128 / 24000))


def plan(sample_rate: int = 24000, hop: Optional[int] = None, fmin: float = 60.0, fmax: float = 500.0) -> Tuple[int, int, int, int]:
    """``(hop, window, min_lag, max_lag)`` of these parameters, or ``ValueError`` with the library's reason."""
    hop = default_hop(sample_rate) if hop is None else int(hop)
    w, lo, hi = C.c_int(), C.c_int(), C.c_int()
    lib = _hip.load()
    if lib.mtts_pitch_plan(int(sample_rate), hop, float(fmin), float(fmax), C.byref(w), C.byref(lo), C.byref(hi)) != 0:
        raise ValueError(lib.mtts_last_error().decode("utf-8", "replace"))
    return hop, w.value, lo.value, hi.value


def n_frames(length: int, hop: int, window: int, max_lag: int) -> int:
    """Frames of a clip of ``length`` samples: 0 below ``window + max_lag``, else ``(length - window - max_lag) // hop + 1``."""
    return 0 if length < window + max_lag else (length - window - max_lag) // hop + 1


def frame_times(n: int, hop: int, window: int, max_lag: int, sample_rate: int) -> torch.Tensor:
    """Nominal times of frames 0 .. n - 1 in seconds (float64, host): ``(k hop + (window + max_lag) / 2) / sample_rate``."""
    k = torch.arange(int(n), dtype=torch.float64)
    return (k * int(hop) + (int(window) + int(max_lag)) / 2.0) / float(int(sample_rate))


@torch.inference_mode()
def track(audio, lengths=None, sample_rate: int = 24000, hop: Optional[int] = None, fmin: float = 60.0, fmax: float = 500.0,
          threshold: float = 0.15, check: bool = True) -> Dict[str, object]:
    """F0 contour of every clip.  ``audio`` / ``lengths`` as for ``corpus.measure_silence`` (a list of 1-D clips or a padded batch).
    Returns ``{"f0": float32 [B, T] in Hz, 0 where unvoiced, "aperiodicity": float32 [B, T] (YIN's d' at the chosen lag; NaN for a
    frame that read a NaN or Inf sample), "frames": int64 [B], "hop", "window", "max_lag"}`` -- device tensors and ints; columns at or
    beyond a row's frame count hold f0 = 0, aperiodicity = 1.  A length outside ``[0, L]`` gives frames = -1 in that row; with
    ``check`` the call waits for that verdict and raises ``ValueError`` naming the row."""
    from . import corpus as CP
    hop, window, _, max_lag = plan(sample_rate, hop, fmin, fmax)
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"threshold must lie in (0, 1), got {threshold}")
    wave, d_len = CP._batch(audio, lengths)
    lib = _hip.load()
    B, ld = wave.shape
    T = max(1, n_frames(ld, hop, window, max_lag))
    f0 = torch.empty(B, T, dtype=torch.float32, device=wave.device)
    aper = torch.empty(B, T, dtype=torch.float32, device=wave.device)
    frames = torch.empty(B, dtype=torch.long, device=wave.device)
    ws = _ws.get("pitch", lib.mtts_pitch_workspace_bytes(ld, B, int(sample_rate), hop, float(fmin), float(fmax)), wave.device)
    with torch.cuda.device(wave.device):
        _hip.check(lib.mtts_pitch_track(_hip.ptr(wave), ld, _hip.ptr(d_len), B, int(sample_rate), hop, float(fmin), float(fmax), float(threshold),
                                        _hip.ptr(f0), _hip.ptr(aper), T, _hip.ptr(frames), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _hip.raise_refused(lib.mtts_pitch_status, ws.data_ptr(), _hip.stream_ptr())
    return {"f0": f0, "aperiodicity": aper, "frames": frames, "hop": hop, "window": window, "max_lag": max_lag}


def _semitones(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    return 12.0 * torch.log2(num.to(torch.float64) / den.to(torch.float64))


@torch.inference_mode()
def stats(f0: torch.Tensor, frames, hop: int, sample_rate: int, tail: float = 0.25) -> Dict[str, torch.Tensor]:
    """Per-clip statistics of a contour of ``track``.  Device tensors [B]: ``median_hz``, ``p05_hz``, ``p95_hz`` (float32: exact order
    statistics of the voiced values, v[(m - 1) p] of the m sorted values), ``tail_median_hz`` (the median of the voiced frames within
    ``tail`` seconds before the last voiced one; NaN with fewer than 3), ``voiced_fraction`` (float64), the counts ``frames``,
    ``voiced``, ``tail_voiced`` (int64), and in float64 ``range_st = 12 log2(p95 / p05)`` and ``final_rise_st = 12 log2(tail_median /
    median)``: positive when the voice ends above its own median, as a question does.  A clip without a voiced frame has NaN."""
    lib = _hip.load()
    if f0.dim() != 2:
        raise ValueError("f0 must be [B, T]")
    if not f0.is_cuda:
        raise RuntimeError("matcha-tts-24k_amd: f0 is not on a HIP device; there is no CPU path")
    f0 = f0.detach().to(torch.float32).contiguous()
    B, T = f0.shape
    if B < 1 or T < 1:
        raise ValueError("f0 must have at least one row and one column")
    d_frames = _hip.row_lengths(frames, B, T, f0.device, "frames")
    tail_frames = int(round(float(tail) * int(sample_rate) / int(hop)))
    if tail_frames < 0:
        raise ValueError("tail must not be negative")
    hz = torch.empty(B, 4, dtype=torch.float32, device=f0.device)
    counts = torch.empty(B, 3, dtype=torch.long, device=f0.device)
    ws = _ws.get("pitch_stats", 512, f0.device)
    with torch.cuda.device(f0.device):
        _hip.check(lib.mtts_pitch_stats(_hip.ptr(f0), T, _hip.ptr(d_frames), B, tail_frames, _hip.ptr(hz), _hip.ptr(counts), ws.data_ptr(),
                                        ws.numel(), _hip.stream_ptr()))
    n, m = counts[:, 0].to(torch.float64), counts[:, 1].to(torch.float64)
    return {"p05_hz": hz[:, 0], "median_hz": hz[:, 1], "p95_hz": hz[:, 2], "tail_median_hz": hz[:, 3],
            "voiced_fraction": torch.where(n > 0, m / n.clamp(min=1.0), torch.zeros_like(n)),
            "frames": counts[:, 0], "voiced": counts[:, 1], "tail_voiced": counts[:, 2],
            "range_st": _semitones(hz[:, 2], hz[:, 0]), "final_rise_st": _semitones(hz[:, 3], hz[:, 1])}

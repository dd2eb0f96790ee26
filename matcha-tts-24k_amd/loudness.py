"""Loudness on MI355X (``mtts_loudness``): integrated loudness of a ragged batch as in ITU-R BS.1770 / EBU R 128 -- K-weighting, 400 ms
blocks at 75 % overlap, the absolute and the relative gate -- and one gain per row towards a target in LUFS, limited so that the
sample peak stays at or under a ceiling.  Measured and applied on the device, in place, without a host synchronisation.
``meter`` and ``normalize(true_peak=)`` (``mtts_loudness_r128``) add the true peak (oversampled), the loudness range, the maximum
momentary and short-term loudness, and a second ceiling on the gain, in dBTP.

Every number is defined by include/mtts.h "loudness"  and restated in tests/loudness_restated.py; there is no CPU
path.  A row shorter than one 400 ms block is one block of its own length (a documented deviation from BS.1770: a short answer must
still be levelled).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import _hip

PEAK_CEILING = 0.95           # the level the reference's own normalisation leaves (inference.py:260-264)
_ws = _hip.Workspaces()


def __getattr__(name):
    if name == "TILE":        # samples per workgroup of the chunk passes at 24 / 48 kHz (MTTS_LOUDNESS_TILE)
        return int(_hip.load().mtts_loudness_tile())
    if name == "TRUE_PEAK_TILE":                                       # samples per workgroup of the true-peak pass
        return int(_hip.load().mtts_true_peak_tile())
    raise AttributeError(name)


def chunk(sample_rate: int = 24000) -> int:
    """Samples per chunk of the time-cut recurrence at ``sample_rate`` (``mtts_loudness_chunk``)."""
    return _hip.size(_hip.load().mtts_loudness_chunk(int(sample_rate)))


def check_rate(sample_rate) -> int:
    rate = int(sample_rate)
    if rate != sample_rate or rate % 100 or not 8000 <= rate <= 192000:
        raise ValueError(f"loudness: sample_rate must be a multiple of 100 in [8000, 192000], got {sample_rate!r}")
    return rate


def check_target(value, what: str = "loudness") -> Optional[float]:
    """A target in LUFS as a float, None for "leave the row alone"; ``ValueError`` / ``TypeError`` for anything that is no number, not
    finite or above 0 LUFS (full scale).  Host-only: callers validate before anything is launched."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"{what} is a number of LUFS or None, got {value!r}")
    v = float(value)
    if not math.isfinite(v) or v > 0.0:
        raise ValueError(f"{what} must be a finite level at or below 0 LUFS, got {value!r}")
    return v


def check_true_peak(value, what: str = "true_peak") -> Optional[float]:
    """A true-peak ceiling in dBTP as a float, None for none; ``ValueError`` / ``TypeError`` for anything that is no number, not finite
    or above 0 dBTP (full scale).  Host-only: callers validate before anything is launched."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"{what} is a number of dBTP or None, got {value!r}")
    v = float(value)
    if not math.isfinite(v) or v > 0.0:
        raise ValueError(f"{what} must be a finite level at or below 0 dBTP, got {value!r}")
    return v


def check_ceiling(true_peak, loudness) -> Optional[float]:
    """``check_true_peak`` of a unit's ceiling beside its checked target ``loudness``: the ceiling limits the gain towards a loudness
    target, so one without a target raises ``ValueError`` too.  The one rule of every entry that takes the pair.  Host-only."""
    ceiling = check_true_peak(true_peak)
    if ceiling is not None and loudness is None:
        raise ValueError(f"true_peak = {true_peak!r} limits the gain towards a loudness target, and none is named (loudness=)")
    return ceiling


def dbtp(x):
    """A linear peak -- a number or a tensor -- in dB relative to full scale: ``20 log10(x)``, -inf for 0."""
    if torch.is_tensor(x):
        return 20.0 * torch.log10(x.to(torch.float64))
    x = float(x)
    return 20.0 * math.log10(x) if x > 0.0 else (-math.inf if x == 0.0 else math.nan)


def true_peak_filter(sample_rate: int = 24000):
    """``(F, h)``: the oversampling factor at ``sample_rate`` and the float32 [F, 12] table of the interpolator
    (``mtts_true_peak_filter``; host only)."""
    import ctypes as C
    out, F = (C.c_float * 96)(), C.c_int(0)
    _hip.check(_hip.load().mtts_true_peak_filter(check_rate(sample_rate), out, C.byref(F)))
    return F.value, torch.tensor(list(out)[:12 * F.value], dtype=torch.float32).reshape(F.value, 12)


def targets_per_row(target, B: int, what: str = "loudness"):
    """``target`` -- a number, None, or one of them per row -- as a list of B floats with NaN for "measure only"; None when no row
    has a target."""
    if target is None or isinstance(target, (int, float)):
        vals = [check_target(target, what)] * B
    else:
        vals = [check_target(v, what) for v in (target.tolist() if torch.is_tensor(target) else target)]
        if len(vals) != B:
            raise ValueError(f"{what} is a number or one per row ({B}), got {len(vals)}")
    if all(v is None for v in vals):
        return None
    return [math.nan if v is None else v for v in vals]


def _run(audio, lengths, sample_rate, target, peak_ceiling, apply, check, true_peak=None, r128=False):
    lib = _hip.load()
    rate = check_rate(sample_rate)
    tp_db = check_true_peak(true_peak)
    rows, L = _hip.aligned_rows(audio, 4, "audio")
    if apply and rows.data_ptr() != audio.data_ptr():                  # (aligned_rows made a padded or converted copy)
        raise ValueError("loudness.normalize works in place: audio must be a contiguous float32 [B, ld] tensor with ld % 4 == 0 "
                         "and a 16-byte aligned base")
    (B, ld), dev = rows.shape, rows.device
    lengths = _hip.row_lengths(lengths, B, L, dev)
    if target is not None:
        if torch.is_tensor(target) and target.is_cuda:
            target = target.to(torch.float32).contiguous()
            if target.shape != (B,):
                raise ValueError(f"target must have shape ({B},), got {tuple(target.shape)}")
        else:
            if not isinstance(target, (int, float)):                   # (a NaN in a sequence is "leave the row alone", as None is)
                target = [None if isinstance(v, float) and math.isnan(v) else v
                          for v in (target.tolist() if torch.is_tensor(target) else target)]
            vals = targets_per_row(target, B, "target")
            target = None if vals is None else torch.tensor(vals, dtype=torch.float32).to(dev)
    ceiling = float(peak_ceiling)
    if not (math.isfinite(ceiling) and ceiling > 0.0):
        raise ValueError(f"peak_ceiling must be positive and finite, got {peak_ceiling!r}")
    lufs = torch.empty(B, dtype=torch.float64, device=dev)
    gain = torch.empty(B, dtype=torch.float32, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if not r128 and tp_db is None:
            ws = _ws.get("loudness", lib.mtts_loudness_workspace_bytes(ld, B, rate), dev)
            _hip.check(lib.mtts_loudness(_hip.ptr(rows), ld, _hip.ptr(lengths), B, rate, _hip.ptr(target), ceiling, int(bool(apply)),
                                         _hip.ptr(lufs), _hip.ptr(gain), _hip.ptr(peak), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
            more = None
        else:
            tp = torch.empty(B, dtype=torch.float32, device=dev)
            more = torch.empty(3, B, dtype=torch.float64, device=dev)  # lra, momentary_max, short_term_max
            ws = _ws.get("r128", lib.mtts_loudness_r128_workspace_bytes(ld, B, rate), dev)
            _hip.check(lib.mtts_loudness_r128(_hip.ptr(rows), ld, _hip.ptr(lengths), B, rate, _hip.ptr(target), ceiling,
                                              math.nan if tp_db is None else tp_db, int(bool(apply)), _hip.ptr(lufs), _hip.ptr(gain),
                                              _hip.ptr(peak), _hip.ptr(tp), _hip.ptr(more[0]), _hip.ptr(more[1]), _hip.ptr(more[2]),
                                              ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
            more = dict(lufs=lufs, lra=more[0], momentary_max=more[1], short_term_max=more[2], peak=peak, true_peak=tp, gain=gain)
        if check:
            _hip.raise_refused(lib.mtts_loudness_status, ws.data_ptr(), _hip.stream_ptr())
    return lufs, gain, peak, more


@torch.inference_mode()
def measure(audio: torch.Tensor, lengths=None, sample_rate: int = 24000) -> torch.Tensor:
    """Integrated loudness in LUFS of every row of ``audio`` [B, L] (or [L]) on the device, ``lengths`` [B] valid samples (tensor or
    sequence; default all L): a float64 device tensor [B], -inf for a row no block of which passes the absolute gate (silence, an
    empty row), NaN for a row whose length is outside its row.  Nothing is read on the host and nothing is waited for."""
    return _run(audio, lengths, sample_rate, None, PEAK_CEILING, False, False)[0]


@torch.inference_mode()
def meter(audio: torch.Tensor, lengths=None, sample_rate: int = 24000) -> Dict[str, torch.Tensor]:
    """What a loudness meter shows of every row of ``audio`` [B, L] (or [L]), as a dict of device tensors [B]: ``lufs`` (integrated, as
    ``measure``), ``lra`` (loudness range in LU, EBU Tech 3342; 0 for a row under 3 s), ``momentary_max`` and ``short_term_max`` (LUFS;
    the latter -inf for a row under 3 s) in float64, ``peak`` and ``true_peak`` (linear; ``dbtp`` gives dB) in float32.  NaN / 0 for
    a row whose length is outside its row.  The audio is not written; nothing is read on the host and nothing is waited for."""
    m = _run(audio, lengths, sample_rate, None, PEAK_CEILING, False, False, None, True)[3]
    return {k: m[k] for k in ("lufs", "lra", "momentary_max", "short_term_max", "peak", "true_peak")}


@torch.inference_mode()
def normalize(audio: torch.Tensor, lengths, target, sample_rate: int = 24000, peak_ceiling: float = PEAK_CEILING, check: bool = True,
              true_peak: Optional[float] = None, return_meter: bool = False):
    """Bring every row of ``audio`` [B, ld] (float32, contiguous, ld % 4 == 0, on the device) to ``target`` LUFS IN PLACE: ``target`` a
    number, or one per row where None / NaN leaves a row alone (a host sequence, or a float32 device tensor [B]).  Returns device
    tensors ``(lufs float64 [B], gain float32 [B], peak float32 [B])``: the loudness and the sample peak as measured BEFORE the gain,
    and the gain applied -- ``10 ** ((target - lufs) / 20)``, limited to ``peak_ceiling / peak`` where the scaled sample peak would
    exceed the ceiling, and exactly 1 (the row keeps its bits) for a row without a target, an empty row and a row whose loudness is
    not finite.  Samples at or beyond a row's length are not written.  ``check`` waits for the device's verdict on the lengths and
    raises ``ValueError`` naming the first refused row; without it nothing is waited for.

    ``true_peak``: None (exactly the call above), or a ceiling in dBTP (finite, at most 0; typically -1): the gain of a row that has a
    target is then also limited to ``10 ** (true_peak / 20) / true_peak_b``, the true peak being the row's level between the samples
    as the device's 12-tap interpolator reads it, so that what the rate conversion and the encoder behind reconstruct stays under
    the ceiling.  ``return_meter``: also return the dict of ``meter`` -- measured BEFORE the gain -- with ``"gain"`` added."""
    lufs, gain, peak, more = _run(audio, lengths, sample_rate, target, peak_ceiling, True, check, true_peak, bool(return_meter))
    return (lufs, gain, peak, more) if return_meter else (lufs, gain, peak)

"""Pitch on MI355X: the F0 contour of every clip of a ragged batch and its per-clip statistics -- how high a voice speaks, how wide
it ranges and whether it rises at the end, which is what the reference's documentation/pitch_raise_transfer.md needs to know about a
speaker (steps 1-2) and what a synthesised question can be checked for.

* ``track``  -- YIN (de Cheveigne & Kawahara 2002) cut into blocks (``mtts_pitch_track``): ``f0`` in Hz (0 = unvoiced) and
  ``aperiodicity`` per frame; frames step by ``hop`` samples (default: the model's fine-mel hop of 128 at 24 kHz, so pitch frames
  step with fine mel frames and with ``token_ends``), a frame reads ``8 hop + max_lag`` samples and nothing is padded.
* ``frame_times`` -- the nominal time of every frame, in seconds.
* ``stats``  -- exact order statistics of the voiced values (``mtts_pitch_stats``): median, 5 % and 95 % points, the median of the
  last ``tail`` seconds of voicing, and from them ``range_st`` and ``final_rise_st`` in semitones.

* ``candidates`` / ``viterbi`` / ``track_viterbi`` -- a pYIN-style tracker: up to 8 candidate periods per frame with a probability
  mass each (``mtts_pitch_candidates``) and one shortest path per clip through them (``mtts_pitch_viterbi``), which removes the
  octave excursions plain YIN makes where it decides a frame alone.  Opt-in: ``track`` keeps its launches and its bits;
  ``contour(method=)`` chooses between the two.
* ``fold``   -- a contour folded onto the token marks of ``timing.token_marks``: median / first / last Hz and energy per token
  (``mtts_pitch_fold``).
* ``compare`` -- F0 RMSE in cents, log-F0 correlation, gross and voicing error of two frame-aligned contours (plain torch).

Arithmetic runs in libmtts_hip.so (include/mtts.h "pitch" and "prosody" state every order of operations); there is no CPU
path.
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


CANDS = 8                 # include/mtts.h MTTS_PITCH_CANDS
UNVOICED = 8              # the state index of "unvoiced" on a path
LATTICE = ("period", "mass", "depth", "count", "unvoiced_mass", "floor")


@torch.inference_mode()
def candidates(audio, lengths=None, sample_rate: int = 24000, hop: Optional[int] = None, fmin: float = 60.0, fmax: float = 500.0,
               threshold: float = 0.15, check: bool = True) -> Dict[str, object]:
    """The candidate lattice of every clip (``mtts_pitch_candidates``): per frame up to 8 record-setting dips of YIN's d' with their
    probability mass under a threshold prior uniform on ``[0, 2 threshold]`` (pYIN's idea).  Arguments as for ``track``.  Returns
    ``{"period", "mass", "depth": float32 [B, T, 8] in ascending lag, "count": int32 [B, T] (-1: the frame read a NaN or Inf sample),
    "unvoiced_mass", "floor": float32 [B, T], "frames": int64 [B], "hop", "window", "max_lag", "sample_rate"}``; columns at or beyond a
    row's frame count hold count = 0, unvoiced_mass = 1, floor = 1."""
    from . import corpus as CP
    hop, window, _, max_lag = plan(sample_rate, hop, fmin, fmax)
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError(f"threshold must lie in (0, 1), got {threshold}")
    wave, d_len = CP._batch(audio, lengths)
    lib = _hip.load()
    B, ld = wave.shape
    T = max(1, n_frames(ld, hop, window, max_lag))
    f3 = [torch.empty(B, T, CANDS, dtype=torch.float32, device=wave.device) for _ in range(3)]
    count = torch.empty(B, T, dtype=torch.int32, device=wave.device)
    f2 = [torch.empty(B, T, dtype=torch.float32, device=wave.device) for _ in range(2)]
    frames = torch.empty(B, dtype=torch.long, device=wave.device)
    ws = _ws.get("pitch", lib.mtts_pitch_workspace_bytes(ld, B, int(sample_rate), hop, float(fmin), float(fmax)), wave.device)
    with torch.cuda.device(wave.device):
        _hip.check(lib.mtts_pitch_candidates(_hip.ptr(wave), ld, _hip.ptr(d_len), B, int(sample_rate), hop, float(fmin), float(fmax),
                                             float(threshold), _hip.ptr(f3[0]), _hip.ptr(f3[1]), _hip.ptr(f3[2]), _hip.ptr(count),
                                             _hip.ptr(f2[0]), _hip.ptr(f2[1]), T, _hip.ptr(frames), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _hip.raise_refused(lib.mtts_pitch_status, ws.data_ptr(), _hip.stream_ptr())
    return {"period": f3[0], "mass": f3[1], "depth": f3[2], "count": count, "unvoiced_mass": f2[0], "floor": f2[1], "frames": frames,
            "hop": hop, "window": window, "max_lag": max_lag, "sample_rate": int(sample_rate)}


@torch.inference_mode()
def viterbi(lattice: Dict[str, object], jump: float = 2.0, switch: float = 0.5, sample_rate: Optional[int] = None,
            check: bool = True) -> Dict[str, object]:
    """One shortest path per clip through a lattice of ``candidates`` (``mtts_pitch_viterbi``; a lattice made by hand works too: it
    needs the tensors of ``LATTICE``, ``"frames"`` and a sample rate).  A candidate costs ``1 - mass``, unvoiced ``1 - unvoiced_mass``;
    moving between two periods costs ``jump`` per octave-sized relative step, entering or leaving unvoiced costs ``switch``.  Returns
    ``track``'s keys -- ``f0``, ``aperiodicity`` (the chosen dip's depth; the frame's floor where unvoiced), ``frames`` and the plan --
    plus ``"state"``: int8 [B, T], the chosen candidate, 8 = unvoiced, -1 beyond the row's frames.

    The defaults ``jump = 2.0``, ``switch = 0.5`` were chosen on synthetic signals only (any jump in 2 .. 8 behaves the same there;
    jump = 1 does not smooth an octave excursion); nobody has tried them on real speech."""
    lib = _hip.load()
    if not 0.0 <= float(jump) <= 1e6 or not 0.0 <= float(switch) <= 1e6:
        raise ValueError(f"jump and switch must lie in [0, 1e6], got {jump}, {switch}")
    fs = int(lattice["sample_rate"] if sample_rate is None else sample_rate)
    period = lattice["period"]
    if not (torch.is_tensor(period) and period.dim() == 3 and period.shape[2] == CANDS):
        raise ValueError("lattice['period'] must be [B, T, 8]")
    if not period.is_cuda:
        raise RuntimeError("matcha-tts-24k_amd: the lattice is not on a HIP device; there is no CPU path")
    dev = period.device
    B, T = period.shape[:2]
    if B < 1 or T < 1:
        raise ValueError("the lattice must have at least one row and one column")
    t = {}
    for k in LATTICE:
        want = (B, T, CANDS) if k in ("period", "mass", "depth") else (B, T)
        t[k] = lattice[k].detach().to(device=dev, dtype=torch.int32 if k == "count" else torch.float32).contiguous()
        if tuple(t[k].shape) != want:
            raise ValueError(f"lattice[{k!r}] must have shape {want}, got {tuple(t[k].shape)}")
    d_frames = _hip.row_lengths(lattice["frames"], B, T, dev, "frames")
    f0 = torch.empty(B, T, dtype=torch.float32, device=dev)
    aper = torch.empty(B, T, dtype=torch.float32, device=dev)
    state = torch.empty(B, T, dtype=torch.int8, device=dev)
    ws = _ws.get("pitch_viterbi", lib.mtts_pitch_viterbi_workspace_bytes(T, B), dev)
    with torch.cuda.device(dev):
        _hip.check(lib.mtts_pitch_viterbi(*[_hip.ptr(t[k]) for k in LATTICE], T, _hip.ptr(d_frames), B, fs, float(jump), float(switch),
                                          _hip.ptr(f0), _hip.ptr(aper), _hip.ptr(state), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _hip.raise_refused(lib.mtts_pitch_status, ws.data_ptr(), _hip.stream_ptr())
    out = {"f0": f0, "aperiodicity": aper, "frames": d_frames, "state": state}
    for k in ("hop", "window", "max_lag"):
        if k in lattice:
            out[k] = lattice[k]
    return out


@torch.inference_mode()
def track_viterbi(audio, lengths=None, sample_rate: int = 24000, hop: Optional[int] = None, fmin: float = 60.0, fmax: float = 500.0,
                  threshold: float = 0.15, check: bool = True, jump: float = 2.0, switch: float = 0.5) -> Dict[str, object]:
    """``track`` with octave errors smoothed: ``candidates`` then ``viterbi`` -- the same keys as ``track`` plus ``"state"``, so
    ``stats`` and ``fold`` take the result unchanged.  ``track`` itself (plain YIN, every frame decided alone) is untouched."""
    return viterbi(candidates(audio, lengths, sample_rate, hop, fmin, fmax, threshold, check), jump, switch, check=check)


METHODS = {"yin": track, "viterbi": track_viterbi}


def contour(audio, lengths=None, sample_rate: int = 24000, method: str = "yin", **params) -> Dict[str, object]:
    """``track`` (``method="yin"``: exactly its calls) or ``track_viterbi`` (``"viterbi"``, which also takes ``jump=`` and ``switch=``)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
    return METHODS[method](audio, lengths, sample_rate, **params)


@torch.inference_mode()
def fold(tracked: Dict[str, object], marks, x_lengths, audio=None, lengths=None, check: bool = True) -> Dict[str, torch.Tensor]:
    """Pitch and energy per token (``mtts_pitch_fold``): a contour of ``track`` / ``track_viterbi`` folded onto ``marks`` int64
    [B, Tx, 2], the (start, end) of every token in samples of the clip exactly as ``timing.token_marks`` returns them (-1: no token).
    Frame k belongs to the token whose marks hold its nominal centre.  Returns device tensors [B, Tx]: ``frames``, ``voiced`` (int32),
    ``median_hz`` (the exact order statistic v[(m - 1) / 2] of the token's voiced values), ``first_hz``, ``last_hz`` (float32; NaN
    without a voiced frame) and, with ``audio`` (a padded batch or a list of clips, with ``lengths``), ``mean_square`` (float64: 0 for
    an empty token) and ``energy_db`` = 10 log10(mean_square).  ``lengths`` alone bounds the marks.  A row with a mark outside
    ``[0, length]``, ``start > end``, marks that do not ascend or frames = -1 is refused (frames = -1 in that row; with ``check`` a
    ``ValueError`` names it) and the other rows are untouched."""
    lib = _hip.load()
    f0 = tracked["f0"]
    if not (torch.is_tensor(f0) and f0.dim() == 2):
        raise ValueError("tracked['f0'] must be [B, T]")
    if not f0.is_cuda:
        raise RuntimeError("matcha-tts-24k_amd: the contour is not on a HIP device; there is no CPU path")
    dev = f0.device
    f0 = f0.detach().to(torch.float32).contiguous()
    B, T = f0.shape
    marks = torch.as_tensor(marks).to(device=dev, dtype=torch.long).contiguous()
    if marks.dim() != 3 or marks.shape[0] != B or marks.shape[2] != 2 or marks.shape[1] < 1:
        raise ValueError(f"marks must be [{B}, Tx, 2], got {tuple(marks.shape)}")
    Tx = marks.shape[1]
    d_frames = _hip.row_lengths(tracked["frames"], B, T, dev, "frames")
    d_xl = _hip.row_lengths(x_lengths, B, Tx, dev, "x_lengths")
    wave = d_len = ms = None
    ld = 0
    if audio is not None:
        from . import corpus as CP
        wave, d_len = CP._batch(audio, lengths, dev)
        if wave.shape[0] != B:
            raise ValueError(f"audio has {wave.shape[0]} rows, the contour {B}")
        ld = wave.shape[1]
        ms = torch.empty(B, Tx, dtype=torch.float64, device=dev)
    elif lengths is not None:
        d_len = _hip.row_lengths(lengths, B, 0, dev)
    counts = torch.empty(B, Tx, 2, dtype=torch.int32, device=dev)
    hz = torch.empty(B, Tx, 3, dtype=torch.float32, device=dev)
    ws = _ws.get("pitch_fold", 512, dev)
    with torch.cuda.device(dev):
        _hip.check(lib.mtts_pitch_fold(_hip.ptr(f0), T, _hip.ptr(d_frames), B, int(tracked["hop"]), int(tracked["window"]), int(tracked["max_lag"]),
                                       _hip.ptr(marks), Tx, _hip.ptr(d_xl), _hip.ptr(wave), ld, _hip.ptr(d_len), _hip.ptr(counts), _hip.ptr(hz),
                                       _hip.ptr(ms), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _hip.raise_refused(lib.mtts_pitch_status, ws.data_ptr(), _hip.stream_ptr())
    out = {"frames": counts[..., 0], "voiced": counts[..., 1], "median_hz": hz[..., 0], "first_hz": hz[..., 1], "last_hz": hz[..., 2]}
    if ms is not None:
        out["mean_square"] = ms
        out["energy_db"] = 10.0 * torch.log10(ms)
    return out


def compare(a, b, frames=None) -> Dict[str, torch.Tensor]:
    """Two frame-aligned contours [B, T] in Hz (0 = unvoiced; dicts of ``track`` work too), e.g. a recording and
    ``synthesise(durations=align(...))`` of it.  Plain torch on whatever device they are on.  Per row, over the first ``frames``
    columns (default: all; or the smaller ``"frames"`` of the dicts): ``rmse_cents`` and ``corr`` (Pearson, of log-F0) over the frames
    voiced in both, ``gross_error`` (the share of those off by more than 20 %), ``voicing_error`` (the share of all frames where
    exactly one is voiced) and the counts ``frames``, ``both_voiced``.  float64; NaN where a share has no frames (corr: fewer than 2,
    or a constant contour)."""
    if isinstance(a, dict) and isinstance(b, dict) and frames is None:
        frames = torch.minimum(torch.as_tensor(a["frames"]), torch.as_tensor(b["frames"]).to(torch.as_tensor(a["frames"]).device))
    a = a["f0"] if isinstance(a, dict) else torch.as_tensor(a)
    b = b["f0"] if isinstance(b, dict) else torch.as_tensor(b)
    if a.dim() == 1:
        a, b = a[None], b[None]
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"contours must be two [B, T] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = a.to(torch.float64), b.to(device=a.device, dtype=torch.float64)
    B, T = a.shape
    n = torch.full((B,), T, dtype=torch.long, device=a.device) if frames is None else torch.as_tensor(frames).to(a.device).long().clamp(0, T)
    inside = torch.arange(T, device=a.device)[None, :] < n[:, None]
    va, vb = (a > 0) & inside, (b > 0) & inside
    both = va & vb
    m = both.sum(1).to(torch.float64)
    nan = torch.full_like(m, float("nan"))
    one = torch.ones_like(a)
    la, lb = torch.log2(torch.where(both, a, one)), torch.log2(torch.where(both, b, one))
    d = 1200.0 * (la - lb)
    rmse = torch.where(m > 0, torch.sqrt((d * d).sum(1) / m.clamp(min=1.0)), nan)
    ma, mb = la.sum(1) / m.clamp(min=1.0), lb.sum(1) / m.clamp(min=1.0)
    ca, cb = torch.where(both, la - ma[:, None], 0.0 * one), torch.where(both, lb - mb[:, None], 0.0 * one)
    den = torch.sqrt((ca * ca).sum(1) * (cb * cb).sum(1))
    corr = torch.where((m > 1) & (den > 0), (ca * cb).sum(1) / torch.where(den > 0, den, torch.ones_like(den)), nan)
    gross = (both & ((a / torch.where(both, b, one) - 1.0).abs() > 0.2)).sum(1).to(torch.float64)
    nf = n.to(torch.float64)
    return {"rmse_cents": rmse, "corr": corr, "gross_error": torch.where(m > 0, gross / m.clamp(min=1.0), nan),
            "voicing_error": torch.where(nf > 0, (va ^ vb).sum(1).to(torch.float64) / nf.clamp(min=1.0), nan),
            "frames": n, "both_voiced": both.sum(1)}


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

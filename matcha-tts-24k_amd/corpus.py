"""Corpus preparation on MI355X: what the reference does to a corpus before training, one file at a time on the CPU, for a ragged
batch of clips on the device.

* ``measure_silence``  -- reference matcha/utils/measure_silence.py:66-132 and the content bounds of
  matcha/utils/normalize_silence.py:86-136 (``mtts_silence_measure``);
* ``normalize_silence`` -- reference matcha/utils/normalize_silence.py:157-220: every clip rebuilt as
  ``[target leading zeros] + content + [target trailing zeros]`` (``mtts_silence_normalize``);
* ``MelStatistics``    -- reference matcha/utils/generate_data_statistics.py:120-154: the ``mel_mean`` / ``mel_std`` every
  normalised mel of this package depends on (``mtts_mel_stats`` on the front end's un-normalised log-mel);
* ``precompute_mels``  -- reference matcha/utils/precompute_mels.py:100-116: the normalised mel at ``hop`` and at ``hop // 2``;
* ``measure_pitch``    -- median F0, range and final rise of every clip (``pitch.track`` + ``pitch.stats``): what the reference's
  documentation/pitch_raise_transfer.md needs to know about a speaker.

All of them take a list of 1-D clips (host or device) or a padded batch ``[B, L]`` with ``lengths``.  Arithmetic runs in
libmtts_hip.so (include/mtts.h "corpus preparation"); there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip

COLUMNS = ("content_start", "content_end", "leading_eff", "leading_abs", "trailing_eff", "trailing_abs")
_ws = _hip.Workspaces()


def window(sample_rate: int) -> int:
    """Samples of the 10 ms window: ``int(0.01 * sample_rate)`` (reference measure_silence.py:94)."""
    return int(_hip.load().mtts_silence_window(int(sample_rate)))


def target_samples(seconds: Optional[float], sample_rate: int, label: str = "leading") -> int:
    """A target in seconds as samples (-1 for None), a whole multiple of the window or ``ValueError`` -- reference
    normalize_silence.py:139-154."""
    if seconds is None:
        return -1
    n = int(round(float(seconds) * int(sample_rate)))
    if n < 0 or n % window(sample_rate) != 0:
        raise ValueError(f"{label} silence target of {float(seconds)} s is {n} samples at {int(sample_rate)} Hz: not a whole, non-negative "
                         f"multiple of 10 ms (the window of {window(sample_rate)} samples), so a second pass would move the content")
    return n


def _batch(audio, lengths=None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Clips -> ``(wave [B, ld] fp32 on the device with ld % 4 == 0, lengths int64 [B] on the device)``.  ``audio``: a list of
    1-D waveforms (``lengths``: samples to use of each, default all) or a padded batch [B, L] (or [L]) with ``lengths`` (tensor or
    sequence, default all L).  Host data -- clips, a tensor or a NumPy batch -- is uploaded to ``device`` (default: the current HIP
    device); device lengths are not read on the host."""
    if torch.is_tensor(audio) or isinstance(audio, np.ndarray):
        audio = torch.as_tensor(audio)
        if audio.dim() not in (1, 2):
            raise ValueError("audio must be [B, L] or a list of 1-D clips")
        if device is not None or not audio.is_cuda:
            audio = audio.to(device if device is not None else torch.device("cuda"))
        wave, full = _hip.aligned_rows(audio, 4, "audio")
    else:
        clips = [torch.as_tensor(c) for c in audio]
        if len(clips) == 0:
            raise ValueError("no clips")
        if any(c.dim() != 1 for c in clips):
            raise ValueError("a clip is a 1-D waveform (mono)")
        if device is None:
            device = next((c.device for c in clips if c.is_cuda), torch.device("cuda"))
        B, full = len(clips), None
        if lengths is None:
            lengths = [int(c.numel()) for c in clips]
        wave = torch.zeros(B, max(4, (max(int(c.numel()) for c in clips) + 3) // 4 * 4), dtype=torch.float32, device=device)
        for b, c in enumerate(clips):
            wave[b, :c.numel()].copy_(c.to(torch.float32))
    return wave, _hip.row_lengths(lengths, wave.shape[0], full, wave.device)


def _seconds(samples: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """samples / sample_rate in fp64, correctly rounded (tensor by tensor: a scalar divisor becomes a multiplication by its inverse)."""
    s = samples.to(torch.float64)
    return s / torch.full_like(s, float(int(sample_rate)))


def _status(fn, ws) -> None:
    _hip.raise_refused(fn, ws.data_ptr(), _hip.stream_ptr())


def _measure(wave: torch.Tensor, lengths: torch.Tensor, sample_rate: int, effective_db: float, absolute_db: float):
    lib = _hip.load()
    B, ld = wave.shape
    out = torch.empty(B, 6, dtype=torch.long, device=wave.device)
    ws = _ws.get("silence", lib.mtts_silence_workspace_bytes(ld, B, int(sample_rate)), wave.device)
    with torch.cuda.device(wave.device):
        _hip.check(lib.mtts_silence_measure(_hip.ptr(wave), ld, _hip.ptr(lengths), B, int(sample_rate), float(effective_db), float(absolute_db),
                                            _hip.ptr(out), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    return out, ws


@torch.inference_mode()
def measure_silence(audio, lengths=None, sample_rate: int = 24000, effective_db: float = -60.0, absolute_db: float = -90.0,
                    check: bool = True) -> Dict[str, torch.Tensor]:
    """Leading and trailing silence of every clip by RMS in 10 ms windows, at two thresholds, and the content bounds at the
    effective one.  Returns device tensors: ``samples`` (int64 [B, 6], columns ``COLUMNS``), ``seconds`` (float64 [B, 6] =
    samples / sample_rate) and each column by name (int64 [B], samples).  The numbers are the reference's, quirks included (a
    trailing run counts the zero-padded last window; include/mtts.h).  A length outside ``[0, L]`` gives -1 in that row; with
    ``check`` the call waits for that verdict and raises ``ValueError`` naming the row."""
    wave, d_len = _batch(audio, lengths)
    out, ws = _measure(wave, d_len, sample_rate, effective_db, absolute_db)
    if check:
        _status(_hip.load().mtts_silence_status, ws)
    res = {"samples": out, "seconds": _seconds(out, sample_rate)}
    for k, name in enumerate(COLUMNS):
        res[name] = out[:, k]
    return res


@torch.inference_mode()
def measure_loudness(audio, lengths=None, sample_rate: int = 24000, check: bool = True) -> Dict[str, torch.Tensor]:
    """Integrated loudness (ITU-R BS.1770 K-weighting and gates, ``loudness.measure``) and sample peak of every clip: what spots a
    recording that is far too quiet or too hot before it is trained on.  ``audio`` / ``lengths`` as for ``measure_silence``; any
    ``sample_rate`` that is a multiple of 100 in [8000, 192000].  Returns device tensors ``{"lufs": float64 [B], "peak": float32
    [B]}`` and, beside them, what else ``loudness.meter`` reads: ``"true_peak"`` (float32, linear: a clip recorded too hot shows here
    before it shows in the sample peak), ``"lra"``, ``"momentary_max"`` and ``"short_term_max"`` (float64; a clip under 3 s has range 0
    and a short-term maximum of -inf); -inf marks a clip with no block above the absolute gate of -70 LUFS.  Nothing is changed: the recordings keep their
    level, since the mel statistics are computed without a level change.  A length outside ``[0, L]`` gives NaN in that row; with
    ``check`` the call waits for that verdict and raises ``ValueError`` naming the row."""
    from . import loudness as LD
    wave, d_len = _batch(audio, lengths)
    m = LD._run(wave, d_len, sample_rate, None, LD.PEAK_CEILING, False, check, None, True)[3]
    return {k: m[k] for k in ("lufs", "peak", "true_peak", "lra", "momentary_max", "short_term_max")}


@torch.inference_mode()
def measure_pitch(audio, lengths=None, sample_rate: int = 24000, **params) -> Dict[str, torch.Tensor]:
    """How high every clip speaks and whether it rises at the end: ``pitch.track`` and ``pitch.stats`` in one call -- steps 1-2 of the
    reference's documentation/pitch_raise_transfer.md (which speakers raise a question, which stay flat).  ``audio`` / ``lengths`` as
    for ``measure_silence``; a list may also hold ``audio_codec.Encoded`` / ``audio_codec.FlacClip`` recordings, which go through the
    recording entries' reader (``inference.recordings``: decoded on the device, converted to 24 kHz, and measured at 24 kHz).
    ``params``: ``hop``, ``fmin``, ``fmax``, ``threshold``, ``check`` of ``pitch.track`` and ``tail`` of ``pitch.stats``;
    ``method="viterbi"`` (with ``jump``, ``switch``) tracks with ``pitch.track_viterbi`` instead, the default ``"yin"`` makes exactly
    the calls it always made.  Returns the device tensors of ``pitch.stats`` (``median_hz``, ``p05_hz``, ``p95_hz``,
    ``tail_median_hz``, ``voiced_fraction``, ``range_st``, ``final_rise_st``, the counts) and the contour itself (``f0``,
    ``aperiodicity``, ``hop``, ``window``, ``max_lag``)."""
    from . import audio_codec as AC
    from . import pitch as P
    tail = {k: params.pop(k) for k in ("tail",) if k in params}
    track = P.METHODS.get(params.pop("method", "yin"))
    if track is None:
        raise ValueError(f"method must be one of {sorted(P.METHODS)}")
    if not (torch.is_tensor(audio) or isinstance(audio, np.ndarray)) and any(isinstance(c, (AC.Encoded, AC.FlacClip)) for c in audio):
        from .inference import SAMPLE_RATE, recordings
        audio = list(audio)
        dev = next((c.device for c in audio if torch.is_tensor(c) and c.is_cuda), torch.device("cuda"))
        audio, lengths = recordings(audio, dev, sample_rate, lengths)
        sample_rate = SAMPLE_RATE
    got = track(audio, lengths, sample_rate, **params)
    res = P.stats(got["f0"], got["frames"], got["hop"], sample_rate, **tail)
    return {**res, **{k: got[k] for k in ("f0", "aperiodicity", "hop", "window", "max_lag")}}


@torch.inference_mode()
def normalize_silence(audio, lengths=None, leading: Optional[float] = None, trailing: Optional[float] = None, threshold_db: float = -60.0,
                      sample_rate: int = 24000, check: bool = True) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
    """Every clip rebuilt with exactly ``leading`` / ``trailing`` seconds of zeros around its content (None leaves that end as
    it is): ``(audio_out [B, ld_out], out_lengths int64 [B], info)`` on the device, row b holding ``out_lengths[b]`` samples and
    zeros beyond.  Content samples are moved, bit for bit.  ``info``: ``changed`` (bool [B]; False = the row is a copy, every
    end being normalised already had its target count), ``bounds`` (the measured int64 [B, 6]), ``current_leading`` /
    ``current_trailing`` (float64 seconds) and ``leading_delta`` / ``trailing_delta`` (seconds; positive = silence added,
    negative = trimmed, 0 for an end that is not normalised or a clip that did not change) -- the reference's return values.
    Targets must be whole multiples of 10 ms (``ValueError``).  Nothing is read on the host unless ``check`` (the lengths'
    verdict)."""
    lib = _hip.load()
    sr = int(sample_rate)
    lead, trail = target_samples(leading, sr, "leading"), target_samples(trailing, sr, "trailing")
    wave, d_len = _batch(audio, lengths)
    B, ld = wave.shape
    bounds, ws = _measure(wave, d_len, sr, threshold_db, threshold_db)
    ld_out = (ld + max(lead, 0) + max(trail, 0) + 3) // 4 * 4          # no row can become longer than this
    out = torch.empty(B, ld_out, dtype=torch.float32, device=wave.device)
    out_len = torch.empty(B, dtype=torch.long, device=wave.device)
    changed = torch.empty(B, dtype=torch.int32, device=wave.device)
    with torch.cuda.device(wave.device):
        _hip.check(lib.mtts_silence_normalize(_hip.ptr(wave), ld, _hip.ptr(d_len), _hip.ptr(bounds), B, sr, lead, trail, _hip.ptr(out), ld_out,
                                              _hip.ptr(out_len), _hip.ptr(changed), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _status(lib.mtts_silence_status, ws)
    did = changed != 0
    cur_lead, cur_trail = bounds[:, 0], d_len - bounds[:, 1]
    zero = torch.zeros(B, dtype=torch.float64, device=wave.device)
    info = {"changed": did, "bounds": bounds, "current_leading": _seconds(cur_lead, sr), "current_trailing": _seconds(cur_trail, sr),
            "leading_delta": zero if lead < 0 else torch.where(did, _seconds(lead - cur_lead, sr), zero),
            "trailing_delta": zero if trail < 0 else torch.where(did, _seconds(trail - cur_trail, sr), zero)}
    return out, out_len, info


@torch.inference_mode()
def mel_sums(mel: torch.Tensor, mel_lengths=None, check: bool = True) -> Dict[str, torch.Tensor]:
    """``mtts_mel_stats`` of a ragged mel [B, F, T] on the device: ``sum`` and ``sum_sq`` (float64 [B], over f < F and
    t < len_b, in the documented fixed order), ``frames`` (int64 [B]) and ``nonfinite`` (bool [B]: a NaN or Inf among those
    values).  Frames at or beyond ``len_b`` are not read."""
    lib = _hip.load()
    if mel.dim() != 3:
        raise ValueError("mel must be [B, F, T]")
    if not mel.is_cuda:
        raise RuntimeError("matcha-tts-24k_amd: mel is not on a HIP device; there is no CPU path")
    mel = mel.detach().to(torch.float32).contiguous()
    B, F, T = mel.shape
    if B < 1 or F < 1 or T < 1:
        raise ValueError("mel must have at least one clip, one band and one frame")
    d_len = _hip.row_lengths(mel_lengths, B, T, mel.device, "mel_lengths")
    sums = torch.empty(B, 2, dtype=torch.float64, device=mel.device)
    frames = torch.empty(B, dtype=torch.long, device=mel.device)
    flags = torch.empty(B, dtype=torch.int32, device=mel.device)
    ws = _ws.get("mel_stats", lib.mtts_mel_stats_workspace_bytes(B, T), mel.device)
    with torch.cuda.device(mel.device):
        _hip.check(lib.mtts_mel_stats(_hip.ptr(mel), F, T, _hip.ptr(d_len), B, _hip.ptr(sums), _hip.ptr(frames), _hip.ptr(flags),
                                      ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _status(lib.mtts_mel_stats_status, ws)
    return {"sum": sums[:, 0], "sum_sq": sums[:, 1], "frames": frames, "nonfinite": flags != 0}


def _host_lengths(lengths: torch.Tensor) -> List[int]:
    return [int(v) for v in lengths.tolist()]


class MelStatistics:
    """``mel_mean`` / ``mel_std`` of a corpus -- reference generate_data_statistics.py:60-154 -- accumulated over ``update``
    calls: per-clip fp64 sums from the device, added up on the host in fp64 in call order, clips with a NaN or Inf left out and
    listed in ``failures`` as (index of the clip over all calls, message)."""

    def __init__(self, n_mels: int = 100, hop: int = 256, sample_rate: int = 24000, n_fft: int = 1024):
        self.n_mels, self.hop, self.sample_rate, self.n_fft = int(n_mels), int(hop), int(sample_rate), int(n_fft)
        self.total_sum = 0.0
        self.total_sq_sum = 0.0
        self.total_frames = 0
        self.ok = 0
        self.seen = 0
        self.failures: List[Tuple[int, str]] = []

    def update(self, audio, lengths=None) -> Dict[str, torch.Tensor]:
        """Clips -> the front end's un-normalised log-mel at ``hop`` (``mel_mean = 0, mel_std = 1``) -> ``update_mel``."""
        from . import mel as M
        wave, d_len = _batch(audio, lengths)
        mel, mel_len = M.extract(wave, _host_lengths(d_len), self.hop, 0.0, 1.0, sample_rate=self.sample_rate, n_fft=self.n_fft, n_mels=self.n_mels)
        return self.update_mel(mel, mel_len)

    def update_mel(self, mel: torch.Tensor, mel_lengths=None) -> Dict[str, torch.Tensor]:
        """An un-normalised mel [B, n_mels, T] with its lengths.  Returns this call's per-clip sums (``mel_sums``)."""
        if mel.dim() != 3 or mel.shape[1] != self.n_mels:
            raise ValueError(f"mel must be [B, {self.n_mels}, T], got {tuple(mel.shape)}")
        res = mel_sums(mel, mel_lengths)
        s, q = res["sum"].cpu().numpy(), res["sum_sq"].cpu().numpy()
        n, bad = res["frames"].cpu().numpy(), res["nonfinite"].cpu().numpy()
        for b in range(len(n)):
            if bad[b]:
                self.failures.append((self.seen + b, "the mel holds a NaN or an Inf"))
                continue
            self.total_sum += float(s[b])                  # reference :128-130
            self.total_sq_sum += float(q[b])
            self.total_frames += int(n[b])
            self.ok += 1
        self.seen += len(n)
        return res

    def raw(self) -> Tuple[float, float]:
        """(mean, std) before rounding: reference :151-152 in fp64."""
        if self.ok == 0 or self.total_frames == 0:
            raise RuntimeError("no clip was accumulated")
        count = self.total_frames * self.n_mels
        mean = self.total_sum / count
        return float(mean), float(np.sqrt((self.total_sq_sum / count) - (mean ** 2)))

    def result(self) -> Dict[str, float]:
        mean, std = self.raw()
        return {"mel_mean": round(mean, 6), "mel_std": round(std, 6)}


@torch.inference_mode()
def precompute_mels(audio, lengths=None, mel_mean: float = 0.0, mel_std: float = 1.0, hop: int = 256, sample_rate: int = 24000,
                    n_fft: int = 1024, n_mels: int = 100) -> Dict[str, torch.Tensor]:
    """The mel cache of a batch -- reference precompute_mels.py:100-116: ``mel`` [B, n_mels, T] at ``hop`` and ``mel_fine``
    [B, n_mels, Tf] at ``hop // 2``, both ``(log_mel - mel_mean) / mel_std``, with ``mel_lengths`` / ``mel_fine_lengths`` and
    ``ok`` (bool [B]: neither mel of the clip holds a NaN or Inf; the reference writes no file otherwise)."""
    from . import mel as M
    wave, d_len = _batch(audio, lengths)
    host = _host_lengths(d_len)
    kw = dict(sample_rate=int(sample_rate), n_fft=int(n_fft), n_mels=int(n_mels))
    mel, mel_len = M.extract(wave, host, int(hop), float(mel_mean), float(mel_std), **kw)
    fine, fine_len = M.extract(wave, host, int(hop) // 2, float(mel_mean), float(mel_std), **kw)
    ok = ~(mel_sums(mel, mel_len, check=False)["nonfinite"] | mel_sums(fine, fine_len, check=False)["nonfinite"])
    return {"mel": mel, "mel_lengths": mel_len, "mel_fine": fine, "mel_fine_lengths": fine_len, "ok": ok}

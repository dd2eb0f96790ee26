"""Sample-rate conversion of a ragged batch on MI355X (``mtts_resample_forward``): what the reference does with
``torchaudio.functional.resample`` (matcha/utils/utmos_validate.py:78) for recordings on the way in, and what a telephony or
browser client needs on the way out.

The algorithm is torchaudio's documented default -- windowed-sinc polyphase interpolation, ``sinc_interp_hann``,
``lowpass_filter_width=6``, ``rolloff=0.99`` -- restated from its formulae (include/mtts.h "sample-rate conversion", DESIGN.md
section 4); torchaudio is not a dependency and there is no CPU path.  Every output sample is one fixed-order fp32 sum: a clip's
samples do not depend on the batch it is in.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch

from . import _hip


def __getattr__(name):
    if name == "TILE":                          # output samples per workgroup of the kernel as built (MTTS_RESAMPLE_TILE)
        return int(_hip.load().mtts_resample_tile())
    raise AttributeError(name)


class Resampler:
    """One ``mtts_resampler``: the polyphase bank of a rate pair (built on the host at creation) and, after the first call, its
    banded copy on that call's device.  Use one object per device (``resample`` keeps them)."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.lib = _hip.load()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.ctx = self.lib.mtts_resampler_create(self.orig_freq, self.new_freq, int(lowpass_filter_width), float(rolloff))
        if not self.ctx:
            raise ValueError("mtts_resampler_create: " + self.lib.mtts_last_error().decode("utf-8", "replace"))
        v = [C.c_int(0) for _ in range(5)]
        _hip.check(self.lib.mtts_resample_factors(self.ctx, *[C.byref(x) for x in v]))
        self.o, self.n, self.width, self.taps, self.band = (int(x.value) for x in v)
        self._ws = _hip.Workspaces()

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.mtts_resampler_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    def out_length(self, L: int) -> int:
        """Samples a clip of ``L`` samples becomes: ``ceil(new_freq * L / orig_freq)`` in integer arithmetic."""
        m = self.lib.mtts_resample_out_length(self.ctx, int(L))
        if m < 0:
            raise ValueError("mtts: " + self.lib.mtts_last_error().decode("utf-8", "replace"))
        return int(m)

    def bank(self) -> np.ndarray:
        """The dense fp32 table K [n, taps] (the definition of the filter)."""
        out = np.empty((self.n, self.taps), dtype=np.float32)
        _hip.check(self.lib.mtts_resample_bank(self.ctx, out.ctypes.data, out.size))
        return out

    @torch.inference_mode()
    def __call__(self, audio: torch.Tensor, lengths=None, check: bool = True, ld_out: int = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """audio [B, L] (or [L]) float32 on the device + lengths [B] (samples; tensor or sequence, default all L) ->
        ``(out [B, L_out], out_lengths int64 [B])`` on the device: row b holds ``out_length(len_b)`` samples, then zeros.
        ``L_out`` is ``ld_out`` or ``out_length(L)``, rounded up to a multiple of 4.  Nothing is read on the host: a length outside
        ``[0, L]`` (or with more than ``L_out`` outputs) gives a zero row and ``out_lengths[b] = -1`` on the device; with ``check``
        the call waits for that verdict and raises ``ValueError`` naming the row, ``check=False`` leaves it to the caller
        (``status``)."""
        audio, L = _hip.aligned_rows(audio, 4, "audio")
        B, ld_in = audio.shape
        lengths = _hip.row_lengths(lengths, B, L, audio.device)
        ld_out = max(4, ((self.out_length(L) if ld_out is None else int(ld_out)) + 3) // 4 * 4)
        out = torch.empty(B, ld_out, dtype=torch.float32, device=audio.device)
        out_lengths = torch.empty(B, dtype=torch.long, device=audio.device)
        ws = self._ws.get("resample", self.lib.mtts_resample_workspace_bytes(self.ctx, B, ld_in), audio.device)
        with torch.cuda.device(audio.device):
            _hip.check(self.lib.mtts_resample_forward(self.ctx, _hip.ptr(audio), ld_in, _hip.ptr(lengths), B, _hip.ptr(out), ld_out,
                                                      _hip.ptr(out_lengths), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        if check:
            self.status()
        return out, out_lengths

    def status(self) -> None:
        """Wait for this stream's latest call and raise ``ValueError`` naming the first row the device refused."""
        ws = self._ws.latest("resample")
        if ws is not None:
            _hip.raise_refused(self.lib.mtts_resample_status, ws.data_ptr(), _hip.stream_ptr())


_resamplers: Dict[Tuple[int, int, str], Resampler] = {}


def resampler(orig_freq: int, new_freq: int, device) -> Resampler:
    """The process-wide resampler of a (rate pair, device): its bank is built once."""
    key = (int(orig_freq), int(new_freq), str(torch.device(device)))
    if key not in _resamplers:
        _resamplers[key] = Resampler(int(orig_freq), int(new_freq))
    return _resamplers[key]


def cached() -> int:
    """How many resamplers the process holds: 0 as long as every rate has been 24 kHz (nothing was converted)."""
    return len(_resamplers)


def clear_cache() -> None:
    _resamplers.clear()


def resample(audio: torch.Tensor, lengths, orig_freq: int, new_freq: int, check: bool = True, ld_out: int = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``Resampler(orig_freq, new_freq)(audio, lengths)`` with the cached object of that pair on ``audio``'s device."""
    if int(orig_freq) == int(new_freq):
        raise ValueError("resample: the two rates are equal (nothing to convert)")
    return resampler(orig_freq, new_freq, audio.device)(audio, lengths, check=check, ld_out=ld_out)


def rates_per_row(sample_rate, B: int, what: str = "sample_rate"):
    """``sample_rate`` as a list of B ints: an int for all rows, or one per row."""
    if isinstance(sample_rate, (int, np.integer)):
        return [int(sample_rate)] * B
    if torch.is_tensor(sample_rate):
        sample_rate = sample_rate.reshape(-1).tolist()
    rates = [int(v) for v in sample_rate]
    if len(rates) != B:
        raise ValueError(f"{what} is an int or one int per row ({B}), got {len(rates)}")
    return rates

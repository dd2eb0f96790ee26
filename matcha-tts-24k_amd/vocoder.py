"""Vocos-24k head on MI355X: drop-in for the reference's ``matcha.vocos24k.vocos_wrapper`` (VocosWrapper / load_model,
reference matcha/vocos24k/vocos_wrapper.py:3-16) and for ``vocos.Vocos.decode``.

The reference fetches pretrained weights by name from the HF hub (``charactr/vocos-mel-24khz``); there is no network
here, so ``load_model`` reads a local state dict (``VOCOS_CHECKPOINT`` or an explicit path) in the vocos package's
key layout.  Arithmetic runs in libmtts_hip.so (``mtts_vocos_decode``, ``mtts_vocos_decode_ragged``); there is no CPU path.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _hip
from .modules import ParamTree
from .synthetic import vocos_spec

# reference matcha/vocos24k/config.yaml:10-24
DEFAULT_CFG = dict(n_mels=100, dim=512, inter=1536, layers=8, n_fft=1024, hop=256)


class Vocos(_hip.DeviceComponent, ParamTree):
    """Parameter holder under the vocos state-dict names + ``decode(mel, lengths=None)``."""
    _abi, _what = "mtts_vocos", "vocoder"

    def __init__(self, **cfg):
        super().__init__()
        self.cfg = {**DEFAULT_CFG, **cfg}
        c = self.cfg
        for key, shape, kind in vocos_spec(n_mels=c["n_mels"], dim=c["dim"], inter=c["inter"], layers=c["layers"], n_fft=c["n_fft"]):
            self.attach(key, shape, kind)
        self._init_component()

    def _create_args(self):
        c = self.cfg
        return c["n_mels"], c["dim"], c["inter"], c["layers"], c["n_fft"], c["hop"]

    def _tensors(self):
        tensors = dict(self.state_dict())
        tensors["aux.window"] = torch.hann_window(self.cfg["n_fft"], dtype=torch.float32)   # as torch.istft's caller passes it
        return tensors

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # the published checkpoint also carries feature-extractor buffers and the iSTFT window; only the decoder is used
        sd = {k: v for k, v in state_dict.items() if k.startswith(("backbone.", "head.out."))}
        return super().load_state_dict(sd, strict=strict, assign=assign)

    @torch.inference_mode()
    def decode(self, mel: torch.Tensor, lengths=None, check: bool = True) -> torch.Tensor:
        """mel [B, n_mels, T] (or [n_mels, T]) -> audio [B, hop*(T-1)].

        ``lengths`` ([B] frames, tensor or sequence): a ragged batch.  Row b is what ``decode(mel[b:b+1, :, :len_b])`` gives
        (to rounding), followed by zeros; the padded part of ``mel`` is not read as data.  Without it every row is decoded
        over all T frames, which changes the last ~27 frames of an utterance shorter than T (seven-tap convolutions, nine deep).
        A length outside [1, T] raises, naming the row; the lengths are checked on the device after the decode has been
        enqueued, and ``check=False`` leaves that wait to the caller (``inference.to_waveforms`` reads the verdict with its
        one copy)."""
        lib = self._ready()
        if mel.dim() == 2:
            mel = mel[None]
        if not mel.is_cuda:
            raise RuntimeError("matcha-tts-24k_amd: mel is not on a HIP device; there is no CPU path")
        mel = mel.detach().to(torch.float32).contiguous()
        B, _, T = mel.shape
        audio = torch.empty(B, self.cfg["hop"] * (T - 1), dtype=torch.float32, device=mel.device)
        if lengths is None:
            ws = self._ws.get("decode", lib.mtts_vocos_workspace_bytes(self._ctx, B, T), mel.device)
            _hip.check(lib.mtts_vocos_decode(self._ctx, _hip.ptr(mel), B, T, _hip.ptr(audio), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
            return audio
        lengths = _hip.row_lengths(lengths, B, T, mel.device)
        ws = self._ws.get("decode", lib.mtts_vocos_ragged_workspace_bytes(self._ctx, B, T), mel.device)
        _hip.check(lib.mtts_vocos_decode_ragged(self._ctx, _hip.ptr(mel), _hip.ptr(lengths), B, T, _hip.ptr(audio), ws.data_ptr(),
                                                ws.numel(), _hip.stream_ptr()))
        if check:
            _hip.raise_refused(lib.mtts_vocos_ragged_status, ws.data_ptr(), _hip.stream_ptr(), prefix="mtts: ")
        return audio


class VocosWrapper(nn.Module):
    """reference matcha/vocos24k/vocos_wrapper.py:3-9"""

    def __init__(self, model: Vocos):
        super().__init__()
        self.model = model

    def forward(self, mel, lengths=None):
        """``lengths`` ([B] frames): ragged batch, see ``Vocos.decode``."""
        if lengths is None:
            return self.model.decode(mel)
        return self.model.decode(mel, lengths)


def load_model(device="cuda", checkpoint: Optional[str] = None, state_dict: Optional[Dict[str, torch.Tensor]] = None):
    """reference matcha/vocos24k/vocos_wrapper.py:11-16, from a local file instead of the HF hub."""
    model = Vocos()
    if state_dict is None:
        path = checkpoint or os.environ.get("VOCOS_CHECKPOINT")
        if not path:
            raise RuntimeError("no network: point VOCOS_CHECKPOINT at a local charactr/vocos-mel-24khz state dict "
                               "(pytorch_model.bin) or pass state_dict=")
        state_dict = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(state_dict, strict=True)
    return VocosWrapper(model.to(device).eval())

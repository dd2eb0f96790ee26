"""Style encoder on MI355X: the forward pass of the reference's ``StyleEncoder`` (reference matcha/models/style_encoder.py:42-72)
and the clip average of its enrolment tool (reference matcha/add_speaker.py:40-62).

The module holds the parameters under the reference's names (``convs.N.weight/bias``, ``proj_enc.*``, ``proj_dur.*``) and
``forward`` calls libmtts_hip.so (``mtts_style_forward``); there is no PyTorch arithmetic and no CPU path.  Training it
(``StyleEncoderLightningModule``) stays with the reference.  Its author reports that voices predicted this way keep the timbre
but can carry an odd accent and mispronunciations (style_encoder.py:17-19): this is parity with that tool, not a quality claim.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _hip

# reference configs/model/style_encoder/default.yaml
DEFAULT_CFG = dict(n_feats=100, hidden_channels=256, n_layers=4, spk_emb_dim=96)
STYLE_WEIGHTS = "style_encoder.safetensors"
STYLE_HPARAMS = "style_encoder.json"
STYLE_FORMAT_VERSION = 1
FINE_HOP = 128          # hop of the "fine" mel the style encoder is trained on (reference precompute_mels.py:100-113)


class StyleEncoder(_hip.DeviceComponent, nn.Module):
    """``forward(mel, mel_mask_or_lengths) -> (e_enc, e_dur)`` -- reference style_encoder.py:60-72."""
    _abi, _what = "mtts_style", "style encoder"

    def __init__(self, n_feats: int = 100, hidden_channels: int = 256, n_layers: int = 4, spk_emb_dim: int = 96):
        super().__init__()
        self.cfg = dict(n_feats=int(n_feats), hidden_channels=int(hidden_channels), n_layers=int(n_layers), spk_emb_dim=int(spk_emb_dim))
        self.convs = nn.ModuleList()
        in_ch = n_feats
        for _ in range(n_layers):
            self.convs.append(nn.Conv1d(in_ch, hidden_channels, kernel_size=5, padding=2))     # parameter holders only
            in_ch = hidden_channels
        self.proj_enc = nn.Linear(hidden_channels, spk_emb_dim)
        self.proj_dur = nn.Linear(hidden_channels, spk_emb_dim)
        for p in self.parameters():
            p.requires_grad_(False)
        self._init_component()

    def _create_args(self):
        c = self.cfg
        return c["n_feats"], c["hidden_channels"], c["n_layers"], c["spk_emb_dim"]

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # a StyleEncoderLightningModule checkpoint prefixes these with "style_encoder." and also carries the frozen Matcha model
        if any(k.startswith("style_encoder.") for k in state_dict):
            state_dict = {k[len("style_encoder."):]: v for k, v in state_dict.items() if k.startswith("style_encoder.")}
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    @torch.inference_mode()
    def forward(self, mel: torch.Tensor, mel_mask=None, lengths=None, group=None, n_groups: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """mel [B, n_feats, T] normalised fine mel; ``mel_mask`` [B, 1, T] prefix mask as the reference passes it, or ``lengths``
        [B] frames (neither: every row has T frames).  ``group`` [B] ints (clip -> voice) with ``n_groups``: the rows of each
        voice's clips are averaged (reference add_speaker.py:60-62) and [n_groups, spk_emb_dim] x 2 comes back."""
        lib = self._ready()
        if not mel.is_cuda:
            raise RuntimeError("matcha-tts-24k_amd: mel is not on a HIP device; there is no CPU path")
        mel = mel.detach().to(torch.float32).contiguous()
        B, C, T = mel.shape
        if C != self.cfg["n_feats"]:
            raise ValueError(f"mel has {C} channels, the style encoder expects {self.cfg['n_feats']}")
        if lengths is None and mel_mask is not None:
            lengths = mel_mask.reshape(B, -1).sum(-1)
        lengths = _hip.row_lengths(lengths, B, T, mel.device)
        d_group, n_out = None, B
        if group is not None:
            d_group = torch.as_tensor(group).to(device=mel.device, dtype=torch.int32).contiguous()
            if d_group.shape != (B,):
                raise ValueError(f"group must have shape ({B},), got {tuple(d_group.shape)}")
            n_out = int(n_groups) if n_groups is not None else int(d_group.max().item()) + 1
        E = self.cfg["spk_emb_dim"]
        e_enc = torch.empty(n_out, E, dtype=torch.float32, device=mel.device)
        e_dur = torch.empty(n_out, E, dtype=torch.float32, device=mel.device)
        ws = self._ws.get("forward", lib.mtts_style_workspace_bytes(self._ctx, B, T), mel.device)
        _hip.check(lib.mtts_style_forward(self._ctx, _hip.ptr(mel), _hip.ptr(lengths), B, T, _hip.ptr(d_group), n_out if d_group is not None else 0,
                                          _hip.ptr(e_enc), _hip.ptr(e_dur), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        return e_enc, e_dur


def style_cfg_from_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, int]:
    """The four sizes, read off the tensors' shapes (keys with or without the ``style_encoder.`` prefix)."""
    sd = {(k[len("style_encoder."):] if k.startswith("style_encoder.") else k): v for k, v in sd.items()}
    n_layers = 0
    while f"convs.{n_layers}.weight" in sd:
        n_layers += 1
    if n_layers == 0 or "proj_enc.weight" not in sd:
        raise KeyError("not a style-encoder state dict: no convs.0.weight / proj_enc.weight")
    w0 = sd["convs.0.weight"]
    return dict(n_feats=int(w0.shape[1]), hidden_channels=int(w0.shape[0]), n_layers=n_layers, spk_emb_dim=int(sd["proj_enc.weight"].shape[0]))


def select_style_tensors(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The style encoder's own tensors under their un-prefixed names, fp32 on the host."""
    cfg = style_cfg_from_state_dict(sd)
    pre = "style_encoder." if any(k.startswith("style_encoder.") for k in sd) else ""
    names = [f"convs.{i}.{p}" for i in range(cfg["n_layers"]) for p in ("weight", "bias")]
    names += [f"proj_{h}.{p}" for h in ("enc", "dur") for p in ("weight", "bias")]
    return {n: sd[pre + n].detach().to(torch.float32).contiguous().cpu() for n in names}


def is_converted_style(path) -> bool:
    p = Path(path)
    return p.is_dir() and (p / STYLE_WEIGHTS).exists() and (p / STYLE_HPARAMS).exists()


def load_style_encoder(path, device="cuda") -> StyleEncoder:
    """A directory written by ``checkpoint.convert_style_checkpoint`` (flat safetensors + JSON), or the Lightning ``.ckpt`` of a
    ``StyleEncoderLightningModule`` where it can be unpickled (its hyper-parameters name the sizes; the shapes confirm them)."""
    if is_converted_style(path):
        from safetensors.torch import load_file
        meta = json.loads((Path(path) / STYLE_HPARAMS).read_text())
        if meta.get("format_version") != STYLE_FORMAT_VERSION:
            raise ValueError(f"unsupported converted style-encoder version {meta.get('format_version')!r}")
        cfg, sd = meta["style_encoder"], load_file(str(Path(path) / STYLE_WEIGHTS), device="cpu")
    else:
        ckpt = torch.load(str(path), map_location="cpu", weights_only=False)
        sd = select_style_tensors(ckpt["state_dict"] if "state_dict" in ckpt else ckpt)
        cfg = style_cfg_from_state_dict(sd)
    model = StyleEncoder(**cfg)
    model.load_state_dict(sd, strict=True)
    return model.to(device).eval()

"""Style encoder on MI355X: the forward pass of the reference's ``StyleEncoder`` (reference matcha/models/style_encoder.py:42-72)
and the clip average of its enrolment tool (reference matcha/add_speaker.py:40-62).

The module holds the parameters under the reference's names (``convs.N.weight/bias``, ``proj_enc.*``, ``proj_dur.*``) and
``forward`` calls libmtts_hip.so (``mtts_style_forward``); there is no PyTorch arithmetic in it and no CPU path.  Training it
(the reference's ``StyleEncoderLightningModule``, style_encoder.py:75-160) runs on the device as well: ``forward_taped`` /
``backward`` give the gradient of every parameter (csrc/style_grad.hip), ``MatchaTTSInfer.style_match_grad`` the matching loss and
its gradient with respect to the predicted rows, and ``StyleTrainer`` the loop around them with ``torch.optim.AdamW`` on the flat
parameter buffer.  Its author reports that voices predicted this way keep the timbre but can carry an odd accent and
mispronunciations (style_encoder.py:17-19): this is parity with that tool, not a quality claim.
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

    # ------------------------------------------------------------------------------------------ parameter gradients
    def _mel_and_lengths(self, mel, lengths):
        if not mel.is_cuda:
            raise RuntimeError("matcha-tts-24k_amd: mel is not on a HIP device; there is no CPU path")
        mel = mel.detach().to(torch.float32).contiguous()
        B, C, T = mel.shape
        if C != self.cfg["n_feats"]:
            raise ValueError(f"mel has {C} channels, the style encoder expects {self.cfg['n_feats']}")
        return mel, _hip.row_lengths(lengths, B, T, mel.device)

    @torch.inference_mode()
    def forward_taped(self, mel: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``forward(mel, lengths=lengths)`` bit for bit (``mtts_style_forward_taped``), with every layer's activations kept on the
        device for one following ``backward``.  No clip average."""
        lib = self._ready()
        mel, lengths = self._mel_and_lengths(mel, lengths)
        B, _, T = mel.shape
        E = self.cfg["spk_emb_dim"]
        e_enc = torch.empty(B, E, dtype=torch.float32, device=mel.device)
        e_dur = torch.empty(B, E, dtype=torch.float32, device=mel.device)
        ws = self._ws.get("grad", lib.mtts_style_grad_workspace_bytes(self._ctx, B, T), mel.device)
        _hip.check(lib.mtts_style_forward_taped(self._ctx, _hip.ptr(mel), _hip.ptr(lengths), B, T, _hip.ptr(e_enc), _hip.ptr(e_dur),
                                                ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        object.__setattr__(self, "_tape", (B, T, lengths, ws, self._weights))
        return e_enc, e_dur

    def tape(self, which: int) -> torch.Tensor:
        """What the latest ``forward_taped`` kept: 0 the masked input rows [B*T, round_up(n_feats, 4)], 1 .. n_layers a layer's ReLU
        output [B*T, hidden], n_layers + 1 the pooled rows [B, hidden] (a copy)."""
        B, T, _, ws, _ = self._tape
        L, H = self.cfg["n_layers"], self.cfg["hidden_channels"]
        off = _hip.size(_hip.load().mtts_style_grad_tape_offset(self._ctx, B, T, which))
        shape = (B * T, (self.cfg["n_feats"] + 3) // 4 * 4) if which == 0 else (B * T, H) if which <= L else (B, H) if which == L + 1 else (B * T,)
        n = shape[0] * (shape[1] if len(shape) > 1 else 1)
        return ws[off:off + 4 * n].view(torch.float32).reshape(shape).clone()

    @torch.inference_mode()
    def backward(self, g_enc: torch.Tensor, g_dur: torch.Tensor) -> torch.Tensor:
        """Gradient of ``sum_b <g_enc_b, e_enc_b> + <g_dur_b, e_dur_b>`` of the latest ``forward_taped`` with respect to every
        parameter: one flat fp32 device tensor in state-dict order (``parameter_views`` names its parts)."""
        tape = getattr(self, "_tape", None)
        if tape is None or tape[4] is not self._weights or self._dirty:
            raise RuntimeError("StyleEncoder.backward needs a forward_taped call with the current parameters first")
        lib = self._ready()
        B, T, lengths, ws, _ = tape
        E = self.cfg["spk_emb_dim"]
        g = [t.detach().to(device=ws.device, dtype=torch.float32).contiguous() for t in (g_enc, g_dur)]
        if g[0].shape != (B, E) or g[1].shape != (B, E):
            raise ValueError(f"g_enc and g_dur must be [{B}, {E}]")
        held = getattr(self, "_grad_weights", None)
        if held is None or held[1] is not self._weights:           # packed from the tensors registered with that upload
            n = _hip.size(lib.mtts_style_grad_weights_bytes(self._ctx))
            buf = torch.empty(n, dtype=torch.uint8, device=ws.device)
            _hip.check(lib.mtts_style_grad_upload_weights(self._ctx, buf.data_ptr(), n))
            held = (buf, self._weights)
            object.__setattr__(self, "_grad_weights", held)
        out = torch.empty(_hip.size(lib.mtts_style_param_count(self._ctx)), dtype=torch.float32, device=ws.device)
        _hip.check(lib.mtts_style_backward(self._ctx, _hip.ptr(lengths), B, T, _hip.ptr(g[0]), _hip.ptr(g[1]), _hip.ptr(out),
                                           held[0].data_ptr(), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        return out

    def parameter_layout(self):
        """(name, offset, shape) of every parameter inside the flat buffer, in state-dict order (``mtts_style_param_offset``)."""
        lib = self._ready() if self._ctx is None else _hip.load()
        return [(k, _hip.size(lib.mtts_style_param_offset(self._ctx, k.encode())), tuple(v.shape)) for k, v in self.state_dict().items()]

    def parameter_views(self) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """The parameters as ONE flat fp32 device buffer plus named views into it in state-dict order.  The module's own parameters
        become those views, so an optimiser that updates the flat buffer updates the module; call ``mark_updated()`` afterwards."""
        lib = self._ready()
        p0 = next(self.parameters())
        flat = torch.empty(_hip.size(lib.mtts_style_param_count(self._ctx)), dtype=torch.float32, device=p0.device)
        views = {}
        params = dict(self.named_parameters())
        for k, off, shape in self.parameter_layout():
            n = 1
            for d in shape:
                n *= d
            view = flat[off:off + n].view(shape)
            view.copy_(params[k].detach())
            params[k].data = view
            views[k] = view
        return flat, views

    def mark_updated(self) -> None:
        """The parameters changed in place: the next call registers and uploads them again (forward image and backward panels)."""
        object.__setattr__(self, "_dirty", True)


STYLE_OPTIMIZER = "style_optimizer.pt"


class StyleTrainer:
    """Training of the style encoder on the device: the reference's ``StyleEncoderLightningModule`` (matcha/models/style_encoder.py:
    75-160) with the Matcha model frozen in ``eval()``, as a thin loop around three device calls.

    ``model`` is a loaded ``MatchaTTSInfer`` (frozen: only its text encoder runs), ``style_encoder`` the ``StyleEncoder`` to train,
    both on the device.  The optimiser is ``torch.optim.AdamW`` on ONE flat fp32 device buffer that holds every style parameter
    (``StyleEncoder.parameter_views``); the defaults are the reference's configs/model/optimizer/adamw.yaml and
    configs/train_style_encoder.yaml, and weight decay applies to every style parameter, as the reference's ungrouped
    ``self.parameters()`` does.  Out of scope: an optimiser kernel, Lightning / Hydra, bf16 training, resuming from a Lightning
    checkpoint's optimiser state, the clip average in the taped forward, and a device-side repack of the updated parameters -- after
    each step the parameters make one host round trip through the ``set_tensor`` / upload life cycle (forward image and backward
    panels)."""

    def __init__(self, model, style_encoder: StyleEncoder, lr: float = 1e-4, weight_decay: float = 1e-4, betas=(0.9, 0.99), eps: float = 1e-8,
                 beta_mu: float = 0.002, beta_logw: float = 0.004):
        self.model, self.style = model, style_encoder
        self.beta_mu, self.beta_logw = float(beta_mu), float(beta_logw)
        flat, self.views = style_encoder.parameter_views()
        self.flat = flat.requires_grad_(True)
        self.optimizer = torch.optim.AdamW([self.flat], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.steps = 0

    def step(self, x, x_lengths, mel_fine, mel_fine_lengths, spks) -> Dict[str, torch.Tensor]:
        """One training step on a batch: ``x`` [B, Tx] phoneme ids, ``x_lengths`` [B], ``mel_fine`` [B, n_feats, T] the normalised
        fine mels of the clips (``corpus.precompute_mels``), ``mel_fine_lengths`` [B], ``spks`` [B] speaker ids.  Taped style forward,
        the reference encoder forward and the matching loss with its gradient with respect to the predicted rows
        (``model.style_match_grad``), the style backward with the upstream gradients divided by the batch's token count, one AdamW
        step, and the updated parameters registered again.  Returns the reference's logged quantities (style_encoder.py:146-149) as
        0-dim device tensors, as they were BEFORE the update: ``acoustic_loss``, ``rhythm_loss``, ``emb_dist_enc``, ``emb_dist_dur``."""
        dev = self.flat.device
        x, x_lengths = x.to(dev), torch.as_tensor(x_lengths).to(device=dev, dtype=torch.long)
        p_enc, p_dur = self.style.forward_taped(mel_fine.to(dev), torch.as_tensor(mel_fine_lengths).to(dev))
        out = self.model.style_match_grad(x, x_lengths, (p_enc, p_dur), speaker=torch.as_tensor(spks).to(dev), beta_mu=self.beta_mu,
                                          beta_logw=self.beta_logw)
        tokens = x_lengths.to(torch.float32).sum()
        grads = self.style.backward(out["g_enc"] / tokens, out["g_dur"] / tokens)
        self.flat.grad = grads.clone()                      # (an ordinary tensor: the device call ran in inference mode)
        self.optimizer.step()
        self.style.mark_updated()
        self.steps += 1
        return {k: out[k] for k in ("acoustic_loss", "rhythm_loss", "emb_dist_enc", "emb_dist_dur")}

    def fit(self, batches, epochs: int = 1) -> Dict[str, list]:
        """``epochs`` passes over ``batches`` (a sequence of ``(x, x_lengths, mel_fine, mel_fine_lengths, spks)`` tuples or dicts with
        those keys) -> the per-step history of the four logged quantities as floats (read once, at the end)."""
        keys = ("x", "x_lengths", "mel_fine", "mel_fine_lengths", "spks")
        batches = list(batches)
        log = []
        for _ in range(int(epochs)):
            for b in batches:
                log.append(self.step(*([b[k] for k in keys] if isinstance(b, dict) else b)))
        names = ("acoustic_loss", "rhythm_loss", "emb_dist_enc", "emb_dist_dur")
        if not log:
            return {k: [] for k in names}
        table = torch.stack([torch.stack([r[k] for k in names]) for r in log]).cpu()
        return {k: [float(v) for v in table[:, i]] for i, k in enumerate(names)}

    def save(self, out_dir) -> Path:
        """The converted format ``load_style_encoder`` reads (``checkpoint.convert_style_checkpoint``'s two files) plus the optimiser
        state in ``style_optimizer.pt`` beside them."""
        from safetensors.torch import save_file
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        sd = {k: v.detach().to("cpu", torch.float32).clone().contiguous() for k, v in self.views.items()}
        save_file(sd, str(out / STYLE_WEIGHTS), metadata={"format": "matcha-tts-24k_amd-style", "version": str(STYLE_FORMAT_VERSION)})
        (out / STYLE_HPARAMS).write_text(json.dumps({"format_version": STYLE_FORMAT_VERSION, "style_encoder": self.style.cfg}, indent=1, sort_keys=True))
        torch.save({"optimizer": self.optimizer.state_dict(), "steps": self.steps}, str(out / STYLE_OPTIMIZER))
        return out


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

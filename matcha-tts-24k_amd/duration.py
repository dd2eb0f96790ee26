"""Training the duration predictor on the device (csrc/dp_grad.hip; include/mtts.h mtts_dp_grad).

In the reference ``logw = proj_w(x.detach(), x_mask, e_dur)`` (matcha/models/components/text_encoder.py:404) and the duration Huber loss
(matcha/models/matcha_tts.py:117,128) is the only loss that reaches ``encoder.proj_w.*``: training those tensors with everything else
frozen is the reference's own gradient for them.  ``MatchaTTSInfer.duration_grad`` gives that gradient for one batch; ``DurationTrainer``
is the loop around it: AdamW on one flat device buffer, a 2.5 MB host repack of the predictor per step, and ONE rebuild of the model's
weight image when training ends (``commit``).  (``dp.py`` is data parallelism; this module is the duration predictor.)"""
from pathlib import Path
from typing import Dict

import torch

DURATION_WEIGHTS = "duration_predictor.safetensors"
DURATION_OPTIMIZER = "duration_optimizer.pt"
PREFIX = "encoder.proj_w."


def is_decayed(key: str) -> bool:
    """The reference's ``configure_optimizers`` (matcha/models/baselightningmodule.py:29-59): every ``bias`` and every parameter of a
    LayerNorm (``gamma``, ``beta``) sits in the no-decay group, the other weights decay."""
    return key.rsplit(".", 1)[-1] not in ("bias", "gamma", "beta")


def load_tensors(path) -> Dict[str, torch.Tensor]:
    """The tensors ``DurationTrainer.save`` wrote, under their full state-dict keys."""
    from safetensors.torch import load_file
    return load_file(str(Path(path) / DURATION_WEIGHTS), device="cpu")


class DurationTrainer:
    """``model`` is a loaded ``MatchaTTSInfer`` on the device; only its duration predictor is trained, on a copy: the model itself
    does not change until ``commit()``.

    The optimiser is ``torch.optim.AdamW`` over views of ONE flat fp32 device buffer (``hip.dp_layout()``) in the reference's two
    groups; the defaults are the reference's configs/model/optimizer/adamw.yaml.  Out of scope: an optimiser kernel, a device-side
    repack, training the speaker rows in the same step (``step`` returns ``g_dur`` for callers who want to), dropout (this is the
    dropout-free gradient; the reference trains with ``p_dropout``), bf16 and Lightning."""

    def __init__(self, model, lr: float = 5e-5, weight_decay: float = 1e-4, betas=(0.9, 0.99), eps: float = 1e-8):
        self.model = model
        hip = model.hip
        flat, self.layout = hip.dp_params()
        self.flat = flat.to(hip.device)
        self.views = {}
        for key, off, shape in self.layout:
            n = 1
            for d in shape:
                n *= d
            self.views[key] = self.flat[off:off + n].view(shape).requires_grad_(True)
        decay = [v for k, v in self.views.items() if is_decayed(k)]
        no_decay = [v for k, v in self.views.items() if not is_decayed(k)]
        self.optimizer = torch.optim.AdamW([{"params": decay}, {"params": no_decay, "weight_decay": 0.0}], lr=lr, betas=tuple(betas),
                                           eps=eps, weight_decay=weight_decay)
        self.steps = 0
        self.last = None

    def step(self, x, x_lengths, durations, speaker=0, speaker_embeddings=None) -> torch.Tensor:
        """One training step: ``x`` [B, Tx] phoneme ids, ``x_lengths`` [B], ``durations`` int [B, Tx] (``model.align``'s), the voice as
        ``speaker`` id(s) or ``speaker_embeddings=(e_enc, e_dur)``.  The 2.5 MB component is repacked from the flat buffer, the device
        computes the gradient, AdamW takes one step.  Returns ``dur_loss`` as it was BEFORE the update (a 0-dim device tensor); the
        whole result of ``duration_grad`` stays in ``self.last``."""
        dev = self.flat.device
        out = self.model.duration_grad(x.to(dev), torch.as_tensor(x_lengths).to(dev), durations=torch.as_tensor(durations).to(dev),
                                       speaker=speaker, speaker_embeddings=speaker_embeddings, params=self.flat)
        grad = out["grad"].clone()                          # (an ordinary tensor: the device call ran in inference mode)
        for key, off, shape in self.layout:
            v = self.views[key]
            v.grad = grad[off:off + v.numel()].view(shape)
        self.optimizer.step()
        self.steps += 1
        self.last = out
        return out["dur_loss"]

    def fit(self, batches, epochs: int = 1) -> Dict[str, list]:
        """``epochs`` passes over ``batches`` (a sequence of ``(x, x_lengths, durations, speaker)`` tuples or dicts with the keys ``x``,
        ``x_lengths``, ``durations`` and ``speaker`` or ``speaker_embeddings``) -> ``{"dur_loss": [...]}``, one float per step (read
        once, at the end)."""
        batches = list(batches)
        log = []
        for _ in range(int(epochs)):
            for b in batches:
                if isinstance(b, dict):
                    log.append(self.step(b["x"], b["x_lengths"], b["durations"], speaker=b.get("speaker", 0),
                                         speaker_embeddings=b.get("speaker_embeddings")))
                else:
                    log.append(self.step(*b))
        return {"dur_loss": [float(v) for v in torch.stack(log).cpu()] if log else []}

    def tensors(self) -> Dict[str, torch.Tensor]:
        """The trained tensors under their full state-dict keys, fp32 on the host."""
        return {PREFIX + k: v.detach().to("cpu", torch.float32).clone().contiguous() for k, v in self.views.items()}

    @torch.no_grad()
    def commit(self) -> None:
        """Push the trained tensors into the model, once: its parameters are overwritten in place and its weight image is repacked and
        uploaded (``HipModel.update_tensors``).  After it ``synthesise``, ``score`` and ``speaker_grad`` see the new predictor."""
        tensors = self.tensors()
        rt = self.model._rt
        rt.ready()
        sd = self.model.state_dict()
        for k, t in tensors.items():
            sd[k].copy_(t.to(sd[k].device))
        for hip in (rt.hip, rt.wide):
            if hip is not None and hip.weights is not None:
                hip.update_tensors(tensors)

    def save(self, out_dir) -> Path:
        """The trained tensors as safetensors (full state-dict keys: merge them into a checkpoint's state dict, or ``load_tensors``)
        plus the optimiser state in ``duration_optimizer.pt`` beside them."""
        from safetensors.torch import save_file
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        save_file(self.tensors(), str(out / DURATION_WEIGHTS), metadata={"format": "matcha-tts-24k_amd-duration-predictor", "version": "1"})
        torch.save({"optimizer": self.optimizer.state_dict(), "steps": self.steps}, str(out / DURATION_OPTIMIZER))
        return out

"""Drop-in for the reference's ``matcha.inference`` module (reference matcha/inference.py) on MI355X.

Same public names and call signatures -- ``load_matcha``, ``load_vocoder``, ``pipeline``, ``process_text``,
``to_waveform``, ``MatchaTTSInfer.synthesise``, ``VOICES`` and the constants -- so that the reference's
``matcha/cli.py`` and ``matcha/server.py`` keep working when their import is pointed here.
The arithmetic of ``synthesise`` runs in libmtts_hip.so; there is no CPU path (only the ``debug=True`` extras and
the two-term voice mix use a few PyTorch elementwise ops on device tensors, as the reference does).

Extensions (backwards compatible): ``x`` may hold B > 1 utterances and ``speaker`` may be a LongTensor[B]
(the reference builds a batch-1 speaker embedding and fails for B > 1, inference.py:118-121); ``synthesise``
accepts ``z=`` (explicit noise) for parity checks against the CPU reference stream.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _hip
from .hparams import N_VOCAB, PathHParams, from_reference_kwargs
from .modules import PAIR_TIMEOUT_ERROR, Runtime, build_trees
# the waveform tail lives in waveform.py; its public names (and the 24 kHz constant, defined there) stay importable from here
from .waveform import (METER_FIGURES, SAMPLE_RATE, _waveform_on_device, document_csr, finish_request, finish_waveforms,  # noqa: F401
                       join_waveforms, to_waveforms, trim_trailing_silence)

# Voice table of the shipped model: id, language, per-speaker duration scale correction (reference inference.py:16-32).
VOICES = [
    {"id": str(i), "lang": lang, "gender": gender, "name": name, "scale_correction": sc}
    for i, (lang, gender, name, sc) in enumerate([
        ("en-us", "male", "Kai", 1.08), ("en-us", "female", "Jane", 1.05), ("en-us", "female", "Aria", 1.05),
        ("en-us", "female", "Bella", 1.03), ("en-gb", "male", "Brian", 1.08), ("en-gb", "male", "Arthur", 1.08),
        ("en-us", "female", "Nicole", 1.05), ("ro", "male", "Emil", 1.04), ("fr-fr", "female", "Denise", 1.05),
        ("fr-fr", "male", "Henri", 1.03), ("en-us", "male", "Matthew", 1.06), ("en-us", "male", "Lewis", 1.08),
        ("en-us", "male", "Michael", 1.03), ("it", "female", "Isabella", 1.07), ("it", "male", "Marcello", 1.07),
    ])
]

STD_RES_HOP_LENGTH = 256
HIGH_RES_HOP_LENGTH = 128
DEFAULT_ODE_SOLVER = "midpoint"
DEFAULT_NUM_STEPS = 4
DEVICE = torch.device("cuda")


def fix_len_compatibility(length: int, num_downsamplings_in_unet: int = 1) -> int:
    """ceil(length / 2^n) * 2^n (reference utils/model.py:15-21)."""
    f = 2 ** num_downsamplings_in_unet
    return int(math.ceil(int(length) / f) * f)


class MatchaTTSInfer(nn.Module):
    """Inference model: speaker tables + text encoder + CFM decoder (reference inference.py:44-183)."""

    def __init__(self, n_spks, n_feats, encoder, decoder, cfm, data_statistics, spk_emb_dim, prior_loss_threshold=None,
                 duration_loss_threshold=None, **_):
        super().__init__()
        hp = from_reference_kwargs(n_spks, n_feats, encoder, decoder, cfm, data_statistics, spk_emb_dim,
                                   prior_loss_threshold=prior_loss_threshold, duration_loss_threshold=duration_loss_threshold)
        self._init_from_hparams(hp)

    @classmethod
    def from_hparams(cls, hp: PathHParams) -> "MatchaTTSInfer":
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._init_from_hparams(hp)
        return self

    def _init_from_hparams(self, hp: PathHParams) -> None:
        object.__setattr__(self, "hp", hp)
        object.__setattr__(self, "_rt", Runtime(hp, self))
        build_trees(hp, self, self._rt)
        with torch.no_grad():
            self.mel_mean.fill_(hp.mel_mean)
            self.mel_std.fill_(hp.mel_std)

    # ---- parameter changes invalidate the packed device image
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = {k.replace("_orig_mod.", ""): v for k, v in state_dict.items() if "rope." not in k}
        out = super().load_state_dict(sd, strict=strict, assign=assign)
        self._rt.dirty = True
        return out

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._rt.dirty = True
        return r

    @property
    def hip(self):
        return self._rt.ready()

    # ---- reference inference.py:57-76
    def mix_speakers(self, speaker_mix):
        dev = next(self.parameters()).device
        mixed_enc = mixed_dur = None
        hip = self._rt.ready()
        for spk_id, weight in speaker_mix:
            ids = torch.tensor([spk_id], device=dev, dtype=torch.long)
            e_enc, e_dur = hip.speaker_embedding(0, ids), hip.speaker_embedding(1, ids)
            mixed_enc = weight * e_enc if mixed_enc is None else mixed_enc + weight * e_enc
            mixed_dur = weight * e_dur if mixed_dur is None else mixed_dur + weight * e_dur
        return mixed_enc, mixed_dur

    def _voice_rows(self, B, dev, speaker=0, voice_mix=None, speaker_embeddings=None):
        """The ``(e_enc, e_dur)`` rows of a call's speaker arguments: ``speaker_embeddings`` as given, else the ``voice_mix``, else the
        rows of the ``speaker`` id(s); one row for the batch or one per utterance."""
        if speaker_embeddings is not None:      # (e_enc, e_dur) [B, spk_emb_dim] each: a batch that mixes plain voices and voice mixes
            e_enc, e_dur = speaker_embeddings
        elif voice_mix is not None:
            e_enc, e_dur = self.mix_speakers(voice_mix)
        else:
            hip = self._rt.ready()
            ids = torch.as_tensor(speaker, dtype=torch.long, device=dev).reshape(-1)
            e_enc, e_dur = hip.speaker_embedding(0, ids), hip.speaker_embedding(1, ids)
        if e_enc.shape[0] not in (1, B):
            raise ValueError("speaker must be an int or a LongTensor with one id per utterance")
        return e_enc, e_dur

    #: what to do when the default arithmetic (fp16 two-term split) met an operand beyond +-65504 (include/mtts.h "range
    #: guard"): "rerun" the call on the full-range arithmetic (three bf16 terms), "raise", or "ignore" (no flag read, no sync).
    #: ``Runtime.guarded`` (modules.py) is the one guard of ``synthesise``, ``align``, ``score`` and ``speaker_grad``
    range_policy = "rerun"

    def synthesise(self, x, x_lengths, n_timesteps, speaker=0, voice_mix=None, scale_correction=1.0, length_scale=1.0,
                   debug=False, z=None, sync_max=None, per_request_padding=False, speaker_embeddings=None, durations=None, *,
                   token_scale=None, token_extend=None, return_timing=False):
        """``_synthesise`` under the range guard (``Runtime.guarded``): one read of the sticky device flags per call (a stream
        synchronisation)."""
        rt = self._rt

        def verdict(_):
            hip = rt.ready()
            flags = torch.cat([hip.range_flags(), hip.pair_timeouts()]).tolist()       # one read, one synchronisation
            return bool(flags[0] or flags[1]), bool(flags[2])

        def run():
            if token_scale is None and token_extend is None and not return_timing:
                return self._synthesise(x, x_lengths, n_timesteps, speaker, voice_mix, scale_correction, length_scale, debug, z, sync_max,
                                        per_request_padding, speaker_embeddings, durations)
            return self._synthesise(x, x_lengths, n_timesteps, speaker, voice_mix, scale_correction, length_scale, debug, z, sync_max,
                                    per_request_padding, speaker_embeddings, durations, token_scale=token_scale,
                                    token_extend=token_extend, return_timing=return_timing)
        return rt.guarded(self.range_policy, run, verdict, can_rerun=sync_max is None)      # (a rank-local rerun would repeat sync_max's collective)

    @torch.inference_mode()
    def speaker_rows(self, voices):
        """One (e_enc, e_dur) row per entry of ``voices``: an int speaker id, a voice mix ``[(id, weight), ...]`` combined as
        ``mix_speakers`` does (reference inference.py:57-76), or a pre-computed ``(e_enc, e_dur)`` pair of tensors (an enrolled
        voice, ``enroll_voice``).  Returns two [len(voices), spk_emb_dim] device tensors."""
        dev = next(self.parameters()).device
        hip = self._rt.ready()
        enc, dur = [], []
        for v in voices:
            if isinstance(v, (list, tuple)) and len(v) == 2 and torch.is_tensor(v[0]) and torch.is_tensor(v[1]):
                # a pre-computed (e_enc, e_dur) pair, e.g. one voice of ``enroll_voice``
                e, d = (t.detach().to(device=dev, dtype=torch.float32).reshape(1, -1) for t in v)
                if e.shape[1] != self.hp.spk_emb_dim or d.shape[1] != self.hp.spk_emb_dim:
                    raise ValueError(f"an enrolled voice is a pair of rows of {self.hp.spk_emb_dim} values")
            elif isinstance(v, (list, tuple)):
                e, d = self.mix_speakers(v)
            else:
                ids = torch.tensor([int(v)], device=dev, dtype=torch.long)
                e, d = hip.speaker_embedding(0, ids), hip.speaker_embedding(1, ids)
            enc.append(e)
            dur.append(d)
        return torch.cat(enc, 0), torch.cat(dur, 0)

    @torch.inference_mode()
    def speaker_delta(self, plus, minus):
        """The direction between two groups of voices -- ``(delta_enc, delta_dur)``, each [1, spk_emb_dim]: the mean of
        ``speaker_rows(plus)`` minus the mean of ``speaker_rows(minus)``, e.g. the speakers that raise a question against the ones that
        stay flat (``corpus.measure_pitch``'s ``final_rise_st`` tells them apart; the reference's
        documentation/pitch_raise_transfer.md).  With ``(e_enc, e_dur) = speaker_rows([voice])`` a voice is moved along it as

            synthesise(..., speaker_embeddings=(e_enc + alpha * delta_enc, e_dur + alpha * delta_dur))
        """
        if len(plus) == 0 or len(minus) == 0:
            raise ValueError("speaker_delta needs at least one voice on each side")
        (pe, pd), (me, md) = self.speaker_rows(plus), self.speaker_rows(minus)
        return pe.mean(0, keepdim=True) - me.mean(0, keepdim=True), pd.mean(0, keepdim=True) - md.mean(0, keepdim=True)

    @torch.inference_mode()
    def enroll_voice(self, clips, style_encoder, silence=None, sample_rate=24000):
        """Speaker rows from audio -- the reference's offline chain matcha/vocos24k/mel_extractor.py (audio -> log-mel),
        matcha/utils/precompute_mels.py:100-113 (normalise with this model's mel statistics, hop 128), StyleEncoder.forward and
        matcha/add_speaker.py:40-62 (average over the clips) -- as one front-end call and one encoder call on the device.

        ``clips``: a list of 1-D waveforms (host or device, mono in [-1, 1]; or ``audio_codec.Encoded`` clips, still PCM16 / G.711
        bytes, decoded on the device -- ``recordings``) of ONE voice -> ``(e_enc, e_dur)`` of shape
        [1, spk_emb_dim]; or a list of such lists for several voices -> [n_voices, spk_emb_dim].  The rows are what
        ``synthesise(speaker_embeddings=...)``, ``speaker_rows`` and ``add_speaker`` take.  ``sample_rate``: the clips' rate, an int
        or one int per clip (in the order of the flattened list); clips at another rate than 24 kHz are converted on the device
        first (``resample.resample``, one call per distinct rate).  ``silence``: None, or ``(leading_s, trailing_s)`` (either may be
        None) -- the clips' leading / trailing silence is normalised to exactly those durations on the device
        (``corpus.normalize_silence``, the reference's matcha/utils/normalize_silence.py) after the conversion to 24 kHz and before
        the mel front end."""
        from . import mel as M
        from .style import FINE_HOP
        if len(clips) == 0:
            raise ValueError("no clips")
        from .audio_codec import Encoded, FlacClip
        voices = [clips] if torch.is_tensor(clips[0]) or isinstance(clips[0], (np.ndarray, Encoded, FlacClip)) else list(clips)
        dev = next(self.parameters()).device
        self._rt.ready()                                   # mel statistics come from the loaded checkpoint's buffers
        flat, group = [], []
        for g, vc in enumerate(voices):
            if len(vc) == 0:
                raise ValueError(f"voice {g} has no clips")
            for c in vc:
                flat.append(c)
                group.append(g)
        audio, lengths = recordings(flat, dev, sample_rate, silence=silence)
        n_feats = style_encoder.cfg["n_feats"]
        if n_feats != self.hp.n_feats or style_encoder.cfg["spk_emb_dim"] != self.hp.spk_emb_dim:
            raise ValueError("the style encoder's n_feats / spk_emb_dim do not match this model")
        mel, mel_len = M.extract(audio, lengths, FINE_HOP, self._rt.mel_mean, self._rt.mel_std, sample_rate=24000, n_mels=n_feats)
        return style_encoder(mel, lengths=mel_len, group=group, n_groups=len(voices))

    def add_speaker(self, e_enc, e_dur) -> int:
        """Append a voice to both speaker tables (reference matcha/add_speaker.py:65-70) and return its id.  The table size is a
        create-time parameter of the device context, so the next call builds a new context and repacks the weights (one host
        packing pass); graphs captured on the old context are dropped.  For serving, passing the rows per request
        (``speaker_embeddings=`` / the batcher's ``speaker_embedding``) touches neither weights nor graphs."""
        import dataclasses
        E = self.hp.spk_emb_dim
        for name, row in (("speaker_embeddings_enc", e_enc), ("speaker_embeddings_dur", e_dur)):
            tree = getattr(self, name)
            w = tree.weight
            r = torch.as_tensor(row).detach().reshape(1, -1).to(device=w.device, dtype=w.dtype)
            if r.shape[1] != E:
                raise ValueError(f"{name}: a speaker row has {E} values, got {r.shape[1]}")
            tree.weight = nn.Parameter(torch.cat([w.detach(), r], 0), requires_grad=False)
        hp = dataclasses.replace(self.hp, n_spks=self.hp.n_spks + 1)
        object.__setattr__(self, "hp", hp)
        rt = self._rt
        rt.hp, rt.hip, rt.wide, rt.use_wide, rt.dirty = hp, None, None, False, True
        self.decoder._graphs.clear()
        return hp.n_spks - 1

    @staticmethod
    def _given_durations(hip, given, logw, x_mask, scale_correction, length_scale):
        """``hip.durations_given`` for ``synthesise(durations=...)``: a [B, Tx] tensor, or B rows of which some are None -- those
        get the predictor's durations first (one ``hip.durations`` call for the batch) and the given rows overwrite them on the
        device before the scan."""
        B, _, Tx = x_mask.shape
        dev = x_mask.device
        if torch.is_tensor(given):
            if given.dim() == 1:
                given = given[None]
            return hip.durations_given(given.to(dev), x_mask, length_scale)
        if len(given) != B:
            raise ValueError(f"durations need one row per utterance ({B}), got {len(given)}")
        host = torch.zeros(B, Tx, dtype=torch.float32)
        for b, row in enumerate(given):
            if row is None:
                continue
            row = torch.as_tensor(row).detach().to("cpu", torch.float32).reshape(-1)
            if row.numel() > Tx:
                raise ValueError(f"durations[{b}] has {row.numel()} values for {Tx} tokens")
            host[b, :row.numel()] = row
        rows = [row is not None for row in given]
        if all(rows):
            return hip.durations_given(host.to(dev), x_mask, length_scale)
        predicted, _, _ = hip.durations(logw, x_mask, scale_correction, length_scale)
        return hip.durations_given(host.to(dev), x_mask, length_scale, given_rows=rows, out=predicted)

    @staticmethod
    def _rows_or_tensor(v, B, Tx, dev, fill, name):
        """``token_scale`` / ``token_extend`` as a float32 [B, Tx] device tensor: a tensor as it is, or B rows (None, or up to Tx
        values) laid over ``fill``; None stays None."""
        if v is None:
            return None
        if torch.is_tensor(v):
            v = v[None] if v.dim() == 1 else v
            if v.shape != (B, Tx):
                raise ValueError(f"{name} must have shape ({B}, {Tx}), got {tuple(v.shape)}")
            return v.to(device=dev, dtype=torch.float32)
        if len(v) != B:
            raise ValueError(f"{name} needs one row per utterance ({B}), got {len(v)}")
        host = torch.full((B, Tx), float(fill), dtype=torch.float32)
        for b, row in enumerate(v):
            if row is None:
                continue
            row = torch.as_tensor(row).detach().to("cpu", torch.float32).reshape(-1)
            if row.numel() > Tx:
                raise ValueError(f"{name}[{b}] has {row.numel()} values for {Tx} tokens")
            host[b, :row.numel()] = row
        return host.to(dev)

    @classmethod
    def _shaped_durations(cls, hip, given, logw, x_mask, scale_correction, length_scale, token_scale, token_extend):
        """``hip.durations_shaped`` for ``synthesise(token_scale=, token_extend=)``: predicted rows, given rows (``durations=`` as
        ``_given_durations`` takes it) and the shaping of both in one launch."""
        B, _, Tx = x_mask.shape
        dev = x_mask.device
        s = cls._rows_or_tensor(token_scale, B, Tx, dev, 1.0, "token_scale")
        a = cls._rows_or_tensor(token_extend, B, Tx, dev, 0.0, "token_extend")
        rows = None
        if given is not None and not torch.is_tensor(given):
            if len(given) != B:
                raise ValueError(f"durations need one row per utterance ({B}), got {len(given)}")
            rows = [row is not None for row in given]
            given = cls._rows_or_tensor(given, B, Tx, dev, 0.0, "durations") if any(rows) else None
            rows = None if given is None or all(rows) else rows
        elif given is not None:
            given = (given[None] if given.dim() == 1 else given).to(dev)
        return hip.durations_shaped(logw, x_mask, scale_correction, length_scale, given=given, given_rows=rows, token_scale=s,
                                    token_extend=a)

    @torch.inference_mode()
    def align(self, x, x_lengths, audio=None, audio_lengths=None, mel_fine=None, mel_fine_lengths=None, speaker=0, voice_mix=None,
              speaker_embeddings=None, return_path=False, silence=None, sample_rate=24000):
        """Forced alignment of text to a recording: per-token durations in fine frames (hop 128) by Monotonic Alignment Search of
        the text encoder's ``mu_x`` against the recording's normalised fine mel -- the alignment of the reference's training
        forward (matcha/models/matcha_tts.py:184-201), here for inference-time use: ``synthesise(durations=...)`` re-times or
        re-voices with the speaker's own rhythm, and ``scale_correction`` is the number the reference's ``VOICES`` table holds per
        voice ("measured after training, by comparing generated speech to ground truth", reference inference.py:131-133).

        The recording: ``audio`` -- mono clips, a list of 1-D waveforms (host or device) or a [B, L] tensor with
        ``audio_lengths``, at ``sample_rate`` (an int or one int per clip; anything but 24 kHz is converted on the device first,
        ``resample.resample``; ``silence=(leading_s, trailing_s)`` normalises the clips' silence first, as for ``enroll_voice``) --
        whose fine mel is extracted as ``enroll_voice`` does; or ``mel_fine`` [B, n_feats, Tm], already
        normalised with this model's mel statistics, with ``mel_fine_lengths`` (default: all Tm).  Speaker arguments as for
        ``synthesise``.  Returns ``durations`` (int32 [B, Tx]), ``predicted_durations`` (the predictor's raw
        ``(exp(logw) - 2) * mask``), ``scale_correction`` ([B]: aligned total / predicted total), ``score`` ([B]: the path's
        log-prior sum), ``mel_fine_lengths`` and, with ``return_path``, ``path`` ([B, Tx, Tm] 0/1).  One synchronisation per call
        (the lengths' verdict and the range flag, under the guard of ``Runtime.guarded``); ``ValueError`` names an utterance with
        fewer frames than tokens."""
        rt = self._rt

        def run():
            hip = rt.ready()
            y, y_lengths = self._fine_recording(x, audio, audio_lengths, mel_fine, mel_fine_lengths, "align", sample_rate, silence)
            e_enc, e_dur = self._voice_rows(x.shape[0], x.device, speaker, voice_mix, speaker_embeddings)
            mu_x, logw, x_mask = self.encoder(x, x_lengths, e_enc, e_dur)
            durations, score, path = hip.mas(x_lengths, y_lengths, mu_x=mu_x, y=y, return_path=return_path)
            predicted = ((torch.exp(logw) - 2) * x_mask).squeeze(1)
            out = {"durations": durations, "predicted_durations": predicted,
                   "scale_correction": durations.sum(1).to(torch.float32) / predicted.sum(1), "score": score,
                   "mel_fine_lengths": y_lengths}
            if return_path:
                out["path"] = path
            return out
        # (no estimator call, so no time-out word; the stream is already drained: no second wait)
        return rt.guarded(self.range_policy, run, lambda _: (bool(rt.ready().range_flags()[0].item()), False))

    @torch.inference_mode()
    def prosody(self, x, x_lengths, audio=None, audio_lengths=None, speaker=0, voice_mix=None, speaker_embeddings=None, silence=None,
                sample_rate=24000, method="viterbi", **pitch_params):
        """Pitch and energy of every token of a recording, in one call: ``align`` (which fine frames belong to which token), then
        ``timing.token_marks`` (keep = the clip's length at 24 kHz, as tools/align.py --marks does), ``pitch.contour`` at the fine-mel
        hop and ``pitch.fold`` -- does this voice raise the ``?``, and does a moved voice raise it more (the reference's
        documentation/pitch_raise_transfer.md).  The recording, ``sample_rate``, ``silence`` and the speaker arguments as for
        ``align``; ``method`` and ``pitch_params`` (``fmin``, ``fmax``, ``threshold``, ``jump``, ``switch``) as for ``pitch.contour``.
        Returns the tensors of ``pitch.fold`` ([B, Tx]: ``frames``, ``voiced``, ``median_hz``, ``first_hz``, ``last_hz``,
        ``mean_square``, ``energy_db``) and ``marks`` (int64 [B, Tx, 2], samples at 24 kHz), ``durations``, ``scale_correction``, the
        contour ``f0`` with its ``pitch_frames``, ``hop``, ``window``, ``max_lag``, and the clips' ``audio_lengths``."""
        from . import pitch as P
        from . import timing as TM
        if audio is None:
            raise ValueError("prosody needs audio=")
        if "hop" in pitch_params:
            raise ValueError("prosody tracks at the fine-mel hop, so that pitch frames step with the alignment's frames")
        wave, lengths = recordings(self._clips(audio, x.shape[0], "prosody"), x.device, sample_rate, audio_lengths, silence)
        aligned = self.align(x, x_lengths, audio=wave, audio_lengths=lengths, speaker=speaker, voice_mix=voice_mix,
                             speaker_embeddings=speaker_embeddings)
        cum = torch.cumsum(aligned["durations"].to(torch.int32), 1).to(torch.int32)
        marks, kept, _ = TM.token_marks(cum, x_lengths, lengths)
        tracked = P.contour(wave, lengths, SAMPLE_RATE, method, hop=TM.FINE_HOP, **pitch_params)
        out = P.fold(tracked, marks, x_lengths, audio=wave, lengths=lengths)
        out.update(marks=marks, durations=aligned["durations"], scale_correction=aligned["scale_correction"], f0=tracked["f0"],
                   pitch_frames=tracked["frames"], hop=tracked["hop"], window=tracked["window"], max_lag=tracked["max_lag"],
                   audio_lengths=kept)
        return out

    @staticmethod
    def _clips(audio, B, who):
        """The ``audio`` argument of the recording entries as a list of ``B`` clips: a [B, L] tensor's rows, one 1-D waveform, or a list."""
        from .audio_codec import Encoded, FlacClip
        clips = [audio[b] for b in range(audio.shape[0])] if torch.is_tensor(audio) and audio.dim() == 2 else (
            [audio] if torch.is_tensor(audio) or isinstance(audio, (np.ndarray, Encoded, FlacClip)) else list(audio))
        if len(clips) != B:
            raise ValueError(f"{who} needs one clip per utterance ({B}), got {len(clips)}")
        return clips

    def _recorded_mels(self, x, audio, audio_lengths, who, sample_rate, silence, *hops):
        """The normalised mel of ``audio`` (one clip per row of ``x``) at each of ``hops``, extracted as ``enroll_voice`` does from
        one conversion to 24 kHz: ``([(mel, mel_lengths), ...], the clips' sample counts)``."""
        from . import mel as M
        wave, lengths = recordings(self._clips(audio, x.shape[0], who), x.device, sample_rate, audio_lengths, silence)
        return [M.extract(wave, lengths, hop, self._rt.mel_mean, self._rt.mel_std, sample_rate=24000, n_mels=self.hp.n_feats)
                for hop in hops], lengths

    def _mel_arg(self, name, frames, m, lengths, B, dev):
        """A normalised mel [B, n_feats, ``frames``] as fp32 on the device, and its lengths (default: the whole tensor) as a long tensor
        there."""
        if m.dim() != 3 or m.shape[0] != B or m.shape[1] != self.hp.n_feats:
            raise ValueError(f"{name} must be [{B}, {self.hp.n_feats}, {frames}], got {tuple(m.shape)}")
        if lengths is None:
            lengths = torch.full((B,), m.shape[2], dtype=torch.long, device=dev)
        return m.to(dev, torch.float32), torch.as_tensor(lengths).to(device=dev, dtype=torch.long)

    def _fine_recording(self, x, audio, audio_lengths, mel_fine, mel_fine_lengths, who, sample_rate=24000, silence=None):
        """The recording of ``align`` / ``speaker_grad`` as ``(mel_fine [B, n_feats, Tm >= Tx], mel_fine_lengths)`` on the device: the
        fine mel of ``audio`` extracted as ``enroll_voice`` does, or the given normalised ``mel_fine``."""
        B, Tx = x.shape
        if (audio is None) == (mel_fine is None):
            raise ValueError(f"{who} needs either audio= or mel_fine=")
        if mel_fine is None:
            from .style import FINE_HOP
            ((mel_fine, mel_fine_lengths),), _ = self._recorded_mels(x, audio, audio_lengths, who, sample_rate, silence, FINE_HOP)
        mel_fine, mel_fine_lengths = self._mel_arg("mel_fine", "Tm", mel_fine, mel_fine_lengths, B, x.device)
        if mel_fine.shape[2] < Tx:              # (the padded shapes: the device checks each utterance's own lengths)
            mel_fine = torch.nn.functional.pad(mel_fine, (0, Tx - mel_fine.shape[2]))
        return mel_fine, mel_fine_lengths

    @torch.inference_mode()
    def speaker_grad(self, x, x_lengths, audio=None, audio_lengths=None, mel_fine=None, mel_fine_lengths=None, speaker=0, voice_mix=None,
                     speaker_embeddings=None, durations=None, silence=None, sample_rate=24000):
        """Gradient of the training forward's prior and duration losses with respect to the two speaker rows, per utterance, on the
        device (``HipModel.speaker_grad``; include/mtts.h mtts_spk_grad): what the reference's matcha/finetune_speaker.py
        back-propagates with everything but one row of each speaker table frozen.  The recording (and ``sample_rate``, ``silence``) as for ``align``; speaker arguments
        as for ``synthesise``; ``durations`` (int [B, Tx], fine frames) replaces the alignment search.

        Returns ``g_enc``, ``g_dur`` [B, spk_emb_dim] (gradients of the per-utterance sums ``prior_sum``, ``dur_sum`` [B]),
        ``durations`` (int32 [B, Tx]), ``mel_fine_lengths`` and the two batch losses ``dur_loss``, ``prior_loss`` as ``score``
        reports them.  The gradients of those batch losses are ``g_dur.sum(0) / x_lengths.sum()`` and
        ``g_enc.sum(0) / mel_fine_lengths.sum()``.  One synchronisation per call (under the guard of ``Runtime.guarded``);
        ``ValueError`` names a refused utterance."""
        rt = self._rt
        dev = x.device
        hp = self.hp

        def run():
            hip = rt.ready()
            y, y_lengths = self._fine_recording(x, audio, audio_lengths, mel_fine, mel_fine_lengths, "speaker_grad", sample_rate, silence)
            rows = speaker_embeddings       # (given rows may come flat: shaped before the count is checked)
            if rows is not None:
                rows = tuple(e.to(dev).reshape(-1, hp.spk_emb_dim) for e in rows)
            e_enc, e_dur = self._voice_rows(x.shape[0], dev, speaker, voice_mix, rows)
            x_len = x_lengths.to(device=dev, dtype=torch.long)
            out = hip.speaker_grad(x, x_len, e_enc, e_dur, y.contiguous(), y_lengths, hp.prior_loss_threshold, hp.duration_loss_threshold,
                                   durations=durations)
            out["mel_fine_lengths"] = y_lengths
            out["dur_loss"] = out["dur_sum"].sum() / x_len.to(torch.float32).sum()
            out["prior_loss"] = out["prior_sum"].sum() / y_lengths.to(torch.float32).sum()
            return out
        # (the stream is already drained: no second wait)
        return rt.guarded(self.range_policy, run, lambda _: (bool(rt.ready().call_flags("spk_grad")[0].item()), False))

    @torch.inference_mode()
    def style_match_grad(self, x, x_lengths, rows_pred, speaker=0, voice_mix=None, speaker_embeddings=None, beta_mu=0.002, beta_logw=0.004):
        """The loss of the reference's style-encoder training and its gradient with respect to the predicted rows, on the device
        (``HipModel.speaker_grad_match``; include/mtts.h mtts_spk_grad_match; reference matcha/models/style_encoder.py:119-149): the
        frozen text encoder's ``mu_x`` and ``logw`` under ``rows_pred = (e_enc, e_dur)`` [B, spk_emb_dim] against those under the real
        rows of ``speaker`` (speaker arguments as for ``synthesise``), smooth-L1 with the reference's betas.  The reference freezes
        Matcha in ``eval()`` for this training: this is exactly its gradient.

        Returns ``g_enc``, ``g_dur`` [B, spk_emb_dim] -- gradients of the per-utterance sums ``ac_sum``, ``rh_sum`` [B]; the
        reference's batch losses ``acoustic_loss``, ``rhythm_loss`` (the batch sums over ``x_lengths.sum()``: tokens, not tokens x
        channels, for both) whose gradients are ``g_enc / x_lengths.sum()`` and ``g_dur / x_lengths.sum()`` row by row; and the logged
        ``emb_dist_enc``, ``emb_dist_dur`` (batch mean of the root-mean-square difference between predicted and real rows).  One synchronisation per call
        (under the guard of ``Runtime.guarded``); ``ValueError`` names a refused utterance."""
        rt = self._rt
        dev = x.device
        hp = self.hp

        def run():
            hip = rt.ready()
            B = x.shape[0]
            rows = speaker_embeddings
            if rows is not None:
                rows = tuple(e.to(dev).reshape(-1, hp.spk_emb_dim) for e in rows)
            e_enc, e_dur = self._voice_rows(B, dev, speaker, voice_mix, rows)
            e_enc, e_dur = e_enc.expand(B, -1).contiguous(), e_dur.expand(B, -1).contiguous()
            p_enc, p_dur = (torch.as_tensor(r).to(device=dev, dtype=torch.float32).reshape(B, hp.spk_emb_dim) for r in rows_pred)
            x_len = x_lengths.to(device=dev, dtype=torch.long)
            mu_ref, logw_ref, _ = hip.text_encoder(x, x_len, e_enc, e_dur)
            out = hip.speaker_grad_match(x, x_len, p_enc, p_dur, mu_ref, logw_ref, beta_mu, beta_logw)
            tokens = x_len.to(torch.float32).sum()
            out["acoustic_loss"] = out["ac_sum"].sum() / tokens
            out["rhythm_loss"] = out["rh_sum"].sum() / tokens
            out["emb_dist_enc"] = (p_enc - e_enc).pow(2).mean(dim=1).sqrt().mean()
            out["emb_dist_dur"] = (p_dur - e_dur).pow(2).mean(dim=1).sqrt().mean()
            out["mu_ref"], out["logw_ref"] = mu_ref, logw_ref
            return out
        # (the stream is already drained: no second wait)
        return rt.guarded(self.range_policy, run, lambda _: (bool(rt.ready().call_flags("spk_grad_match")[0].item()), False))

    @torch.inference_mode()
    def duration_grad(self, x, x_lengths, durations=None, audio=None, audio_lengths=None, mel_fine=None, mel_fine_lengths=None, speaker=0,
                      voice_mix=None, speaker_embeddings=None, sample_rate=24000, silence=None, params=None):
        """Gradient of the training forward's duration loss with respect to every parameter of the duration predictor
        (``encoder.proj_w.*``), on the device (``HipModel.dp_grad``; include/mtts.h mtts_dp_grad).  In the reference the predictor reads
        ``x.detach()`` and the duration Huber loss is the only loss that reaches it, so with everything else frozen this is the
        reference's gradient for those tensors -- the dropout-free one (the reference trains with ``p_dropout``).

        ``durations`` (int [B, Tx], fine frames) are the targets; without them ``align`` runs first on the recording (``audio`` at
        ``sample_rate`` with ``silence``, or ``mel_fine``, as for ``speaker_grad``).  Speaker arguments as for ``synthesise``.
        ``params``: the predictor as one flat vector in the layout of ``hip.dp_layout()`` (None: the model's own predictor).

        Returns ``grad`` (flat, the gradient of ``dur_loss``: already divided by the token count), ``g_dur`` [B, spk_emb_dim] (gradient
        of the per-utterance sums ``dur_sum`` [B] with respect to the ``e_dur`` rows), ``dur_loss``, ``dur_loss_per_utterance``,
        ``durations`` (int32 [B, Tx]) and ``logw`` [B, 1, Tx] of the predictor in ``params``, computed in native fp32 (not bit-equal to
        ``text_encoder``'s under the default arithmetic).  One synchronisation per call; ``ValueError`` names a refused utterance."""
        rt = self._rt
        dev = x.device
        hp = self.hp
        if durations is None:
            durations = self.align(x, x_lengths, audio=audio, audio_lengths=audio_lengths, mel_fine=mel_fine, mel_fine_lengths=mel_fine_lengths,
                                   speaker=speaker, voice_mix=voice_mix, speaker_embeddings=speaker_embeddings, silence=silence,
                                   sample_rate=sample_rate)["durations"]

        def run():
            hip = rt.ready()
            rows = speaker_embeddings
            if rows is not None:
                rows = tuple(e.to(dev).reshape(-1, hp.spk_emb_dim) for e in rows)
            e_enc, e_dur = self._voice_rows(x.shape[0], dev, speaker, voice_mix, rows)
            x_len = x_lengths.to(device=dev, dtype=torch.long)
            dur = torch.as_tensor(durations).to(device=dev, dtype=torch.int32)
            out = hip.dp_grad(x, x_len, e_enc, e_dur, dur, hp.duration_loss_threshold, hip.dp_train_buffer(params))
            tokens = x_len.to(torch.float32).sum()
            out["grad"] = out["grad"] / tokens
            out["dur_loss"] = out["dur_sum"].sum() / tokens
            out["dur_loss_per_utterance"] = out["dur_sum"] / x_len.to(torch.float32)
            out["durations"] = dur
            return out
        # (the stream is already drained: no second wait)
        return rt.guarded(self.range_policy, run, lambda _: (bool(rt.ready().call_flags("dp_grad")[0].item()), False))

    @torch.inference_mode()
    def finetune_speaker(self, x, x_lengths, audio=None, audio_lengths=None, mel_fine=None, mel_fine_lengths=None, speaker=0,
                         speaker_embeddings=None, steps=100, lr=5e-5, betas=(0.9, 0.999), eps=1e-8, batch_size=None, shuffle_seed=0,
                         silence=None, sample_rate=24000):
        """Fine-tune one voice on its recordings: the reference's matcha/finetune_speaker.py (all parameters frozen but one row of
        ``speaker_embeddings_enc.weight`` and one of ``speaker_embeddings_dur.weight``, trained with the ordinary training loss) as
        ``steps`` device gradient calls and Adam updates of the two rows.

        ``x`` [N, Tx], ``x_lengths`` [N] and the recordings (``audio`` at ``sample_rate``, or ``mel_fine``, as for ``align``; converted to
        24 kHz, silence-normalised with ``silence=(leading_s, trailing_s)``, and turned into the fine mel once, before the loop) are the voice's utterances;
        the start is ``speaker`` (an id) or ``speaker_embeddings=(e_enc, e_dur)`` (e.g. of ``enroll_voice``).  Each step runs one
        ``speaker_grad`` over a batch (``batch_size`` utterances in the order of a ``shuffle_seed``-seeded permutation per epoch;
        None: all of them), every utterance with the current rows and a freshly searched alignment (as the reference's forward
        does), forms the reference's batch normalisation ``g_dur.sum(0) / sum(x_lengths)``, ``g_enc.sum(0) / sum(mel_fine_lengths)``
        and applies one Adam step in torch on the device.  Adam without weight decay: the reference's AdamW puts ``nn.Embedding``
        parameters in the no-decay group (matcha/models/baselightningmodule.py:29-59); ``lr`` defaults to
        configs/model/optimizer/adamw.yaml.

        Returns ``(e_enc, e_dur, history)``: the rows [1, spk_emb_dim] for ``synthesise(speaker_embeddings=...)``, a batcher request
        or ``add_speaker``, and ``history`` = ``{"dur_loss": [...], "prior_loss": [...]}`` per step (before that step's update).

        Two deviations from the reference.  It fine-tunes in train mode with dropout active; this is the dropout-free (eval)
        gradient, deterministic.  The flow-matching loss is not evaluated: it cannot move the rows, because ``mu_y`` is detached
        before ``decoder.compute_loss`` (matcha_tts.py:154-162) and the estimator has no speaker input."""
        self._rt.ready()                                   # mel statistics come from the loaded checkpoint's buffers
        dev = x.device
        N, Tx = x.shape
        if int(steps) < 1:
            raise ValueError("steps must be >= 1")
        mel_fine, mel_fine_lengths = self._fine_recording(x, audio, audio_lengths, mel_fine, mel_fine_lengths, "finetune_speaker", sample_rate, silence)
        x_lengths = x_lengths.to(device=dev, dtype=torch.long)
        if speaker_embeddings is not None:
            speaker_embeddings = [torch.as_tensor(r).reshape(1, -1) for r in speaker_embeddings]
        E = self.hp.spk_emb_dim
        rows = [r.detach().to(device=dev, dtype=torch.float32).clone() for r in self._voice_rows(1, dev, int(speaker), None, speaker_embeddings)]
        if any(r.shape[1] != E for r in rows):
            raise ValueError(f"a speaker row has {E} values")
        m = [torch.zeros_like(r) for r in rows]
        v = [torch.zeros_like(r) for r in rows]
        b1, b2 = float(betas[0]), float(betas[1])
        bs = N if batch_size is None else max(1, min(int(batch_size), N))
        gen = torch.Generator().manual_seed(int(shuffle_seed))
        order, at = None, 0
        history = {"dur_loss": [], "prior_loss": []}
        for step in range(1, int(steps) + 1):
            if bs == N:
                idx = None
            else:
                if order is None or at + bs > N:
                    order, at = torch.randperm(N, generator=gen), 0
                idx = order[at:at + bs].to(dev)
                at += bs
            sel = (lambda t: t) if idx is None else (lambda t: t.index_select(0, idx))
            out = self.speaker_grad(sel(x), sel(x_lengths), mel_fine=sel(mel_fine), mel_fine_lengths=sel(mel_fine_lengths),
                                    speaker_embeddings=(rows[0], rows[1]))
            grads = (out["g_enc"].sum(0, keepdim=True) / out["mel_fine_lengths"].to(torch.float32).sum(),
                     out["g_dur"].sum(0, keepdim=True) / sel(x_lengths).to(torch.float32).sum())
            history["dur_loss"].append(out["dur_loss"])
            history["prior_loss"].append(out["prior_loss"])
            for k, g in enumerate(grads):              # torch.optim.Adam, weight_decay 0
                m[k] = b1 * m[k] + (1 - b1) * g
                v[k] = b2 * v[k] + (1 - b2) * g * g
                denom = (v[k] / (1 - b2 ** step)).sqrt() + eps
                rows[k] = rows[k] - (lr / (1 - b1 ** step)) * m[k] / denom
        history = {k: [float(t) for t in torch.stack(val).cpu()] for k, val in history.items()}
        return rows[0], rows[1], history

    @torch.inference_mode()
    def score(self, x, x_lengths, audio=None, audio_lengths=None, mel=None, mel_lengths=None, mel_fine=None, mel_fine_lengths=None,
              speaker=0, voice_mix=None, speaker_embeddings=None, t=None, noise=None, per_request_padding=False, return_frames=False,
              silence=None, sample_rate=24000):
        """How well does this model, with this voice, explain this recording: the three numbers of the reference's training forward
        (``MatchaTTS.forward``, matcha/models/matcha_tts.py:64-164), forward pass only, on the device.

        ``dur_loss``: Huber distance between the predictor's ``logw`` and ``log(2 + MAS durations)``; ``prior_loss``: Huber distance
        between the recording's fine mel and ``mu_x`` expanded along the MAS path; ``diff_loss``: the conditional-flow-matching loss
        of ``BASECFM.compute_loss`` (flow_matching.py:65-107), one estimator evaluation at time ``t[b]`` per utterance.  The Huber
        thresholds are the checkpoint's (``hp.prior_loss_threshold``, ``hp.duration_loss_threshold``).

        The recording: ``audio`` (and ``sample_rate``, ``silence``) as for ``align`` -- both mels are extracted (hop 256 and hop 128) and padded as the reference's
        collate pads them (matcha/data/text_mel_datamodule.py:481-499) -- or ``mel`` [B, n_feats, T] and ``mel_fine`` [B, n_feats,
        Tm], normalised with this model's mel statistics, with their lengths (default: the whole tensors).  Speaker arguments as
        for ``synthesise``.  ``t``: [B] (default ``torch.rand``) or a grid [K, B] -- K evaluations with the same ``noise``
        ([B, n_feats, T], default ``randn``); a single random ``t`` is a very noisy estimate, a fixed grid is what makes two voices
        comparable.  ``per_request_padding``: the estimator treats every utterance as padded to its own length (one more host read).

        Returns 0-dim ``dur_loss``, ``prior_loss``, ``diff_loss`` with the reference's batch normalisation (``/ sum(x_lengths)``,
        ``/ sum(y_fine_mask)``, ``/ (sum(y_mask) * n_feats)``; ``diff_loss`` is [K] for a grid), the same three ``*_per_utterance``
        ([B]; [K, B]), the raw sums ``dur_sum``, ``prior_sum``, ``sq_sum``, ``durations`` (int32 [B, Tx]), ``mas_score`` [B],
        ``mel_lengths``, ``mel_fine_lengths`` and, with ``return_frames``, ``prior_frame`` [B, Tm] and ``dur_err`` [B, Tx].  One
        synchronisation per call (under the guard of ``Runtime.guarded``); ``ValueError`` names an utterance with fewer frames
        than tokens."""
        rt = self._rt
        rt.ready()                                         # mel statistics come from the loaded checkpoint's buffers
        dev = x.device
        rec = self._score_recording(x, audio, audio_lengths, mel, mel_lengths, mel_fine, mel_fine_lengths, sample_rate, silence)
        B, nf, T = rec[0].shape
        if noise is None:
            noise = torch.randn(B, nf, T, dtype=torch.float32, device=dev)
        elif tuple(noise.shape) != (B, nf, T):
            raise ValueError(f"noise must be [{B}, {nf}, {T}] (the padded coarse mel), got {tuple(noise.shape)}")
        noise = noise.to(dev)
        t = torch.rand(B, device=dev) if t is None else torch.as_tensor(t, dtype=torch.float32).to(dev)
        if t.dim() not in (1, 2) or t.shape[-1] != B:
            raise ValueError(f"t must be [{B}] or [K, {B}], got {tuple(t.shape)}")

        def run():
            return self._score(x, x_lengths, rec, speaker, voice_mix, speaker_embeddings, t, noise, per_request_padding, return_frames)
        # the flags that _score read with its own wait (host copy: no second wait); it raises the time-out itself, under every policy
        out, _ = rt.guarded(self.range_policy, run, lambda r: (bool(r[1][:2].any()), False))
        return out

    def _score_recording(self, x, audio, audio_lengths, mel, mel_lengths, mel_fine, mel_fine_lengths, sample_rate=24000, silence=None):
        """(mel [B, nf, T], mel_lengths, mel_fine [B, nf, Tm], mel_fine_lengths, host coarse lengths or None) padded like the
        reference's collate: T = fix_len_compatibility(longest coarse mel), Tm = 2 T (more only if a given tensor is longer or
        there are more tokens than that)."""
        dev = x.device
        B, Tx = x.shape
        host_len = None
        if audio is not None:
            if mel is not None or mel_fine is not None:
                raise ValueError("score needs either audio= or mel= and mel_fine=")
            from .style import FINE_HOP
            ((mel_fine, mel_fine_lengths), (mel, mel_lengths)), lengths = self._recorded_mels(
                x, audio, audio_lengths, "score", sample_rate, silence, FINE_HOP, STD_RES_HOP_LENGTH)
            host_len = [n // STD_RES_HOP_LENGTH + 1 for n in lengths]
        elif mel is None or mel_fine is None:
            raise ValueError("score needs either audio= or mel= and mel_fine=")
        mel, mel_lengths = self._mel_arg("mel", "T", mel, mel_lengths, B, dev)
        mel_fine, mel_fine_lengths = self._mel_arg("mel_fine", "T", mel_fine, mel_fine_lengths, B, dev)
        T = fix_len_compatibility(mel.shape[2])
        Tm = max(2 * T, mel_fine.shape[2], Tx)
        if mel.shape[2] < T:
            mel = torch.nn.functional.pad(mel, (0, T - mel.shape[2]))
        if mel_fine.shape[2] < Tm:
            mel_fine = torch.nn.functional.pad(mel_fine, (0, Tm - mel_fine.shape[2]))
        return mel.contiguous(), mel_lengths, mel_fine.contiguous(), mel_fine_lengths, host_len

    def _score(self, x, x_lengths, rec, speaker, voice_mix, speaker_embeddings, t, noise, per_request_padding, return_frames):
        hip = self._rt.ready()
        dev = x.device
        B, Tx = x.shape
        mel, mel_lengths, mel_fine, mel_fine_lengths, host_len = rec
        nf, T = mel.shape[1], mel.shape[2]
        e_enc, e_dur = self._voice_rows(B, dev, speaker, voice_mix, speaker_embeddings)
        x_lengths = x_lengths.to(device=dev, dtype=torch.long)
        hp = self.hp
        mu_x, logw, x_mask = self.encoder(x, x_lengths, e_enc, e_dur)
        durations, mas_score, _ = hip.mas(x_lengths, mel_fine_lengths, mu_x=mu_x, y=mel_fine, check_lengths=False)
        prior_sum, dur_sum, prior_frame, dur_err = hip.score_prior_dur(
            mu_x, logw, durations, mel_fine, x_lengths, mel_fine_lengths, hp.prior_loss_threshold, hp.duration_loss_threshold,
            return_frames=return_frames, check_lengths=False)
        # the coarse mu_y of matcha_tts.py:124,154: (mu_x @ path) pooled k3 s2 p1, from the same durations
        _, cum, fine_total = hip.durations_given(durations, x_mask, 1.0)
        mu_y, _, _ = hip.align_pool(mu_x, cum, fine_total, T)
        y_mask = (torch.arange(T, device=dev)[None, :] < mel_lengths[:, None]).to(torch.float32)[:, None, :]
        if per_request_padding:
            own = host_len if host_len is not None else [int(v) for v in mel_lengths.tolist()]
            hip.set_frame_limits(torch.tensor([min(fix_len_compatibility(max(v, 1)), T) for v in own], dtype=torch.int32, device=dev))
        flags = None
        try:
            sq = []
            for tk in (t if t.dim() == 2 else t[None]):
                sq.append(hip.cfm_loss(mel, mu_y, y_mask, noise, tk.contiguous(), self.decoder.use_mu_prior, self.decoder.sigma_min)[0])
                f = torch.cat([hip.range_flags(), hip.pair_timeouts()])
                flags = f if flags is None else flags | f
        finally:
            if per_request_padding:
                hip.set_frame_limits(None)
        sq_sum = torch.stack(sq) if t.dim() == 2 else sq[0]
        hip.mas_status()                       # the call's one wait; raises ValueError for an utterance the device refused
        hip.score_status()
        flags = flags.cpu()
        if int(flags[2]):
            raise RuntimeError(PAIR_TIMEOUT_ERROR)
        n_tok, n_fine, n_coarse = x_lengths.to(torch.float32), mel_fine_lengths.to(torch.float32), y_mask.sum((1, 2))
        out = {"dur_loss": dur_sum.sum() / n_tok.sum(), "prior_loss": prior_sum.sum() / n_fine.sum(),
               "diff_loss": sq_sum.sum(-1) / (n_coarse.sum() * nf),
               "dur_loss_per_utterance": dur_sum / n_tok, "prior_loss_per_utterance": prior_sum / n_fine,
               "diff_loss_per_utterance": sq_sum / (n_coarse * nf),
               "dur_sum": dur_sum, "prior_sum": prior_sum, "sq_sum": sq_sum, "durations": durations, "mas_score": mas_score,
               "mel_lengths": mel_lengths, "mel_fine_lengths": mel_fine_lengths}
        if return_frames:
            out["prior_frame"], out["dur_err"] = prior_frame, dur_err
        return out, flags

    @torch.inference_mode()
    def _synthesise(self, x, x_lengths, n_timesteps, speaker=0, voice_mix=None, scale_correction=1.0, length_scale=1.0,
                    debug=False, z=None, sync_max=None, per_request_padding=False, speaker_embeddings=None, durations=None, *,
                    token_scale=None, token_extend=None, return_timing=False):
        """Text ids -> mel (reference inference.py:78-183).  Returns ``{"mel": [B, n_feats, T_valid_max]}`` (+ the
        reference's debug tensors when ``debug``).

        ``z``: explicit noise [B, n_feats, T_pad], or a callable ``T_pad -> noise``; default = the device seed-42
        generator like the reference.  ``sync_max``: callable mapping this process's maximum fine length to the
        batch-wide one (data-parallel shards must pad like the whole batch, see dp.py).
        ``speaker_embeddings``: per-utterance ``(e_enc, e_dur)`` rows, e.g. from ``speaker_rows`` (overrides speaker / voice_mix).
        ``per_request_padding``: the reference derives the padded length, and with it the GroupNorm statistics, the
        attention key set and the noise shape, from the longest utterance of the call, so a request's mel depends on what
        it is batched with.  With this flag every utterance is padded (logically) to its OWN length: each row of a ragged
        batch equals the batch-of-one result for that request to rounding (what a dynamic batcher in front of the reference's
        one-request-at-a-time server needs); one extra host read of the B fine lengths.
        ``durations``: fine frames per token to speak with instead of the duration predictor's -- a [B, Tx] tensor (e.g.
        ``align(...)["durations"]``, or this method's own debug ``phoneme_durations``, which reproduces the default call bit for
        bit), or a list of B rows where None leaves a row to the predictor (the batcher's mix).  ``scale_correction`` corrects the
        predictor and is ignored on given rows; ``length_scale`` still multiplies.  A zero drops a token.
        ``token_scale`` / ``token_extend`` (keyword-only): a rate and an extension in fine frames per token -- [B, Tx] tensors, or lists
        of B rows where None leaves a row alone -- applied to predicted and given rows alike in ONE launch (``hip.durations_shaped``:
        ``d = round(d_unrounded * scale + extend)``; a scale of exactly 0 drops the token).  Host values outside [0, 16] /
        [-4096, 4096] raise ``ValueError`` before anything is launched.  ``return_timing``: the result also carries ``"token_ends"``
        (the inclusive cumulative durations in fine frames, int32 [B, Tx]: what ``to_waveforms(token_ends=)`` takes) and
        ``"durations"``.  Without the three, exactly the calls of before are made."""
        shaped = token_scale is not None or token_extend is not None
        if shaped:
            from . import timing as TM
            TM.check_shaping(token_scale, "token_scale")
            TM.check_shaping(token_extend, "token_extend")
        hip = self._rt.ready()
        dev = x.device
        B = x.shape[0]
        e_enc, e_dur = self._voice_rows(B, dev, speaker, voice_mix, speaker_embeddings)

        mu_x, logw, x_mask = self.encoder(x, x_lengths, e_enc, e_dur)
        if shaped:
            durations, cum, y_fine_lengths = self._shaped_durations(hip, durations, logw, x_mask, scale_correction, length_scale,
                                                                    token_scale, token_extend)
        elif durations is None:
            durations, cum, y_fine_lengths = hip.durations(logw, x_mask, scale_correction, length_scale)
        else:
            durations, cum, y_fine_lengths = self._given_durations(hip, durations, logw, x_mask, scale_correction, length_scale)
        # the one host sync of the path, as in the reference (utils/model.py:19: .item())
        max_fine = int(y_fine_lengths.max().item())
        if sync_max is not None:
            max_fine = int(sync_max(max_fine))
        t_pad = fix_len_compatibility(max_fine)
        if callable(z):
            z = z(t_pad)
        mu_y, y_mask, y_lengths = hip.align_pool(mu_x, cum, y_fine_lengths, t_pad)
        y_max_length = max((max_fine + 1) // 2, 1)

        t_len = None
        if per_request_padding:
            if sync_max is not None:
                raise ValueError("per_request_padding needs no batch-wide length: do not combine it with sync_max")
            t_len = [fix_len_compatibility(max(int(v), 1)) for v in y_fine_lengths.tolist()]
        mel = self.decoder(mu_y, y_mask, n_timesteps, z=z, t_out=y_max_length, out_scale=self._rt.mel_std,
                           out_shift=self._rt.mel_mean, t_len=t_len, y_lengths=y_lengths, y_max=y_max_length)
        timing = {"token_ends": cum, "durations": durations} if return_timing else {}
        if not debug:
            return {"mel": mel, "mel_lengths": y_lengths, **timing}
        encoder_mel = mu_y[:, :, :y_max_length] * self._rt.mel_std + self._rt.mel_mean
        raw = ((torch.exp(logw) - 2) * x_mask).squeeze(1)
        return {"mel": mel, "encoder_mel": encoder_mel, "phoneme_durations": durations, "raw_phoneme_durations": raw,
                "mel_lengths": y_lengths, "mu_y": mu_y, "y_mask": y_mask, "logw": logw, "mu_x": mu_x, **timing}


def _recordings_24k(clips, dev, sample_rate=24000, lengths=None):
    """Clips -> ``(wave [B, ld] fp32 on ``dev``, lengths: list of B ints)`` at 24 kHz, ld a multiple of 4: the padded buffer the mel
    front end takes.  ``clips``: 1-D waveforms (host or device); ``lengths``: samples to use of each (default: all);
    ``sample_rate``: an int or one per clip.  Clips at another rate are padded into one buffer per distinct rate and converted on
    the device (``resample.resample``, the given length as the row length); rows at 24 kHz are copied.  With every clip at 24 kHz
    nothing but the copies is launched.  The converted lengths are ``ceil(24000 * len / rate)``, known without a host read."""
    from . import resample as R
    clips, sample_rate = _decoded_clips(list(clips), dev, sample_rate)
    clips = [torch.as_tensor(c).to(torch.float32) for c in clips]
    if any(c.dim() != 1 for c in clips):
        raise ValueError("a clip is a 1-D waveform (mono)")
    B = len(clips)
    rates = R.rates_per_row(sample_rate, B)
    lengths = [int(c.numel()) for c in clips] if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
    if len(lengths) != B:
        raise ValueError(f"lengths need one entry per clip ({B}), got {len(lengths)}")
    converted = {}                                         # rate -> (rows, out [len(rows), ld_r], kept samples per row)
    for rate in sorted(set(rates) - {SAMPLE_RATE}):
        rows = [b for b in range(B) if rates[b] == rate]
        rs = R.resampler(rate, SAMPLE_RATE, dev)
        src = torch.zeros(len(rows), (max(int(clips[b].numel()) for b in rows) + 3) // 4 * 4, dtype=torch.float32, device=dev)
        for i, b in enumerate(rows):
            if lengths[b] < 0 or lengths[b] > clips[b].numel():
                raise ValueError(f"lengths[{b}] = {lengths[b]} is outside [0, {clips[b].numel()}]")
            src[i, :clips[b].numel()].copy_(clips[b])
        out, _ = rs(src, [lengths[b] for b in rows], check=False)      # (the lengths were checked above: no wait)
        converted[rate] = (rows, out, [rs.out_length(lengths[b]) for b in rows])
    width = [int(clips[b].numel()) for b in range(B)]
    for rows, out, keep in converted.values():
        for i, b in enumerate(rows):
            width[b], lengths[b] = keep[i], keep[i]
    ld = (max(width) + 3) // 4 * 4
    wave = torch.zeros(B, ld, dtype=torch.float32, device=dev)
    for b, c in enumerate(clips):
        if rates[b] == SAMPLE_RATE:
            wave[b, :c.numel()].copy_(c)
    for rows, out, keep in converted.values():
        for i, b in enumerate(rows):
            wave[b, :keep[i]].copy_(out[i, :keep[i]])
    return wave, lengths


def _decoded_clips(clips, dev, sample_rate):
    """``audio_codec.Encoded`` and ``audio_codec.FlacClip`` clips among ``clips`` decoded on the device (one launch for all the
    ``Encoded`` ones, one ``decode_flac`` call for all the FLAC files, ahead of the rate conversion), and the clips' rates:
    ``sample_rate`` as given where it names a rate for a clip -- an int names one for every clip -- and, where it is None (as a whole,
    or that clip's entry of a list), the clip's own ``sample_rate`` (24 kHz for a waveform).  Without such a clip and with every rate
    named, both arguments come back as they are and nothing is launched.  A FLAC file comes from outside, so its verdict is read (the
    one wait here): a stream the device refuses raises ``ValueError``; ``Encoded`` clips alone are decoded without a wait, as before."""
    from . import audio_codec as AC
    at = [i for i, c in enumerate(clips) if isinstance(c, (AC.Encoded, AC.FlacClip))]
    own = [clips[i].sample_rate if i in at else SAMPLE_RATE for i in range(len(clips))]
    if sample_rate is None:
        sample_rate = own
    elif not isinstance(sample_rate, (int, np.integer)) and not torch.is_tensor(sample_rate):
        sample_rate = [own[i] if r is None else r for i, r in enumerate(sample_rate)] if len(sample_rate) == len(clips) else sample_rate
    if at:
        wave, counts = AC.decode_clips([clips[i] for i in at], dev, check=any(isinstance(clips[i], AC.FlacClip) for i in at))
        for k, i in enumerate(at):
            clips[i] = wave[k, :counts[k]]
    return clips, sample_rate


def _silence_normalised(wave, lengths, silence):
    """``silence=`` of the recording entries: None returns the arguments (nothing is launched); ``(leading_s, trailing_s)`` (either
    may be None) rebuilds every 24 kHz row of ``_recordings_24k`` with exactly that much silence around its content
    (``corpus.normalize_silence``) and reads the new lengths, which the mel front end needs on the host."""
    if silence is None:
        return wave, lengths
    from . import corpus as CP
    if len(silence) != 2:
        raise ValueError("silence is None or (leading seconds or None, trailing seconds or None)")
    out, out_len, _ = CP.normalize_silence(wave, lengths, silence[0], silence[1], sample_rate=SAMPLE_RATE)   # (ValueError names a refused row)
    return out, [int(v) for v in out_len.tolist()]


def recordings(clips, dev, sample_rate=24000, lengths=None, silence=None):
    """What the recording entries (``enroll_voice``, ``align``, ``score``, ``speaker_grad``, ``finetune_speaker``) make of their clips
    before the mel front end: ``(wave [B, ld] fp32 on ``dev`` at 24 kHz, lengths: list of B ints)``.  ``clips``: 1-D waveforms (host
    or device) at ``sample_rate`` (an int or one per clip; converted on the device), ``audio_codec.Encoded`` clips -- still bytes,
    PCM16 / mu-law / A-law, decoded on the device in one launch -- or ``audio_codec.FlacClip`` files, decoded on the device in one
    ``decode_flac`` call (channel 0); where ``sample_rate`` is None, or None for that clip, the clip's own ``sample_rate`` is used --,
    ``lengths``: samples to use of each;
    ``silence``: None or ``(leading_s, trailing_s)``, normalised after the conversion (``corpus.normalize_silence``).  For a
    caller that needs the lengths ahead of the call, e.g. to size ``score``'s noise."""
    return _silence_normalised(*_recordings_24k(clips, dev, sample_rate, lengths), silence)


def _plain(obj):
    """OmegaConf containers -> plain python, when omegaconf is importable (it is not on the GPU box)."""
    try:
        from omegaconf import OmegaConf  # type: ignore
        if OmegaConf.is_config(obj):
            return OmegaConf.to_container(obj, resolve=True)
    except Exception:
        pass
    return obj


def load_matcha(model_name, checkpoint_path):
    """reference inference.py:186-197: Lightning checkpoint with ``hyper_parameters`` + ``state_dict``; also accepts a
    directory written by ``checkpoint.convert_lightning_checkpoint`` (flat safetensors + JSON, no lightning / omegaconf)."""
    print(f"[!] Loading {model_name}!")
    from . import checkpoint as ck
    if ck.is_converted(checkpoint_path):
        hp, sd = ck.load_converted(checkpoint_path)
        model = MatchaTTSInfer(**hp.as_reference_kwargs())
        model.load_state_dict(sd, strict=True)
        model._rt.cache_dir = checkpoint_path        # the packed weight image is cached beside the converted tensors
    else:
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        hparams = dict(_plain(ckpt["hyper_parameters"]))
        hparams.pop("optimizer", None)
        hparams.pop("scheduler", None)
        model = MatchaTTSInfer(**hparams)
        model.load_state_dict(ckpt["state_dict"], strict=False)
    model = model.to(DEVICE).eval()
    print(f"[+] {model_name} loaded!")
    return model


def process_text(text: str, language: str):
    """reference inference.py:212-220.  The phonemizer (eSpeak + NeMo) is a CPU front end outside this package; it is
    taken from the reference's ``matcha.text`` when that package is installed."""
    try:
        from matcha.text.phonemizers import multilingual_phonemizer  # type: ignore
    except Exception as e:  # pragma: no cover - depends on the host installation
        raise RuntimeError("process_text needs the reference's matcha.text phonemizer (eSpeak/NeMo); "
                           "feed phoneme ids to synthesise() directly otherwise") from e
    import re
    emphasized = re.sub(r"(?<![?!])\?(?![?!])", "??", text)
    separated, ids = multilingual_phonemizer(emphasized, language)
    x = torch.tensor(ids, dtype=torch.long, device=DEVICE)[None]
    x_lengths = torch.tensor([x.shape[-1]], dtype=torch.long, device=DEVICE)
    return {"x_orig": text, "x": x, "x_lengths": x_lengths, "x_phones": "".join(separated), "x_phone_ids": ids}


def load_vocoder(vocoder_name, checkpoint=None, state_dict=None):
    """reference inference.py:223-231.  The Vocos-24k head runs on the HIP library (vocoder.py); weights come from a local
    file (``VOCOS_CHECKPOINT``) because the reference's ``from_pretrained`` hub fetch needs a network."""
    print(f"[!] Loading {vocoder_name}!")
    if vocoder_name != "vocos":
        raise NotImplementedError(f"Vocoder {vocoder_name} not implemented!")
    from .vocoder import load_model
    vocoder = load_model(DEVICE, checkpoint=checkpoint, state_dict=state_dict)
    print(f"[+] {vocoder_name} loaded!")
    return vocoder


def to_waveform(mel, vocoder):
    """reference inference.py:260-265."""
    return _waveform_on_device(mel, vocoder).cpu().squeeze()


@torch.inference_mode()
def pipeline(model, vocoder, text, speaker=0, voice_mix=None, n_timesteps=DEFAULT_NUM_STEPS, scale_correction=1.0,
             length_scale=1.0, debug=False, *, encoding=None, loudness=None, true_peak=None, sample_rate=24000):
    """reference inference.py:233-257.  The reference wraps ``synthesise`` in ``torch.autocast`` (fp16 on its CUDA device);
    here the estimator's arithmetic is chosen when the model is created (``MTTS_GEMM_TERMS``: default fp32-equivalent; 1 = fp16
    operands / fp32 accumulate, the autocast arithmetic), not per call.  The trailing-silence trim runs on the device.
    ``sample_rate``: the rate of the returned waveform; anything but 24 kHz is converted on the device after the normalisation and
    the trim (``resample.resample``; the band-limited result may overshoot the 0.95 peak slightly, nothing is re-normalised).
    ``encoding``: None (a float32 waveform), or ``"pcm16"`` / ``"ulaw"`` / ``"alaw"``: the waveform is encoded on the device
    (``audio_codec.encode``) and returned as a 1-D uint8 host tensor of raw samples; ``"flac"``: as one complete FLAC stream
    (``audio_codec.encode_flac``), a file as it is.
    ``loudness``: None, or a target in LUFS the waveform is brought to on the device (``loudness.normalize``: BS.1770 integrated
    loudness, the sample peak held at or under 0.95), at 24 kHz after the trim and ahead of the rate conversion and the encoder.
    ``true_peak``: None, or a ceiling in dBTP on the true peak of the levelled waveform (``loudness.normalize(true_peak=)``); it
    needs a ``loudness`` target."""
    from . import loudness as LD
    target = LD.check_target(loudness)                                 # (a value that is no level raises before anything runs)
    ceiling = LD.check_ceiling(true_peak, target)
    primary = voice_mix[0][0] if voice_mix is not None else speaker
    language = next(v["lang"] for v in VOICES if v["id"] == str(primary))
    tp = process_text(text, language)
    out = model.synthesise(tp["x"], tp["x_lengths"], n_timesteps=n_timesteps, speaker=speaker, voice_mix=voice_mix,
                           scale_correction=scale_correction, length_scale=length_scale, debug=debug)
    waveform, _ = finish_request(trim_trailing_silence(_waveform_on_device(out["mel"], vocoder).squeeze()), loudness=target,
                                 true_peak=ceiling, sample_rate=sample_rate, encoding=encoding)
    if not debug:
        return waveform
    durs = out["phoneme_durations"].squeeze(0).tolist()
    raws = out["raw_phoneme_durations"].squeeze(0).tolist()
    pairs = list(zip(tp["x_phones"], raws, durs))
    return waveform, to_waveform(out["encoder_mel"], vocoder), pairs


def convert_to_mp3(waveform):
    """reference inference.py:290-298: int16 PCM -> MP3 through the reference installation's LAME binding
    (matcha.utils.mp3_converter.encode_mp3, vbr_quality=5, algorithm_quality=5).  The codec is a post-waveform CPU step outside
    the synthesis path: it is delegated, not re-implemented, and raises ImportError where the reference
    package (and its lameenc dependency) is not installed."""
    import time
    import numpy as np
    from matcha.utils.mp3_converter import encode_mp3  # type: ignore
    start = time.perf_counter()
    audio_np = (waveform.detach().cpu().numpy() * 32767).astype(np.int16)
    wav_size = audio_np.size * 2
    mp3_data = encode_mp3(audio_np, sample_rate=SAMPLE_RATE, vbr_quality=5, algorithm_quality=5)
    pct = (len(mp3_data) / wav_size * 100) if wav_size > 0 else 0
    print(f"MP3 conversion: {(time.perf_counter() - start) * 1000:.1f}ms | {pct:.0f}% size")
    return mp3_data


def convert_to_opus_ogg(waveform):
    """reference inference.py:301-322: int16 mono PCM -> Ogg/Opus with PyAV (libopus, 48 kbit/s, compression_level 5), the
    reference's own settings and call sequence.  PyAV is imported here, as the reference imports it at module load; where it is
    not installed the ImportError says so (no silent fallback)."""
    import io
    import time
    import numpy as np
    try:
        import av  # type: ignore
    except ImportError as e:
        raise ImportError("convert_to_opus_ogg needs PyAV (`av`), as the reference's matcha/inference.py does") from e
    start = time.perf_counter()
    audio_np = (waveform.detach().cpu().numpy() * 32767).astype(np.int16).reshape(1, -1)
    wav_size = audio_np.size * 2
    buffer = io.BytesIO()
    container = av.open(buffer, mode="w", format="ogg")
    stream = container.add_stream("libopus", rate=SAMPLE_RATE)
    stream.layout = "mono"
    stream.bit_rate = 48000
    stream.options = {"compression_level": "5"}
    frame = av.AudioFrame.from_ndarray(audio_np, format="s16", layout="mono")
    frame.sample_rate = SAMPLE_RATE
    for packet in stream.encode(frame):
        container.mux(packet)
    for packet in stream.encode():
        container.mux(packet)
    container.close()
    ogg_data = buffer.getvalue()
    pct = (len(ogg_data) / wav_size * 100) if wav_size > 0 else 0
    print(f"OGG conversion: {(time.perf_counter() - start) * 1000:.1f}ms | {pct:.0f}% size")
    return bytes(ogg_data)

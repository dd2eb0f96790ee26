"""Token timing: when each token and word is spoken in the audio a call returns, and pauses cut into that audio after chosen tokens
(include/mtts.h "token timing" has the arithmetic; csrc/timing.hip the kernels).

``token_marks`` and ``apply_breaks`` are the two device calls; ``to_waveforms(token_ends=, breaks=, return_marks=)`` runs them between
the trim and the join.  ``word_groups`` / ``word_marks`` fold token marks into word marks on the host, after the copy; ``webvtt`` /
``srt`` write cues.  Marks are nominal: a boundary is the midpoint between the centres of two fine frames, and the decoder's
receptive field smears what is heard around it."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _hip

SAMPLE_RATE = 24000
FINE_HOP = 128                     # half the vocoder hop: one fine frame of the durations
SCALE_RANGE = (0.0, 16.0)          # token_scale, as the kernel clamps it
EXTEND_RANGE = (-4096.0, 4096.0)   # token_extend (fine frames)
PAUSE_MAX_MS = 60000.0             # the longest break a host layer accepts

_timing_ws = _hip.Workspaces()


def check_shaping(values, name: str) -> None:
    """``token_scale`` / ``token_extend`` values the host can see (numbers, lists, arrays, host tensors; rows may be None) against the
    range the kernel clamps to: ``ValueError`` for a value outside it or a NaN.  A device tensor is not read: the kernel clamps it."""
    lo, hi = SCALE_RANGE if name == "token_scale" else EXTEND_RANGE
    if values is None or (torch.is_tensor(values) and values.is_cuda):
        return
    if torch.is_tensor(values) or not isinstance(values, (list, tuple)):
        t = torch.as_tensor(values, dtype=torch.float64).reshape(-1)
        if t.numel() and not bool(((t >= lo) & (t <= hi)).all()):
            raise ValueError(f"{name}: every value must lie inside [{lo:g}, {hi:g}]")
        return
    for row in values:
        check_shaping(row, name)


def check_breaks(row, n_tokens: Optional[int] = None, pause_max: float = PAUSE_MAX_MS, what: str = "breaks") -> List[Tuple[int, float]]:
    """One row's breaks ``[(token, pause), ...]`` as the device wants them: token indices strictly increasing and inside
    ``[0, n_tokens)``, pauses finite and inside ``[0, pause_max]`` (the caller's unit).  Returns the list; ``ValueError`` otherwise."""
    out, last = [], -1
    for item in row or ():
        try:
            tok, pause = item
            tok_i, pause = int(tok), float(pause)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: an entry is (token, pause), got {item!r}") from None
        if tok_i != tok or tok_i < 0 or (n_tokens is not None and tok_i >= n_tokens):
            raise ValueError(f"{what}: token {tok!r} is outside [0, {n_tokens if n_tokens is not None else 'x_length'})")
        if tok_i <= last:
            raise ValueError(f"{what}: token indices must strictly increase ({tok_i} after {last})")
        if not (math.isfinite(pause) and 0 <= pause <= pause_max):
            raise ValueError(f"{what}: a pause must lie inside [0, {pause_max:g}], got {pause!r}")
        out.append((tok_i, pause))
        last = tok_i
    return out


@dataclass
class BreakPlan:
    """What ``token_marks`` leaves for ``apply_breaks`` and the status reader: the workspace that holds the device's plan, the CSR of
    the breaks, the row stride the lengthened rows need and the new lengths (device int64 [B], -1 = refused)."""
    ws: torch.Tensor
    first: Optional[torch.Tensor]
    B: int
    NB: int
    out_ld: int
    lengths: torch.Tensor

    def raise_refused(self) -> None:
        """Wait for the stream and raise ``ValueError`` naming the first refused row, when there is one."""
        with torch.cuda.device(self.ws.device):
            _hip.raise_refused(_hip.load().mtts_token_timing_status, self.ws.data_ptr(), self.B, _hip.stream_ptr())


@torch.inference_mode()
def token_marks(cum, x_lengths, keep, breaks=None, *, fine_hop: int = FINE_HOP, keep_max: Optional[int] = None, out_ld: Optional[int] = None,
                pause_max: Optional[int] = None, check: bool = True):
    """Marks of every token of a ragged batch in its finished audio, and the plan of its breaks, in one launch (mtts_token_timing).

    ``cum`` [B, Tx] int32: the inclusive cumulative durations in fine frames (``synthesise(return_timing=True)["token_ends"]``);
    ``x_lengths`` [B]; ``keep`` [B]: the kept samples of each row at 24 kHz (``finish_waveforms``' lengths; -1 = refused upstream).
    ``breaks``: None; a host list of B rows ``[(token, pause_samples), ...]`` (None or empty: no break), checked here; or the CSR
    ``(first [B + 1] int32, token [NB] int32, pause [NB] int64)`` as tensors, which only the device judges (``out_ld`` and
    ``pause_max`` are then the caller's).  ``keep_max``: the row stride ``keep`` must fit (default 2^40: any).

    Returns ``(marks, lengths, plan)``: ``marks`` int64 [B, Tx, 2] on the device, (start, end) of each token in samples of the
    lengthened row, -1 for tokens at or beyond a row's length and for a refused row; ``lengths`` int64 [B] = keep + the applied
    pauses (-1: refused); ``plan`` a ``BreakPlan`` for ``apply_breaks``.  Nothing is read on the host unless ``check``, which waits for
    the device's verdict and raises ``ValueError`` naming the row."""
    lib = _hip.load()
    if not (torch.is_tensor(cum) and cum.is_cuda and cum.dim() == 2):
        raise RuntimeError("token_marks: cum must be a [B, Tx] tensor on a HIP device; there is no CPU path")
    dev = cum.device
    cum = cum.detach().to(torch.int32).contiguous()
    B, Tx = cum.shape
    x_lengths = _hip.row_lengths(x_lengths, B, Tx, dev, "x_lengths")
    keep = _hip.row_lengths(keep, B, 0, dev, "keep")
    keep_max = (1 << 40) if keep_max is None else int(keep_max)
    first = tok = pause = None
    NB, extra = 0, 0
    if breaks is not None and isinstance(breaks, tuple) and len(breaks) == 3 and all(torch.is_tensor(t) for t in breaks):
        first, tok, pause = (t.to(device=dev, dtype=d).contiguous() for t, d in zip(breaks, (torch.int32, torch.int32, torch.long)))
        if first.shape != (B + 1,) or tok.shape != pause.shape or tok.dim() != 1:
            raise ValueError(f"breaks as a CSR are (first [{B + 1}], token [NB], pause [NB])")
        NB = int(tok.numel())
        if out_ld is None or pause_max is None:
            raise ValueError("token_marks: breaks as device tensors need out_ld= and pause_max=")
        if NB == 0:
            first = tok = pause = None
    elif breaks is not None:
        if len(breaks) != B:
            raise ValueError(f"breaks need one row per utterance ({B}), got {len(breaks)}")
        pause_max = int(round(PAUSE_MAX_MS * SAMPLE_RATE / 1000.0)) if pause_max is None else int(pause_max)
        rows = [check_breaks(r, None, pause_max, f"breaks[{b}]") for b, r in enumerate(breaks)]
        csr = [0]
        for r in rows:
            csr.append(csr[-1] + len(r))
        NB = csr[-1]
        if NB:
            first = torch.tensor(csr, dtype=torch.int32).to(dev)
            tok = torch.tensor([t for r in rows for t, _ in r], dtype=torch.int32).to(dev)
            pause = torch.tensor([int(round(p)) for r in rows for _, p in r], dtype=torch.long).to(dev)
            extra = max(sum(int(round(p)) for _, p in r) for r in rows)
    pause_max = 0 if pause_max is None else int(pause_max)
    if out_ld is None:
        if NB and keep_max >= 1 << 40:
            raise ValueError("token_marks: breaks need keep_max= (the row stride of the audio they are cut into) or out_ld=")
        out_ld = keep_max + extra if NB else keep_max
    out_ld = max(4, (int(out_ld) + 3) // 4 * 4)
    marks = torch.empty(B, Tx, 2, dtype=torch.long, device=dev)
    lengths = torch.empty(B, dtype=torch.long, device=dev)
    ws = _timing_ws.get("timing", lib.mtts_token_timing_workspace_bytes(B, NB), dev)
    with torch.cuda.device(dev):
        _hip.check(lib.mtts_token_timing(_hip.ptr(cum), _hip.ptr(x_lengths), _hip.ptr(keep), B, Tx, int(fine_hop), keep_max, _hip.ptr(first),
                                         _hip.ptr(tok), _hip.ptr(pause), NB, pause_max, max(out_ld, keep_max), _hip.ptr(marks),
                                         _hip.ptr(lengths), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    plan = BreakPlan(ws=ws, first=first, B=B, NB=NB, out_ld=out_ld, lengths=lengths)
    if check:
        plan.raise_refused()
    return marks, lengths, plan


@torch.inference_mode()
def apply_breaks(audio, plan: BreakPlan, fade: int = 0):
    """The rows of ``audio`` [B, ld] (float32, as ``finish_waveforms`` leaves them) with the pauses of ``plan`` cut in
    (mtts_wave_breaks): row b of the result [B, plan.out_ld] holds the segments between its cuts in order, the zeros of a pause after
    each applied cut -- ``fade`` samples faded on both sides of it, by the join's rule -- and zeros from ``plan.lengths[b]`` on.  Rows
    without breaks are copied bit for bit.  ``plan`` must be the latest ``token_marks`` call of this stream."""
    lib = _hip.load()
    audio, _ = _hip.aligned_rows(audio, 4, "audio")
    B, ld = audio.shape
    if B != plan.B:
        raise ValueError(f"apply_breaks: the plan is of {plan.B} rows, audio has {B}")
    out_ld = max(4, (int(plan.out_ld) + 3) // 4 * 4)
    out = torch.empty(B, out_ld, dtype=torch.float32, device=audio.device)
    with torch.cuda.device(audio.device):
        _hip.check(lib.mtts_wave_breaks(_hip.ptr(audio), ld, _hip.ptr(plan.first), B, plan.NB, int(fade), _hip.ptr(out), out_ld,
                                        plan.ws.data_ptr(), plan.ws.numel(), _hip.stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------------ words (host, after the copy)
def word_groups(symbols: Sequence[str], space: str = " ") -> List[int]:
    """The word of each token of the phonemizer's ``separated`` symbol list: tokens between space symbols form a word (numbered from
    0 in speaking order); a space symbol itself is in none (-1)."""
    groups, word, open_ = [], -1, False
    for s in symbols:
        if s == space or (isinstance(s, str) and s != "" and s.strip() == ""):
            groups.append(-1)
            open_ = False
            continue
        if not open_:
            word += 1
            open_ = True
        groups.append(word)
    return groups


def word_marks(marks_row: Sequence[Tuple[float, float]], groups: Sequence[int]) -> List[Tuple[float, float]]:
    """``[(start, end)]`` per word from one row's token marks: the start of a word's first token and the end of its last.  Tokens of
    group -1 (and tokens the marks do not cover) belong to no word."""
    spans: dict = {}
    for (start, end), g in zip(marks_row, groups):
        if g is None or g < 0:
            continue
        if g in spans:
            spans[g] = (spans[g][0], end)
        else:
            spans[g] = (start, end)
    return [spans[g] for g in sorted(spans)]


def marks_rows(marks_host, n_rows: Optional[int] = None, offsets: Optional[Sequence[int]] = None) -> List[List[Tuple[float, float]]]:
    """The host copy of a marks tensor [B, Tx, 2] as ``[(start_s, end_s)]`` per row in seconds at 24 kHz, ``offsets[b]`` samples added
    (a row's start inside its document); a row ends at its first -1."""
    rows = marks_host.tolist()
    out = []
    for b, row in enumerate(rows[:n_rows]):
        off = 0 if offsets is None else int(offsets[b])
        out.append([((s + off) / SAMPLE_RATE, (e + off) / SAMPLE_RATE) for s, e in row if s >= 0])
    return out


# ------------------------------------------------------------------------------------------------ captions
def _stamp(t: float, sep: str) -> str:
    ms = int(round(max(float(t), 0.0) * 1000.0))
    h, ms = divmod(ms, 3600000)
    m, ms = divmod(ms, 60000)
    s, ms = divmod(ms, 1000)
    return f"{h:02d}:{m:02d}:{s:02d}{sep}{ms:03d}"


def _cue_text(text) -> str:
    return " ".join(str(text).replace("-->", "->").split())


def webvtt(cues) -> str:
    """``[(start_s, end_s, text)]`` as a WebVTT document (one cue each, in the order given)."""
    lines = ["WEBVTT", ""]
    for start, end, text in cues:
        lines += [f"{_stamp(start, '.')} --> {_stamp(end, '.')}", _cue_text(text), ""]
    return "\n".join(lines)


def srt(cues) -> str:
    """``[(start_s, end_s, text)]`` as a SubRip document (cues numbered from 1)."""
    lines = []
    for n, (start, end, text) in enumerate(cues, 1):
        lines += [str(n), f"{_stamp(start, ',')} --> {_stamp(end, ',')}", _cue_text(text), ""]
    return "\n".join(lines)

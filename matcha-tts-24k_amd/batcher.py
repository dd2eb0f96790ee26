"""Dynamic batching in front of ``MatchaTTSInfer.synthesise``.

The reference server handles one request at a time on the event-loop thread (server.py:93-127).  On an MI355X one request
uses a few percent of the chip (batch sweep), so a serving process wants to run whatever is waiting as
ONE ragged batch -- without changing any request's audio.  ``per_request_padding`` (inference.py) makes that exact: each row
of the batch equals the batch-of-one result (to rounding: tile shapes, hence summation order, depend on the grid).

``FrameBudgetBatcher`` is the queue + grouping policy:
  * requests are grouped by what must be uniform inside one call (solver, n_timesteps); voices, their duration scale
    corrections, client speeds and given durations are per-utterance inputs (mtts_durations_per_utterance, mtts_durations_given);
  * a batch takes the oldest waiting request and then the waiting requests of the same group that are closest to it in token
    count (padding wastes MFMA work: the estimator's cost is ~linear in padded frames), up to ``max_batch`` utterances and
    ``max_tokens`` padded tokens (B * longest), the frame budget idea of the reference's training sampler
    (text_mel_datamodule.py:111-154) applied to inference;
  * one worker thread drives the model (the HIP context is not re-entrant: model.decoder.solver is per-call state).

The class is transport-agnostic: an HTTP handler submits and awaits the future (``submit(...).result()``), see INTEGRATION.md.

``StepBatcher`` (below, opt-in) has the same contract and schedules at the solver step instead of the request: requests join a
running ODE solve at the next step and leave after their last one (include/mtts.h mtts_cfm_step).
"""
from __future__ import annotations

import os
import threading
import time
from concurrent.futures import Future
from dataclasses import KW_ONLY, dataclass, field, fields
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch


@dataclass
class _Unit:
    """What a unit of the queue -- a ``Request`` or a ``Document`` -- wants out, declared and checked once; keyword-only, so the fields of
    a unit itself come first.  A document's rows are requests too: what THEY say here is not looked at."""
    _: KW_ONLY
    sample_rate: int = 24000                # rate of the result's "audio" (with a vocoder); anything else is converted on the device and named in the result
    encoding: Optional[str] = None          # "pcm16" / "ulaw" / "alaw": the result's "audio" is then raw bytes (a 1-D uint8 tensor) encoded on the device, and named in the result; "flac": one complete FLAC stream (audio_codec.encode_flac)
    dither: bool = False                    # TPDF dither on a "pcm16" result
    dither_key: int = 0                     # selects the dither sequence: a field of the unit, so its bytes do not depend on who shared its batch
    flac_lpc: int = 0                       # a "flac" result also tries linear prediction up to this order (1..12; audio_codec.encode_flac(lpc_order=)): fewer bytes, the same words; a value without encoding="flac" is refused
    loudness: Optional[float] = None        # target in LUFS (BS.1770 integrated loudness) the "audio" -- of a document: the JOINED audio, one gain -- is brought to on the device at 24 kHz; the result then carries "loudness" (measured, before the gain) and "gain"
    true_peak: Optional[float] = None       # ceiling in dBTP on the true peak of the levelled "audio" (needs ``loudness``); the result then also carries "true_peak" (dBTP, measured before the gain) and "lra"
    marks: bool = False                     # the result then carries "marks": {"tokens": [(start_s, end_s)] per token -- of a document: one such list per sentence, in its timeline -- (+ "words" with ``word_groups``)}, in seconds at 24 kHz
    future: Future = field(default_factory=Future, repr=False)
    t_submit: float = field(default_factory=time.monotonic, repr=False)

    def __post_init__(self):                # (a wrong field fails its own unit here, not the batch it would have joined)
        if self.encoding is not None:
            from .audio_codec import encoding_id
            encoding_id(self.encoding)
        if self.flac_lpc != 0 or isinstance(self.flac_lpc, bool):
            from .audio_codec import FLAC, encoding_id, flac_lpc_order
            flac_lpc_order(self.flac_lpc)
            if self.encoding is None or encoding_id(self.encoding) != FLAC:
                raise ValueError(f"flac_lpc = {self.flac_lpc} belongs to encoding=\"flac\", got encoding={self.encoding!r}")
        if self.loudness is not None or self.true_peak is not None:
            from .loudness import check_ceiling, check_target
            self.loudness = check_target(self.loudness)
            self.true_peak = check_ceiling(self.true_peak, self.loudness)


OUTPUT_FIELDS = tuple(f.name for f in fields(_Unit) if f.repr)     # sample_rate ... marks: all but the queue's own two


@dataclass
class Request(_Unit):
    ids: Sequence[int]                      # phoneme ids of one utterance
    speaker: int = 0
    voice_mix: Optional[Sequence[Tuple[int, float]]] = None    # [(id, weight), ...] as reference server.py:96-101; overrides speaker
    speaker_embedding: Optional[Tuple[torch.Tensor, torch.Tensor]] = None   # (e_enc, e_dur) rows of an enrolled voice (enroll_voice); overrides both
    solver: str = "midpoint"
    n_timesteps: int = 4
    scale_correction: float = 1.0
    length_scale: float = 1.0
    durations: Optional[Sequence[float]] = None    # fine frames per token (e.g. ``align(...)["durations"]``) instead of the predictor's; length_scale still applies
    token_scale: Optional[Sequence[float]] = None    # a rate per token, inside [0, 16]: its duration is multiplied by it (exactly 0 drops the token)
    token_extend: Optional[Sequence[float]] = None   # fine frames added to each token's duration, inside [-4096, 4096]
    breaks: Optional[Sequence[Tuple[int, float]]] = None    # [(token, pause_ms), ...]: a pause cut into the audio after that token; token indices strictly increase
    word_groups: Optional[Sequence[int]] = None      # the word of each token (-1: none; ``timing.word_groups``): "marks" then has "words" too

    def __post_init__(self):
        if self.token_scale is not None or self.token_extend is not None or self.breaks is not None or self.word_groups is not None:
            from .timing import check_breaks, check_shaping
            for name in ("token_scale", "token_extend", "word_groups"):
                v = getattr(self, name)
                if v is not None and len(v) != len(self.ids):
                    raise ValueError(f"a request's {name} needs one value per token ({len(self.ids)}), got {len(v)}")
            check_shaping(None if self.token_scale is None else list(self.token_scale), "token_scale")
            check_shaping(None if self.token_extend is None else list(self.token_extend), "token_extend")
            if self.breaks is not None:
                self.breaks = check_breaks(self.breaks, len(self.ids), what="a request's breaks")
        super().__post_init__()

    @property
    def group(self) -> Tuple[Any, ...]:
        return (self.solver, int(self.n_timesteps))


def duration_rows(batch: List[Request]) -> Optional[List[Optional[Sequence[float]]]]:
    """What ``synthesise(durations=...)`` takes for a batch: one entry per request (None = the predictor), or None when no request
    brings durations.  Pure function: unit-tested on the CPU."""
    if all(r.durations is None for r in batch):
        return None
    for r in batch:
        if r.durations is not None and len(r.durations) != len(r.ids):
            raise ValueError(f"a request's durations need one value per token ({len(r.ids)}), got {len(r.durations)}")
    return [r.durations for r in batch]


def shaping_kwargs(rows: List[Request], units: Optional[List[Any]] = None) -> Dict[str, Any]:
    """The keyword arguments token timing adds to a ``synthesise`` call over ``rows``; none when nobody asks anything (the call is then
    exactly the one made before there was a choice).  ``token_scale`` / ``token_extend``: one entry per row (None = leave it alone), when
    a row names one; ``return_timing`` when a row has a break or a unit (by default the rows are the units) wants its marks: the tail
    then needs ``token_ends``.  Pure function: unit-tested on the CPU."""
    kw = {}
    for name in ("token_scale", "token_extend"):
        vals = [getattr(r, name) for r in rows]
        if any(v is not None for v in vals):
            kw[name] = vals
    if any(r.breaks for r in rows) or any(u.marks for u in (rows if units is None else units)):
        kw["return_timing"] = True
    return kw


def plan_batch(waiting: List[Request], max_batch: int, max_tokens: int) -> List[int]:
    """Indices (into ``waiting``, which is in arrival order) of the next batch.  Pure function: unit-tested on the CPU."""
    if not waiting:
        return []
    head = waiting[0]
    n0 = len(head.ids)
    same = [i for i, r in enumerate(waiting) if i > 0 and r.group == head.group]
    same.sort(key=lambda i: (abs(len(waiting[i].ids) - n0), i))     # nearest in length first, then oldest
    chosen, longest = [0], n0
    for i in same:
        if len(chosen) >= max_batch:
            break
        cand = max(longest, len(waiting[i].ids))
        if cand * (len(chosen) + 1) > max_tokens:
            continue
        chosen.append(i)
        longest = cand
    return sorted(chosen)


@dataclass
class Document(_Unit):
    """A text longer than one utterance: its sentences as ``rows`` (one ``Request`` each, in speaking order; what they say about the
    output -- rate, encoding, dither, level, marks -- is not looked at: the document says it once, for the joined audio) and the pause
    after each.  The rows run as rows of ONE ragged batch and are joined on the device (``inference.to_waveforms(documents=...)``);
    the document has one future and one result."""
    rows: List[Request]
    pauses_ms: Sequence[float]              # silence after each row; the last entry is ignored
    level: str = "document"                 # "document": one gain for the whole text; "sentence": each row keeps its own

    def __post_init__(self):
        super().__post_init__()
        if len(self.rows) == 0:
            raise ValueError("a document has at least one segment")
        if any(len(r.ids) == 0 for r in self.rows):
            raise ValueError("empty segment in a document")
        if len(self.pauses_ms) != len(self.rows):
            raise ValueError(f"a document's pauses need one value per segment ({len(self.rows)}), got {len(self.pauses_ms)}")
        if any(float(p) < 0 for p in self.pauses_ms):
            raise ValueError("a pause is not negative")
        if self.level not in ("document", "sentence"):
            raise ValueError(f"level is 'document' or 'sentence', got {self.level!r}")
        if len({r.group for r in self.rows}) != 1:
            raise ValueError("the rows of a document share solver and n_timesteps")

    @property
    def group(self) -> Tuple[Any, ...]:
        return self.rows[0].group

    def gaps(self, sample_rate: int = 24000) -> List[int]:
        """The pauses in samples of the join (which runs at the model's 24 kHz)."""
        return [int(round(float(p) * sample_rate / 1000.0)) for p in self.pauses_ms]


def unit_rows(unit) -> List[Request]:
    """The rows a unit of the queue -- a ``Request`` or a ``Document`` -- adds to a batch."""
    return list(unit.rows) if isinstance(unit, Document) else [unit]


def _unit_size(unit) -> Tuple[int, int]:
    """(rows, tokens of the longest row) of a unit."""
    if isinstance(unit, Document):
        return len(unit.rows), max(len(r.ids) for r in unit.rows)
    return 1, len(unit.ids)


def plan_units(waiting: List[Any], max_batch: int, max_tokens: int) -> List[int]:
    """``plan_batch`` over units -- a ``Request`` or a ``Document`` with its rows: indices (into ``waiting``, arrival order) of the next
    batch.  The head unit is taken whole; then the units of its group, nearest to it in the token count of their longest row first,
    each whole or not at all, while the rows stay within ``max_batch`` and rows x longest within ``max_tokens``.  On a queue without
    documents this is ``plan_batch``'s answer.  Pure function: unit-tested on the CPU."""
    if not waiting:
        return []
    rows, longest = _unit_size(waiting[0])
    n0 = longest
    same = [i for i, u in enumerate(waiting) if i > 0 and u.group == waiting[0].group]
    same.sort(key=lambda i: (abs(_unit_size(waiting[i])[1] - n0), i))
    chosen = [0]
    for i in same:
        if rows >= max_batch:
            break
        n, own = _unit_size(waiting[i])
        cand = max(longest, own)
        if rows + n > max_batch or cand * (rows + n) > max_tokens:
            continue
        chosen.append(i)
        rows, longest = rows + n, cand
    return sorted(chosen)


class _Queue:
    """The producer side the two batchers share: the waiting units under one condition, ``submit``'s checks, ``close`` and the context
    manager.  A batcher sets its own state, then ``_open``s -- which starts its worker, ``_loop`` -- last."""

    def _open(self, model, vocoder, max_batch: int, max_tokens: int, name: str) -> None:
        self.model = model
        self.vocoder = vocoder
        self.wave_batch = os.environ.get("MTTS_WAVE_BATCH", "1") != "0"      # (read here, per batcher)
        self.max_batch = int(max_batch)
        self.max_tokens = int(max_tokens)
        self._waiting: List[Any] = []
        self._cv = threading.Condition()
        self._stop = False
        self.batches_run = 0
        self.busy_s = 0.0                   # wall time the worker spent inside batches (device work + its host side): a load gauge
        self._thread = threading.Thread(target=self._loop, name=name, daemon=True)
        self._thread.start()

    def _request(self, ids: Sequence[int], fields: Dict[str, Any]) -> Request:
        """The checked ``Request`` of a ``submit``: a wrong one fails here, not the batch it would have joined."""
        if len(ids) == 0:
            raise ValueError("empty utterance")
        if len(ids) > self.max_tokens:
            raise ValueError(f"utterance of {len(ids)} tokens exceeds the batch budget of {self.max_tokens}")
        r = Request(ids=list(ids), **fields)
        duration_rows([r])
        return r

    def _enqueue(self, unit) -> Future:
        with self._cv:
            if self._stop:
                raise RuntimeError("batcher is closed")
            self._waiting.append(unit)
            self._cv.notify()
        return unit.future

    def close(self) -> None:
        """Stop taking requests; everything submitted before is served."""
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FrameBudgetBatcher(_Queue):
    """``submit()`` from any thread; results arrive on the request's future as ``{"mel": [n_feats, T_b], "mel_length": T_b}``."""

    def __init__(self, model, max_batch: int = 32, max_tokens: int = 8192, max_wait_ms: float = 2.0,
                 run_batch: Optional[Callable[[List[Request]], List[Dict[str, Any]]]] = None, vocoder=None, fade_ms: float = 5.0):
        """``vocoder``: a ``load_vocoder("vocos")`` object; results then also carry ``"audio"`` = the reference handler's
        ``trim_trailing_silence(to_waveform(mel, vocoder))`` (reference inference.py:246, server.py:116) of that request's own
        mel.  The whole batch goes through ``inference.to_waveforms`` (ragged decode + finish on the device, one copy, one
        synchronisation); ``MTTS_WAVE_BATCH=0``, read here per batcher, restores the per-request loop on exact-length mels.
        ``fade_ms``: the fade at the joints between the sentences of a document (``submit_document``)."""
        self.fade_ms = float(fade_ms)
        self.max_wait = float(max_wait_ms) / 1e3
        self._run = run_batch or self._run_on_model
        self._open(model, vocoder, max_batch, max_tokens, "mtts-batcher")

    # ------------------------------------------------------------------ producer side
    def submit(self, ids: Sequence[int], **kw) -> Future:
        return self._enqueue(self._request(ids, kw))

    def submit_document(self, segments_ids: Sequence[Sequence[int]], pauses_ms: Sequence[float], **request_fields) -> Future:
        """A text of several utterances: ``segments_ids`` the phoneme ids of each segment in speaking order, ``pauses_ms`` the silence
        after each (the last is ignored).  ``request_fields``: the fields of a ``Request`` -- voice, solver, speeds apply to every
        segment; ``sample_rate`` / ``encoding`` / ``dither`` / ``dither_key`` / ``flac_lpc`` / ``loudness`` / ``true_peak`` to the joined result -- and ``level`` (``Document``).
        ``marks`` (of the joined result) asks for ``"marks"``: ``{"tokens": one list of (start_s, end_s) per segment}`` in the document's
        timeline, ``"words"`` too when every segment brings ``word_groups``.  ``breaks`` / ``token_scale`` / ``token_extend`` /
        ``word_groups`` differ from segment to segment: each is a list of one entry (or None) per segment, as the ``Request`` field.
        The segments run as rows of one ragged batch, together with whatever else is waiting, and are joined on the device.  One
        future: ``{"audio", "segments": [(start_s, end_s)] per segment, "mel_lengths"}``, plus ``"sample_rate"`` / ``"encoding"``
        when asked.  A document is admitted whole or not at all: more segments than ``max_batch`` or segments x longest above
        ``max_tokens`` raises ``ValueError`` here, as does an empty segment."""
        once = {k: request_fields.pop(k) for k in ("level", *OUTPUT_FIELDS) if k in request_fields}
        segments = [list(ids) for ids in segments_ids]
        if any(len(ids) == 0 for ids in segments):
            raise ValueError("empty segment in a document")
        # what differs from sentence to sentence rides per row: a list of one entry (or None) per segment
        per_row = {k: request_fields.pop(k) for k in ("breaks", "token_scale", "token_extend", "word_groups") if k in request_fields}
        for k, v in per_row.items():
            if v is not None and len(v) != len(segments):
                raise ValueError(f"a document's {k} need one entry per segment ({len(segments)}), got {len(v)}")
        rows = [Request(ids=ids, **request_fields, **{k: v[i] for k, v in per_row.items() if v is not None})
                for i, ids in enumerate(segments)]
        d = Document(rows=rows, pauses_ms=[float(p) for p in pauses_ms], **once)
        duration_rows(d.rows)
        n, longest = _unit_size(d)
        if n > self.max_batch:
            raise ValueError(f"a document of {n} segments exceeds the batch of {self.max_batch} utterances")
        if n * longest > self.max_tokens:
            raise ValueError(f"a document of {n} segments of up to {longest} tokens exceeds the batch budget of {self.max_tokens}")
        return self._enqueue(d)

    # ------------------------------------------------------------------ worker
    def _loop(self) -> None:
        while True:
            with self._cv:
                while not self._waiting and not self._stop:
                    self._cv.wait()
                if self._stop and not self._waiting:
                    return
                # give concurrent submitters a moment to arrive, bounded by the oldest request's age
                deadline = self._waiting[0].t_submit + self.max_wait
                while sum(_unit_size(u)[0] for u in self._waiting) < self.max_batch and not self._stop:     # (rows: a document counts its own)
                    left = deadline - time.monotonic()
                    if left <= 0:
                        break
                    self._cv.wait(left)
                take = plan_units(self._waiting, self.max_batch, self.max_tokens)
                batch = [self._waiting[i] for i in take]
                for i in reversed(take):
                    del self._waiting[i]
            t_run = time.monotonic()
            try:
                results = self._run(batch)
                self.busy_s += time.monotonic() - t_run
                for r, res in zip(batch, results):
                    r.future.set_result(res)
            except BaseException as e:  # noqa: BLE001 - every waiter must be released
                for r in batch:
                    if not r.future.done():
                        r.future.set_exception(e)
            self.batches_run += 1

    def _run_on_model(self, batch: List[Request]) -> List[Dict[str, Any]]:
        return synthesise_batch(self.model, batch, self.vocoder, self.wave_batch, self.fade_ms)


def request_inputs(model, batch: List[Request]):
    """Padded ids, lengths and speaker rows of a batch of requests on the model's device."""
    dev = next(iter(model.state_dict().values())).device       # where load_matcha / .to() put the model
    B, n_max = len(batch), max(len(r.ids) for r in batch)
    x = torch.zeros(B, n_max, dtype=torch.long)
    for b, r in enumerate(batch):
        x[b, :len(r.ids)] = torch.as_tensor(r.ids, dtype=torch.long)
    x_len = torch.tensor([len(r.ids) for r in batch], dtype=torch.long)
    emb = model.speaker_rows([tuple(r.speaker_embedding) if r.speaker_embedding is not None else
                              list(r.voice_mix) if r.voice_mix is not None else r.speaker for r in batch])
    return x.to(dev), x_len.to(dev), emb


def tail_options(units: List[Any], timing=None, fade_ms: float = 5.0) -> Dict[str, Any]:
    """The keyword arguments of ``waveform.tail`` for a batch of units (``Request | Document``), one entry per unit.  A stage's keywords
    appear only when a unit asks for that stage -- another rate, an encoding, a loudness target (a unit without one passes None: its
    row is measured with a NaN target and keeps its bits), a true-peak ceiling -- so a batch in which nobody asks makes exactly the
    call made before there was a choice.  ``timing``: None, or ``(token_ends, x_lengths)`` of the ``synthesise`` call that was asked for
    them (``shaping_kwargs``): the timing plan then runs, with the rows' breaks.  Only a batch that holds a ``Document`` goes through
    the join: a plain request is a document of one row there (no joint, its own gain: its samples are its batch-of-one samples).
    Pure function: unit-tested on the CPU."""
    asked = lambda name: any(getattr(u, name) is not None for u in units)
    kw: Dict[str, Any] = {}
    if any(int(u.sample_rate) != 24000 for u in units):
        kw.update(sample_rate=[int(u.sample_rate) for u in units])
    if asked("encoding"):
        kw.update(encoding=[u.encoding for u in units], dither=[bool(u.dither) for u in units], dither_keys=[int(u.dither_key) for u in units])
        orders = [int(u.flac_lpc) for u in units]
        if any(orders):                     # per unit: a stream's bytes do not depend on who shared its batch
            kw.update(flac_lpc=orders)
    if asked("loudness"):                   # (a report alone would run the meter: it is asked for only where a unit is levelled)
        kw.update(loudness=[u.loudness for u in units], return_loudness=True)
        if asked("true_peak"):
            kw.update(true_peak=[u.true_peak for u in units], return_meter=True)
    if timing is not None:
        breaks = [list(r.breaks) if r.breaks else None for u in units for r in unit_rows(u)]
        kw.update(token_ends=timing[0], x_lengths=timing[1], breaks=breaks if any(breaks) else None, return_marks=True)
    if any(isinstance(u, Document) for u in units):
        kw.update(documents=[len(unit_rows(u)) for u in units], gaps=[g for u in units for g in (u.gaps() if isinstance(u, Document) else [0])],
                  level=[u.level if isinstance(u, Document) else "sentence" for u in units], fade_ms=fade_ms, return_segments=True)
    return kw


def results_into(res: List[Dict[str, Any]], units: List[Any], out) -> None:
    """What a ``Tail`` leaves in the result of each unit: ``"audio"``; a document's ``"segments"``; ``"sample_rate"`` / ``"encoding"`` when
    the unit named one; for a levelled unit ``"loudness"`` (LUFS before the gain) and ``"gain"`` from its report -- a ``(lufs, gain)`` pair
    or the meter's dict -- and, under its own ceiling, ``"true_peak"`` (dBTP, before the gain) and ``"lra"``; ``"marks"`` when it asked:
    ``{"tokens"}`` -- one list for a request, one per sentence for a document -- with ``"words"`` when its rows bring ``word_groups``.
    A float result at 24 kHz that asked nothing keeps exactly the keys it had before there was a choice."""
    from .loudness import dbtp
    from .timing import word_marks
    for g, (r, u) in enumerate(zip(res, units)):
        r["audio"] = out.rows[g]
        if isinstance(u, Document):
            r["segments"] = out.segments[g]
        if int(u.sample_rate) != 24000:
            r["sample_rate"] = int(u.sample_rate)
        if u.encoding is not None:
            r["encoding"] = u.encoding
        rep = None if out.report is None else out.report[g]
        if u.loudness is not None and rep is not None:
            metered = isinstance(rep, dict)
            r["loudness"], r["gain"] = (float(rep["lufs"]), float(rep["gain"])) if metered else (float(rep[0]), float(rep[1]))
            if metered and u.true_peak is not None:
                r["true_peak"], r["lra"] = dbtp(rep["true_peak"]), float(rep["lra"])
        if u.marks and out.marks is not None:
            rows, tokens = unit_rows(u), out.marks[g] if out.segments is not None else [out.marks[g]]      # (behind the join: per row of the unit)
            marks = {"tokens": tokens}
            if all(row.word_groups is not None for row in rows):
                marks["words"] = [word_marks(t, row.word_groups) for t, row in zip(tokens, rows)]
            r["marks"] = marks if isinstance(u, Document) else {k: v[0] for k, v in marks.items()}


def waveforms_into(res: List[Dict[str, Any]], mel, mel_lengths, vocoder, wave_batch: bool, units: List[Any], timing=None,
                   fade_ms: float = 5.0) -> None:
    """The tail of a batch of finished mels (``mel`` [B, n_feats, T], ``mel_lengths`` [B]): ``res[g]["audio"]`` for every unit, in what
    the unit asks for (``tail_options``: rate, encoding, loudness, ceiling, marks; a document's rows joined) and with the keys that say
    so (``results_into``).  ``res[g]["mel"]``: the exact-length mel of a request.  ``wave_batch``: one ``waveform.tail`` call for the
    batch; without it the per-request loop (``waveform.finish_request`` on each request's own mel), which knows no join and no timing.
    Without a vocoder nothing is touched."""
    if vocoder is None:
        return
    if timing is not None and not wave_batch:
        raise ValueError("marks and breaks run in the batched tail: they need wave_batch=True")
    if wave_batch:
        from .waveform import tail
        out = tail(mel, mel_lengths, vocoder, **tail_options(units, timing, fade_ms))
    else:
        from .waveform import Tail, _waveform_on_device, finish_request, trim_trailing_silence
        done = [finish_request(trim_trailing_silence(_waveform_on_device(r["mel"][None], vocoder).squeeze()), loudness=u.loudness,
                               true_peak=u.true_peak, report=True, sample_rate=int(u.sample_rate), encoding=u.encoding, dither=bool(u.dither),
                               dither_key=int(u.dither_key), **(dict(flac_lpc=int(u.flac_lpc)) if u.flac_lpc else {})) for r, u in zip(res, units)]
        out = Tail(rows=[a for a, _ in done], report=[rep for _, rep in done])
    results_into(res, units, out)


def synthesise_batch(model, units: List[Any], vocoder=None, wave_batch: bool = True, fade_ms: float = 5.0) -> List[Dict[str, Any]]:
    """One ``synthesise(per_request_padding=True)`` call for the units of one group -- requests, and documents with their rows -- then
    one tail (``waveforms_into``), and one result per unit: ``{"mel", "mel_length"[, "audio", ...]}`` for a request, ``{"audio",
    "segments", "mel_lengths"[, ...]}`` for a document.  A request keeps exactly the keys and values it has without documents in its
    batch.  The join is part of the batched tail: there is no per-request loop for it, and no host-side join."""
    joined = any(isinstance(u, Document) for u in units)
    if joined and vocoder is None:
        raise ValueError("a document needs a vocoder: its result is the joined audio")
    rows = [r for u in units for r in unit_rows(u)]
    x, x_len, emb = request_inputs(model, rows)
    head = rows[0]
    model.decoder.solver = head.solver
    shaping = shaping_kwargs(rows, units)
    if vocoder is None and "return_timing" in shaping:
        raise ValueError("marks and breaks need a vocoder: they are positions in the audio")
    out = model.synthesise(x, x_len, head.n_timesteps, speaker_embeddings=emb,
                           scale_correction=[r.scale_correction for r in rows],
                           length_scale=[r.length_scale for r in rows], per_request_padding=True,
                           durations=duration_rows(rows), **shaping)
    lens = [int(v) for v in out["mel_lengths"].tolist()]
    res, b = [], 0
    for u in units:
        n = len(unit_rows(u))
        res.append({"mel_lengths": lens[b:b + n]} if isinstance(u, Document) else {"mel": out["mel"][b, :, :lens[b]], "mel_length": lens[b]})
        b += n
    waveforms_into(res, out["mel"], out["mel_lengths"], vocoder, wave_batch or joined, units,
                   (out["token_ends"], x_len) if "token_ends" in out else None, fade_ms)
    return res


# ====================================================================================================== step-level batching
# FrameBudgetBatcher schedules at the request: a batch is formed, its WHOLE solve runs, then the queue is looked at again -- a
# request that arrives just after a solve started waits for it, then runs nearly alone itself.  StepBatcher schedules at the
# solver step (the iteration of this model, 1-4 estimator evaluations): every iteration it admits who is waiting into free slots,
# advances everybody who is active by ONE step -- each request at its own point (t0, t1) of its own grid, include/mtts.h
# mtts_cfm_step -- and lets those leave that made their last step.  What a request gets back is unchanged: per-request padding
# makes a row of a ragged batch equal its batch-of-one result (to rounding), and with one time per utterance that holds for
# rows at different times too, so requests with different n_timesteps share launches (only the solver must be common).

def step_grid(n_timesteps: int) -> List[Tuple[float, float]]:
    """The ``(t0, t1)`` of a request's steps: neighbours of ``t_span = linspace(0, 1, n + 1)`` in fp32 as ``CFM.forward`` builds it
    (the values are exact fp32 numbers; ``dt = t1 - t0`` is taken in fp32 on the device, torchdiffeq's fixed-grid loop).  Pure."""
    if int(n_timesteps) < 1:
        raise ValueError("n_timesteps must be at least 1")
    t = torch.linspace(0, 1, int(n_timesteps) + 1, dtype=torch.float32).tolist()
    return list(zip(t[:-1], t[1:]))


class SlotBook:
    """Which slots of the pool are free; lowest index first, so a small pool region stays warm.  Pure bookkeeping."""

    def __init__(self, n_slots: int):
        self.n_slots = int(n_slots)
        self._free = list(range(self.n_slots))
        self._held: set = set()

    @property
    def n_free(self) -> int:
        return len(self._free)

    def take(self) -> int:
        if not self._free:
            raise RuntimeError("no free slot")
        s = min(self._free)
        self._free.remove(s)
        self._held.add(s)
        return s

    def release(self, slot: int) -> None:
        if slot not in self._held:
            raise RuntimeError(f"slot {slot} is not held")
        self._held.remove(slot)
        self._free.append(slot)


def plan_admission(waiting: List[Request], n_active: int, active_longest: int, n_free_slots: int, max_batch: int, max_tokens: int) -> List[int]:
    """Indices (into ``waiting``, arrival order) of the requests that join at this iteration: oldest first, while a slot is free, the
    active set stays within ``max_batch`` requests and within the ``max_tokens`` budget of padded tokens (requests x longest, as
    ``plan_batch``).  A request that does not fit the budget is skipped, not waited for, unless nothing is active (the head then
    always goes, alone if need be).  Pure function."""
    chosen: List[int] = []
    n, longest = int(n_active), int(active_longest)
    for i, r in enumerate(waiting):
        if len(chosen) >= n_free_slots or n >= max_batch:
            break
        cand = max(longest, len(r.ids))
        if n > 0 and cand * (n + 1) > max_tokens:
            continue
        chosen.append(i)
        n, longest = n + 1, cand
    return chosen


def next_solver(active_solvers: Sequence[str], last: Optional[str]) -> Optional[str]:
    """Round-robin over the solvers that have active requests: the one after ``last`` in sorted order.  Pure function."""
    names = sorted(set(active_solvers))
    if not names:
        return None
    later = [s for s in names if last is not None and s > last]
    return later[0] if later else names[0]


@dataclass
class StepEntry:
    """One active request: where its state lives and where it is on its grid."""
    request: Request
    slot: int
    grid: List[Tuple[float, float]]
    i: int = 0                       # steps done
    y_len: int = 0                   # valid mel frames
    t_len: int = 0                   # its own padded length (per-request padding)

    @property
    def t0(self) -> float:
        return self.grid[self.i][0]

    @property
    def t1(self) -> float:
        return self.grid[self.i][1]

    @property
    def done(self) -> bool:
        return self.i >= len(self.grid)


class StepBatcher(_Queue):
    """Same contract as ``FrameBudgetBatcher`` -- ``submit(ids, **kw) -> Future`` of ``{"mel", "mel_length"[, "audio"]}`` -- scheduled
    at the solver step.  One worker thread drives the model.  Per iteration: admit (text encoder, durations and ``align_pool`` of the
    newcomers as one small ragged batch, then into free slots), one step for all active requests of one solver (round-robin over
    solvers), and the requests that made their last step leave (mel read out, the finishers' waveforms as one ``to_waveforms``
    batch).  A request whose folded rows exceed ``slot_frames`` runs through ``synthesise`` as a batch of its own.

    ``run_step(solver, entries)`` replaces the device step (tests); admission and read-out then touch no device either."""

    def __init__(self, model, max_batch: int = 32, max_tokens: int = 16384, n_slots: Optional[int] = None, slot_frames: int = 2048,
                 run_step: Optional[Callable[[str, List[StepEntry]], None]] = None, vocoder=None):
        self.slot_frames = int(slot_frames)
        self.slots = SlotBook(int(n_slots) if n_slots is not None else int(max_batch))
        self._fake = run_step is not None
        self._run_step = run_step or self._step_on_model
        self._pool = None
        self._flags = None                  # device int32 [3]: encoder range flag, estimator range flag, pair time-out, OR-ed over calls
        self._active: List[StepEntry] = []
        self._last_solver: Optional[str] = None
        self.utterance_steps = 0            # requests x steps served: utterance_steps / batches_run (iterations that ran a step) = mean utterances per step
        self.whole_solves = 0               # requests that did not fit a slot
        self.phase_s = {"admit": 0.0, "step": 0.0, "leave": 0.0}     # where busy_s went (host wall time; "leave" holds the iteration's wait)
        self._open(model, vocoder, max_batch, max_tokens, "mtts-step-batcher")

    # ------------------------------------------------------------------ producer side
    def submit(self, ids: Sequence[int], **kw) -> Future:
        r = self._request(ids, kw)
        if shaping_kwargs([r]):
            raise ValueError("token_scale, token_extend, breaks and marks are served by FrameBudgetBatcher: the step-level admission "
                             "path does not take them")
        step_grid(r.n_timesteps)
        return self._enqueue(r)

    # ------------------------------------------------------------------ worker
    def _loop(self) -> None:
        with torch.inference_mode():        # (thread-local: everything the worker touches on the device is inference state)
            self._serve()

    def _serve(self) -> None:
        while True:
            with self._cv:
                while not self._waiting and not self._active and not self._stop:
                    self._cv.wait()
                if self._stop and not self._waiting and not self._active:
                    return
                longest = max((len(e.request.ids) for e in self._active), default=0)
                take = plan_admission(self._waiting, len(self._active), longest, self.slots.n_free, self.max_batch, self.max_tokens)
                newcomers = [self._waiting[i] for i in take]
                for i in reversed(take):
                    del self._waiting[i]
            t_run = time.monotonic()
            if newcomers:
                try:
                    self._active.extend(self._admit(newcomers))
                except BaseException as e:  # noqa: BLE001 - the newcomers' waiters must be released; who is mid-solve goes on
                    self._fail(newcomers, e)
            t_admitted = time.monotonic()
            self.phase_s["admit"] += t_admitted - t_run
            solver = next_solver([e.request.solver for e in self._active], self._last_solver)
            if solver is not None:
                entries = [e for e in self._active if e.request.solver == solver]
                try:
                    self._run_step(solver, entries)
                    t_stepped = time.monotonic()
                    self.phase_s["step"] += t_stepped - t_admitted
                    for e in entries:
                        e.i += 1
                    self.batches_run += 1
                    self.utterance_steps += len(entries)
                    self._last_solver = solver
                    finished = [e for e in entries if e.done]
                    if finished:
                        self._finish(finished)
                        self.phase_s["leave"] += time.monotonic() - t_stepped
                except BaseException as e:  # noqa: BLE001 - every waiter must be released: the pool's state is void
                    self._abort(e)
            self.busy_s += time.monotonic() - t_run

    @staticmethod
    def _fail(requests: List[Request], exc: BaseException) -> None:
        for r in requests:
            if not r.future.done():
                r.future.set_exception(exc)

    def _abort(self, exc: BaseException) -> None:
        """Fail every active request and free its slot."""
        self._fail([e.request for e in self._active], exc)
        for e in self._active:
            self.slots.release(e.slot)
        self._active = []

    def _leave(self, entries: List[StepEntry]) -> None:
        gone = {id(e) for e in entries}
        self._active = [e for e in self._active if id(e) not in gone]
        for e in entries:
            self.slots.release(e.slot)

    # ------------------------------------------------------------------ admission
    def _admit(self, newcomers: List[Request]) -> List[StepEntry]:
        if self._fake:
            return [StepEntry(r, self.slots.take(), step_grid(r.n_timesteps), y_len=len(r.ids), t_len=2 * len(r.ids)) for r in newcomers]
        return self._admit_on_model(newcomers)

    def _admit_on_model(self, newcomers: List[Request]) -> List[StepEntry]:
        from .inference import fix_len_compatibility
        model = self.model
        hip = model._rt.ready()
        x, x_len, (e_enc, e_dur) = request_inputs(model, newcomers)
        mu_x, logw, x_mask = model.encoder(x, x_len, e_enc, e_dur)
        sc, ls = [r.scale_correction for r in newcomers], [r.length_scale for r in newcomers]
        given = duration_rows(newcomers)
        if given is None:
            _, cum, y_fine = hip.durations(logw, x_mask, sc, ls)
        else:
            _, cum, y_fine = model._given_durations(hip, given, logw, x_mask, sc, ls)
        self._note_flags(hip, "enc")
        fine = [int(v) for v in y_fine.tolist()]                 # the one host read of an admission (as synthesise)
        t_pad = fix_len_compatibility(max(fine))
        mu_y, _, _ = hip.align_pool(mu_x, cum, y_fine, t_pad)
        if self._pool is None:
            self._pool = model.decoder.step_pool(self.slots.n_slots, self.slot_frames, mu_y.device)
        entries, oversize = [], []
        for b, r in enumerate(newcomers):
            y_len = max((fine[b] + 1) // 2, 1)                   # (align_pool's y_lengths)
            if model.decoder.step_rows(y_len) > self.slot_frames:
                oversize.append(r)
                continue
            e = StepEntry(r, self.slots.take(), step_grid(r.n_timesteps), y_len=y_len, t_len=fix_len_compatibility(max(fine[b], 1)))
            model.decoder.step_prepare(self._pool, e.slot, mu_y[b], e.t_len)
            entries.append(e)
        for r in oversize:                                       # longer than a slot: the whole-solve path, a batch of its own
            try:
                r.future.set_result(synthesise_batch(model, [r], self.vocoder, self.wave_batch)[0])
            except BaseException as exc:  # noqa: BLE001
                self._fail([r], exc)
            self.whole_solves += 1
        return entries

    # ------------------------------------------------------------------ one step
    def _step_on_model(self, solver: str, entries: List[StepEntry]) -> None:
        dec = self.model.decoder
        dec.step_advance(self._pool, [e.slot for e in entries], [e.t0 for e in entries], [e.t1 for e in entries],
                         [e.y_len for e in entries], [e.t_len for e in entries], solver=solver)
        self._note_flags(self.model._rt.ready(), "dec")

    def _note_flags(self, hip, kind: str) -> None:
        """OR this stream's latest call's header words into the batcher's sticky copy (a call clears its own flag when it begins); no
        synchronisation.  Nothing to note where the model's range guard has nothing to read (``Runtime.guards``)."""
        if not self._guarded():
            return
        w = hip.call_flags(kind)
        if w is None:
            return
        if self._flags is None:
            self._flags = torch.zeros(3, dtype=torch.int32, device=w.device)
        dst = self._flags[0:1] if kind == "enc" else self._flags[1:3]
        torch.maximum(dst, w[0:1] if kind == "enc" else w[0:2], out=dst)

    def _guarded(self) -> bool:
        return self.model._rt.guards(self.model.range_policy)

    # ------------------------------------------------------------------ leaving
    def _finish(self, finished: List[StepEntry]) -> None:
        if self._fake:
            self._leave(finished)
            for e in finished:
                e.request.future.set_result({"mel": None, "mel_length": e.y_len})
            return
        from .modules import PAIR_TIMEOUT_ERROR, RANGE_ERROR
        model, rt = self.model, self.model._rt
        hip = rt.ready()
        if self._guarded() and self._flags is not None:
            flags = self._flags.tolist()                         # the iteration's one synchronisation
            self._flags.zero_()
            if flags[2]:
                raise RuntimeError(PAIR_TIMEOUT_ERROR)
            if flags[0] or flags[1] or hip.weights_saturate():
                if model.range_policy == "raise":
                    raise FloatingPointError(RANGE_ERROR)
                # rerun: the model switches to the wide arithmetic (sticky, as Runtime.guarded) and everybody who is active starts over
                rt.use_wide = True
                again = [e.request for e in self._active]
                self._leave(list(self._active))
                with self._cv:
                    self._waiting[:0] = again
                return
        mel_std, mel_mean = rt.mel_std, rt.mel_mean
        res = []
        for e in finished:
            res.append({"mel": model.decoder.step_read(self._pool, e.slot, e.y_len, mel_std, mel_mean), "mel_length": e.y_len})
        self._leave(finished)
        if self.vocoder is not None:
            t_max = max(e.y_len for e in finished)
            mel = torch.zeros(len(finished), res[0]["mel"].shape[0], t_max, device=res[0]["mel"].device)
            for b, r in enumerate(res):
                mel[b, :, :r["mel_length"]] = r["mel"]
            lengths = torch.tensor([r["mel_length"] for r in res], dtype=torch.long, device=mel.device)
            try:
                waveforms_into(res, mel, lengths, self.vocoder, self.wave_batch, [e.request for e in finished])
            except BaseException as exc:  # noqa: BLE001 - the finishers only: who is mid-solve is not affected
                self._fail([e.request for e in finished], exc)
                return
        for e, r in zip(finished, res):
            e.request.future.set_result(r)

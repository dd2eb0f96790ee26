"""The waveform tail, for a batch with one synchronisation (``to_waveforms``) and for one request (``finish_request``): Vocos decode,
peak normalisation and trailing-silence trim (reference inference.py:246,260-287), then what a row asks for -- token timing and breaks,
the document join, loudness, rate conversion, encoding.  ``_resolve`` turns the keyword arguments into one ``_Plan`` before anything is
launched, ``tail`` runs the stages over ``(rows, lengths, plan)``, ``_ending`` makes the one copy that waits for the stream.
``inference`` re-exports the public names; this module does not import it."""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass
from typing import Any, Callable, Optional

import torch

from . import _hip, audio_codec as AC, loudness as LD, resample as R, timing as TM

SAMPLE_RATE = 24000
METER_FIGURES = ("lufs", "gain", "lra", "momentary_max", "short_term_max", "peak", "true_peak")
_finish_ws, _join_ws = _hip.Workspaces(), _hip.Workspaces()            # scratch of kernels that write every word they read


def _waveform_on_device(mel, vocoder):
    """Vocoder + peak normalisation of reference inference.py:260-264, left on the device."""
    audio = vocoder(mel)
    max_abs = audio.abs().max()
    if max_abs > 1.0:
        audio = audio / max_abs * 0.95
    return audio


@torch.inference_mode()
def finish_waveforms(audio, lengths, hop=0, silence_threshold_db=-60.0):
    """Peak normalisation (reference inference.py:260-264) and the trim length of ``trim_trailing_silence`` (reference
    inference.py:268-287) for every row of ``audio`` [B, L] on the device, in place, without a host synchronisation
    (``mtts_waveform_finish``).  ``lengths`` [B]: valid samples per row, or frames when ``hop`` is given (row b then has
    ``hop * (frames - 1)`` samples, as ``Vocos.decode(mel, lengths)`` leaves them).  Returns device tensors
    ``(out_lengths int64 [B], scale float32 [B])``: the caller keeps ``audio[b, :out_lengths[b]]``; -1 marks a row whose length
    is outside its row."""
    lib = _hip.load()
    if audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_cuda or not audio.is_contiguous():
        raise RuntimeError("finish_waveforms: audio must be a contiguous float32 [B, L] tensor on a HIP device")
    B, L = audio.shape
    lengths = _hip.row_lengths(lengths, B, L, audio.device)
    ws = _finish_ws.get("finish", lib.mtts_waveform_workspace_bytes(L, B, SAMPLE_RATE), audio.device)
    scale = torch.empty(B, dtype=torch.float32, device=audio.device)
    out_lengths = torch.empty(B, dtype=torch.long, device=audio.device)
    _hip.check(lib.mtts_waveform_finish(_hip.ptr(audio), L, _hip.ptr(lengths), int(hop), B, SAMPLE_RATE, float(silence_threshold_db),
                                        _hip.ptr(scale), _hip.ptr(out_lengths), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    return out_lengths, scale


def document_csr(documents, B, pad=False):
    """``documents`` -- a host list of row counts, or the CSR ``[0, n0, n0 + n1, ...]`` (it begins with 0, which no count can be) -- as
    the CSR list the device takes.  Counts are checked here (each at least 1, their sum ``B``); a CSR is passed on as it is, for the
    device to judge.  ``pad``: rows behind the last document become documents of one row each."""
    docs = [int(v) for v in (documents.tolist() if torch.is_tensor(documents) else documents)]
    if len(docs) == 0:
        raise ValueError("documents: no document")
    if docs[0] == 0:
        csr = docs
    else:
        if any(n < 1 for n in docs):
            raise ValueError("documents: a document has at least one row")
        csr = [0]
        for n in docs:
            csr.append(csr[-1] + n)
        if csr[-1] > B or (csr[-1] < B and not pad):
            raise ValueError(f"documents: the row counts add up to {csr[-1]}, the batch has {B} rows")
    if pad and len(csr) > 1 and 0 <= csr[-1] < B:
        csr = csr + list(range(csr[-1] + 1, B + 1))
    if len(csr) < 2:
        raise ValueError("documents: no document")
    return csr


@torch.inference_mode()
def join_waveforms(audio, lengths, documents, gaps, fade=0, scale=None, check=True, out_ld=None):
    """Finished rows joined into documents on the device (``mtts_wave_join``; include/mtts.h has the arithmetic): ``audio`` [B, ld]
    float32 and ``lengths`` [B] as ``finish_waveforms`` leaves them (a tensor stays on the device; -1 = refused row), ``documents`` a
    host list of row counts or a CSR (``document_csr``), ``gaps`` a host list of B sample counts (silence after each row; the entry
    of a document's last row is ignored; None: none), ``fade`` samples faded at each interior joint, ``scale`` the [B] gains of
    ``finish_waveforms`` (one gain per document) or None (every row keeps its own).  Returns device tensors ``(out [G, out_ld],
    out_lengths int64 [G], starts int64 [B])``: document g holds ``out_lengths[g]`` samples, zeros beyond; ``starts[b]`` is where row b
    begins inside its document.  ``out_ld`` defaults to the host-known bound ``max_g(rows_g * ld + gaps_g)``, rounded up to 4.
    Nothing is read on the host: a document with a refused row, a bad gap or no room gets length -1 and zeros, its rows start -1;
    with ``check`` the call waits for that verdict and raises ``ValueError`` naming the row and the reason."""
    lib = _hip.load()
    audio, L = _hip.aligned_rows(audio, 4, "audio")
    B, ld = audio.shape
    dev = audio.device
    lengths = _hip.row_lengths(lengths, B, L, dev)
    csr = document_csr(documents, B)
    G = len(csr) - 1
    gaps = [0] * B if gaps is None else [int(v) for v in (gaps.tolist() if torch.is_tensor(gaps) else gaps)]
    if len(gaps) != B:
        raise ValueError(f"gaps need one entry per row ({B}), got {len(gaps)}")
    if scale is not None:
        scale = scale.to(device=dev, dtype=torch.float32).contiguous()
        if scale.shape != (B,):
            raise ValueError(f"scale must have shape ({B},), got {tuple(scale.shape)}")
    if out_ld is None:
        out_ld = max((b - a) * ld + sum(max(v, 0) for v in gaps[max(a, 0):max(b - 1, 0)]) for a, b in zip(csr[:-1], csr[1:]))
    out_ld = max(4, (int(out_ld) + 3) // 4 * 4)
    first_row = torch.tensor(csr, dtype=torch.int32).to(dev)
    gap = torch.tensor(gaps, dtype=torch.long).to(dev)
    out = torch.empty(G, out_ld, dtype=torch.float32, device=dev)
    out_lengths = torch.empty(G, dtype=torch.long, device=dev)
    starts = torch.empty(B, dtype=torch.long, device=dev)
    ws = _join_ws.get("join", lib.mtts_wave_join_workspace_bytes(B, G), dev)
    with torch.cuda.device(dev):
        _hip.check(lib.mtts_wave_join(_hip.ptr(audio), ld, _hip.ptr(lengths), _hip.ptr(scale), _hip.ptr(first_row), _hip.ptr(gap), B, G,
                                      int(fade), max([0] + gaps), _hip.ptr(out), out_ld, _hip.ptr(out_lengths), _hip.ptr(starts),
                                      ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _hip.raise_refused(lib.mtts_wave_join_status, ws.data_ptr(), _hip.stream_ptr())
    return out, out_lengths, starts


def trim_trailing_silence(audio, silence_threshold_db=-60.0):
    """reference inference.py:268-287, window for window: 10 ms windows anchored at sample 0 (the ``len % window`` remainder is
    never examined), RMS per window, count the run of trailing windows with ``rms < threshold`` (strict; a NaN window stops the
    run as in the reference's loop), drop ``count * window`` samples from the END of the signal.  All full windows may go.
    Works on a 1-D tensor on any device: the window RMS and the run length are computed where the audio lives (one scalar
    comes back to the host), so ``pipeline`` trims before the device-to-host copy."""
    win = int(0.01 * SAMPLE_RATE)
    thr = 10 ** (silence_threshold_db / 20.0)
    n_full = len(audio) // win
    if n_full == 0:
        return audio
    rms = audio[: n_full * win].reshape(n_full, win).pow(2).mean(dim=1).sqrt()
    loud = torch.logical_not(rms < thr)
    idx = torch.arange(1, n_full + 1, device=audio.device)
    last_loud = int((loud * idx).max())            # 1-based index of the last window that is not silent; 0 = none
    trim = (n_full - last_loud) * win
    if trim == 0:
        return audio
    return audio[:-trim]


@dataclass
class _Plan:
    """What a ``to_waveforms`` call asks for, resolved and validated once, before anything is launched.  A per-result list has ``n``
    entries, or is None when no result asks for its stage: the stage is then not entered and nothing is allocated for it."""
    n: int                          # results: one per row, or per document when ``csr`` (the CSR the join takes) is given
    csr: Optional[list]
    gaps: Any
    fade: int                       # samples faded at a joint and at a cut
    levels: Optional[list]          # per document
    rates: list
    encs: Optional[list]            # format ids; None in a row that stays float (an encoder sees the rows of another with length 0)
    dither: Optional[list]
    keys: Any
    targets: Optional[list]         # LUFS; NaN: measure the row and leave it alone
    ceilings: Optional[list]        # dBTP or None
    meter: bool
    timed: bool
    break_rows: Optional[list]      # per ROW [(token, pause_samples)]
    segments: bool                  # what is returned beside the results
    report: bool
    marks: bool


def _spread(vals, one, n, what):
    """Per-row values that were validated on their own length as ``n`` of them: a value given once is repeated."""
    if vals is None or one:
        return None if vals is None else vals * n
    if len(vals) != n:
        raise ValueError(f"{what} is a number or one per row ({n}), got {len(vals)}")
    return vals


def _resolve(rows: Callable[[], int], *, encoding=None, dither=False, dither_keys=None, documents=None, gaps=None, fade_ms=5.0,
             level="document", return_segments=False, loudness=None, return_loudness=False, true_peak=None, return_meter=False,
             token_ends=None, x_lengths=None, breaks=None, return_marks=False, sample_rate=SAMPLE_RATE) -> _Plan:
    """The plan of ``to_waveforms(**options)``.  ``rows()`` gives the batch's row count: it looks at the mel, so it is asked only
    where a value cannot be judged without it -- a level, a target or a ceiling that is none raises before."""
    timed = token_ends is not None or breaks is not None or bool(return_marks)
    if timed and (token_ends is None or x_lengths is None):
        raise ValueError("to_waveforms: breaks and return_marks need token_ends= and x_lengths= (synthesise(return_timing=True))")
    if breaks is not None and len(breaks) != rows():
        raise ValueError(f"breaks need one entry per row ({rows()}), got {len(breaks)}")
    break_rows = None if breaks is None else [
        [(t, int(round(p * SAMPLE_RATE / 1000.0))) for t, p in TM.check_breaks(r, None, TM.PAUSE_MAX_MS, f"breaks[{b}]")]
        for b, r in enumerate(breaks)]
    if documents is None and (gaps is not None or return_segments):
        raise ValueError("to_waveforms: gaps and return_segments belong to documents=")
    # targets and ceilings are judged on their own length here and spread over the results once their number is known
    listed = [v for v in (true_peak, loudness) if v is not None and not isinstance(v, (int, float))]
    one_target = loudness is None or isinstance(loudness, (int, float))
    targets = None if loudness is None else LD.targets_per_row(loudness, 1 if one_target else len(loudness))
    n = len(listed[0]) if listed else 1                                # (a ceiling on a row without a target raises here)
    ceilings = None if true_peak is None else _true_peak_ceilings(true_peak, _spread(targets, one_target, n, "loudness"), n)
    if any(v not in ("document", "sentence") for v in ([level] if isinstance(level, str) else level)):
        raise ValueError(f"to_waveforms: level is 'document' or 'sentence' (or one of them per document), got {level!r}")
    csr = None if documents is None else document_csr(documents, rows(), pad=True)
    n = rows() if csr is None else len(csr) - 1
    rates = R.rates_per_row(sample_rate, n)
    encs = _encodings_per_row(encoding, n)                             # (an unknown name raises before anything is launched)
    report = bool(return_loudness or return_meter)
    targets = _spread(targets, one_target, n, "loudness")
    if targets is None and report:                                     # a report alone: every row is measured and left alone
        targets = [math.nan] * n
    levels = None if csr is None else [level] * n if isinstance(level, str) else list(level)
    if csr is not None and len(levels) != n:
        raise ValueError(f"level is a name or one per document ({n}), got {len(levels)}")
    on = None if encs is None else [bool(dither)] * n if isinstance(dither, (bool, int)) else [bool(v) for v in dither]
    return _Plan(n=n, csr=csr, gaps=gaps, fade=int(round(float(fade_ms) * SAMPLE_RATE / 1000.0)), levels=levels, rates=rates, encs=encs,
                 dither=on, keys=dither_keys, targets=targets, ceilings=_spread(ceilings, not listed, n, "true_peak"),
                 meter=bool(return_meter), timed=timed, break_rows=break_rows, segments=bool(return_segments), report=report,
                 marks=bool(return_marks))


def _flac_orders(flac_lpc, plan):
    """``flac_lpc=`` of ``tail`` as ``lpc_order`` per result, 0 where a row is no stream; None when every one is 0.  A value that
    is no order, and an order where no FLAC row takes it, raise here, before anything is launched."""
    one = not isinstance(flac_lpc, (list, tuple))
    orders = _spread([AC.flac_lpc_order(v) for v in ([flac_lpc] if one else flac_lpc)], one, plan.n, "flac_lpc")
    streamed = [plan.encs is not None and e == AC.FLAC for e in (plan.encs or [None] * plan.n)]
    if one and orders[0] and not any(streamed):
        raise ValueError(f"tail: flac_lpc = {flac_lpc} belongs to encoding=\"flac\", and no row names it")
    if not one and any(o and not on for o, on in zip(orders, streamed)):
        raise ValueError(f"tail: flac_lpc = {list(flac_lpc)} names an order on a row whose encoding is not \"flac\"")
    orders = [o if on else 0 for o, on in zip(orders, streamed)]
    return orders if any(orders) else None


def _true_peak_ceilings(true_peak, targets, n):
    """``true_peak=`` of ``to_waveforms`` as n ceilings in dBTP or None per row; None when no row names one.  A value that is no
    ceiling, and a ceiling on a row without a loudness target, raise here, before anything is launched."""
    if isinstance(true_peak, (int, float)) and not isinstance(true_peak, bool):
        c = LD.check_true_peak(true_peak)                              # one ceiling for the call: it binds the rows that have a target
        vals = [c if t == t else None for t in (targets or [math.nan] * n)]
        if all(v is None for v in vals):
            raise ValueError("to_waveforms: true_peak limits the gain towards a loudness target, and no row names one (loudness=)")
        return vals
    vals = [LD.check_true_peak(v) for v in (true_peak.tolist() if torch.is_tensor(true_peak) else true_peak)]
    if len(vals) != n:
        raise ValueError(f"true_peak is a number or one per row ({n}), got {len(vals)}")
    for b, v in enumerate(vals):
        if v is not None and (targets is None or targets[b] != targets[b]):
            raise ValueError(f"to_waveforms: true_peak[{b}] = {v} limits the gain towards a loudness target, and row {b} names none")
    return vals if any(v is not None for v in vals) else None


def _encodings_per_row(encoding, B):
    """``encoding=`` of ``to_waveforms`` as a list of B format ids or None per row; None when no row names one."""
    if encoding is None or isinstance(encoding, str):
        return None if encoding is None else [AC.encoding_id(encoding)] * B
    encs = [None if e is None else AC.encoding_id(e) for e in encoding]
    if len(encs) != B:
        raise ValueError(f"encoding is a name or one per row ({B}), got {len(encs)}")
    return encs if any(e is not None for e in encs) else None


@dataclass
class Tail:
    """What ``tail`` returns: one host tensor per row or document, and what ``to_waveforms`` describes, each None unless asked for."""
    rows: list
    segments: Optional[list] = None
    report: Optional[list] = None
    marks: Optional[list] = None


def to_waveforms(mel, mel_lengths, vocoder, trim=True, silence_threshold_db=-60.0, *, encoding=None, dither=False, dither_keys=None,
                 documents=None, gaps=None, fade_ms=5.0, level="document", return_segments=False, loudness=None, return_loudness=False,
                 true_peak=None, return_meter=False, token_ends=None, x_lengths=None, breaks=None, return_marks=False, sample_rate=24000):
    """``trim_trailing_silence(to_waveform(mel[b:b+1, :, :len_b], vocoder))`` (reference inference.py:246) for every row of a
    ragged batch in one device pass: ragged Vocos decode, per-row peak normalisation, per-row trim lengths, then ONE copy of the
    audio and one of the [B] lengths -- one synchronisation for the whole batch.  Returns a list of B 1-D host tensors
    (``trim=False``: normalised but not trimmed, i.e. ``to_waveform`` per row); they are views of the batch's one host buffer.

    ``sample_rate``: an int, or one per row.  Rows that ask for another rate than 24 kHz are converted on the device after the
    normalisation and the trim, which run at 24 kHz exactly as without it: the kept samples of those rows go through
    ``resample.resample`` (one call per distinct rate, the trim length as the row length, no extra host read) ahead of the copy.
    The band-limited output of a row normalised to a 0.95 peak may overshoot that peak slightly; nothing is re-normalised, but
    ``true_peak=`` (below) holds the level between the samples, which is what the conversion reconstructs, under a ceiling.

    ``encoding``: None (float32 rows, as ever), a name -- ``"pcm16"`` (s16le), ``"ulaw"``, ``"alaw"`` (G.711), ``"flac"`` (below) -- or one
    per row, where None leaves a row float.  The rows that name one are encoded on the device (``audio_codec.encode``: one launch after the trim
    and the rate conversion, on their device lengths, no extra host read) and come back as 1-D uint8 host tensors: raw samples, no
    container, views of the batch's one host buffer of bytes; the one copy is then of bytes and the single synchronisation stays.
    ``dither`` (a bool, or one per row): TPDF dither on the PCM16 rows, the sequence of row b selected by ``dither_keys[b]`` (default
    0) and by nothing else, so a row's bytes do not depend on the batch it is in.  The keyword-only arguments follow a ``*``.
    A ``"flac"`` row comes back as one complete FLAC stream (``audio_codec.encode_flac``: mono, 16 bits, blocks of 4096 samples, at
    the row's converted rate), a file as it is, holding exactly the words ``"pcm16"`` gives for it -- dithered the same way when
    ``dither`` is on.  Batches may mix the names: the PCM / G.711 launch and the FLAC call each see only their rows; the stream lengths
    ride in the same ``meta`` copy, and only the columns of the longest stream are copied.  (LPC subframes in those streams:
    ``tail(..., flac_lpc=)``, which is this call with one more option.)

    ``documents``: None (every row is its own result, as ever: nothing below is launched or allocated), or the rows that belong
    together as a host list -- row counts in speaking order, or the CSR ``[0, n0, n0 + n1, ...]``; rows behind the last document are
    documents of one row each.  The rows of a document are then joined on the device into one waveform (``join_waveforms``: once, at
    24 kHz, after the normalisation and the trim and ahead of the rate conversion and the encoding, which see one row per document
    and its joined device length) and the call returns one entry per DOCUMENT; ``sample_rate``, ``encoding``, ``dither`` and
    ``dither_keys`` are then one per document.  ``gaps``: samples of silence (24 kHz) after each row, a host list of B (the entry of
    a document's last row is ignored; default none).  ``fade_ms``: the fade at the interior joints.  ``level`` (a name, or one per
    document): ``"document"`` gives a document one gain, that of its loudest sentence; ``"sentence"`` leaves each row the gain the
    normalisation gave it.
    ``return_segments``: also return, per document, ``[(start_s, end_s)]`` of its rows in seconds of the 24 kHz join (so they do
    not depend on the output rate): ``(results, segments)``.  The single synchronisation stays.

    ``loudness``: None (nothing below is launched or allocated), a target in LUFS, or one per row -- per document with
    ``documents=`` -- where None leaves a row alone, bit for bit.  The rows that name one are brought to it on the device
    (``loudness.normalize``: integrated loudness as in ITU-R BS.1770, one gain per row or document, limited so that the sample peak
    stays at or under 0.95, the level the peak normalisation leaves).  The stage runs once, at 24 kHz: after the normalisation and the
    trim, and after the join when there is one, so it sees one row per document on its device length; the rate conversion and the
    encoder come behind it.  ``return_loudness``: also return ``[(lufs, gain)]`` per row or document -- the loudness measured BEFORE the
    gain and the gain applied (1.0 for a row left alone); they ride in the one ``meta`` copy, so the single synchronisation stays.
    With ``return_segments`` too the call returns ``(results, segments, loudness)``.

    ``true_peak``: None (exactly the calls above are made), a ceiling in dBTP (finite, at most 0; EBU R 128 delivery is -1), or one per
    row -- per document with ``documents=`` -- where None names none.  The gain of a row that names one is also limited so that its TRUE
    peak, the level between the samples as an oversampling 12-tap interpolator reads it (``loudness.normalize(true_peak=)``), stays at
    or under the ceiling.  A ceiling on a row without a loudness target raises ``ValueError`` before anything is launched: the
    ceiling limits a gain, and such a row has none.  ``return_meter``: the report entries (returned as with ``return_loudness``) are
    dicts of seven figures -- ``lufs``, ``gain``, ``lra``, ``momentary_max``, ``short_term_max``, ``peak``, ``true_peak`` (``loudness.meter``;
    the peaks linear), all measured BEFORE the gain; they ride in the same ``meta`` copy.

    ``token_ends`` / ``x_lengths`` / ``breaks`` / ``return_marks``: None / False (exactly the calls above are made), or token timing
    (``timing.token_marks``, one planning launch after the normalisation and the trim, ahead of the join).  ``token_ends`` [B, Tx] and
    ``x_lengths`` [B] are ``synthesise(return_timing=True)["token_ends"]`` and the token counts.  ``breaks``: per ROW a list of
    ``(token, pause_ms)`` (None: none) -- a pause is cut into the row after that token (``timing.apply_breaks``, launched only when a row
    has a break; the fade at a cut is ``fade_ms``), and the join, the loudness stage, the rate conversion and the encoder see the
    lengthened rows through the device lengths they already take.  ``return_marks``: also return, LAST in the tuple, the marks
    ``[(start_s, end_s)]`` per token of each row -- with ``documents=`` one list per row of each document, a row's start inside its
    document added -- in seconds of the 24 kHz result like the segments, so they do not depend on the output rate.  The marks are copied
    behind the batch's one synchronisation; no further wait is added."""
    out = tail(mel, mel_lengths, vocoder, trim, silence_threshold_db, encoding=encoding, dither=dither, dither_keys=dither_keys,
               documents=documents, gaps=gaps, fade_ms=fade_ms, level=level, return_segments=return_segments, loudness=loudness,
               return_loudness=return_loudness, true_peak=true_peak, return_meter=return_meter, token_ends=token_ends, x_lengths=x_lengths,
               breaks=breaks, return_marks=return_marks, sample_rate=sample_rate)
    asked = tuple(v for v in (out.rows, out.segments, out.report, out.marks) if v is not None)     # in this order, the marks last
    return asked if len(asked) > 1 else out.rows


@torch.inference_mode()
def tail(mel, mel_lengths, vocoder, trim=True, silence_threshold_db=-60.0, **options) -> Tail:
    """``to_waveforms`` (``options``: its keyword-only arguments) with its result as a record in place of a tuple whose arity depends
    on the flags.  The stages, in their one order: decode, finish, [timing plan (+ breaks gather)], [join], [loudness], [rate
    conversion], [encode], ending; a bracketed stage is not entered when the plan has no row for it.
    One option is this entry's own: ``flac_lpc``, 0 (FIXED predictors, as ever) or 1..12 -- the FLAC rows of the call also try linear
    prediction up to that order (``encode_flac(lpc_order=)``: the same words in fewer bytes).  One value for the call's FLAC rows
    (without such a row it raises ``ValueError``), or one per row, 0 on every row that is no stream: the FLAC call is then made once
    per distinct order over its own rows, so a row's bytes do not depend on its batch."""
    flac_lpc = options.pop("flac_lpc", 0)                             # (the FLAC stage's own: the plan is what it was without it)
    plan = _resolve(lambda: 1 if mel.dim() == 2 else mel.shape[0], **options)
    orders = _flac_orders(flac_lpc, plan)
    model = vocoder.model if hasattr(vocoder, "model") else vocoder
    mel = mel[None] if mel.dim() == 2 else mel
    (B, _, T), hop = mel.shape, model.cfg["hop"]
    mel_lengths = torch.as_tensor(mel_lengths).to(device=mel.device, dtype=torch.long)
    rows = model.decode(mel, mel_lengths, check=False)
    trimmed, scale = finish_waveforms(rows, mel_lengths, hop=hop, silence_threshold_db=silence_threshold_db)
    # the kept samples of every row (-1: refused): the trim length, or all of ``hop * (frames - 1)``
    lengths = trimmed if trim else torch.where(trimmed < 0, trimmed, hop * (mel_lengths - 1))
    meta, data = {"frames": mel_lengths}, None                         # (what rides in the ending's one copy, by name)
    verdict, marks_host = (lambda: None), None
    if plan.timed:                                                     # from here on the rows are as long as the timing plan says
        rows, _ = _hip.aligned_rows(rows, 4, "audio")
        marks, lengths, breaks = TM.token_marks(options["token_ends"], options["x_lengths"], lengths, plan.break_rows, fine_hop=hop // 2,
                                                keep_max=rows.shape[1], check=False)
        verdict = breaks.raise_refused
        if breaks.NB:
            rows = TM.apply_breaks(rows, breaks, plan.fade)
        if plan.marks:
            marks_host = torch.empty(marks.shape, dtype=marks.dtype, pin_memory=True)
            marks_host.copy_(marks, non_blocking=True)                # complete at the batch's one synchronisation, in the ending
    if plan.csr is not None:                                           # the stages behind see one row per document
        meta["kept"] = lengths
        rows, lengths, meta["starts"] = join_waveforms(rows, lengths, plan.csr, plan.gaps, fade=plan.fade,
                                                       scale=_document_scales(scale, plan), check=False)
    if plan.targets is not None:
        rows, meta["loud"] = _loudness_stage(rows, lengths, plan)
    if any(r != SAMPLE_RATE for r in plan.rates):
        rows, lengths = _convert_rows(rows, lengths, plan.rates)
    flac = None
    if plan.encs is not None:
        # one launch over the finished rows on their device lengths; rows without an encoding take part with length 0 and stay float.
        # FLAC rows go through their own call (three launches), likewise: each encoder sees the other's rows with length 0
        sampled = [e is not None and e != AC.FLAC for e in plan.encs]
        streamed = [e == AC.FLAC for e in plan.encs]
        dither = plan.dither if len(set(plan.dither)) > 1 else plan.dither[0]
        if any(sampled) or not any(streamed):
            named = torch.tensor(sampled, dtype=torch.bool, device=rows.device)
            data, meta["nbytes"] = AC.encode(rows, torch.where(named, lengths, torch.zeros_like(lengths)), [e if on else AC.PCM16 for e, on in zip(plan.encs, sampled)],
                                             dither=dither, keys=plan.keys)
        if any(streamed):
            flac, nbytes = _flac_stage(rows, lengths, plan, streamed, dither, orders)
            mine = torch.tensor(streamed, dtype=torch.bool, device=rows.device)
            meta["nbytes"] = torch.where(mine, nbytes, meta["nbytes"]) if data is not None else nbytes
    try:
        out, starts = _ending(rows, lengths, plan, meta, data, T, flac)
    except ValueError:
        verdict()                                                      # the timing plan's own verdict names the row and the reason
        raise
    if plan.marks:
        per_row = TM.marks_rows(marks_host, B, starts)
        out.marks = per_row if plan.csr is None else [per_row[a:b] for a, b in zip(plan.csr[:-1], plan.csr[1:])]
    return out


def _flac_stage(rows, lengths, plan, streamed, dither, orders):
    """The FLAC rows of the plan as streams: ``(data, byte counts)`` of ``audio_codec.encode_flac`` over all rows, the others taking
    part with length 0.  One call; with ``orders`` (``_flac_orders``) one per distinct order, each over its own rows."""
    orders = orders or [0] * plan.n
    data = nbytes = None
    for order in sorted({o for o, on in zip(orders, streamed) if on}):
        mine = torch.tensor([on and o == order for o, on in zip(orders, streamed)], dtype=torch.bool, device=rows.device)
        kw = dict(lpc_order=order) if order else {}
        d, n = AC.encode_flac(rows, torch.where(mine, lengths, torch.zeros_like(lengths)), plan.rates, dither=dither, keys=plan.keys, **kw)
        data, nbytes = (d, n) if data is None else (torch.where(mine[:, None], d, data), torch.where(mine, n, nbytes))
    return data, nbytes


def _document_scales(scale, plan):
    """``scale=`` of the join for the plan's levels: the rows' gains where a document takes one gain, 1 on the rows of a document
    whose sentences keep theirs (its gain is then 1 and nothing is multiplied), None when no document takes one."""
    if all(v == "sentence" for v in plan.levels):
        return None
    if all(v == "document" for v in plan.levels):
        return scale
    own = torch.tensor([v == "sentence" for v, a, b in zip(plan.levels, plan.csr[:-1], plan.csr[1:]) for _ in range(a, b)], dtype=torch.bool,
                       device=scale.device)
    return torch.where(own, torch.ones_like(scale), scale)


def _loudness_stage(rows, lengths, plan):
    """The loudness stage: ``rows`` [n, L] at 24 kHz on their device lengths, in place (a padded copy when L is no multiple of 4).
    Returns the rows and what rides in the ``meta`` copy, int64 [k * n]: the bits of the measured LUFS and of the gains -- with
    ``plan.meter`` of the seven ``METER_FIGURES``.  Without ceilings and meter exactly one ``mtts_loudness`` call is made; rows that name
    different ceilings take one call per distinct ceiling, each row levelled in its own (elsewhere its target is NaN: it keeps its bits)."""
    rows, _ = _hip.aligned_rows(rows, 4, "audio")
    if plan.ceilings is None and not plan.meter:
        lufs, gain, _ = LD.normalize(rows, lengths, plan.targets, SAMPLE_RATE, LD.PEAK_CEILING, check=False)
        return rows, torch.cat([lufs.view(torch.long), gain.to(torch.float64).view(torch.long)])
    ceilings = [None] * plan.n if plan.ceilings is None else plan.ceilings
    out = None
    for c in sorted(set(ceilings), key=lambda v: (v is not None, v)):
        mine = [v == c for v in ceilings]
        m = LD.normalize(rows, lengths, [t if own else math.nan for t, own in zip(plan.targets, mine)], SAMPLE_RATE, LD.PEAK_CEILING,
                         check=False, true_peak=c, return_meter=True)[3]
        if out is None:
            out = m
        else:
            mask = torch.tensor(mine, dtype=torch.bool, device=rows.device)
            out = {k: torch.where(mask, m[k], out[k]) for k in out}
    names = METER_FIGURES if plan.meter else METER_FIGURES[:2]
    return rows, torch.cat([out[k].to(torch.float64).view(torch.long) for k in names])


def _convert_rows(audio, lengths, rates):
    """Rows of ``audio`` [B, L] (24 kHz, ``lengths`` [B] kept samples on the device, -1 = refused row) at the rates they ask for:
    ``(audio' [B, L'], lengths')`` on the device.  Rows at 24 kHz are copied, the others converted with one ``resample`` call per
    distinct rate; a refused row stays refused (-1).  Nothing is read on the host."""
    (B, L), dev, parts = audio.shape, audio.device, []
    for rate in sorted(set(rates) - {SAMPLE_RATE}):
        rows = torch.tensor([b for b in range(B) if rates[b] == rate], dtype=torch.long, device=dev)
        out, n = R.resample(audio.index_select(0, rows), lengths.index_select(0, rows), SAMPLE_RATE, rate, check=False)
        parts.append((rows, out, n))
    same = [b for b in range(B) if rates[b] == SAMPLE_RATE]
    ld = max([L] * bool(same) + [out.shape[1] for _, out, _ in parts])
    wave = torch.zeros(B, ld, dtype=torch.float32, device=dev)
    new_lengths = lengths.clone()
    if same:
        rows = torch.tensor(same, dtype=torch.long, device=dev)
        wave[rows, :L] = audio.index_select(0, rows)
    for rows, out, n in parts:
        wave[rows, :out.shape[1]] = out
        new_lengths[rows] = n
    return wave, new_lengths


def _ending(rows, lengths, plan, meta, data, T, flac=None):
    """The end of the tail: the ``meta`` words -- the result lengths, then the named sections the stages left -- in the batch's one
    device-to-host copy that waits for the stream, the refusals it shows, then one copy of the floats and/or one of the bytes, of
    which the results are views.  ``data``: the rows ``audio_codec.encode`` wrote; ``flac``: those of ``encode_flac``, of which only
    the columns of the longest stream are copied.  Returns ``(Tail, starts)``: the start of every row inside its document (None without documents)."""
    joined = plan.csr is not None
    words = {"got": lengths, **meta}
    flat = torch.cat(list(words.values())).cpu().tolist()              # waits for the stream: the batch's one synchronisation
    ends = list(itertools.accumulate(w.numel() for w in words.values()))
    host = {k: flat[e - w.numel():e] for (k, w), e in zip(words.items(), ends)}
    got, frames, kept, nb, starts = host["got"], host["frames"], host.get("kept", host["got"]), host.get("nbytes"), host.get("starts")
    for b in range(len(kept)):
        if kept[b] < 0 or (not joined and nb is not None and nb[b] < 0):
            raise ValueError(f"to_waveforms: mel_lengths[{b}] = {frames[b]} is outside [1, T = {T}]")
    for g in range(plan.n if joined else 0):
        if got[g] < 0:
            raise ValueError(f"to_waveforms: document {g} (rows {plan.csr[g]} to {plan.csr[g + 1] - 1}) could not be joined")
    # a joined buffer is as wide as the host's bound on a document: no more columns are copied than the longest result has
    floats = coded = streams = None
    if plan.encs is None or not all(e is not None for e in plan.encs):
        floats = rows[:, :max(got)].cpu() if joined else rows.cpu()
    if data is not None:
        sampled = [g for g in range(plan.n) if plan.encs[g] not in (None, AC.FLAC)]
        width = max([nb[g] for g in sampled] + [1]) if joined else max(AC.BYTES_PER_SAMPLE[AC.PCM16 if e is None else e] for e in plan.encs if e != AC.FLAC) * rows.shape[1]
        coded = data[:, :width].cpu() if width < data.shape[1] else data.cpu()
    if flac is not None:
        streams = flac[:, :max(nb[g] for g in range(plan.n) if plan.encs[g] == AC.FLAC)].cpu()
    pick = lambda g: floats[g, :got[g]] if plan.encs is None or plan.encs[g] is None else (streams if plan.encs[g] == AC.FLAC else coded)[g, :nb[g]]
    out = Tail([pick(g) for g in range(plan.n)])
    if plan.segments:
        out.segments = [[(starts[b] / SAMPLE_RATE, (starts[b] + kept[b]) / SAMPLE_RATE) for b in range(plan.csr[g], plan.csr[g + 1])]
                        for g in range(plan.n)]
    if plan.report:                                                    # (lufs, gain); dicts when the stage left all METER_FIGURES
        vals = torch.tensor(host["loud"]).reshape(-1, plan.n).view(torch.float64).tolist()
        out.report = list(zip(*vals)) if len(vals) == 2 else [dict(zip(METER_FIGURES, row)) for row in zip(*vals)]
    return out, starts


def finish_request(waveform, *, loudness=None, true_peak=None, report=False, sample_rate=SAMPLE_RATE, encoding=None, dither=False,
                   dither_key=None, flac_lpc=0):
    """The tail of one request behind the normalisation and the trim, in the order of the batched tail: ``waveform`` 1-D float32 on
    the device at 24 kHz -> ``(host tensor, report)``.  The loudness step (``loudness`` a checked target in LUFS, its gain also limited
    by a ``true_peak`` ceiling in dBTP), the rate conversion, the encoding (``dither`` / ``dither_key`` as ``audio_codec.encode`` takes
    them; raw uint8 samples, or with ``"flac"`` one FLAC stream at the converted rate, ``audio_codec.encode_flac``, ``flac_lpc`` its ``lpc_order``: a value without ``"flac"`` raises ``ValueError``).  ``report``: what the loudness step measured BEFORE the gain, ``(lufs, gain)`` -- the dict of
    ``loudness.normalize(return_meter=True)`` under a ceiling; the meter runs only then -- else None.  An empty waveform passes through."""
    rep, n, rate = None, waveform.numel(), int(sample_rate)
    flac_lpc = AC.flac_lpc_order(flac_lpc)
    if flac_lpc and (encoding is None or AC.encoding_id(encoding) != AC.FLAC):
        raise ValueError(f"finish_request: flac_lpc = {flac_lpc} belongs to encoding=\"flac\", got {encoding!r}")
    if loudness is not None and n > 0:
        rows = torch.zeros(1, (n + 3) // 4 * 4, dtype=torch.float32, device=waveform.device)
        rows[0, :n] = waveform
        out = LD.normalize(rows, [n], loudness, SAMPLE_RATE, check=False, true_peak=true_peak,
                           return_meter=bool(report and true_peak is not None))
        if report:
            rep = {k: float(v[0]) for k, v in out[3].items()} if true_peak is not None else (float(out[0][0]), float(out[1][0]))
        waveform = rows[0, :n]
    if rate != SAMPLE_RATE and n > 0:
        conv, _ = R.resample(waveform.reshape(1, -1), None, SAMPLE_RATE, rate, check=False)
        waveform = conv[0, :R.resampler(SAMPLE_RATE, rate, conv.device).out_length(n)]
    if encoding is not None and AC.encoding_id(encoding) == AC.FLAC:           # a stream at any length: an empty one is its 42 header bytes
        rows = waveform.reshape(1, -1) if n > 0 else torch.zeros(1, 4, dtype=torch.float32, device=waveform.device)
        data, nbytes = AC.encode_flac(rows, [waveform.numel()], rate, dither=dither, keys=None if dither_key is None else [dither_key],
                                        **(dict(lpc_order=flac_lpc) if flac_lpc else {}))
        size = int(nbytes[0])
        if size < 0:
            raise ValueError(f"finish_request: a FLAC stream names its rate in 20 bits, sample_rate = {rate} is outside [1, 1048575]")
        waveform = data[0, :size]
    elif encoding is not None and n > 0:
        data, _ = AC.encode(waveform.reshape(1, -1), None, encoding, dither=dither, keys=None if dither_key is None else [dither_key])
        waveform = data[0, :waveform.numel() * AC.BYTES_PER_SAMPLE[AC.format_id(encoding)]]
    elif encoding is not None:
        waveform = torch.zeros(0, dtype=torch.uint8)
    return waveform.cpu(), rep

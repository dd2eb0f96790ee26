"""Handler-level adapter for the reference's HTTP server.

The reference handler (reference matcha/server.py:93-127) turns one POST /v1/audio/speech body into
``pipeline(model, vocoder, text, speaker, voice_mix, steps, scale_correction, length_scale)`` and runs it on the event-loop
thread, one request at a time.  ``request_params`` is that mapping (voice / voice-mix parsing, the per-voice duration scale
correction of ``VOICES``, the speed -> length_scale clamp) as a pure function, and ``SpeechService`` is the piece a maintainer
puts behind the same route: it phonemizes, submits to a ``FrameBudgetBatcher`` (so concurrent requests share estimator
launches without changing anybody's audio) and awaits the trimmed waveform.  ``response_format`` names the plain formats of the
route -- ``pcm`` (s16le), ``wav`` (RIFF + PCM16) -- and the two G.711 laws of a telephony leg; their samples are encoded on the device
(``audio_codec``).  A service built with ``flac=True`` also answers ``response_format="flac"``: the route's lossless compressed format,
one FLAC stream per request, encoded on the device too (``audio_codec.encode_flac``).  Transport, the lossy response encodings (MP3 /
OGG, with their psychoacoustic models) and the phonemizer stay the reference's (out of the path's scope).
"""
from __future__ import annotations

import asyncio
import re
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

from .inference import DEFAULT_NUM_STEPS, DEFAULT_ODE_SOLVER, VOICES
from .loudness import check_ceiling as checked_ceiling, check_target      # (the ceiling rule under the name it has here)

LENGTH_SCALE_MIN = 0.1      # fastest (client speed 2.0 clamps here; reference server.py:34-36)
LENGTH_SCALE_MAX = 2.0      # slowest
MAX_TEXT_LENGTH = 1000      # reference server.py:30
MAX_DOCUMENT_LENGTH = 20000 # characters of a text spoken as a document (submit_long); the reference has no such route

#: ``response_format`` -> the encoding a request asks of the batcher; "wav" is that payload behind a RIFF header
RESPONSE_FORMATS = {"pcm": "pcm16", "wav": "pcm16", "ulaw": "ulaw", "alaw": "alaw"}
#: what a service built with ``flac=True`` answers besides: the stream is a file as it is
COMPRESSED_FORMATS = {"flac": "flac"}

_MIX = re.compile(r"^\s*(\d+)\((\d+)\)\s*$")


def parse_voice_mix(voice: str) -> List[Tuple[int, float]]:
    """'2(70)+6(30)' -> [(2, 0.7), (6, 0.3)] (reference server.py:64-69)."""
    parts = voice.split("+")
    if len(parts) != 2:
        raise ValueError("a voice mix names exactly two voices: 'id(weight)+id(weight)'")
    out = []
    for p in parts:
        m = _MIX.match(p)
        if not m:
            raise ValueError(f"malformed voice mix term {p!r}")
        out.append((int(m.group(1)), int(m.group(2)) / 100))
    return out


@dataclass
class SpeechParams:
    speaker: int
    voice_mix: Optional[List[Tuple[int, float]]]
    language: str
    scale_correction: float
    length_scale: float
    n_timesteps: int
    solver: str


def response_encoding(response_format: Optional[str], flac: bool = False) -> Optional[str]:
    """The ``Request.encoding`` of a ``response_format``: None for None (a float waveform), else ``RESPONSE_FORMATS`` -- with ``flac``
    (a service that opted in) ``COMPRESSED_FORMATS`` too; ``ValueError`` for a name that is none of them (mp3 / opus are the
    reference's post-waveform codecs, ``inference.convert_to_*``)."""
    if response_format is None:
        return None
    known = {**RESPONSE_FORMATS, **COMPRESSED_FORMATS} if flac else RESPONSE_FORMATS
    if response_format not in known:
        hint = " (\"flac\" is answered by a service built with flac=True)" if response_format in COMPRESSED_FORMATS else ""
        raise ValueError(f"unknown response_format {response_format!r}: one of {sorted(known)} (or None for float samples){hint}")
    return known[response_format]


def response_body(res, response_format: Optional[str], sample_rate: int = 24000):
    """What ``speak`` returns for a batcher result: the ``"audio"`` (or the mel, without a vocoder) as it is when no
    ``response_format`` was named, else ``bytes`` -- the raw encoded samples, behind a RIFF header for ``"wav"``; a ``"flac"`` stream as
    it is, since it already is a file."""
    audio = res["audio"] if "audio" in res else res["mel"]
    if response_format is None:
        return audio
    from .audio_codec import _payload_bytes, wav_bytes
    raw = _payload_bytes(audio)
    return wav_bytes(raw, "pcm16", sample_rate) if response_format == "wav" else raw


def request_params(voice=0, speed: float = 1.0, steps: int = DEFAULT_NUM_STEPS, solver: str = DEFAULT_ODE_SOLVER) -> SpeechParams:
    """The request -> synthesis parameters of reference server.py:96-115 (and the language lookup of inference.py:235-236)."""
    if "+" in str(voice):
        mix = parse_voice_mix(str(voice))
        speaker, primary = 0, mix[0][0]
        scale_correction = sum(VOICES[i]["scale_correction"] * w for i, w in mix)
    else:
        mix, speaker = None, int(voice)
        primary = speaker
        scale_correction = VOICES[speaker]["scale_correction"]
    language = next(v["lang"] for v in VOICES if v["id"] == str(primary))
    length_scale = max(LENGTH_SCALE_MIN, min(LENGTH_SCALE_MAX, 1.0 / speed))
    return SpeechParams(speaker, mix, language, scale_correction, length_scale, int(steps), solver)


_SERVICE = object()      # default of ``submit_long / speak_long(loudness=)``: the service's own target


class SpeechService:
    """``await service.speak(text, voice, speed, steps, solver)`` -> 1-D waveform tensor on the host (``bytes`` with ``response_format``).

    ``phonemize(text, language) -> list of phoneme ids`` is the reference's front end (``process_text``); ``batcher`` a
    ``FrameBudgetBatcher`` or a ``StepBatcher`` (same ``submit`` contract; the second schedules at the solver step, so requests with
    different ``steps`` share launches) built with ``vocoder=`` so that results carry ``"audio"``."""

    def __init__(self, batcher, phonemize: Callable[[str, str], Sequence[int]], max_text_length: int = MAX_TEXT_LENGTH,
                 loudness: Optional[float] = None, true_peak: Optional[float] = None, marks: bool = False,
                 word_groups: Optional[Callable[[str, str, Sequence[int]], Sequence[int]]] = None, flac: bool = False,
                 flac_lpc: int = 0):
        """``flac``: this service also answers ``response_format="flac"`` (one FLAC stream per request, encoded on the device); without
        it the name is refused as every unknown one is.  ``flac_lpc``: 0, or the LPC order (1..12) its FLAC streams also try
        (``Request.flac_lpc``: the same words in fewer bytes, about 0.82 of the bytes at 12); it needs ``flac=True``.
        ``marks``: every request of this service asks for token marks -- ``submit``'s future then carries ``"marks"``: ``{"tokens":
        [(start_s, end_s)] per token}`` in seconds of the 24 kHz result (``timing.token_marks``; nominal positions) -- and
        ``word_groups(text, language, ids)``, when given, names the word of each token (-1: none; ``timing.word_groups`` over the
        phonemizer's separated symbols is the usual source), so that ``"marks"`` has ``"words"`` too.  ``timed()`` gives a view of the
        service with marks on, for one request.  ``speak`` returns what it returns without them.
        ``loudness``: None, or the target in LUFS every request of this service is brought to on the device (BS.1770 integrated
        loudness, ``loudness.normalize``; typically -16, -19 or -23).  ``levelled(target)`` gives a view of the service with another
        target, for one request: ``await service.levelled(-16).speak(text)``.  ``true_peak``: None, or the ceiling in dBTP the true
        peak of every levelled request is held under (EBU R 128 delivery: -1); it limits the gain towards the target, so it needs
        ``loudness``.  Results then also carry ``"true_peak"`` (dBTP, before the gain) and ``"lra"``."""
        self.batcher = batcher
        self.phonemize = phonemize
        self.max_text_length = int(max_text_length)
        self.loudness = check_target(loudness)
        self.true_peak = checked_ceiling(true_peak, self.loudness)
        self.marks = bool(marks)
        self.word_groups = word_groups
        self.flac = bool(flac)
        from .audio_codec import flac_lpc_order
        self.flac_lpc = flac_lpc_order(flac_lpc)
        if self.flac_lpc and not self.flac:
            raise ValueError(f"flac_lpc = {flac_lpc} belongs to a service built with flac=True")

    def timed(self, marks: bool = True) -> "SpeechService":
        """This service -- the same batcher, front end, target and ceiling -- with token marks on (or off): ``service.timed().submit(text)``
        gives a future whose result carries ``"marks"``.  ``submit`` and ``speak`` keep their signatures, so marks for a single request
        are asked for this way; ``submit_long`` and ``speak_long`` also take ``marks=`` themselves."""
        return SpeechService(self.batcher, self.phonemize, self.max_text_length, self.loudness, self.true_peak, marks, self.word_groups, self.flac, self.flac_lpc)

    def _fields(self, speaker_embedding, sample_rate, encoding, target, ceiling, marks, word_groups: Callable[[], list]) -> dict:
        """The fields a submission names beside its voice and speeds -- only those that differ from a ``Request``'s defaults, so a plain
        one names none.  ``word_groups()``: the word of each token, asked for only with marks and a ``word_groups`` front end."""
        named = dict(speaker_embedding=None if speaker_embedding is None else tuple(speaker_embedding),
                     sample_rate=int(sample_rate) if int(sample_rate) != 24000 else None, encoding=encoding, loudness=target, true_peak=ceiling,
                     flac_lpc=self.flac_lpc if encoding in COMPRESSED_FORMATS.values() and self.flac_lpc else None,
                     marks=True if marks else None, word_groups=word_groups() if marks and self.word_groups is not None else None)
        return {k: v for k, v in named.items() if v is not None}

    def levelled(self, loudness: Optional[float], true_peak: Optional[float] = None) -> "SpeechService":
        """This service -- the same batcher and front end -- with ``loudness`` as its target (None: none) and ``true_peak`` as its
        true-peak ceiling in dBTP (None: none).  A value that is no level, and a ceiling without a target, raise here, before
        anything is submitted.  ``submit`` and ``speak`` keep their positional signatures, so the target of a
        single request is named this way; ``submit_long`` and ``speak_long`` also take ``loudness=`` themselves."""
        return SpeechService(self.batcher, self.phonemize, self.max_text_length, loudness, true_peak, self.marks, self.word_groups, self.flac, self.flac_lpc)

    def submit(self, text: str, voice=0, speed: float = 1.0, steps: int = DEFAULT_NUM_STEPS, solver: str = DEFAULT_ODE_SOLVER,
               speaker_embedding=None, sample_rate: int = 24000, response_format: Optional[str] = None):
        """``speaker_embedding``: the ``(e_enc, e_dur)`` rows of an enrolled voice (``MatchaTTSInfer.enroll_voice``); the request is
        then spoken with them, and ``voice`` only picks the language and the duration scale correction.  ``sample_rate``: the rate
        of the result's ``"audio"`` (8 or 16 kHz for telephony, 48 kHz for a browser); the batcher converts on the device.
        ``response_format``: None (float samples), ``"pcm"`` (raw s16le), ``"wav"`` (the same samples; ``speak`` adds the RIFF
        header), ``"ulaw"`` / ``"alaw"`` (raw G.711), ``"flac"`` (a service built with ``flac=True``: one FLAC stream, a file as it
        is), all at ``sample_rate`` and encoded on the device; an unknown name raises
        ``ValueError`` before anything is submitted.  With a loudness target (the service's, or ``levelled(target)``) the result
        also carries ``"loudness"`` -- the LUFS measured before the gain -- and ``"gain"``."""
        encoding = response_encoding(response_format, self.flac)
        if len(text) > self.max_text_length:
            raise ValueError(f"Text exceeds {self.max_text_length} characters")       # the handler's HTTP 400
        p = request_params(voice, speed, steps, solver)
        ids = self.phonemize(text.strip(), p.language)
        extra = self._fields(speaker_embedding, sample_rate, encoding, self.loudness, self.true_peak, self.marks,
                             lambda: list(self.word_groups(text.strip(), p.language, ids)))
        return self.batcher.submit(ids, speaker=p.speaker, voice_mix=p.voice_mix, solver=p.solver, n_timesteps=p.n_timesteps,
                                   scale_correction=p.scale_correction, length_scale=p.length_scale, **extra)

    async def speak(self, text: str, voice=0, speed: float = 1.0, steps: int = DEFAULT_NUM_STEPS, solver: str = DEFAULT_ODE_SOLVER,
                    speaker_embedding=None, sample_rate: int = 24000, response_format: Optional[str] = None):
        """The waveform (a 1-D float tensor on the host), or with ``response_format`` the response body as ``bytes``."""
        res = await asyncio.wrap_future(self.submit(text, voice, speed, steps, solver, speaker_embedding, sample_rate, response_format))
        return response_body(res, response_format, int(sample_rate))

    def submit_long(self, text: str, voice=0, speed: float = 1.0, steps: int = DEFAULT_NUM_STEPS, solver: str = DEFAULT_ODE_SOLVER,
                    speaker_embedding=None, sample_rate: int = 24000, response_format: Optional[str] = None,
                    max_document_length: int = MAX_DOCUMENT_LENGTH, *, loudness=_SERVICE, true_peak=_SERVICE, marks=_SERVICE,
                    **split_options):
        """A text longer than one utterance: cut into sentences (``longform.split_text(text, **split_options)``; the abbreviation set
        is that of the voice's language unless given), each phonemized on its own -- so the phonemizer's intonation marks stay per
        sentence --, and submitted as ONE document (``FrameBudgetBatcher.submit_document``): the sentences run as rows of one ragged
        batch and are joined on the device with the splitter's pauses between them.  The other arguments are ``submit``'s and apply to
        the joined result.  The future's result carries ``"audio"`` and ``"segments"`` (seconds of each sentence in the 24 kHz join).
        A batcher without ``submit_document`` raises ``TypeError``: there is no host-side join to fall back to.  ``submit`` and its
        cap are unchanged.  ``loudness``: the target in LUFS of the JOINED audio -- one gain per document, so its sentences keep
        their balance -- or None; by default the service's own.  The result then carries ``"loudness"`` and ``"gain"``.
        ``true_peak``: the ceiling in dBTP on the true peak of the joined, levelled audio, or None; by default the service's own
        where the document has a target.  The result then also carries ``"true_peak"`` and ``"lra"``.
        ``marks``: whether the result carries ``"marks"`` -- ``{"tokens": one list of (start_s, end_s) per sentence}`` in the document's
        timeline, ``"words"`` too with the service's ``word_groups`` -- by default as the service says."""
        encoding = response_encoding(response_format, self.flac)
        target = self.loudness if loudness is _SERVICE else check_target(loudness)
        ceiling = (self.true_peak if target is not None else None) if true_peak is _SERVICE else checked_ceiling(true_peak, target)
        if not hasattr(self.batcher, "submit_document"):
            raise TypeError(f"{type(self.batcher).__name__} has no submit_document: long texts need a FrameBudgetBatcher")
        if len(text) > int(max_document_length):
            raise ValueError(f"Text exceeds {int(max_document_length)} characters")
        from .longform import split_text
        p = request_params(voice, speed, steps, solver)
        split_options.setdefault("language", p.language)
        pieces = split_text(text, **split_options)
        if not pieces:
            raise ValueError("empty text")
        ids = [self.phonemize(segment, p.language) for segment, _ in pieces]
        extra = self._fields(speaker_embedding, sample_rate, encoding, target, ceiling, self.marks if marks is _SERVICE else marks,
                             lambda: [list(self.word_groups(segment, p.language, i)) for (segment, _), i in zip(pieces, ids)])
        return self.batcher.submit_document(ids, [pause for _, pause in pieces], speaker=p.speaker, voice_mix=p.voice_mix, solver=p.solver,
                                            n_timesteps=p.n_timesteps, scale_correction=p.scale_correction, length_scale=p.length_scale,
                                            **extra)

    async def speak_long(self, text: str, voice=0, speed: float = 1.0, steps: int = DEFAULT_NUM_STEPS, solver: str = DEFAULT_ODE_SOLVER,
                         speaker_embedding=None, sample_rate: int = 24000, response_format: Optional[str] = None,
                         max_document_length: int = MAX_DOCUMENT_LENGTH, *, loudness=_SERVICE, true_peak=_SERVICE, marks=_SERVICE,
                         **split_options):
        """The joined waveform of a long text (a 1-D float tensor on the host), or with ``response_format`` the response body as
        ``bytes`` -- ``response_body``, as ``speak``."""
        res = await asyncio.wrap_future(self.submit_long(text, voice, speed, steps, solver, speaker_embedding, sample_rate, response_format,
                                                         max_document_length, loudness=loudness, true_peak=true_peak, marks=marks, **split_options))
        return response_body(res, response_format, int(sample_rate))

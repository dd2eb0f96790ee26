"""Encoded audio in and out on MI355X (``mtts_pcm_encode`` / ``mtts_pcm_decode``): the last stage of the waveform tail -- fp32 rows to
the bytes a client is sent, s16le for the OpenAI route's ``pcm`` / ``wav`` and G.711 mu-law / A-law for an 8 kHz telephony leg -- and
the first stage of the recording entries, which take clips that are still bytes (``Encoded``).  ``encode_flac`` is the compressed way
out: one complete FLAC stream per row (``mtts_flac_encode``, include/mtts.h "FLAC out"), the same PCM16 words without loss.

One launch per ragged batch, a format per row, lengths checked on the device.  Every byte is defined by include/mtts.h "encoded
audio" (DESIGN.md section 4); there is no CPU path.  The RIFF container (``wav_bytes`` / ``read_wav``) is host code: a header in
front of the payload the device produced.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip

PCM16, ULAW, ALAW, FLAC = 0, 1, 2, 3
FORMATS = {"pcm16": PCM16, "ulaw": ULAW, "alaw": ALAW}      # samples of a fixed size: what ``encode`` writes and ``decode`` reads
NAMES = {v: k for k, v in FORMATS.items()}
ENCODINGS = {**FORMATS, "flac": FLAC}                       # what a finished row can leave the tail as (``encoding_id``)
BYTES_PER_SAMPLE = {PCM16: 2, ULAW: 1, ALAW: 1}             # (FLAC has none: a stream's length is ``encode_flac``'s second result)
WAV_TAGS = {PCM16: 1, ULAW: 7, ALAW: 6}          # WAVE_FORMAT_PCM, WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW
FLAC_BLOCK_SIZES = (256, 512, 1024, 2048, 4096)


def __getattr__(name):
    if name == "TILE":                          # samples per workgroup of the kernels as built (MTTS_CODEC_TILE)
        return int(_hip.load().mtts_codec_tile())
    raise AttributeError(name)


def _is_flac(fmt) -> bool:
    return fmt == "flac" if isinstance(fmt, str) else isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and int(fmt) == FLAC


def format_id(fmt) -> int:
    """``"pcm16"`` / ``"ulaw"`` / ``"alaw"`` (or the id itself) -> MTTS_PCM16 / MTTS_ULAW / MTTS_ALAW; ``ValueError`` otherwise.  FLAC
    is none of them -- a stream has no fixed size per sample -- and its ``ValueError`` says where it is written."""
    if isinstance(fmt, str) and fmt in FORMATS:
        return FORMATS[fmt]
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and int(fmt) in NAMES:
        return int(fmt)
    if _is_flac(fmt):
        raise ValueError("FLAC is no format of encode / decode / Encoded / wav_bytes, whose rows are samples of a fixed size: a FLAC "
                         "stream is written by encode_flac -> (data, byte counts), and is not read back (decoding FLAC is out of scope)")
    raise ValueError(f"unknown audio format {fmt!r}: one of {sorted(FORMATS)}")


def encoding_id(enc) -> int:
    """``format_id`` with ``"flac"`` (MTTS_FLAC): the names ``to_waveforms(encoding=)`` and ``Request.encoding`` take."""
    return FLAC if _is_flac(enc) else format_id(enc)


def formats_per_row(formats, B: int, what: str = "formats"):
    """``formats`` as a list of B ids: one name (or id) for all rows, or one per row."""
    if isinstance(formats, (str, int, np.integer)):
        return [format_id(formats)] * B
    if torch.is_tensor(formats):
        formats = formats.reshape(-1).tolist()
    ids = [format_id(f) for f in formats]
    if len(ids) != B:
        raise ValueError(f"{what} is a name or one name per row ({B}), got {len(ids)}")
    return ids


@dataclass
class Encoded:
    """A clip that is still bytes: ``data`` (``bytes`` or a 1-D uint8 tensor, raw samples without a container) in ``format``
    (``"pcm16"``, ``"ulaw"``, ``"alaw"``) at ``sample_rate``.  The recording entries decode it on the device."""
    data: Union[bytes, torch.Tensor]
    format: str
    sample_rate: int = 24000

    def __post_init__(self):
        format_id(self.format)
        if torch.is_tensor(self.data) and (self.data.dim() != 1 or self.data.dtype != torch.uint8):
            raise ValueError("Encoded.data is bytes or a 1-D uint8 tensor")

    @property
    def nbytes(self) -> int:
        return int(self.data.numel()) if torch.is_tensor(self.data) else len(self.data)

    @property
    def samples(self) -> int:
        """Whole samples the payload holds."""
        return self.nbytes // BYTES_PER_SAMPLE[format_id(self.format)]

    def numel(self) -> int:
        """As a waveform's ``numel()``: the clip's samples (callers that size buffers from their clips need no special case)."""
        return self.samples

    def tensor(self) -> torch.Tensor:
        """The payload as a 1-D uint8 tensor (where it lives)."""
        if torch.is_tensor(self.data):
            return self.data
        return torch.frombuffer(bytearray(self.data), dtype=torch.uint8) if len(self.data) else torch.zeros(0, dtype=torch.uint8)


def _status(lib, verdict: torch.Tensor) -> None:
    _hip.raise_refused(lib.mtts_pcm_status, _hip.ptr(verdict), verdict.numel(), _hip.stream_ptr())


@torch.inference_mode()
def encode(audio: torch.Tensor, lengths, formats, dither=False, seed: int = 0, keys=None, check: bool = False
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """audio [B, L] (or [L]) float32 on the device + lengths [B] (samples; tensor or sequence, default all L) + ``formats`` (a name
    or one per row; names or a device int32 tensor) -> ``(data uint8 [B, 2 * ld], byte lengths int64 [B])`` on the device, ld = L
    rounded up to a multiple of 4.  Row b holds ``byte_lengths[b]`` bytes from its start (a G.711 row uses the front half of the
    stride); bytes beyond are not written (the buffer is ``torch.empty``).  Nothing is read on the host: a length outside [0, L]
    (or one that already is -1) gives ``byte_lengths[b] = -1``; ``check=True`` waits for that verdict and raises ``ValueError``.

    ``dither``: TPDF dither of one LSB on the PCM16 rows (G.711 rows compand the undithered value), a bool or one per row (two
    launches then, each over its rows); ``seed`` per call and ``keys`` (int64 per row, default 0) select the sequence, which is a
    function of (seed, key, sample index) only: a row's bytes do not depend on the batch it is in.  ``"flac"`` is no format of this
    entry -- its output has another shape -- and raises ``ValueError`` naming ``encode_flac``."""
    if _is_flac(formats) or (isinstance(formats, (list, tuple)) and any(_is_flac(f) for f in formats)):
        format_id("flac")                       # (raises, before anything else is looked at)
    lib = _hip.load()
    audio, L = _hip.aligned_rows(audio, 4, "audio")
    (B, ld), dev = audio.shape, audio.device
    lengths = _hip.row_lengths(lengths, B, L, dev)
    if torch.is_tensor(formats) and formats.is_cuda:
        fmt = formats.to(torch.int32).contiguous()
        if fmt.shape != (B,):
            raise ValueError(f"formats must have shape ({B},), got {tuple(fmt.shape)}")
    else:
        fmt = torch.tensor(formats_per_row(formats, B), dtype=torch.int32, device=dev)
    if keys is not None:
        keys = torch.as_tensor(keys).to(device=dev, dtype=torch.long).contiguous()
        if keys.shape != (B,):
            raise ValueError(f"keys must have shape ({B},), got {tuple(keys.shape)}")
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 63):
        raise ValueError("seed must fit a signed 64-bit integer")
    out = torch.empty(B, 2 * ld, dtype=torch.uint8, device=dev)

    def launch(row_lengths, on):
        nbytes = torch.empty(B, dtype=torch.long, device=dev)
        with torch.cuda.device(dev):
            _hip.check(lib.mtts_pcm_encode(_hip.ptr(audio), ld, _hip.ptr(row_lengths), _hip.ptr(fmt), _hip.ptr(keys), B, int(on), seed,
                                           _hip.ptr(out), _hip.ptr(nbytes), _hip.stream_ptr()))
        return nbytes

    if isinstance(dither, (bool, int, np.bool_)):
        nbytes = launch(lengths, bool(dither))
    else:
        on = [bool(v) for v in dither]
        if len(on) != B:
            raise ValueError(f"dither is a bool or one per row ({B}), got {len(on)}")
        if all(on) or not any(on):
            nbytes = launch(lengths, on[0])
        else:
            # one launch per value over its own rows: the other rows take part with length 0 (no byte written)
            mask = torch.tensor(on, dtype=torch.bool, device=dev)
            zero = torch.zeros_like(lengths)
            nbytes = torch.where(mask, launch(torch.where(mask, lengths, zero), True), launch(torch.where(mask, zero, lengths), False))
    if check:
        _status(lib, nbytes)
    return out, nbytes


_flac_ws = _hip.Workspaces()                    # staging slots: every word the call reads it has written


def flac_block_size(block_size) -> int:
    if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or int(block_size) not in FLAC_BLOCK_SIZES:
        raise ValueError(f"a FLAC block size is one of {FLAC_BLOCK_SIZES}, got {block_size!r}")
    return int(block_size)


@torch.inference_mode()
def encode_flac(audio: torch.Tensor, lengths, sample_rates, block_size: int = 4096, dither=False, seed: int = 0, keys=None,
                check: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """audio [B, L] (or [L]) float32 on the device + lengths [B] (samples; default all L) + ``sample_rates`` (Hz: an int, one per row,
    or a device int32 tensor) -> ``(data uint8 [B, stride], byte counts int64 [B])`` on the device: row b holds one complete mono
    16-bit FLAC stream of ``nbytes[b]`` bytes, a file as it is (include/mtts.h "FLAC out"; ``stride = mtts_flac_row_bytes``).  It
    holds exactly the words ``encode(..., "pcm16")`` gives for the row -- with ``dither`` (a bool, or one per row), ``seed`` and
    ``keys`` the same dithered words -- in frames of ``block_size`` samples; an empty row is the 42 header bytes.  Bytes at or beyond
    ``nbytes[b]`` are not written.  Nothing is read on the host: a length outside [0, L] (or one that already is -1) and a rate
    outside [1, 1048575] give ``nbytes[b] = -1`` and an unwritten row; ``check=True`` waits for that verdict and raises ``ValueError``."""
    lib = _hip.load()
    bs = flac_block_size(block_size)
    audio, L = _hip.aligned_rows(audio, 4, "audio")
    (B, ld), dev = audio.shape, audio.device
    lengths = _hip.row_lengths(lengths, B, L, dev)
    if isinstance(sample_rates, (int, np.integer)) and not isinstance(sample_rates, bool):
        sample_rates = [int(sample_rates)] * B
    rates = torch.as_tensor(sample_rates).to(device=dev, dtype=torch.int32).contiguous()
    if rates.shape != (B,):
        raise ValueError(f"sample_rates is an int or one per row ({B}), got shape {tuple(rates.shape)}")
    if keys is not None:
        keys = torch.as_tensor(keys).to(device=dev, dtype=torch.long).contiguous()
        if keys.shape != (B,):
            raise ValueError(f"keys must have shape ({B},), got {tuple(keys.shape)}")
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 63):
        raise ValueError("seed must fit a signed 64-bit integer")
    stride = _hip.size(lib.mtts_flac_row_bytes(ld, bs))
    out = torch.empty(B, stride, dtype=torch.uint8, device=dev)
    ws = _flac_ws.get("flac", lib.mtts_flac_workspace_bytes(B, ld, bs), dev)

    def launch(row_lengths, on):
        nbytes = torch.empty(B, dtype=torch.long, device=dev)
        with torch.cuda.device(dev):
            _hip.check(lib.mtts_flac_encode(_hip.ptr(audio), ld, _hip.ptr(row_lengths), _hip.ptr(rates), _hip.ptr(keys), B, bs, int(on), seed,
                                            _hip.ptr(out), stride, _hip.ptr(nbytes), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
        return nbytes

    if isinstance(dither, (bool, int, np.bool_)):
        nbytes = launch(lengths, bool(dither))
    else:
        on = [bool(v) for v in dither]
        if len(on) != B:
            raise ValueError(f"dither is a bool or one per row ({B}), got {len(on)}")
        if all(on) or not any(on):
            nbytes = launch(lengths, on[0])
        else:
            # one call per value over its own rows: the other rows take part refused (-1: no byte written, the header included)
            mask = torch.tensor(on, dtype=torch.bool, device=dev)
            off = torch.full_like(lengths, -1)
            nbytes = torch.where(mask, launch(torch.where(mask, lengths, off), True), launch(torch.where(mask, off, lengths), False))
    if check:
        _status(lib, nbytes)
    return out, nbytes


@torch.inference_mode()
def decode(data: torch.Tensor, lengths, formats, check: bool = True, ld: int = None) -> torch.Tensor:
    """data uint8 [B, ld_bytes] (or 1-D) on the device + lengths [B] in SAMPLES + ``formats`` (a name or one per row) -> float32
    [B, ld] on the device, ld = ``ld`` rounded up to a multiple of 4 (default: ld_bytes, the longest row the bytes can hold): PCM16 words
    ``/ 32768``, G.711 codes as their linear value ``/ 32768``, zeros from a row's length on.  ``check`` waits for the device's verdict
    on the lengths and raises ``ValueError`` naming the first refused row (a length whose bytes exceed the row)."""
    lib = _hip.load()
    data, _ = _hip.aligned_rows(data, 16, "data", "a uint8 [B, ld_bytes] tensor")
    (B, ld_bytes), dev = data.shape, data.device
    fmt = torch.tensor(formats_per_row(formats, B), dtype=torch.int32, device=dev)
    lengths = _hip.row_lengths(lengths, B, 0, dev)
    ld = ld_bytes if ld is None else max(4, (int(ld) + 3) // 4 * 4)
    out = torch.zeros(B, ld, dtype=torch.float32, device=dev)
    out_lengths = torch.empty(B, dtype=torch.long, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.mtts_pcm_decode(_hip.ptr(data), ld_bytes, _hip.ptr(lengths), _hip.ptr(fmt), B, _hip.ptr(out), ld,
                                       _hip.ptr(out_lengths), _hip.stream_ptr()))
    if check:
        _status(lib, out_lengths)
    return out


def decode_clips(clips: Sequence[Encoded], dev) -> Tuple[torch.Tensor, list]:
    """``Encoded`` clips -> ``(float32 [n, ld] on ``dev``, sample counts)`` with one copy of the bytes and one decode launch.  The
    sample counts come from the payload sizes on the host, so nothing is waited for."""
    counts = [c.samples for c in clips]
    ids = [format_id(c.format) for c in clips]
    nb = max(16, (max(n * BYTES_PER_SAMPLE[f] for n, f in zip(counts, ids)) + 15) // 16 * 16)
    host = torch.zeros(len(clips), nb, dtype=torch.uint8)
    on_device = []
    for i, c in enumerate(clips):
        t = c.tensor()[: counts[i] * BYTES_PER_SAMPLE[ids[i]]]
        if t.is_cuda:
            on_device.append((i, t))
        else:
            host[i, :t.numel()].copy_(t)
    data = host.to(dev)
    for i, t in on_device:
        data[i, :t.numel()].copy_(t.to(dev))
    return decode(data, counts, ids, check=False, ld=max(counts)), counts     # (the lengths fit by construction: no wait)


# ------------------------------------------------------------------------------------------------ the RIFF container (host)
def _payload_bytes(payload) -> bytes:
    if torch.is_tensor(payload):
        if payload.dtype != torch.uint8 or payload.dim() != 1:
            raise ValueError("a payload is bytes or a 1-D uint8 tensor")
        return payload.detach().cpu().contiguous().numpy().tobytes()
    return bytes(payload)


def wav_bytes(payload, format, sample_rate: int) -> bytes:
    """The RIFF/WAVE file of mono ``payload`` (raw samples as ``to_waveforms(encoding=...)`` returns them): format tag 1 with 16
    bits for ``"pcm16"``; tag 7 (mu-law) / 6 (A-law) with 8 bits, block align 1, ``cbSize = 0`` and a ``fact`` chunk holding the
    sample count for G.711, as the WAVE specification asks of every non-PCM form."""
    fid = format_id(format)
    raw = _payload_bytes(payload)
    bps = BYTES_PER_SAMPLE[fid]
    if len(raw) % bps:
        raise ValueError(f"a {NAMES[fid]} payload holds whole samples of {bps} bytes, got {len(raw)} bytes")
    rate = int(sample_rate)
    if fid == PCM16:
        fmt = struct.pack("<4sIHHIIHH", b"fmt ", 16, 1, 1, rate, rate * 2, 2, 16)
        extra = b""
    else:
        fmt = struct.pack("<4sIHHIIHHH", b"fmt ", 18, WAV_TAGS[fid], 1, rate, rate, 1, 8, 0)
        extra = struct.pack("<4sII", b"fact", 4, len(raw))
    data = struct.pack("<4sI", b"data", len(raw)) + raw + (b"\x00" if len(raw) & 1 else b"")
    body = b"WAVE" + fmt + extra + data
    return struct.pack("<4sI", b"RIFF", len(body)) + body


def read_wav(path_or_bytes) -> Encoded:
    """A RIFF/WAVE file (a path, or its bytes) in one of the three forms ``wav_bytes`` writes -- 16-bit PCM, 8-bit mu-law, 8-bit
    A-law -- as an ``Encoded`` clip: mono, or channel 0 of a multi-channel file.  The stdlib ``wave`` module refuses the G.711 forms
    ("unknown format: 7").  ``ValueError`` for a truncated file and for any other form."""
    raw = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else Path(path_or_bytes).read_bytes()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    at, fmt, payload = 12, None, None
    while at + 8 <= len(raw) and payload is None:
        tag, size = struct.unpack_from("<4sI", raw, at)
        body = at + 8
        if body + size > len(raw):
            raise ValueError(f"truncated WAVE file: chunk {tag!r} claims {size} bytes, {len(raw) - body} are there")
        if tag == b"fmt ":
            if size < 16:
                raise ValueError("truncated WAVE file: a fmt chunk has at least 16 bytes")
            fmt = struct.unpack_from("<HHIIHH", raw, body)
        elif tag == b"data":
            payload = raw[body:body + size]
        at = body + size + (size & 1)
    if fmt is None or payload is None:
        raise ValueError("truncated WAVE file: no fmt chunk ahead of a data chunk")
    wtag, channels, rate, _, block, bits = fmt
    forms = {(1, 16): "pcm16", (7, 8): "ulaw", (6, 8): "alaw"}
    if (wtag, bits) not in forms or channels < 1:
        raise ValueError(f"unsupported WAVE form: format tag {wtag} with {bits} bits (16-bit PCM, 8-bit mu-law and 8-bit A-law are read)")
    name = forms[(wtag, bits)]
    bps = BYTES_PER_SAMPLE[FORMATS[name]]
    frame = bps * channels
    payload = payload[: len(payload) // frame * frame]
    if channels > 1:
        payload = np.frombuffer(payload, dtype=np.uint8).reshape(-1, channels, bps)[:, 0, :].tobytes()
    return Encoded(payload, name, int(rate))

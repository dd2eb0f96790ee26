"""Encoded audio in and out on MI355X (``mtts_pcm_encode`` / ``mtts_pcm_decode``): the last stage of the waveform tail -- fp32 rows to
the bytes a client is sent, s16le for the OpenAI route's ``pcm`` / ``wav`` and G.711 mu-law / A-law for an 8 kHz telephony leg -- and
the first stage of the recording entries, which take clips that are still bytes (``Encoded``).  ``encode_flac`` is the compressed way
out: one complete FLAC stream per row (``mtts_flac_encode``, include/mtts.h "FLAC out"), the same PCM16 words without loss.
``decode_flac`` is the compressed way in: whole FLAC files (``FlacClip``, ``read_flac``) decoded on the device, channel 0, integers to
the bit (``mtts_flac_decode``, include/mtts.h "FLAC in").

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
FLAC_MAX_LPC_ORDER = 12                          # the largest ``lpc_order`` of ``encode_flac`` (include/mtts.h "FLAC out")
FLAC_MAX_BLOCK = 4608                            # the largest block ``decode_flac`` reads (include/mtts.h "FLAC in")


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
                         "stream is written by encode_flac -> (data, byte counts) and read by read_flac / decode_flac (a FlacClip)")
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


def flac_lpc_order(lpc_order) -> int:
    if isinstance(lpc_order, bool) or not isinstance(lpc_order, (int, np.integer)) or not 0 <= int(lpc_order) <= FLAC_MAX_LPC_ORDER:
        raise ValueError(f"a FLAC LPC order lies in 0..{FLAC_MAX_LPC_ORDER} (0: FIXED predictors only), got {lpc_order!r}")
    return int(lpc_order)


@torch.inference_mode()
def encode_flac(audio: torch.Tensor, lengths, sample_rates, block_size: int = 4096, dither=False, seed: int = 0, keys=None,
                check: bool = False, lpc_order: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """audio [B, L] (or [L]) float32 on the device + lengths [B] (samples; default all L) + ``sample_rates`` (Hz: an int, one per row,
    or a device int32 tensor) -> ``(data uint8 [B, stride], byte counts int64 [B])`` on the device: row b holds one complete mono
    16-bit FLAC stream of ``nbytes[b]`` bytes, a file as it is (include/mtts.h "FLAC out"; ``stride = mtts_flac_row_bytes``).  It
    holds exactly the words ``encode(..., "pcm16")`` gives for the row -- with ``dither`` (a bool, or one per row), ``seed`` and
    ``keys`` the same dithered words -- in frames of ``block_size`` samples; an empty row is the 42 header bytes.  Bytes at or beyond
    ``nbytes[b]`` are not written.  Nothing is read on the host: a length outside [0, L] (or one that already is -1) and a rate
    outside [1, 1048575] give ``nbytes[b] = -1`` and an unwritten row; ``check=True`` waits for that verdict and raises ``ValueError``.
    ``lpc_order``: 0 writes CONSTANT / FIXED / VERBATIM subframes (``mtts_flac_encode``); 1..12 also tries linear prediction up to that
    order per frame (``mtts_flac_encode_lpc``: the same words in fewer bytes, about 0.82 of the FIXED stream on speech at 12, for a
    longer frame kernel); anything else raises ``ValueError``."""
    lib = _hip.load()
    bs = flac_block_size(block_size)
    lpc = flac_lpc_order(lpc_order)
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
            tail = (int(on), seed, _hip.ptr(out), stride, _hip.ptr(nbytes), ws.data_ptr(), ws.numel(), _hip.stream_ptr())
            head = (_hip.ptr(audio), ld, _hip.ptr(row_lengths), _hip.ptr(rates), _hip.ptr(keys), B, bs)
            _hip.check(lib.mtts_flac_encode_lpc(*head, lpc, *tail) if lpc else lib.mtts_flac_encode(*head, *tail))
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


@dataclass
class FlacClip:
    """A recording that is still a FLAC file: ``data`` (``bytes`` or a 1-D uint8 tensor) is the whole native stream -- marker, metadata,
    frames -- and the other fields are what its STREAMINFO block says (``read_flac`` fills them).  The recording entries decode channel
    0 on the device (``decode_flac``).  Separate from ``Encoded``, whose rows are samples of a fixed size."""
    data: Union[bytes, torch.Tensor]
    sample_rate: int
    samples: int
    channels: int = 1
    bits_per_sample: int = 16
    max_block: int = 4608

    def __post_init__(self):
        if torch.is_tensor(self.data) and (self.data.dim() != 1 or self.data.dtype != torch.uint8):
            raise ValueError("FlacClip.data is bytes or a 1-D uint8 tensor")
        if not (1 <= int(self.sample_rate) <= 1048575 and 0 <= int(self.samples) < 1 << 36 and 1 <= int(self.channels) <= 8
                and 8 <= int(self.bits_per_sample) <= 24 and 16 <= int(self.max_block) <= FLAC_MAX_BLOCK):
            raise ValueError("FlacClip: a rate in [1, 1048575], samples in [0, 2^36), 1..8 channels, 8..24 bits and a largest block in "
                             f"[16, {FLAC_MAX_BLOCK}] are read (include/mtts.h \"FLAC in\")")

    @property
    def nbytes(self) -> int:
        return int(self.data.numel()) if torch.is_tensor(self.data) else len(self.data)

    def numel(self) -> int:
        """As a waveform's ``numel()``: the samples of one channel."""
        return int(self.samples)

    def tensor(self) -> torch.Tensor:
        """The stream as a 1-D uint8 tensor (where it lives)."""
        if torch.is_tensor(self.data):
            return self.data
        return torch.frombuffer(bytearray(self.data), dtype=torch.uint8) if len(self.data) else torch.zeros(0, dtype=torch.uint8)


def read_flac(path_or_bytes) -> FlacClip:
    """A native FLAC file (a path, or its bytes) as a ``FlacClip``.  Only the marker and the metadata chain are read here, on the host;
    the frames are decoded on the device.  ``ValueError`` for what include/mtts.h "FLAC in" refuses and the host can see: no ``fLaC``
    marker (an ID3 tag or an Ogg container in front is named), no STREAMINFO block first, a reserved block type, a chain that runs off
    the file, bits per sample outside 8..24, block sizes outside [16, 4608], a rate of 0, an unknown length with frames behind it."""
    raw = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else Path(path_or_bytes).read_bytes()
    if raw[:3] == b"ID3":
        raise ValueError("a FLAC file behind an ID3 tag is not read: strip the tag (the stream starts at 'fLaC')")
    if raw[:4] == b"OggS":
        raise ValueError("Ogg FLAC is not read: only native FLAC streams (starting with 'fLaC')")
    if raw[:4] != b"fLaC":
        raise ValueError("not a FLAC file: no 'fLaC' marker")
    at, blocks, info = 4, 0, None
    while True:
        if at + 4 > len(raw):
            raise ValueError("truncated FLAC file: the metadata chain runs off the file")
        last, kind, size = raw[at] >> 7, raw[at] & 0x7F, int.from_bytes(raw[at + 1:at + 4], "big")
        if blocks == 0 and (kind != 0 or size != 34):
            raise ValueError("not a readable FLAC file: the first metadata block is not a 34-byte STREAMINFO")
        if kind == 127 or (blocks and kind == 0):
            raise ValueError(f"not a readable FLAC file: metadata block type {kind} at byte {at}")
        if at + 4 + size > len(raw):
            raise ValueError(f"truncated FLAC file: metadata block at byte {at} claims {size} bytes, {len(raw) - at - 4} are there")
        if kind == 0:
            info = int.from_bytes(raw[at + 4:at + 38], "big")
        at, blocks = at + 4 + size, blocks + 1
        if last:
            break
    lo, hi, rate = info >> 256, info >> 240 & 0xFFFF, info >> 172 & 0xFFFFF
    channels, bps, total = (info >> 169 & 7) + 1, (info >> 164 & 31) + 1, info >> 128 & (1 << 36) - 1
    if not 8 <= bps <= 24:
        raise ValueError(f"unsupported FLAC form: {bps} bits per sample (8 to 24 are read)")
    if lo < 16 or lo > hi or hi > FLAC_MAX_BLOCK:
        raise ValueError(f"unsupported FLAC form: block sizes {lo}..{hi} (16 to {FLAC_MAX_BLOCK} are read)")
    if rate < 1:
        raise ValueError("unsupported FLAC form: a sample rate of 0")
    if total == 0 and at < len(raw):
        raise ValueError("unsupported FLAC form: STREAMINFO names no length (a stream that was never finished)")
    return FlacClip(raw, int(rate), int(total), int(channels), int(bps), int(hi))


@torch.inference_mode()
def decode_flac(data: torch.Tensor, nbytes, ld: int = None, max_block: int = FLAC_MAX_BLOCK, check: bool = True
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """data uint8 [B, ld_bytes] (or 1-D) on the device, row b one whole FLAC stream of ``nbytes[b]`` bytes -> ``(audio float32 [B, ld],
    lengths int64 [B], rates int32 [B])`` on the device: channel 0 of each stream as ``q / 2^(bits - 1)``, exact, zeros from a row's
    length on (include/mtts.h "FLAC in").  ``ld``: the row capacity in samples, rounded up to a multiple of 4 (default 4 * ld_bytes); a
    stream that holds more is refused.  ``max_block``: the largest block size accepted (16..4608).  Nothing is read on the host: a
    refused row has ``lengths[b] = -1``, rate 0 and zeros; ``check`` waits for that verdict and raises ``ValueError`` naming the row."""
    lib = _hip.load()
    if isinstance(max_block, bool) or not isinstance(max_block, (int, np.integer)) or not 16 <= int(max_block) <= FLAC_MAX_BLOCK:
        raise ValueError(f"max_block lies in [16, {FLAC_MAX_BLOCK}], got {max_block!r}")
    data, _ = _hip.aligned_rows(data, 16, "data", "a uint8 [B, ld_bytes] tensor")
    (B, ld_bytes), dev = data.shape, data.device
    nbytes = _hip.row_lengths(nbytes, B, ld_bytes, dev, "nbytes")
    ld = 4 * ld_bytes if ld is None else max(4, (int(ld) + 3) // 4 * 4)
    out = torch.zeros(B, ld, dtype=torch.float32, device=dev)
    lengths = torch.empty(B, dtype=torch.long, device=dev)
    rates = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _flac_ws.get("flac_in", lib.mtts_flac_decode_workspace_bytes(B, ld_bytes, ld, int(max_block)), dev)
    with torch.cuda.device(dev):
        _hip.check(lib.mtts_flac_decode(_hip.ptr(data), ld_bytes, _hip.ptr(nbytes), B, int(max_block), _hip.ptr(out), ld, _hip.ptr(lengths),
                                        _hip.ptr(rates), ws.data_ptr(), ws.numel(), _hip.stream_ptr()))
    if check:
        _hip.raise_refused(lib.mtts_pcm_status, _hip.ptr(lengths), B, _hip.stream_ptr(), prefix="decode_flac: a stream was refused; ")
    return out, lengths, rates


def _rows_of_bytes(tensors, dev) -> torch.Tensor:
    """1-D uint8 tensors (host or device) as rows of one device buffer [n, nb], nb a multiple of 16: one copy of the host ones."""
    nb = max(16, (max(int(t.numel()) for t in tensors) + 15) // 16 * 16)
    host = torch.zeros(len(tensors), nb, dtype=torch.uint8)
    on_device = []
    for i, t in enumerate(tensors):
        if t.is_cuda:
            on_device.append((i, t))
        else:
            host[i, :t.numel()].copy_(t)
    data = host.to(dev)
    for i, t in on_device:
        data[i, :t.numel()].copy_(t.to(dev))
    return data


def decode_clips(clips: Sequence[Union[Encoded, "FlacClip"]], dev, check: bool = False) -> Tuple[torch.Tensor, list]:
    """``Encoded`` and ``FlacClip`` clips -> ``(float32 [n, ld] on ``dev``, sample counts)``: the ``Encoded`` ones with one copy of
    their bytes and one decode launch, the ``FlacClip`` ones with one copy and one ``decode_flac`` call.  The sample counts come from the
    payload sizes and from the clips' ``samples`` on the host, so nothing is waited for; a FLAC stream the device refuses (or one whose
    STREAMINFO disagrees with the clip's fields) leaves its row zeros, and ``check=True`` waits for that verdict and raises."""
    flac = [i for i, c in enumerate(clips) if isinstance(c, FlacClip)]
    if not flac:
        return _decode_encoded(clips, dev)
    counts = [int(c.numel()) for c in clips]
    ld = max(4, (max(counts) + 3) // 4 * 4)
    streams = [clips[i] for i in flac]
    data = _rows_of_bytes([c.tensor() for c in streams], dev)
    audio, lengths, _ = decode_flac(data, [c.nbytes for c in streams], ld=max(counts[i] for i in flac),
                                    max_block=max(c.max_block for c in streams), check=False)
    if check:
        want = torch.tensor([counts[i] for i in flac], dtype=torch.long, device=audio.device)
        verdict = torch.where(lengths == want, lengths, torch.full_like(lengths, -1))
        _hip.raise_refused(_hip.load().mtts_pcm_status, _hip.ptr(verdict), len(flac), _hip.stream_ptr(),
                           prefix="a FLAC clip was refused (rows count the FLAC clips only); ")
    rest = [i for i in range(len(clips)) if i not in flac]
    if not rest:
        return audio, counts
    wave = torch.zeros(len(clips), ld, dtype=torch.float32, device=audio.device)
    wave[flac, :audio.shape[1]] = audio
    plain, _ = _decode_encoded([clips[i] for i in rest], dev)
    wave[rest, :plain.shape[1]] = plain
    return wave, counts


def _decode_encoded(clips: Sequence[Encoded], dev) -> Tuple[torch.Tensor, list]:
    """``decode_clips`` of ``Encoded`` clips alone: one copy of the bytes and one decode launch."""
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

"""CPU checks of the layer between the queue and the waveform tail (nothing runs on a GPU and the library is not loaded): with a
fake model and fakes for the tail, every kind of batch -- plain requests, documents, both -- makes the one ``synthesise`` call it always
made, asks the tail for the plan it always asked for, and leaves the result dicts it always left; so do the per-request loop
(``wave_batch=False``), ``StepBatcher._finish`` and the service's two entries.  The expected values below are literals recorded from
the commit before the batcher got its one unit-to-tail path: this file, run there as ``RECORD=1 pytest tests/test_batch_units.py -s``,
which prints them in place of asserting.  Every entry point used here (``synthesise_batch``, ``StepBatcher._finish``, the batchers'
and the service's ``submit*``) has the same name and arguments on both sides, so the file needs no switch between them.

The fake tail resolves its options with the real ``waveform._resolve`` and records the plan: which stages run over how many results
with which per-result values, not how the keywords were spelled.  ``keys`` is recorded only where the plan has an encoder, its one
reader."""
import dataclasses
import os
import threading
import types

import pytest
import torch

from conftest import sub

F = 3                       # mel channels of the fake model
RECORD = bool(os.environ.get("RECORD"))


def plain(v):
    """``v`` with tensors reduced to dtype + shape (small integer ones to their values), so that it compares and prints as a literal."""
    if torch.is_tensor(v):
        if v.dtype in (torch.int32, torch.int64) and v.numel() <= 64:
            return v.tolist()
        return f"{str(v.dtype).split('.')[1]}{list(v.shape)}"
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(plain(x) for x in v)
    return "nan" if isinstance(v, float) and v != v else v


class Model:
    """``synthesise`` records what it is asked and returns a mel of ``2 n + 1`` frames for a row of n tokens."""

    def __init__(self, log):
        self.log = log
        self.decoder = types.SimpleNamespace(solver=None)

    def state_dict(self):
        return {"w": torch.zeros(1)}

    def speaker_rows(self, voices):
        return ("rows of", plain(list(voices)))

    def synthesise(self, x, x_lengths, n_timesteps, **kw):
        self.log.append(("synthesise", self.decoder.solver, x.tolist(), x_lengths.tolist(), n_timesteps, plain(kw)))
        lens = [2 * n + 1 for n in x_lengths.tolist()]
        mel = torch.arange(len(lens) * F * max(lens), dtype=torch.float32).reshape(len(lens), F, max(lens))
        out = {"mel": mel, "mel_lengths": torch.tensor(lens)}
        if kw.get("return_timing"):
            out["token_ends"] = (torch.arange(x.shape[1], dtype=torch.int32)[None] + 1).repeat(len(lens), 1) * 4
        return out


@pytest.fixture
def world(monkeypatch):
    """``(bt, log, run)``: the batcher module, the record of every call made, and ``run(units, mode)`` -> what the batch left."""
    bt, wf, hip = sub("batcher"), sub("waveform"), sub("_hip")
    monkeypatch.setattr(hip, "load", lambda: pytest.fail("the library is not loaded in this test"))
    log = []

    def tail(mel, mel_lengths, vocoder, trim=True, silence_threshold_db=-60.0, **options):
        assert vocoder == "vocos" and trim is True
        B = mel.shape[0]
        plan = dataclasses.asdict(wf._resolve(lambda: B, **options))
        if plan["encs"] is None:
            plan["keys"] = None
        log.append(("tail", list(mel.shape), plain(torch.as_tensor(mel_lengths)), plain(plan),
                    {k: plain(options[k]) for k in ("token_ends", "x_lengths") if k in options}))
        n, csr = plan["n"], plan["csr"] or list(range(B + 1))
        out = wf.Tail([torch.zeros(10 + g, dtype=torch.float32 if not plan["encs"] or plan["encs"][g] is None else torch.uint8) for g in range(n)])
        if plan["segments"]:
            out.segments = [[(g + 0.25 * i, g + 0.25 * i + 0.125) for i in range(csr[g + 1] - csr[g])] for g in range(n)]
        if plan["report"]:
            out.report = [dict(lufs=-20.5 - g, gain=0.5 + g, lra=4.25, momentary_max=-18.0, short_term_max=-19.0, peak=0.5, true_peak=0.5)
                          if plan["meter"] else (-20.5 - g, 0.5 + g) for g in range(n)]
        if plan["marks"]:
            x_len = [int(v) for v in torch.as_tensor(options["x_lengths"]).tolist()]
            rows = [[(b + 0.5 * t, b + 0.5 * t + 0.25) for t in range(x_len[b])] for b in range(B)]
            out.marks = rows if plan["csr"] is None else [rows[csr[g]:csr[g + 1]] for g in range(n)]
        return out

    def decode(mel, vocoder):
        log.append(("decode", list(mel.shape)))
        return torch.zeros(1, 16 * mel.shape[2])

    def trim(audio):
        log.append(("trim", list(audio.shape)))
        return audio[:-8]

    def finish(waveform, **kw):
        log.append(("finish_request", list(waveform.shape), kw))
        rep = None if kw["loudness"] is None else (-20.5, 0.75) if kw["true_peak"] is None else dict(
            lufs=-20.5, gain=0.75, lra=4.25, momentary_max=-18.0, short_term_max=-19.0, peak=0.5, true_peak=0.5)
        return torch.zeros(waveform.numel() // 2, dtype=torch.float32 if kw["encoding"] is None else torch.uint8), rep

    monkeypatch.setattr(wf, "tail", tail)
    monkeypatch.setattr(wf, "_waveform_on_device", decode)
    monkeypatch.setattr(wf, "trim_trailing_silence", trim)
    monkeypatch.setattr(wf, "finish_request", finish)

    def run(units, mode):
        log.clear()
        vocoder, wave_batch = (None if mode == "mel" else "vocos"), mode != "loop"
        try:
            res = plain(bt.synthesise_batch(Model(log), units, vocoder, wave_batch, 2.5))
        except ValueError as e:
            res = ("ValueError", str(e))
        return list(log), res
    return bt, log, run


def units_of(bt, name):
    R = lambda n, **kw: bt.Request(ids=list(range(1, n + 1)), **kw)
    D = lambda rows, pauses, **kw: bt.Document(rows=rows, pauses_ms=pauses, **kw)
    return {
        "default": lambda: [R(3), R(5, speaker=4, scale_correction=0.9), R(2, voice_mix=[(2, 0.7), (6, 0.3)], length_scale=1.25,
                                                                             solver="euler", n_timesteps=2)],
        "formats": lambda: [R(3, sample_rate=8000, encoding="ulaw"), R(4, encoding="pcm16", dither=True, dither_key=77), R(2, encoding="flac"),
                            R(6)],
        "loudness": lambda: [R(3, loudness=-16), R(4), R(2, loudness=-23.0)],
        "ceiling": lambda: [R(3, loudness=-16, true_peak=-1), R(4, loudness=-20), R(5)],
        "durations": lambda: [R(3), R(4, durations=[2, 3, 1, 2])],
        "rate_only": lambda: [R(3, token_scale=[1, 2, 1]), R(2)],
        "timing": lambda: [R(4, token_scale=[1, 2, 1, 0.5]), R(3, token_extend=[0, 1, 0], breaks=[(1, 20)]),
                           R(5, marks=True, word_groups=[0, 0, -1, 1, 1]), R(2, marks=True)],
        "breaks_only": lambda: [R(3, breaks=[(0, 10), (2, 5.0)]), R(2)],
        "document": lambda: [D([R(3), R(4)], [100, 0])],
        "document_asks": lambda: [D([R(3, breaks=[(1, 20)], word_groups=[0, 0, 1], encoding="ulaw", loudness=-30), R(5, word_groups=[0, 0, -1, 1, 1]),
                                     R(2, word_groups=[0, -1], sample_rate=8000)],
                                    [100, 250, 0], level="sentence", sample_rate=16000, encoding="pcm16", dither=True, dither_key=5, loudness=-16,
                                    true_peak=-1, marks=True)],
        "document_and_requests": lambda: [R(3, marks=True), D([R(2), R(4, token_scale=[1, 1, 2, 1])], [40, 0], marks=True),
                                          R(4, loudness=-20, sample_rate=8000)],
        "document_and_plain": lambda: [D([R(2), R(6)], [40, 0]), R(3), R(5, encoding="flac", dither_key=7)],
    }[name]()


PLAIN = ("default", "formats", "loudness", "ceiling", "durations", "rate_only", "timing", "breaks_only")
DOCS = ("document", "document_asks", "document_and_requests", "document_and_plain")
BATCHES = [(n, "batched") for n in PLAIN + DOCS] + [(n, "loop") for n in PLAIN] + [("document", "loop")] \
    + [(n, "mel") for n in ("default", "formats", "rate_only", "timing", "breaks_only", "document")]

EXPECTED = {
    'default/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0], [1, 2, 3, 4, 5], [1, 2, 0, 0, 0]], [3, 5, 2], 4, {'speaker_embeddings': ('rows of', [0, 4, [(2, 0.7), (6, 0.3)]]), 'scale_correction': [1.0, 0.9, 1.0], 'length_scale': [1.0, 1.0, 1.25], 'per_request_padding': True, 'durations': None}), ('tail', [3, 3, 11], [7, 11, 5], {'n': 3, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': False, 'report': False, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]'}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'float32[11]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[12]'}]),
    'formats/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 0, 0], [1, 2, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]], [3, 4, 2, 6], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('tail', [4, 3, 13], [7, 9, 5, 13], {'n': 4, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [8000, 24000, 24000, 24000], 'encs': [1, 0, 3, None], 'dither': [False, True, False, False], 'keys': [0, 77, 0, 0], 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': False, 'report': False, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'uint8[10]', 'sample_rate': 8000, 'encoding': 'ulaw'}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'uint8[11]', 'encoding': 'pcm16'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'uint8[12]', 'encoding': 'flac'}, {'mel': 'float32[3, 13]', 'mel_length': 13, 'audio': 'float32[13]'}]),
    'loudness/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 3, 4], [1, 2, 0, 0]], [3, 4, 2], 4, {'speaker_embeddings': ('rows of', [0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('tail', [3, 3, 9], [7, 9, 5], {'n': 3, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': [-16.0, 'nan', -23.0], 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': False, 'report': True, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]', 'loudness': -20.5, 'gain': 0.5}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[11]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[12]', 'loudness': -22.5, 'gain': 2.5}]),
    'ceiling/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0], [1, 2, 3, 4, 0], [1, 2, 3, 4, 5]], [3, 4, 5], 4, {'speaker_embeddings': ('rows of', [0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('tail', [3, 3, 11], [7, 9, 11], {'n': 3, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': [-16.0, -20.0, 'nan'], 'ceilings': [-1.0, None, None], 'meter': True, 'timed': False, 'break_rows': None, 'segments': False, 'report': True, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]', 'loudness': -20.5, 'gain': 0.5, 'true_peak': -6.020599913279624, 'lra': 4.25}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[11]', 'loudness': -21.5, 'gain': 1.5}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'float32[12]'}]),
    'durations/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 3, 4]], [3, 4], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': [None, [2, 3, 1, 2]]}), ('tail', [2, 3, 9], [7, 9], {'n': 2, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': False, 'report': False, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]'}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[11]'}]),
    'rate_only/batched': ([('synthesise', 'midpoint', [[1, 2, 3], [1, 2, 0]], [3, 2], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None, 'token_scale': [[1, 2, 1], None]}), ('tail', [2, 3, 7], [7, 5], {'n': 2, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': False, 'report': False, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[11]'}]),
    'timing/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 4, 0], [1, 2, 3, 0, 0], [1, 2, 3, 4, 5], [1, 2, 0, 0, 0]], [4, 3, 5, 2], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None, 'token_scale': [[1, 2, 1, 0.5], None, None, None], 'token_extend': [None, [0, 1, 0], None, None], 'return_timing': True}), ('tail', [4, 3, 11], [9, 7, 11, 5], {'n': 4, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000, 24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': True, 'break_rows': [[], [(1, 480)], [], []], 'segments': False, 'report': False, 'marks': True}, {'token_ends': [[4, 8, 12, 16, 20], [4, 8, 12, 16, 20], [4, 8, 12, 16, 20], [4, 8, 12, 16, 20]], 'x_lengths': [4, 3, 5, 2]})], [{'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[10]'}, {'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[11]'}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'float32[12]', 'marks': {'tokens': [(2.0, 2.25), (2.5, 2.75), (3.0, 3.25), (3.5, 3.75), (4.0, 4.25)], 'words': [(2.0, 2.75), (3.5, 4.25)]}}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[13]', 'marks': {'tokens': [(3.0, 3.25), (3.5, 3.75)]}}]),
    'breaks_only/batched': ([('synthesise', 'midpoint', [[1, 2, 3], [1, 2, 0]], [3, 2], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None, 'return_timing': True}), ('tail', [2, 3, 7], [7, 5], {'n': 2, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [24000, 24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': True, 'break_rows': [[(0, 240), (2, 120)], []], 'segments': False, 'report': False, 'marks': True}, {'token_ends': [[4, 8, 12], [4, 8, 12]], 'x_lengths': [3, 2]})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[11]'}]),
    'document/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 3, 4]], [3, 4], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('tail', [2, 3, 9], [7, 9], {'n': 1, 'csr': [0, 2], 'gaps': [2400, 0], 'fade': 60, 'levels': ['document'], 'rates': [24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': True, 'report': False, 'marks': False}, {})], [{'audio': 'float32[10]', 'segments': [(0.0, 0.125), (0.25, 0.375)], 'mel_lengths': [7, 9]}]),
    'document_asks/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0], [1, 2, 3, 4, 5], [1, 2, 0, 0, 0]], [3, 5, 2], 4, {'speaker_embeddings': ('rows of', [0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None, 'return_timing': True}), ('tail', [3, 3, 11], [7, 11, 5], {'n': 1, 'csr': [0, 3], 'gaps': [2400, 6000, 0], 'fade': 60, 'levels': ['sentence'], 'rates': [16000], 'encs': [0], 'dither': [True], 'keys': [5], 'targets': [-16.0], 'ceilings': [-1.0], 'meter': True, 'timed': True, 'break_rows': [[(1, 480)], [], []], 'segments': True, 'report': True, 'marks': True}, {'token_ends': [[4, 8, 12, 16, 20], [4, 8, 12, 16, 20], [4, 8, 12, 16, 20]], 'x_lengths': [3, 5, 2]})], [{'audio': 'uint8[10]', 'segments': [(0.0, 0.125), (0.25, 0.375), (0.5, 0.625)], 'mel_lengths': [7, 11, 5], 'sample_rate': 16000, 'encoding': 'pcm16', 'loudness': -20.5, 'gain': 0.5, 'true_peak': -6.020599913279624, 'lra': 4.25, 'marks': {'tokens': [[(0.0, 0.25), (0.5, 0.75), (1.0, 1.25)], [(1.0, 1.25), (1.5, 1.75), (2.0, 2.25), (2.5, 2.75), (3.0, 3.25)], [(2.0, 2.25), (2.5, 2.75)]], 'words': [[(0.0, 0.75), (1.0, 1.25)], [(1.0, 1.75), (2.5, 3.25)], [(2.0, 2.25)]]}}]),
    'document_and_requests/batched': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 0, 0], [1, 2, 3, 4], [1, 2, 3, 4]], [3, 2, 4, 4], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None, 'token_scale': [None, None, [1, 1, 2, 1], None], 'return_timing': True}), ('tail', [4, 3, 9], [7, 5, 9, 9], {'n': 3, 'csr': [0, 1, 3, 4], 'gaps': [0, 960, 0, 0], 'fade': 60, 'levels': ['sentence', 'document', 'sentence'], 'rates': [24000, 24000, 8000], 'encs': None, 'dither': None, 'keys': None, 'targets': ['nan', 'nan', -20.0], 'ceilings': None, 'meter': False, 'timed': True, 'break_rows': None, 'segments': True, 'report': True, 'marks': True}, {'token_ends': [[4, 8, 12, 16], [4, 8, 12, 16], [4, 8, 12, 16], [4, 8, 12, 16]], 'x_lengths': [3, 2, 4, 4]})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[10]', 'marks': {'tokens': [(0.0, 0.25), (0.5, 0.75), (1.0, 1.25)]}}, {'audio': 'float32[11]', 'segments': [(1.0, 1.125), (1.25, 1.375)], 'mel_lengths': [5, 9], 'marks': {'tokens': [[(1.0, 1.25), (1.5, 1.75)], [(2.0, 2.25), (2.5, 2.75), (3.0, 3.25), (3.5, 3.75)]]}}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[12]', 'sample_rate': 8000, 'loudness': -22.5, 'gain': 2.5}]),
    'document_and_plain/batched': ([('synthesise', 'midpoint', [[1, 2, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6], [1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 5, 0]], [2, 6, 3, 5], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('tail', [4, 3, 13], [5, 13, 7, 11], {'n': 3, 'csr': [0, 2, 3, 4], 'gaps': [960, 0, 0, 0], 'fade': 60, 'levels': ['document', 'sentence', 'sentence'], 'rates': [24000, 24000, 24000], 'encs': [None, None, 3], 'dither': [False, False, False], 'keys': [0, 0, 7], 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': True, 'report': False, 'marks': False}, {})], [{'audio': 'float32[10]', 'segments': [(0.0, 0.125), (0.25, 0.375)], 'mel_lengths': [5, 13]}, {'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[11]'}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'uint8[12]', 'encoding': 'flac'}]),
    'default/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0], [1, 2, 3, 4, 5], [1, 2, 0, 0, 0]], [3, 5, 2], 4, {'speaker_embeddings': ('rows of', [0, 4, [(2, 0.7), (6, 0.3)]]), 'scale_correction': [1.0, 0.9, 1.0], 'length_scale': [1.0, 1.0, 1.25], 'per_request_padding': True, 'durations': None}), ('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 11]), ('trim', [176]), ('finish_request', [168], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 5]), ('trim', [80]), ('finish_request', [72], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[52]'}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'float32[84]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[36]'}]),
    'formats/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 0, 0], [1, 2, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]], [3, 4, 2, 6], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 8000, 'encoding': 'ulaw', 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 9]), ('trim', [144]), ('finish_request', [136], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': 'pcm16', 'dither': True, 'dither_key': 77}), ('decode', [1, 3, 5]), ('trim', [80]), ('finish_request', [72], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': 'flac', 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 13]), ('trim', [208]), ('finish_request', [200], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'uint8[52]', 'sample_rate': 8000, 'encoding': 'ulaw'}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'uint8[68]', 'encoding': 'pcm16'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'uint8[36]', 'encoding': 'flac'}, {'mel': 'float32[3, 13]', 'mel_length': 13, 'audio': 'float32[100]'}]),
    'loudness/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 3, 4], [1, 2, 0, 0]], [3, 4, 2], 4, {'speaker_embeddings': ('rows of', [0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': -16.0, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 9]), ('trim', [144]), ('finish_request', [136], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 5]), ('trim', [80]), ('finish_request', [72], {'loudness': -23.0, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[52]', 'loudness': -20.5, 'gain': 0.75}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[68]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[36]', 'loudness': -20.5, 'gain': 0.75}]),
    'ceiling/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0], [1, 2, 3, 4, 0], [1, 2, 3, 4, 5]], [3, 4, 5], 4, {'speaker_embeddings': ('rows of', [0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': -16.0, 'true_peak': -1.0, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 9]), ('trim', [144]), ('finish_request', [136], {'loudness': -20.0, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 11]), ('trim', [176]), ('finish_request', [168], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[52]', 'loudness': -20.5, 'gain': 0.75, 'true_peak': -6.020599913279624, 'lra': 4.25}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[68]', 'loudness': -20.5, 'gain': 0.75}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'float32[84]'}]),
    'durations/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 3, 4]], [3, 4], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': [None, [2, 3, 1, 2]]}), ('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 9]), ('trim', [144]), ('finish_request', [136], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[52]'}, {'mel': 'float32[3, 9]', 'mel_length': 9, 'audio': 'float32[68]'}]),
    'rate_only/loop': ([('synthesise', 'midpoint', [[1, 2, 3], [1, 2, 0]], [3, 2], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None, 'token_scale': [[1, 2, 1], None]}), ('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 5]), ('trim', [80]), ('finish_request', [72], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'float32[52]'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[36]'}]),
    'timing/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 4, 0], [1, 2, 3, 0, 0], [1, 2, 3, 4, 5], [1, 2, 0, 0, 0]], [4, 3, 5, 2], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None, 'token_scale': [[1, 2, 1, 0.5], None, None, None], 'token_extend': [None, [0, 1, 0], None, None], 'return_timing': True})], ('ValueError', 'marks and breaks run in the batched tail: they need wave_batch=True')),
    'breaks_only/loop': ([('synthesise', 'midpoint', [[1, 2, 3], [1, 2, 0]], [3, 2], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None, 'return_timing': True})], ('ValueError', 'marks and breaks run in the batched tail: they need wave_batch=True')),
    'document/loop': ([('synthesise', 'midpoint', [[1, 2, 3, 0], [1, 2, 3, 4]], [3, 4], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None}), ('tail', [2, 3, 9], [7, 9], {'n': 1, 'csr': [0, 2], 'gaps': [2400, 0], 'fade': 60, 'levels': ['document'], 'rates': [24000], 'encs': None, 'dither': None, 'keys': None, 'targets': None, 'ceilings': None, 'meter': False, 'timed': False, 'break_rows': None, 'segments': True, 'report': False, 'marks': False}, {})], [{'audio': 'float32[10]', 'segments': [(0.0, 0.125), (0.25, 0.375)], 'mel_lengths': [7, 9]}]),
    'default/mel': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0], [1, 2, 3, 4, 5], [1, 2, 0, 0, 0]], [3, 5, 2], 4, {'speaker_embeddings': ('rows of', [0, 4, [(2, 0.7), (6, 0.3)]]), 'scale_correction': [1.0, 0.9, 1.0], 'length_scale': [1.0, 1.0, 1.25], 'per_request_padding': True, 'durations': None})], [{'mel': 'float32[3, 7]', 'mel_length': 7}, {'mel': 'float32[3, 11]', 'mel_length': 11}, {'mel': 'float32[3, 5]', 'mel_length': 5}]),
    'formats/mel': ([('synthesise', 'midpoint', [[1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 0, 0], [1, 2, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]], [3, 4, 2, 6], 4, {'speaker_embeddings': ('rows of', [0, 0, 0, 0]), 'scale_correction': [1.0, 1.0, 1.0, 1.0], 'length_scale': [1.0, 1.0, 1.0, 1.0], 'per_request_padding': True, 'durations': None})], [{'mel': 'float32[3, 7]', 'mel_length': 7}, {'mel': 'float32[3, 9]', 'mel_length': 9}, {'mel': 'float32[3, 5]', 'mel_length': 5}, {'mel': 'float32[3, 13]', 'mel_length': 13}]),
    'rate_only/mel': ([('synthesise', 'midpoint', [[1, 2, 3], [1, 2, 0]], [3, 2], 4, {'speaker_embeddings': ('rows of', [0, 0]), 'scale_correction': [1.0, 1.0], 'length_scale': [1.0, 1.0], 'per_request_padding': True, 'durations': None, 'token_scale': [[1, 2, 1], None]})], [{'mel': 'float32[3, 7]', 'mel_length': 7}, {'mel': 'float32[3, 5]', 'mel_length': 5}]),
    'timing/mel': ([], ('ValueError', 'marks and breaks need a vocoder: they are positions in the audio')),
    'breaks_only/mel': ([], ('ValueError', 'marks and breaks need a vocoder: they are positions in the audio')),
    'document/mel': ([], ('ValueError', 'a document needs a vocoder: its result is the joined audio')),
}


@pytest.mark.parametrize("name,mode", BATCHES, ids=[f"{n}-{m}" for n, m in BATCHES])
def test_a_batch_makes_the_calls_and_leaves_the_results_of_before(world, name, mode):
    bt, _, run = world
    got = run(units_of(bt, name), mode)
    if RECORD:
        print(f"    {name + '/' + mode!r}: {got!r},")
        return
    assert got == EXPECTED[f"{name}/{mode}"]


STEP_EXPECTED = {
    True: ([('tail', [3, 3, 11], [7, 11, 5], {'n': 3, 'csr': None, 'gaps': None, 'fade': 120, 'levels': None, 'rates': [8000, 24000, 24000], 'encs': [1, 3, None], 'dither': [False, True, False], 'keys': [0, 7, 0], 'targets': [-16.0, 'nan', -23.0], 'ceilings': [None, None, -1.0], 'meter': True, 'timed': False, 'break_rows': None, 'segments': False, 'report': True, 'marks': False}, {})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'uint8[10]', 'sample_rate': 8000, 'encoding': 'ulaw', 'loudness': -20.5, 'gain': 0.5}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'uint8[11]', 'encoding': 'flac'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[12]', 'loudness': -22.5, 'gain': 2.5, 'true_peak': -6.020599913279624, 'lra': 4.25}]),
    False: ([('decode', [1, 3, 7]), ('trim', [112]), ('finish_request', [104], {'loudness': -16.0, 'true_peak': None, 'report': True, 'sample_rate': 8000, 'encoding': 'ulaw', 'dither': False, 'dither_key': 0}), ('decode', [1, 3, 11]), ('trim', [176]), ('finish_request', [168], {'loudness': None, 'true_peak': None, 'report': True, 'sample_rate': 24000, 'encoding': 'flac', 'dither': True, 'dither_key': 7}), ('decode', [1, 3, 5]), ('trim', [80]), ('finish_request', [72], {'loudness': -23.0, 'true_peak': -1.0, 'report': True, 'sample_rate': 24000, 'encoding': None, 'dither': False, 'dither_key': 0})], [{'mel': 'float32[3, 7]', 'mel_length': 7, 'audio': 'uint8[52]', 'sample_rate': 8000, 'encoding': 'ulaw', 'loudness': -20.5, 'gain': 0.75}, {'mel': 'float32[3, 11]', 'mel_length': 11, 'audio': 'uint8[84]', 'encoding': 'flac'}, {'mel': 'float32[3, 5]', 'mel_length': 5, 'audio': 'float32[36]', 'loudness': -20.5, 'gain': 0.75, 'true_peak': -6.020599913279624, 'lra': 4.25}]),
}


@pytest.mark.parametrize("wave_batch", [True, False])
def test_the_step_batchers_finishers_go_the_same_way(world, wave_batch):
    bt, log, _ = world
    q = bt.StepBatcher.__new__(bt.StepBatcher)                  # the leaving half alone: no thread, no pool
    rt = types.SimpleNamespace(ready=lambda: None, guards=lambda policy: False, mel_std=1.0, mel_mean=0.0)
    q.model = types.SimpleNamespace(_rt=rt, range_policy="raise", decoder=types.SimpleNamespace(
        step_read=lambda pool, slot, y_len, std, mean: torch.full((F, y_len), float(slot))))
    q.vocoder, q.wave_batch, q._fake, q._flags, q._pool, q._cv = "vocos", wave_batch, False, None, None, threading.Condition()
    q.slots = bt.SlotBook(4)
    requests = [bt.Request(ids=[1, 2, 3], sample_rate=8000, encoding="ulaw", loudness=-16),
                bt.Request(ids=[1, 2, 3, 4, 5], encoding="flac", dither=True, dither_key=7), bt.Request(ids=[1, 2], loudness=-23, true_peak=-1)]
    q._active = [bt.StepEntry(r, q.slots.take(), bt.step_grid(1), i=1, y_len=2 * len(r.ids) + 1) for r in requests]
    staying = bt.StepEntry(bt.Request(ids=[1, 2, 3, 4], sample_rate=16000), q.slots.take(), bt.step_grid(2), i=1, y_len=9)
    finished = list(q._active)
    q._active.append(staying)
    q._finish(finished)
    got = (list(log), [plain(r.future.result(timeout=0)) for r in requests])
    assert q._active == [staying] and q.slots.n_free == 3 and not staying.request.future.done()
    if RECORD:
        print(f"    {wave_batch!r}: {got!r},")
        return
    assert got == STEP_EXPECTED[wave_batch]


class Queue:
    """A batcher's producer side: records what the service submits."""

    def __init__(self):
        self.seen = []

    def submit(self, ids, **kw):
        self.seen.append(("submit", list(ids), plain(kw)))

    def submit_document(self, ids, pauses, **kw):
        self.seen.append(("submit_document", [list(i) for i in ids], list(pauses), plain(kw)))


SERVICE_EXPECTED = [
    ('submit', [13, 9, 48, 6, 11], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0}),
    ('submit', [48, 16, 8, 16], {'speaker': 0, 'voice_mix': [(2, 0.7), (6, 0.3)], 'solver': 'euler', 'n_timesteps': 2, 'scale_correction': 1.05, 'length_scale': 0.5, 'speaker_embedding': ('float32[4]', 'float32[4]'), 'sample_rate': 8000, 'encoding': 'ulaw'}),
    ('submit', [9, 2, 19, 2, 9, 9], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0, 'sample_rate': 48000, 'encoding': 'flac', 'loudness': -23.0, 'true_peak': -1.0, 'marks': True, 'word_groups': [0, 0, 1, 1, 2, 2]}),
    ('submit', [48, 33, 19, 6, 2, 20], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0, 'loudness': -16.0, 'true_peak': -2.0, 'marks': True}),
    ('submit_document', [[30, 11, 2, 47], [16, 11, 1, 33, 17, 20]], [300.0, 600.0], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0}),
    ('submit_document', [[30, 11, 2, 47], [16, 11, 1, 33, 17, 20]], [300.0, 600.0], {'speaker': 3, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.03, 'length_scale': 2.0, 'sample_rate': 16000, 'encoding': 'pcm16', 'loudness': -19.0, 'true_peak': -3.0, 'marks': True}),
    ('submit_document', [[30, 11, 2, 47], [16, 11, 1, 33, 17, 20]], [300.0, 600.0], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0, 'speaker_embedding': ('float32[4]', 'float32[4]'), 'loudness': -23.0, 'true_peak': -1.0, 'marks': True, 'word_groups': [[0, 0, 1, 1], [0, 0, 1, 1, 2, 2]]}),
    ('submit_document', [[30, 11, 2, 47], [16, 11, 1, 33, 17, 20]], [300.0, 600.0], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0}),
    ('submit_document', [[30, 11, 2, 47], [16, 11, 1, 33, 17, 20]], [300.0, 600.0], {'speaker': 0, 'voice_mix': None, 'solver': 'midpoint', 'n_timesteps': 4, 'scale_correction': 1.08, 'length_scale': 1.0, 'loudness': -30.0, 'true_peak': -1.0, 'marks': True, 'word_groups': [[0, 0, 1, 1], [0, 0, 1, 1, 2, 2]]}),
]


def test_the_services_entries_name_the_fields_of_before():
    sv = sub("serving")
    q = Queue()
    phonemize = lambda text, lang: [1 + (ord(c) % 50) for c in text][:6]
    words = lambda text, lang, ids: [i // 2 for i in range(len(ids))]
    svc = sv.SpeechService(q, phonemize, flac=True)
    full = sv.SpeechService(q, phonemize, loudness=-23, true_peak=-1, marks=True, word_groups=words, flac=True)
    text = "One. And two."
    svc.submit("plain")
    svc.submit("asks", "2(70)+6(30)", 2.0, 2, "euler", (torch.zeros(4), torch.ones(4)), 8000, "ulaw")
    full.submit("levelled", sample_rate=48000, response_format="flac")
    svc.levelled(-16, -2).timed().submit("a view")
    svc.submit_long(text)
    svc.submit_long(text, 3, 0.5, sample_rate=16000, response_format="wav", loudness=-19, true_peak=-3, marks=True)
    full.submit_long(text, speaker_embedding=(torch.zeros(4), torch.ones(4)))
    full.submit_long(text, loudness=None, marks=False)
    full.submit_long(text, loudness=-30)
    if RECORD:
        print("SERVICE_EXPECTED = [\n" + "".join(f"    {s!r},\n" for s in q.seen) + "]")
        return
    assert q.seen == SERVICE_EXPECTED


def test_refusals_keep_their_type_their_place_and_their_words(world):
    bt, log, run = world
    sv, inf = sub("serving"), sub("inference")
    R = lambda n=2, **kw: bt.Request(ids=list(range(1, n + 1)), **kw)
    # a ceiling needs a target: one rule, wherever it is asked
    document = lambda **kw: bt.Document(rows=[R()], pauses_ms=[0], **kw)
    svc = sv.SpeechService(Queue(), lambda text, lang: [1, 2])
    for make in (lambda: R(true_peak=-1.0), lambda: document(true_peak=-1.0), lambda: sv.SpeechService(None, None, true_peak=-1.0),
                 lambda: svc.levelled(None, -1.0), lambda: svc.submit_long("never submitted", true_peak=-1.0),
                 lambda: svc.submit_long("never submitted", loudness=None, true_peak=-1.0),
                 lambda: inf.pipeline(None, None, "never spoken", true_peak=-1.0), lambda: sv.checked_ceiling(-1.0, None)):
        with pytest.raises(ValueError, match="target"):
            make()
    for make in (R, document):
        with pytest.raises(ValueError, match="dBTP"):
            make(loudness=-23, true_peak=0.5)                     # (what is no ceiling is refused ahead of the rule)
        with pytest.raises(TypeError, match="dBTP"):
            make(true_peak="hot")
        with pytest.raises(ValueError, match="LUFS"):
            make(loudness=1.0)
        with pytest.raises(ValueError, match="unknown audio format 'mp3'"):
            make(encoding="mp3")
    assert svc.batcher.seen == []
    # inside the batch
    said = {
        ("document", "mel"): "a document needs a vocoder: its result is the joined audio",
        ("timing", "mel"): "marks and breaks need a vocoder: they are positions in the audio",
        ("breaks_only", "mel"): "marks and breaks need a vocoder: they are positions in the audio",
        ("timing", "loop"): "marks and breaks run in the batched tail: they need wave_batch=True",
    }
    for (name, mode), words in said.items():
        calls, res = run(units_of(bt, name), mode)
        assert res == ("ValueError", words)
        assert [c[0] for c in calls] == (["synthesise"] if mode == "loop" else [])     # ahead of the solve where it can be known there
    # at submit, before anything is queued
    ran = []
    with bt.FrameBudgetBatcher(None, max_batch=2, max_tokens=8, max_wait_ms=1.0, run_batch=lambda batch: ran.append(batch) or [{}] * len(batch)) as q, \
            bt.StepBatcher(None, max_batch=2, max_tokens=8, run_step=lambda solver, entries: ran.append(entries)) as s:
        for b in (q, s):
            for ids, kw, words in (([], {}, "empty utterance"), ([1] * 9, {}, "utterance of 9 tokens exceeds the batch budget of 8"),
                                   ([1, 2], dict(durations=[1.0]), "a request's durations need one value per token (2), got 1"),
                                   ([1, 2], dict(token_scale=[1.0]), "a request's token_scale needs one value per token (2), got 1")):
                with pytest.raises(ValueError) as e:
                    b.submit(ids, **kw)
                assert str(e.value) == words
        for kw in (dict(marks=True), dict(breaks=[(0, 10)]), dict(token_scale=[1.0, 2.0]), dict(token_extend=[0.0, 1.0])):
            with pytest.raises(ValueError) as e:
                s.submit([1, 2], **kw)
            assert str(e.value) == ("token_scale, token_extend, breaks and marks are served by FrameBudgetBatcher: the step-level admission "
                                    "path does not take them")
        with pytest.raises(ValueError, match="n_timesteps must be at least 1"):
            s.submit([1, 2], n_timesteps=0)
        assert not hasattr(s, "submit_document")
        for segments, pauses, kw, words in (
                ([[1], []], [0, 0], {}, "empty segment in a document"),
                ([[1], [2], [3]], [0, 0, 0], {}, "a document of 3 segments exceeds the batch of 2 utterances"),
                ([[1] * 5, [2]], [0, 0], {}, "a document of 2 segments of up to 5 tokens exceeds the batch budget of 8"),
                ([[1], [2]], [0], {}, "a document's pauses need one value per segment (2), got 1"),
                ([[1], [2]], [0, 0], dict(breaks=[None]), "a document's breaks need one entry per segment (2), got 1"),
                ([[1], [2]], [0, 0], dict(level="word"), "level is 'document' or 'sentence', got 'word'"),
                ([[1], [2]], [0, 0], dict(durations=[1.0, 2.0]), "a request's durations need one value per token (1), got 2")):
            with pytest.raises(ValueError) as e:
                q.submit_document(segments, pauses, **kw)
            assert str(e.value) == words
    assert ran == []
    for b in (q, s):
        with pytest.raises(RuntimeError, match="batcher is closed"):
            b.submit([1, 2])
    with pytest.raises(RuntimeError, match="batcher is closed"):
        q.submit_document([[1], [2]], [0, 0])


def test_the_wave_batch_switch_is_read_per_batcher_at_construction(monkeypatch):
    bt = sub("batcher")
    for value, want in (("0", False), ("1", True), (None, True)):
        monkeypatch.delenv("MTTS_WAVE_BATCH", raising=False)
        if value is not None:
            monkeypatch.setenv("MTTS_WAVE_BATCH", value)
        with bt.FrameBudgetBatcher(None, run_batch=lambda batch: []) as q, bt.StepBatcher(None, run_step=lambda solver, entries: None) as s:
            monkeypatch.setenv("MTTS_WAVE_BATCH", "1" if value == "0" else "0")        # (later changes are not looked at)
            assert q.wave_batch is want and s.wave_batch is want


def test_one_builder_and_no_per_field_lists():
    import inspect
    bt = sub("batcher")
    for gone in ("synthesise_units", "encoding_fields", "loudness_field", "true_peak_field", "timing_fields", "_checked_ceiling"):
        assert not hasattr(bt, gone), gone
    p = inspect.signature(bt.waveforms_into).parameters
    assert not {"sample_rates", "encodings", "dithers", "dither_keys", "loudness", "true_peak"} & set(p) and "units" in p
    src = inspect.getsource(bt)
    for word in ("return_loudness=", "return_meter=", "return_marks="):
        assert src.count(word) == 1, word

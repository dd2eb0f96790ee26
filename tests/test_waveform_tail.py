"""CPU checks of the batched waveform tail (nothing runs on a GPU and the library is not loaded): with fakes for the stages, every
option combination of ``to_waveforms`` makes the stage calls it always made, in the documented order and over the same row counts,
reads the device as often as it did, and returns the tuple shapes it returned.  The expected values below are literals recorded
from the commit before the tail moved to ``waveform.py``: this file with ``TAIL = "inference"`` (the module that then looked the
stages up), run there as ``RECORD=1 pytest tests/test_waveform_tail.py -s``, which prints them in place of asserting."""
import inspect
import math
import os
import types

import pytest
import torch

from conftest import sub

TAIL = "waveform"           # the module that looks the stages up
HOP, T, LENGTHS = 16, 40, [40, 33, 25, 12]
TRIMMED = [600, 480, 300, 100]


class Dev(torch.Tensor):
    """A tensor that stands for device memory: reading it on the host is counted."""
    reads = 0

    def _read(self):
        Dev.reads += 1
        return self.as_subclass(torch.Tensor)

    def cpu(self, *a, **k):
        return self._read()

    def tolist(self):
        return self._read().tolist()

    def item(self):
        return self._read().item()

    def __int__(self):
        return int(self._read())

    def __float__(self):
        return float(self._read())

    def __bool__(self):
        return bool(self._read())

    __index__ = __int__


def dev(t):
    return t.as_subclass(Dev)


def host(t):
    return t.as_subclass(torch.Tensor) if isinstance(t, Dev) else torch.as_tensor(t)


@pytest.fixture
def stages(monkeypatch):
    """The tail module with every stage replaced by a fake that records ``(name, rows, ...)`` and computes something recognisable."""
    inf, tail, hip = sub("inference"), sub(TAIL), sub("_hip")          # (inference binds the real names before any is replaced)
    tm, ld, rs, ac = sub("timing"), sub("loudness"), sub("resample"), sub("audio_codec")
    calls = []

    def on_device(make):
        def f(*a, pin_memory=False, device=None, **kw):
            out = make(*a, **kw)
            return out if device is None else dev(out)
        return f

    for name in ("tensor", "zeros", "empty"):
        monkeypatch.setattr(torch, name, on_device(getattr(torch, name)))

    class Head:
        cfg = {"hop": HOP}

        def decode(self, mel, lengths, check=True):
            calls.append(("decode", mel.shape[0]))
            B = mel.shape[0]
            return dev((torch.arange(B, dtype=torch.float32)[:, None] + 1.0).repeat(1, HOP * mel.shape[2]).contiguous())

    def finish(audio, lengths, hop=0, silence_threshold_db=-60.0):
        calls.append(("finish", audio.shape[0], hop))
        n = host(lengths)
        keep = torch.where((n < 1) | (n > T), torch.full_like(n, -1), torch.tensor(TRIMMED[:len(n)]))
        return dev(keep), dev(torch.full((audio.shape[0],), 0.5))

    def token_marks(cum, x_lengths, keep, breaks=None, **kw):
        calls.append(("token_marks", cum.shape[0], kw["fine_hop"], kw["keep_max"]))
        k = host(keep)
        add = torch.tensor([sum(p for _, p in (r or ())) for r in (breaks or [None] * len(k))])
        new = torch.where(k < 0, k, k + add)
        plan = types.SimpleNamespace(NB=sum(len(r or ()) for r in (breaks or [])), raise_refused=lambda: None, lengths=dev(new),
                                     extra=int(add.max()))
        marks = torch.full((len(k), 3, 2), -1, dtype=torch.long)
        for b, n in enumerate(new.tolist()):
            if n >= 0:
                marks[b, 0, 0], marks[b, 0, 1], marks[b, 1, 0], marks[b, 1, 1] = 0, n // 2, n // 2, n
        return dev(marks), dev(new.clone()), plan

    def apply_breaks(audio, plan, fade):
        calls.append(("apply_breaks", audio.shape[0], fade))
        return dev(torch.cat([host(audio), host(audio)[:, :1].repeat(1, (plan.extra + 3) // 4 * 4)], 1).contiguous())

    def join(audio, lengths, documents, gaps, fade=0, scale=None, check=True, out_ld=None):
        calls.append(("join", audio.shape[0], len(documents) - 1, fade, None if scale is None else host(scale).tolist(), check))
        a, n, B = host(audio), host(lengths).tolist(), audio.shape[0]
        gaps = [0] * B if gaps is None else list(gaps)
        parts, starts = [], [-1] * B
        for lo, hi in zip(documents[:-1], documents[1:]):
            if any(n[b] < 0 for b in range(lo, hi)):
                parts.append(None)
                continue
            row, at = [], 0
            for b in range(lo, hi):
                starts[b] = at
                row += [a[b, :n[b]]] + [torch.zeros(gaps[b])] * (b < hi - 1)
                at += n[b] + (gaps[b] if b < hi - 1 else 0)
            parts.append(torch.cat(row))
        ld = (max([4] + [len(p) for p in parts if p is not None]) + 3 + 8) // 4 * 4
        out = torch.zeros(len(parts), ld)
        for g, p in enumerate(parts):
            if p is not None:
                out[g, :len(p)] = p
        return dev(out), dev(torch.tensor([-1 if p is None else len(p) for p in parts])), dev(torch.tensor(starts))

    def normalize(rows, lengths, target, sample_rate=24000, peak_ceiling=0.95, check=True, true_peak=None, return_meter=False):
        assert rows.shape[1] % 4 == 0
        t = [float(v) for v in target]
        calls.append(("normalize", rows.shape[0], sum(v == v for v in t), true_peak, return_meter, check))
        r, n = host(rows), host(lengths).tolist()
        gain = torch.ones(len(t))
        for b, v in enumerate(t):
            if v == v and n[b] > 0:
                gain[b] = 0.5 if true_peak is None else 0.25
                r[b, :n[b]] *= gain[b]
        lufs = dev(torch.tensor([-20.0 - b for b in range(len(t))], dtype=torch.float64))
        peak = dev(torch.full((len(t),), 0.75))
        if not return_meter:
            return lufs, dev(gain), peak
        more = {k: dev(torch.full((len(t),), float(i), dtype=torch.float64)) for i, k in enumerate(("lra", "momentary_max", "short_term_max"))}
        return lufs, dev(gain), peak, dict(lufs=lufs, gain=dev(gain), peak=peak, true_peak=dev(torch.full((len(t),), 0.8)), **more)

    def resample(audio, lengths, orig_freq, new_freq, check=True, ld_out=None):
        calls.append(("resample", audio.shape[0], new_freq, check))
        a, n = host(audio), host(lengths)
        m = torch.where(n < 0, n, -((-n * new_freq) // orig_freq))
        out = torch.zeros(a.shape[0], (math.ceil(a.shape[1] * new_freq / orig_freq) + 3) // 4 * 4)
        for b, k in enumerate(m.tolist()):
            if k > 0:
                out[b, :k] = a[b, 0]
        return dev(out), dev(m)

    def encode(audio, lengths, formats, dither=False, seed=0, keys=None, check=False):
        calls.append(("encode", audio.shape[0], list(formats), dither, None if keys is None else list(keys), check))
        a, n = host(audio), host(lengths)
        bps = torch.tensor([ac.BYTES_PER_SAMPLE[f] for f in formats])
        data = torch.zeros(a.shape[0], 2 * ((a.shape[1] + 3) // 4 * 4), dtype=torch.uint8)
        for b in range(a.shape[0]):
            data[b] = b + 1
        return dev(data), dev(torch.where(n < 0, n, n * bps))

    monkeypatch.setattr(tail, "finish_waveforms", finish)
    monkeypatch.setattr(tail, "join_waveforms", join)
    monkeypatch.setattr(hip, "aligned_rows", lambda t, q, what, layout="": (t, t.shape[1]) if t.shape[1] % q == 0 else (
        dev(torch.nn.functional.pad(host(t), (0, -t.shape[1] % q))), t.shape[1]))
    monkeypatch.setattr(hip, "load", lambda: pytest.fail("the library is not loaded in this test"))
    monkeypatch.setattr(tm, "token_marks", token_marks)
    monkeypatch.setattr(tm, "apply_breaks", apply_breaks)
    monkeypatch.setattr(ld, "normalize", normalize)
    monkeypatch.setattr(rs, "resample", resample)
    monkeypatch.setattr(ac, "encode", encode)

    def run(**kw):
        calls.clear()
        Dev.reads = 0
        lengths = kw.pop("mel_lengths", LENGTHS)
        out = inf.to_waveforms(dev(torch.zeros(len(lengths), 20, T)), dev(torch.tensor(lengths)), Head(), **kw)
        return list(calls), Dev.reads, out
    return run


def inf_figures():
    return sub("inference").METER_FIGURES


def rows_of(res):
    return [f"{'u8' if a.dtype == torch.uint8 else 'f32'}x{len(a)}:{int(a.double().sum().round())}" for a in res]


def samples(pairs):
    return [(round(s * 24000), round(e * 24000)) for s, e in pairs]


def shape_of(out, kw):
    """The returned value, slot by slot: which slot is what follows from the flags alone, as the docstring of ``to_waveforms`` says."""
    if not isinstance(out, tuple):
        return [("rows", rows_of(out))]
    names = ["rows"] + ["segments"] * bool(kw.get("return_segments")) + ["report"] * bool(kw.get("return_loudness") or kw.get("return_meter")) \
        + ["marks"] * bool(kw.get("return_marks"))
    assert len(names) == len(out)
    got = []
    for name, slot in zip(names, out):
        if name == "rows":
            got.append((name, rows_of(slot)))
        elif name == "segments":
            got.append((name, [samples(doc) for doc in slot]))
        elif name == "report":
            got.append((name, ["meter" if isinstance(r, dict) and tuple(r) == inf_figures() else tuple(round(v, 3) for v in r) for r in slot]))
        else:
            got.append((name, [samples(r) if not r or isinstance(r[0], tuple) else [samples(x) for x in r] for r in slot]))
    return got


ENDS = dict(token_ends=torch.zeros(4, 3, dtype=torch.int32), x_lengths=[2, 2, 2, 2])
DOCS = dict(documents=[2, 2], gaps=[240, 0, 120, 0])
CASES = {
    "plain": dict(),
    "untrimmed": dict(trim=False),
    "rates": dict(sample_rate=[24000, 16000, 8000, 16000]),
    "rates_untrimmed": dict(trim=False, sample_rate=[24000, 16000, 24000, 24000]),
    "mixed_encodings": dict(encoding=["pcm16", None, "ulaw", "alaw"], dither=[True, False, False, True], dither_keys=[1, 2, 3, 4]),
    "all_encoded": dict(encoding="pcm16", dither=True),
    "encoded_untrimmed_rates": dict(trim=False, encoding=["ulaw", None, None, "pcm16"], sample_rate=[8000, 24000, 16000, 24000]),
    "loudness": dict(loudness=[-23.0, None, -16.0, None]),
    "loudness_report": dict(loudness=-23.0, return_loudness=True),
    "report_alone": dict(return_loudness=True),
    "one_ceiling": dict(loudness=[-23.0, None, -16.0, None], true_peak=-1.0, return_loudness=True),
    "two_ceilings": dict(loudness=[-23.0, -20.0, -16.0, None], true_peak=[-1.0, None, -2.0, None]),
    "meter": dict(loudness=[-23.0, None, None, None], return_meter=True),
    "meter_alone_encoded": dict(return_meter=True, encoding=[None, "pcm16", None, None]),
    "documents": dict(**DOCS),
    "documents_padded": dict(documents=[3], level="sentence", return_segments=True),
    "documents_levels": dict(**DOCS, level=["sentence", "document"], return_segments=True),
    "documents_untrimmed": dict(**DOCS, trim=False, return_segments=True),
    "documents_rates": dict(**DOCS, sample_rate=[16000, 24000]),
    "documents_encoded": dict(**DOCS, encoding=["pcm16", None], dither=[True, False], dither_keys=[7, 8], return_segments=True),
    "documents_all_encoded": dict(**DOCS, encoding="alaw", sample_rate=8000),
    "documents_loudness": dict(**DOCS, loudness=[None, -16.0], return_loudness=True),
    "documents_ceilings_meter": dict(**DOCS, loudness=[-23.0, -16.0], true_peak=[-1.0, -2.0], return_meter=True, return_segments=True),
    "marks": dict(**ENDS, return_marks=True),
    "breaks": dict(**ENDS, breaks=[None, [(0, 10.0)], None, [(0, 5.0), (1, 5.0)]]),
    "breaks_marks_untrimmed": dict(**ENDS, trim=False, breaks=[[(1, 20.0)], None, None, None], return_marks=True, fade_ms=2.0),
    "marks_encoded_report": dict(**ENDS, return_marks=True, encoding=["pcm16", None, None, None], loudness=-20.0, return_loudness=True),
    "documents_marks": dict(**DOCS, **ENDS, return_marks=True),
    "documents_breaks_marks": dict(**DOCS, **ENDS, breaks=[None, [(0, 10.0)], None, None], return_marks=True, return_segments=True),
    "everything": dict(**DOCS, **ENDS, breaks=[None, [(0, 10.0)], None, None], fade_ms=2.5, level=["document", "sentence"], trim=False,
                       loudness=[-23.0, None], true_peak=[-1.0, None], return_meter=True, sample_rate=[16000, 24000],
                       encoding=[None, "ulaw"], dither=[False, True], dither_keys=[5, 6], return_segments=True, return_marks=True),
}

EXPECTED = {
    'plain': ([('decode', 4), ('finish', 4, 16)], 2, [('rows', ['f32x600:600', 'f32x480:960', 'f32x300:900', 'f32x100:400'])]),
    'untrimmed': ([('decode', 4), ('finish', 4, 16)], 2, [('rows', ['f32x624:624', 'f32x512:1024', 'f32x384:1152', 'f32x176:704'])]),
    'rates': ([('decode', 4), ('finish', 4, 16), ('resample', 1, 8000, False), ('resample', 2, 16000, False)], 2, [('rows', ['f32x600:600', 'f32x320:640', 'f32x100:300', 'f32x67:268'])]),
    'rates_untrimmed': ([('decode', 4), ('finish', 4, 16), ('resample', 1, 16000, False)], 2, [('rows', ['f32x624:624', 'f32x342:684', 'f32x384:1152', 'f32x176:704'])]),
    'mixed_encodings': ([('decode', 4), ('finish', 4, 16), ('encode', 4, [0, 0, 1, 2], [True, False, False, True], [1, 2, 3, 4], False)], 3, [('rows', ['u8x1200:1200', 'f32x480:960', 'u8x300:900', 'u8x100:400'])]),
    'all_encoded': ([('decode', 4), ('finish', 4, 16), ('encode', 4, [0, 0, 0, 0], True, None, False)], 2, [('rows', ['u8x1200:1200', 'u8x960:1920', 'u8x600:1800', 'u8x200:800'])]),
    'encoded_untrimmed_rates': ([('decode', 4), ('finish', 4, 16), ('resample', 1, 8000, False), ('resample', 1, 16000, False), ('encode', 4, [1, 0, 0, 0], False, None, False)], 3, [('rows', ['u8x208:208', 'f32x512:1024', 'f32x256:768', 'u8x352:1408'])]),
    'loudness': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 2, None, False, False)], 2, [('rows', ['f32x600:300', 'f32x480:960', 'f32x300:450', 'f32x100:400'])]),
    'loudness_report': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 4, None, False, False)], 2, [('rows', ['f32x600:300', 'f32x480:480', 'f32x300:450', 'f32x100:200']), ('report', [(-20.0, 0.5), (-21.0, 0.5), (-22.0, 0.5), (-23.0, 0.5)])]),
    'report_alone': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 0, None, False, False)], 2, [('rows', ['f32x600:600', 'f32x480:960', 'f32x300:900', 'f32x100:400']), ('report', [(-20.0, 1.0), (-21.0, 1.0), (-22.0, 1.0), (-23.0, 1.0)])]),
    'one_ceiling': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 0, None, True, False), ('normalize', 4, 2, -1.0, True, False)], 2, [('rows', ['f32x600:150', 'f32x480:960', 'f32x300:225', 'f32x100:400']), ('report', [(-20.0, 0.25), (-21.0, 1.0), (-22.0, 0.25), (-23.0, 1.0)])]),
    'two_ceilings': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 1, None, True, False), ('normalize', 4, 1, -2.0, True, False), ('normalize', 4, 1, -1.0, True, False)], 2, [('rows', ['f32x600:150', 'f32x480:480', 'f32x300:225', 'f32x100:400'])]),
    'meter': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 1, None, True, False)], 2, [('rows', ['f32x600:300', 'f32x480:960', 'f32x300:900', 'f32x100:400']), ('report', ['meter', 'meter', 'meter', 'meter'])]),
    'meter_alone_encoded': ([('decode', 4), ('finish', 4, 16), ('normalize', 4, 0, None, True, False), ('encode', 4, [0, 0, 0, 0], False, None, False)], 3, [('rows', ['f32x600:600', 'u8x960:1920', 'f32x300:900', 'f32x100:400']), ('report', ['meter', 'meter', 'meter', 'meter'])]),
    'documents': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False)], 2, [('rows', ['f32x1320:1560', 'f32x520:1300'])]),
    'documents_padded': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, None, False)], 2, [('rows', ['f32x1380:2460', 'f32x100:400']), ('segments', [[(0, 600), (600, 1080), (1080, 1380)], [(0, 100)]])]),
    'documents_levels': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [1.0, 1.0, 0.5, 0.5], False)], 2, [('rows', ['f32x1320:1560', 'f32x520:1300']), ('segments', [[(0, 600), (840, 1320)], [(0, 300), (420, 520)]])]),
    'documents_untrimmed': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False)], 2, [('rows', ['f32x1376:1648', 'f32x680:1856']), ('segments', [[(0, 624), (864, 1376)], [(0, 384), (504, 680)]])]),
    'documents_rates': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False), ('resample', 1, 16000, False)], 2, [('rows', ['f32x880:880', 'f32x520:1300'])]),
    'documents_encoded': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False), ('encode', 2, [0, 0], [True, False], [7, 8], False)], 3, [('rows', ['u8x2640:2640', 'f32x520:1300']), ('segments', [[(0, 600), (840, 1320)], [(0, 300), (420, 520)]])]),
    'documents_all_encoded': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False), ('resample', 2, 8000, False), ('encode', 2, [2, 2], False, None, False)], 2, [('rows', ['u8x440:440', 'u8x174:348'])]),
    'documents_loudness': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False), ('normalize', 2, 1, None, False, False)], 2, [('rows', ['f32x1320:1560', 'f32x520:650']), ('report', [(-20.0, 1.0), (-21.0, 0.5)])]),
    'documents_ceilings_meter': ([('decode', 4), ('finish', 4, 16), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False), ('normalize', 2, 1, -2.0, True, False), ('normalize', 2, 1, -1.0, True, False)], 2, [('rows', ['f32x1320:390', 'f32x520:325']), ('segments', [[(0, 600), (840, 1320)], [(0, 300), (420, 520)]]), ('report', ['meter', 'meter'])]),
    'marks': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640)], 2, [('rows', ['f32x600:600', 'f32x480:960', 'f32x300:900', 'f32x100:400']), ('marks', [[(0, 300), (300, 600)], [(0, 240), (240, 480)], [(0, 150), (150, 300)], [(0, 50), (50, 100)]])]),
    'breaks': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640), ('apply_breaks', 4, 120)], 2, [('rows', ['f32x600:600', 'f32x720:1440', 'f32x300:900', 'f32x340:1360'])]),
    'breaks_marks_untrimmed': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640), ('apply_breaks', 4, 48)], 2, [('rows', ['f32x1104:1104', 'f32x512:1024', 'f32x384:1152', 'f32x176:704']), ('marks', [[(0, 552), (552, 1104)], [(0, 256), (256, 512)], [(0, 192), (192, 384)], [(0, 88), (88, 176)]])]),
    'marks_encoded_report': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640), ('normalize', 4, 4, None, False, False), ('encode', 4, [0, 0, 0, 0], False, None, False)], 3, [('rows', ['u8x1200:1200', 'f32x480:480', 'f32x300:450', 'f32x100:200']), ('report', [(-20.0, 0.5), (-21.0, 0.5), (-22.0, 0.5), (-23.0, 0.5)]), ('marks', [[(0, 300), (300, 600)], [(0, 240), (240, 480)], [(0, 150), (150, 300)], [(0, 50), (50, 100)]])]),
    'documents_marks': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False)], 2, [('rows', ['f32x1320:1560', 'f32x520:1300']), ('marks', [[[(0, 300), (300, 600)], [(840, 1080), (1080, 1320)]], [[(0, 150), (150, 300)], [(420, 470), (470, 520)]]])]),
    'documents_breaks_marks': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640), ('apply_breaks', 4, 120), ('join', 4, 2, 120, [0.5, 0.5, 0.5, 0.5], False)], 2, [('rows', ['f32x1560:2040', 'f32x520:1300']), ('segments', [[(0, 600), (840, 1560)], [(0, 300), (420, 520)]]), ('marks', [[[(0, 300), (300, 600)], [(840, 1200), (1200, 1560)]], [[(0, 150), (150, 300)], [(420, 470), (470, 520)]]])]),
    'everything': ([('decode', 4), ('finish', 4, 16), ('token_marks', 4, 8, 640), ('apply_breaks', 4, 60), ('join', 4, 2, 60, [0.5, 0.5, 1.0, 1.0], False), ('normalize', 2, 0, None, True, False), ('normalize', 2, 1, -1.0, True, False), ('resample', 1, 16000, False), ('encode', 2, [0, 1], [False, True], [5, 6], False)], 3, [('rows', ['f32x1078:270', 'u8x680:1360']), ('segments', [[(0, 624), (864, 1616)], [(0, 384), (504, 680)]]), ('report', ['meter', 'meter']), ('marks', [[[(0, 312), (312, 624)], [(864, 1240), (1240, 1616)]], [[(0, 192), (192, 384)], [(504, 592), (592, 680)]]])]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_option_matrix_makes_the_calls_reads_and_shapes_of_before(stages, name):
    kw = CASES[name]
    calls, reads, out = stages(**kw)
    got = (calls, reads, shape_of(out, kw))
    if os.environ.get("RECORD"):
        print(f"    {name!r}: {got!r},")
        return
    assert got == EXPECTED[name]


REFUSALS = {
    "row": (dict(mel_lengths=[40, 0, 25, 12]), "to_waveforms: mel_lengths[1] = 0 is outside [1, T = 40]"),
    "row_encoded": (dict(mel_lengths=[40, 33, 41, 12], encoding="pcm16"), "to_waveforms: mel_lengths[2] = 41 is outside [1, T = 40]"),
    "row_in_document": (dict(mel_lengths=[40, 33, 25, 0], **DOCS), "to_waveforms: mel_lengths[3] = 0 is outside [1, T = 40]"),
}


REFUSAL_READS = {'row': 2, 'row_encoded': 1, 'row_in_document': 1}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refused_row_is_named_behind_the_one_read(stages, name):
    kw, message = REFUSALS[name]
    with pytest.raises(ValueError) as e:
        stages(**kw)
    if os.environ.get("RECORD"):
        print(f"    {name!r}: {Dev.reads},")
    assert str(e.value) == message and 1 <= Dev.reads <= REFUSAL_READS[name]     # (the copies of before the move; never more)


def test_a_document_that_could_not_be_joined_is_named(stages, monkeypatch):
    tail = sub(TAIL)
    join = tail.join_waveforms

    def no_room(*a, **kw):
        out, lens, starts = join(*a, **kw)
        return out, dev(torch.where(torch.tensor([False, True]), torch.tensor(-1), host(lens))), starts
    monkeypatch.setattr(tail, "join_waveforms", no_room)
    with pytest.raises(ValueError) as e:
        stages(**DOCS)
    assert str(e.value) == "to_waveforms: document 1 (rows 2 to 3) could not be joined" and Dev.reads == 1


def test_the_timing_plans_verdict_takes_precedence(stages, monkeypatch):
    tm = sub("timing")
    marks = tm.token_marks

    def refusing(*a, **kw):
        m, n, plan = marks(*a, **kw)

        def verdict():
            raise ValueError("token_marks: row 1 refused")
        plan.raise_refused = verdict
        return m, n, plan
    monkeypatch.setattr(tm, "token_marks", refusing)
    with pytest.raises(ValueError, match="token_marks: row 1 refused"):
        stages(mel_lengths=[40, 0, 25, 12], **ENDS, return_marks=True)


SIGNATURES = {
    'finish_waveforms': '(audio, lengths, hop=0, silence_threshold_db=-60.0)',
    'to_waveforms': "(mel, mel_lengths, vocoder, trim=True, silence_threshold_db=-60.0, *, encoding=None, dither=False, dither_keys=None, documents=None, gaps=None, fade_ms=5.0, level='document', return_segments=False, loudness=None, return_loudness=False, true_peak=None, return_meter=False, token_ends=None, x_lengths=None, breaks=None, return_marks=False, sample_rate=24000)",
    'join_waveforms': '(audio, lengths, documents, gaps, fade=0, scale=None, check=True, out_ld=None)',
    'document_csr': '(documents, B, pad=False)',
    'trim_trailing_silence': '(audio, silence_threshold_db=-60.0)',
    'to_waveform': '(mel, vocoder)',
    'pipeline': '(model, vocoder, text, speaker=0, voice_mix=None, n_timesteps=4, scale_correction=1.0, length_scale=1.0, debug=False, *, encoding=None, loudness=None, true_peak=None, sample_rate=24000)',
    '_waveform_on_device': '(mel, vocoder)',
}


def test_the_moved_names_resolve_from_inference_with_the_signatures_of_before():
    inf = sub("inference")
    got = {name: str(inspect.signature(getattr(inf, name))) for name in (
        "finish_waveforms", "to_waveforms", "join_waveforms", "document_csr", "trim_trailing_silence", "to_waveform", "pipeline",
        "_waveform_on_device")}
    if os.environ.get("RECORD"):
        print(f"SIGNATURES = {got!r}")
        return
    assert got == SIGNATURES
    assert inf.METER_FIGURES == ("lufs", "gain", "lra", "momentary_max", "short_term_max", "peak", "true_peak") and inf.SAMPLE_RATE == 24000
    if TAIL != "inference":
        for name in list(got)[:5] + ["METER_FIGURES", "_waveform_on_device"]:
            assert getattr(inf, name) is getattr(sub(TAIL), name), name

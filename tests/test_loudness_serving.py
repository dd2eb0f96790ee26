"""Loudness targets at the handler level (stub model on the CPU; the GPU path is covered by tests/test_hip_loudness.py): ``loudness=``
reaches the batcher from the service's entries, mixed batches pass None (a NaN target on the device) for the rows without one,
results carry ``"loudness"`` and ``"gain"``, and a value that is no level raises before anything is submitted or launched."""
import asyncio
import inspect
import math

import pytest

from conftest import sub


def service(run, **kw):
    sv, bt = sub("serving"), sub("batcher")
    q = bt.FrameBudgetBatcher(model=None, max_batch=8, max_tokens=4096, max_wait_ms=5.0, run_batch=run)
    return q, sv.SpeechService(q, phonemize=lambda text, lang: [1 + (ord(c) % 50) for c in text], **kw)


def test_request_and_document_fields():
    bt = sub("batcher")
    r = bt.Request(ids=[1, 2])
    loudness_field = lambda batch: bt.tail_options(batch).get("loudness")
    assert r.loudness is None and loudness_field([r, bt.Request(ids=[3])]) is None
    mixed = [r, bt.Request(ids=[3], loudness=-16), bt.Request(ids=[4], loudness=-23.0)]
    assert loudness_field(mixed) == [None, -16.0, -23.0]
    assert isinstance(mixed[1].loudness, float)
    d = bt.Document(rows=[bt.Request(ids=[1]), bt.Request(ids=[2])], pauses_ms=[100, 0], loudness=-19)
    assert d.loudness == -19.0 and loudness_field([d, r]) == [-19.0, None]
    assert bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0]).loudness is None
    for bad in ("loud", True, [-23.0]):
        with pytest.raises(TypeError):
            bt.Request(ids=[1], loudness=bad)
    for bad in (0.5, 3, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="LUFS"):
            bt.Request(ids=[1], loudness=bad)
        with pytest.raises(ValueError, match="LUFS"):
            bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0], loudness=bad)
    # what the device is handed for a mixed batch: NaN for the rows without a target
    L = sub("loudness")
    got = L.targets_per_row(loudness_field(mixed), 3)
    assert math.isnan(got[0]) and got[1:] == [-16.0, -23.0]
    # without a vocoder nothing is touched, whatever the requests ask
    res = [{"mel": None, "mel_length": 3}]
    bt.waveforms_into(res, None, None, None, True, [bt.Request(ids=[1, 2, 3], loudness=-23.0)])
    assert res == [{"mel": None, "mel_length": 3}]
    p = inspect.signature(bt.waveforms_into).parameters
    assert "units" in p and not {"loudness", "true_peak", "sample_rates", "encodings", "dithers", "dither_keys"} & set(p)    # the fields come with the units: there is no per-field list to misplace
    inf = sub("inference")
    for fn in (inf.to_waveforms, inf.pipeline):
        p = inspect.signature(fn).parameters
        assert p["loudness"].default is None and p["loudness"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(inf.to_waveforms).parameters["return_loudness"].default is False
    for bad in ("loud", 1.0):                                     # refused on the host, ahead of the vocoder (None here)
        with pytest.raises((TypeError, ValueError)):
            inf.to_waveforms(None, None, None, loudness=bad)


def test_service_passes_the_target_on_and_results_carry_the_measurement():
    import torch
    seen = []

    def run(batch):
        seen.append(list(batch))
        out = []
        for u in batch:
            res = {"audio": torch.zeros(5)}
            if u.loudness is not None:      # what results_into leaves for such a unit
                res["loudness"], res["gain"] = -20.5, 10 ** ((u.loudness + 20.5) / 20)
            out.append(res)
        return out

    q, svc = service(run)
    with q:
        plain = svc.submit("plain").result(timeout=30)
        levelled = svc.levelled(-16).submit("levelled").result(timeout=30)
        spoken = asyncio.run(svc.levelled(-23.0).speak("spoken aloud"))
        long = svc.submit_long("One sentence. And a second one.", loudness=-19).result(timeout=30)
        long_plain = svc.submit_long("One sentence. And a second one.").result(timeout=30)
        for bad, err in (("loud", TypeError), (0.5, ValueError), (math.nan, ValueError)):
            with pytest.raises(err):
                svc.levelled(bad)
            with pytest.raises(err):
                svc.submit_long("never submitted", loudness=bad)
            with pytest.raises(err):
                asyncio.run(svc.speak_long("never submitted", loudness=bad))
    units = [u for batch in seen for u in batch]
    assert len(units) == 5                                        # the refused ones never reached the batcher
    bt = sub("batcher")
    by_len = {len(u.ids): u for u in units if isinstance(u, bt.Request)}
    assert by_len[len("plain")].loudness is None and by_len[len("levelled")].loudness == -16.0
    assert by_len[len("spoken aloud")].loudness == -23.0
    docs = [u for u in units if isinstance(u, bt.Document)]
    assert [d.loudness for d in docs] == [-19.0, None] and all(r.loudness is None for d in docs for r in d.rows)   # one gain per document
    assert "loudness" not in plain and "gain" not in plain and "loudness" not in long_plain
    assert levelled["loudness"] == -20.5 and abs(levelled["gain"] - 10 ** (4.5 / 20)) < 1e-12
    assert long["loudness"] == -20.5 and torch.is_tensor(spoken)
    # a service-wide target reaches every entry; one call can still name another, or none
    q, svc = service(run, loudness=-23)
    with q:
        a = svc.submit("with the service's").result(timeout=30)
        b = svc.submit_long("A long one. Of two.").result(timeout=30)
        c = svc.submit_long("A long one. Of two.", loudness=None).result(timeout=30)
        d = svc.levelled(None).submit("none at all").result(timeout=30)
    assert abs(a["gain"] - 10 ** (-2.5 / 20)) < 1e-12 and "loudness" in b and "loudness" not in c and "loudness" not in d
    sv = sub("serving")
    with pytest.raises(ValueError):
        sv.SpeechService(None, None, loudness=1.0)


def test_mixed_batches_and_the_step_batcher():
    bt = sub("batcher")
    calls = []

    def run(batch):
        calls.append(bt.tail_options(batch).get("loudness"))
        return [{"mel_length": len(r.ids)} for r in batch]

    q = bt.FrameBudgetBatcher(model=None, max_batch=4, max_tokens=4096, max_wait_ms=200.0, run_batch=run)
    with q:
        futures = [q.submit([1, 2, 3], loudness=-16), q.submit([1, 2, 3]), q.submit([1, 2, 3], loudness=-23.0), q.submit([4, 5, 6])]
        with pytest.raises(ValueError):
            q.submit([1], loudness=2.0)
        with pytest.raises(ValueError):
            q.submit_document([[1], [2]], [10, 0], loudness=math.nan)
        for f in futures:
            f.result(timeout=30)
    flat = [v for c in calls if c is not None for v in c]
    assert sorted(v for v in flat if v is not None) == [-23.0, -16.0]           # every target reached a batch, whatever the batching was
    # one batch of four, built by hand: the rows without a target pass None, which the device is handed as NaN
    batch = [bt.Request(ids=[1, 2, 3], loudness=-16), bt.Request(ids=[1, 2, 3]), bt.Request(ids=[1, 2, 3], loudness=-23.0), bt.Request(ids=[4, 5, 6])]
    calls.clear()
    assert run(batch) == [{"mel_length": 3}] * 4 and calls == [[-16.0, None, -23.0, None]]
    got = sub("loudness").targets_per_row(calls[0], 4)
    assert got[0] == -16.0 and got[2] == -23.0 and math.isnan(got[1]) and math.isnan(got[3])
    assert run(batch[1::2]) == [{"mel_length": 3}] * 2 and calls[1] is None     # no target in the batch: the call made before there was a choice
    with bt.StepBatcher(model=None, max_batch=2, run_step=lambda solver, entries: None) as sq:
        out = sq.submit([1, 2, 3], loudness=-16, n_timesteps=1).result(timeout=30)
        with pytest.raises(TypeError):
            sq.submit([1, 2, 3], loudness="loud")
    assert set(out) == {"mel", "mel_length"}                     # (its fake read-out has no vocoder: nothing to level)

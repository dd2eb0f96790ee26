"""Encoded responses at the handler level (stub model on the CPU; the GPU path is covered by tests/test_hip_audio_codec.py): the
``response_format`` -> ``Request.encoding`` mapping and its ``ValueError``, the new ``Request`` fields and their defaults, and that a
request which names no encoding is submitted, batched and answered exactly as before."""
import asyncio
import inspect
import io
import wave

import pytest

from conftest import sub


def test_response_format_mapping_and_its_value_error():
    sv = sub("serving")
    assert sv.RESPONSE_FORMATS == {"pcm": "pcm16", "wav": "pcm16", "ulaw": "ulaw", "alaw": "alaw"}
    assert [sv.response_encoding(f) for f in (None, "pcm", "wav", "ulaw", "alaw")] == [None, "pcm16", "pcm16", "ulaw", "alaw"]
    for bad in ("mp3", "opus", "PCM", "pcm16", ""):
        with pytest.raises(ValueError, match="response_format"):
            sv.response_encoding(bad)
    for fn in (sv.SpeechService.submit, sv.SpeechService.speak):
        params = inspect.signature(fn).parameters
        assert params["response_format"].default is None and list(params)[-1] == "response_format"     # no positional caller moves


def test_request_defaults_and_validation():
    bt = sub("batcher")
    r = bt.Request(ids=[1, 2])
    assert (r.encoding, r.dither, r.dither_key) == (None, False, 0)
    fields = lambda batch: tuple(bt.tail_options(batch).get(k) for k in ("encoding", "dither", "dither_keys"))
    assert fields([r, bt.Request(ids=[3])]) == (None, None, None)
    mixed = [r, bt.Request(ids=[3], encoding="ulaw"), bt.Request(ids=[4], encoding="pcm16", dither=True, dither_key=77)]
    assert fields(mixed) == ([None, "ulaw", "pcm16"], [False, False, True], [0, 0, 77])
    with pytest.raises(ValueError):
        bt.Request(ids=[1], encoding="mp3")
    # without a vocoder nothing is touched, whatever the requests ask
    res = [{"mel": None, "mel_length": 3}]
    bt.waveforms_into(res, None, None, None, True, [bt.Request(ids=[1, 2, 3], sample_rate=8000, encoding="ulaw")])
    assert res == [{"mel": None, "mel_length": 3}]


def service(run):
    sv, bt = sub("serving"), sub("batcher")
    q = bt.FrameBudgetBatcher(model=None, max_batch=4, max_tokens=4096, max_wait_ms=5.0, run_batch=run)
    return q, sv.SpeechService(q, phonemize=lambda text, lang: [1 + (ord(c) % 50) for c in text])


def test_service_passes_the_encoding_on_and_returns_bytes():
    import torch
    seen = []
    words = torch.arange(-3, 4, dtype=torch.int16)

    def run(batch):
        seen.extend(batch)
        out = []
        for r in batch:
            res = {"mel_length": len(r.ids), "audio": torch.zeros(5)}
            if r.encoding is not None:       # what waveforms_into leaves for such a request
                res["audio"] = words.view(torch.uint8).clone() if r.encoding == "pcm16" else torch.arange(7, dtype=torch.uint8)
                res["encoding"] = r.encoding
            if r.sample_rate != 24000:
                res["sample_rate"] = r.sample_rate
            out.append(res)
        return out

    q, svc = service(run)
    with q:
        async def main():
            return await asyncio.gather(svc.speak("plain"), svc.speak("as pcm", response_format="pcm"),
                                        svc.speak("as a wav", sample_rate=16000, response_format="wav"),
                                        svc.speak("telephony", sample_rate=8000, response_format="ulaw"))

        plain, pcm, wav, ulaw = asyncio.run(main())
        with pytest.raises(ValueError, match="response_format"):
            svc.submit("never submitted", response_format="flac")
    assert len(seen) == 4                                        # the refused one never reached the batcher
    by_len = {len(r.ids): r for r in seen}
    assert by_len[len("plain")].encoding is None and by_len[len("as pcm")].encoding == "pcm16"
    assert (by_len[len("as a wav")].encoding, by_len[len("as a wav")].sample_rate) == ("pcm16", 16000)
    assert (by_len[len("telephony")].encoding, by_len[len("telephony")].sample_rate) == ("ulaw", 8000)
    assert torch.is_tensor(plain) and plain.dtype == torch.float32          # no format named: what speak returned before
    assert isinstance(pcm, bytes) and pcm == words.numpy().tobytes()
    assert isinstance(ulaw, bytes) and ulaw == bytes(range(7))
    assert isinstance(wav, bytes)
    with wave.open(io.BytesIO(wav), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, 7)
        assert w.readframes(7) == pcm


def test_a_result_without_encoding_has_the_keys_it_has_today():
    submitted = []

    def run(batch):
        submitted.extend(batch)
        return [{"mel": None, "mel_length": len(r.ids), "audio": "a"} for r in batch]

    q, svc = service(run)
    with q:
        res = svc.submit("hello").result(timeout=30)
        res8 = svc.submit("hello again", sample_rate=8000).result(timeout=30)
    assert set(res) == set(res8) == {"mel", "mel_length", "audio"}
    assert all(r.encoding is None and r.dither is False and r.dither_key == 0 for r in submitted)
    # the step batcher takes the same fields
    bt = sub("batcher")
    with bt.StepBatcher(model=None, max_batch=2, run_step=lambda solver, entries: None) as sq:
        out = sq.submit([1, 2, 3], encoding="alaw", dither_key=5, n_timesteps=1).result(timeout=30)
    assert set(out) == {"mel", "mel_length"}                     # (its fake read-out has no vocoder: nothing to encode)

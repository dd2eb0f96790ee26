"""FLAC out on the GPU: mtts_flac_encode against the NumPy restatement of its rules (tests/flac_restated.py ``encode``), bit for bit, and
through the independent decoder (``decode``) back to exactly the words ``audio_codec.encode(..., "pcm16")`` gives -- over a ragged batch
of every length at which the encoder takes another path, every subframe kind and every rate-code branch, between sentinel bytes -- and
the wiring into the waveform tail, the batcher, the service and the per-request tail."""
import asyncio

import numpy as np
import pytest
import torch

from conftest import sub
import flac_restated as fr

pytestmark = pytest.mark.gpu

FILL = 0xA5
RATES = [24000, 8000, 16000, 48000, 11025, 100000]
SIGNALS = ("tonal", "white", "constant", "zeros", "alternating", "step", "lsb", "half")
LENGTHS = {256: [0, 1, 3, 4, 5, 255, 256, 257, 2 * 256 + 7, 4 * 256], 4096: [0, 1, 3, 4, 5, 255, 256, 257, 2 * 4096 + 700]}


@pytest.fixture(scope="module")
def ac():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("audio_codec")


def host(t):
    return t.detach().cpu().contiguous().numpy()


def signal(name, n, bs, seed):
    """n int16 words of one of SIGNALS."""
    rng, i = np.random.default_rng(seed), np.arange(n)
    t = i / 24000.0
    if name == "tonal":
        x = 0.3 * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * 180 * t) + 0.1 * np.sin(2 * np.pi * 1900 * t) + 0.002 * rng.standard_normal(n)
        return np.clip(np.rint(x * 32768), -32768, 32767).astype(np.int64)
    if name == "white":
        return rng.integers(-32768, 32768, n)
    if name == "constant":
        return np.full(n, -1234, dtype=np.int64)
    if name == "zeros":
        return np.zeros(n, dtype=np.int64)
    if name == "alternating":
        return np.where(i % 2 == 0, 32767, -32768)
    if name == "step":
        return np.where(i < 300, 100, -2000)
    if name == "lsb":
        return rng.integers(-2, 3, n)
    return np.where(i % bs < bs // 2, 0, rng.integers(-20000, 20001, n))          # half: a frame silent, then loud


def raw_encode(ac, audio, lengths, rates, bs, dither=False, seed=0, keys=None):
    """mtts_flac_encode itself, into a buffer of sentinel bytes: ``(data, nbytes)`` on the host."""
    hip = sub("_hip")
    lib = hip.load()
    B, ld = audio.shape
    stride = lib.mtts_flac_row_bytes(ld, bs)
    assert stride == (42 + -(-ld // bs) * (2 * bs + 16) + 15) // 16 * 16
    out = torch.full((B, stride), FILL, dtype=torch.uint8, device="cuda")
    nbytes = torch.full((B,), -7, dtype=torch.long, device="cuda")
    ws = torch.empty(lib.mtts_flac_workspace_bytes(B, ld, bs), dtype=torch.uint8, device="cuda")
    lengths = torch.tensor(lengths, dtype=torch.long, device="cuda")
    rates = torch.tensor(rates, dtype=torch.int32, device="cuda")
    keys = None if keys is None else torch.tensor(keys, dtype=torch.long, device="cuda")
    hip.check(lib.mtts_flac_encode(hip.ptr(audio), ld, hip.ptr(lengths), hip.ptr(rates), hip.ptr(keys), B, bs, int(dither), seed,
                                   hip.ptr(out), stride, hip.ptr(nbytes), ws.data_ptr(), ws.numel(), hip.stream_ptr()))
    torch.cuda.synchronize()
    return host(out), nbytes.tolist()


@pytest.fixture(scope="module", params=[256, 4096])
def batch(request, ac):
    """One ragged batch per block size: every signal at every length, the rates in turn; ld larger than the longest row."""
    bs = request.param
    rows = [(name, n) for name in SIGNALS for n in LENGTHS[bs]]
    ld = (max(LENGTHS[bs]) + 37 + 3) // 4 * 4
    x = np.zeros((len(rows), ld), dtype=np.float32)
    for b, (name, n) in enumerate(rows):
        x[b, :n] = signal(name, n, bs, b).astype(np.float32) / np.float32(32768.0)
        x[b, n:] = 0.77                                                            # (nothing beyond a row's length is read)
    lengths = [n for _, n in rows]
    rates = [RATES[b % len(RATES)] for b in range(len(rows))]
    return dict(bs=bs, rows=rows, audio=torch.from_numpy(x).cuda(), lengths=lengths, rates=rates, keys=[1000 + 3 * b for b in range(len(rows))])


def pcm_words(ac, batch, **kw):
    data, nbytes = ac.encode(batch["audio"], batch["lengths"], "pcm16", check=True, **kw)
    data = host(data)
    return [data[b, :2 * n].view("<i2").astype(np.int64) for b, n in enumerate(batch["lengths"])]


def check_rows(batch, data, nbytes, words):
    """Assertions 1 to 3 over a batch: the restated encoder's bytes, the decoder's words, the sentinels."""
    kinds = set()
    for b, (name, n) in enumerate(batch["rows"]):
        info = []
        want = fr.encode(words[b], batch["rates"][b], batch["bs"], info)
        assert nbytes[b] == len(want), (name, n, nbytes[b], len(want))
        assert data[b, :nbytes[b]].tobytes() == want, (name, n)
        assert (data[b, nbytes[b]:] == FILL).all(), (name, n)                      # nothing at or beyond the stream
        got = fr.decode(data[b, :nbytes[b]].tobytes())
        assert np.array_equal(got["samples"][0], words[b]) and got["samples"].shape[0] == 1, (name, n)
        assert (got["rate"], got["total"], got["bps"], got["block_sizes"]) == (batch["rates"][b], n, 16, (batch["bs"],) * 2)
        assert all(fm["rate"] == batch["rates"][b] and fm["number"] == j for j, fm in enumerate(got["frames"]))
        kinds |= {(name, k, o) for k, o, _ in info}
    return kinds


def test_device_bytes_are_the_restated_encoder_and_decode_to_the_pcm16_words(ac, batch):
    words = pcm_words(ac, batch)
    for b, (name, n) in enumerate(batch["rows"]):                                  # (the signals are exact in fp32: the words are the signals)
        assert np.array_equal(words[b], signal(name, n, batch["bs"], b))
    data, nbytes = raw_encode(ac, batch["audio"], batch["lengths"], batch["rates"], batch["bs"])
    kinds = check_rows(batch, data, nbytes, words)
    names = {(name, k) for name, k, _ in kinds}
    print(sorted(kinds))
    assert {("white", "VERBATIM"), ("alternating", "VERBATIM"), ("constant", "CONSTANT"), ("zeros", "CONSTANT"), ("step", "CONSTANT"),
            ("step", "FIXED"), ("lsb", "FIXED"), ("half", "FIXED"), ("tonal", "FIXED")} <= names       # every kind was really written
    assert len({o for _, k, o in kinds if k == "FIXED"}) >= 3                      # ... and several orders
    # the wrapper: the same bytes, and a second call gives them again
    for _ in range(2):
        d2, n2 = ac.encode_flac(batch["audio"], batch["lengths"], batch["rates"], block_size=batch["bs"], check=True)
        assert n2.tolist() == nbytes and d2.shape == data.shape
        d2 = host(d2)
        assert all(np.array_equal(d2[b, :nbytes[b]], data[b, :nbytes[b]]) for b in range(len(nbytes)))


def test_dithered_streams_hold_the_dithered_pcm16_words(ac, batch):
    words = pcm_words(ac, batch, dither=True, seed=9, keys=batch["keys"])
    plain = pcm_words(ac, batch)
    assert any(not np.array_equal(a, b) for a, b in zip(words, plain))             # (the dither does something)
    data, nbytes = raw_encode(ac, batch["audio"], batch["lengths"], batch["rates"], batch["bs"], dither=True, seed=9, keys=batch["keys"])
    check_rows(batch, data, nbytes, words)
    # one flag per row: each row as its own flag says
    on = [b % 2 == 0 for b in range(len(nbytes))]
    data_p, nbytes_p = raw_encode(ac, batch["audio"], batch["lengths"], batch["rates"], batch["bs"])
    mixed, n_mixed = ac.encode_flac(batch["audio"], batch["lengths"], batch["rates"], block_size=batch["bs"], dither=on, seed=9, keys=batch["keys"])
    mixed = host(mixed)
    for b in range(len(nbytes)):
        src, n = (data, nbytes) if on[b] else (data_p, nbytes_p)
        assert n_mixed[b] == n[b] and np.array_equal(mixed[b, :n[b]], src[b, :n[b]]), b


def test_a_row_does_not_depend_on_its_batch(ac, batch):
    data, nbytes = raw_encode(ac, batch["audio"], batch["lengths"], batch["rates"], batch["bs"], dither=True, seed=5, keys=batch["keys"])
    for b in sorted({len(nbytes) - 1, 0, LENGTHS[batch["bs"]].index(257), len(LENGTHS[batch["bs"]]) - 1}):      # alone, and at a narrower ld
        n = batch["lengths"][b]
        ld = max(4, (n + 3) // 4 * 4)
        alone = torch.zeros(1, ld, device="cuda")
        alone[0, :n] = batch["audio"][b, :n]
        d1, n1 = raw_encode(ac, alone, [n], [batch["rates"][b]], batch["bs"], dither=True, seed=5, keys=[batch["keys"][b]])
        assert n1 == [nbytes[b]] and np.array_equal(d1[0, :n1[0]], data[b, :nbytes[b]]), b


def test_refused_rows_are_untouched_and_their_neighbours_right(ac):
    bs, ld = 256, 600
    x = torch.from_numpy((signal("tonal", ld, bs, 3).astype(np.float32) / np.float32(32768.0))[None].repeat(7, 0)).cuda()
    lengths = [519, -1, 519, ld + 1, 519, 519, 519]
    rates = [24000, 24000, 8000, 24000, 0, 1048576, 1048575]
    data, nbytes = raw_encode(ac, x, lengths, rates, bs)
    words = signal("tonal", ld, bs, 3)[:519]
    for b in range(7):
        if b in (1, 3, 4, 5):
            assert nbytes[b] == -1 and (data[b] == FILL).all(), b
        else:
            want = fr.encode(words, rates[b], bs)
            assert nbytes[b] == len(want) and data[b, :nbytes[b]].tobytes() == want and (data[b, nbytes[b]:] == FILL).all(), b
    assert fr.decode(data[6, :nbytes[6]].tobytes())["rate"] == 1048575 and fr.decode(data[6, :nbytes[6]].tobytes())["frames"][0]["rate"] == 1048575
    with pytest.raises(ValueError, match="row 1 was refused"):
        ac.encode_flac(x, lengths, rates, block_size=bs, check=True)


# ------------------------------------------------------------------------------------------------ through the interface
SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)             # tests/test_hip_vocos.py's second configuration


@pytest.fixture(scope="module")
def env(ac, hparams, synthetic):
    inf, voc = sub("inference"), sub("vocoder")
    hp = hparams.tiny(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to("cuda").eval()
    model.decoder.solver = "midpoint"
    vocos = voc.Vocos(**SMALL)
    vocos.load_state_dict(synthetic.make_vocos_state_dict(seed=23, **{k: v for k, v in SMALL.items() if k != "hop"}), strict=True)
    mel = (torch.randn(4, SMALL["n_mels"], 40, generator=torch.Generator().manual_seed(3)) * 2.0 - 4.0).cuda()
    return inf, hp, model, voc.VocosWrapper(vocos.to("cuda").eval()), mel, [40, 33, 25, 12]


def words_of(pcm):
    return pcm.numpy().view("<i2").astype(np.int64)


def assert_stream(stream, pcm, rate):
    """A FLAC result decodes to the words of the PCM16 result, and its header names the row's rate and sample count."""
    assert stream.dtype == torch.uint8 and stream.dim() == 1 and stream.device.type == "cpu"
    got = fr.decode(stream.numpy().tobytes())
    want = words_of(pcm)
    assert (got["rate"], got["total"], got["channels"], got["bps"]) == (rate, want.size, 1, 16)
    assert np.array_equal(got["samples"][0], want)


def test_to_waveforms_flac_rows_decode_to_the_pcm16_rows(ac, env, monkeypatch):
    inf, hp, model, vocos, mel, lengths = env
    rates = [24000, 8000, 24000, 24000]
    pcm = inf.to_waveforms(mel, lengths, vocos, encoding="pcm16", sample_rate=rates)
    assert all(p.numel() > 0 for p in pcm)                                          # (nothing below is vacuous)
    calls = []
    for name in ("cpu", "tolist", "item"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                calls.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    streams = inf.to_waveforms(mel, lengths, vocos, encoding="flac", sample_rate=rates)
    print(f"device reads with FLAC rows: {calls}")
    assert calls == ["cpu", "cpu"]                                                  # the meta words (the one wait), then the copy of the bytes
    calls.clear()
    names = [None, "pcm16", "flac", "flac"]
    mixed = inf.to_waveforms(mel, lengths, vocos, encoding=names, sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8])
    assert calls == ["cpu"] * 4                                                     # meta, then floats, samples and streams: copies behind the one wait
    monkeypatch.undo()
    for b in range(4):
        assert_stream(streams[b], pcm[b], rates[b])
    assert streams[0].untyped_storage().data_ptr() == streams[3].untyped_storage().data_ptr()   # views of one host buffer
    assert streams[0].numel() < pcm[0].numel()                                      # (it compresses)
    # a mixed batch: the float and PCM rows keep their bits against the call without FLAC, the FLAC rows hold the dithered words
    without = inf.to_waveforms(mel, lengths, vocos, encoding=[None, "pcm16", None, None], sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8])
    dithered = inf.to_waveforms(mel, lengths, vocos, encoding="pcm16", sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8])
    assert mixed[0].dtype == torch.float32 and torch.equal(mixed[0], without[0]) and torch.equal(mixed[1], without[1])
    assert torch.equal(mixed[1], dithered[1]) and not torch.equal(dithered[2], pcm[2])
    assert_stream(mixed[2], dithered[2], rates[2])
    assert_stream(mixed[3], dithered[3], rates[3])
    # documents: the FLAC stage sees one row per document
    kw = dict(documents=[2, 1, 1], gaps=[300, 0, 0, 0], sample_rate=[8000, 24000, 24000])
    docs = inf.to_waveforms(mel, lengths, vocos, encoding=["flac", "flac", "pcm16"], **kw)
    docs_pcm = inf.to_waveforms(mel, lengths, vocos, encoding="pcm16", **kw)
    assert_stream(docs[0], docs_pcm[0], 8000)
    assert_stream(docs[1], docs_pcm[1], 24000)
    assert torch.equal(docs[2], docs_pcm[2])
    with pytest.raises(ValueError, match=r"mel_lengths\[1\] = 41"):
        inf.to_waveforms(mel, [40, 41, 25, 12], vocos, encoding="flac")


def test_batcher_service_and_per_request_tail_return_streams(ac, env, synthetic):
    inf, hp, model, vocos, mel, lengths = env
    bt, sv = sub("batcher"), sub("serving")
    ids = synthetic.make_inputs(hp, 1, 20, seed=77)[0][0].tolist()
    common = dict(speaker=1, solver="midpoint", n_timesteps=2)
    with bt.FrameBudgetBatcher(model, max_batch=4, max_tokens=4096, max_wait_ms=1.0, vocoder=vocos) as q:
        pcm = q.submit(ids, encoding="pcm16", **common).result(timeout=120)
        plain = q.submit(ids, **common).result(timeout=120)
        flac = q.submit(ids, encoding="flac", **common).result(timeout=120)
        flac8 = q.submit(ids, sample_rate=8000, encoding="flac", dither=True, dither_key=31, **common).result(timeout=120)
        pcm8 = q.submit(ids, sample_rate=8000, encoding="pcm16", dither=True, dither_key=31, **common).result(timeout=120)
        svc = sv.SpeechService(q, phonemize=lambda text, lang: ids, flac=True)
        body = asyncio.run(svc.speak("ignored", voice=1, steps=2, response_format="flac"))
        with pytest.raises(ValueError, match="response_format"):                    # a service that did not opt in answers as it always has
            sv.SpeechService(q, phonemize=lambda text, lang: ids).submit("ignored", response_format="flac")
    assert set(flac) == {"mel", "mel_length", "audio", "encoding"} and flac["encoding"] == "flac" and pcm["audio"].numel() > 0
    assert_stream(flac["audio"], pcm["audio"], 24000)
    assert set(flac8) == {"mel", "mel_length", "audio", "encoding", "sample_rate"}
    assert_stream(flac8["audio"], pcm8["audio"], 8000)
    assert isinstance(body, bytes) and body == flac["audio"].numpy().tobytes()      # the stream as it is: it already is a file
    # the per-request tail: the batched row's stream from the batched row's floats, and its own PCM16 words from its own floats
    wf = sub("waveform")
    again, _ = wf.finish_request(plain["audio"].cuda(), encoding="flac")
    assert torch.equal(again, flac["audio"])
    res, ref = [{"mel": pcm["mel"]}], [{"mel": pcm["mel"]}]
    unit = lambda encoding: bt.Request(ids=[1], sample_rate=8000, encoding=encoding, dither=True, dither_key=31)
    bt.waveforms_into(res, pcm["mel"][None], [pcm["mel_length"]], vocos, False, [unit("flac")])
    bt.waveforms_into(ref, pcm["mel"][None], [pcm["mel_length"]], vocos, False, [unit("pcm16")])
    assert res[0]["encoding"] == "flac" and res[0]["sample_rate"] == 8000
    assert_stream(res[0]["audio"], ref[0]["audio"], 8000)
    empty, _ = wf.finish_request(torch.zeros(0, device="cuda"), encoding="flac", sample_rate=8000)
    got = fr.decode(empty.numpy().tobytes())
    assert empty.numel() == 42 and (got["total"], got["rate"], got["frame_sizes"]) == (0, 8000, (0, 0))

"""The LPC side of FLAC out on the GPU: mtts_flac_encode_lpc against the NumPy restatement of its rules (tests/flac_lpc_restated.py),
bit for bit, over the case list the CPU tests run (tests/test_flac_lpc_abi.py) as one ragged batch per block size and order, between
sentinel bytes; the same streams back through ``audio_codec.decode_flac`` to the PCM16 words on the device; order 0 against the old
entry; dither; independence of the batch; refused rows; and ``flac_lpc`` through the waveform tail, the batcher, the service and the
per-request tail."""
import asyncio
import functools

import numpy as np
import pytest
import torch

from conftest import sub
import flac_in_restated as fi
import flac_lpc_restated as fl

pytestmark = pytest.mark.gpu

FILL = 0xA5
LD = 2 * 4096 + 4                                                                   # every row <= 8197 samples


@pytest.fixture(scope="module")
def ac():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("audio_codec")


def host(t):
    return t.detach().cpu().contiguous().numpy()


def raw_encode(audio, lengths, rates, bs, lpc, dither=False, seed=0, keys=None, entry="mtts_flac_encode_lpc"):
    """The C entry itself, into a buffer of sentinel bytes: ``(data on the device, data on the host, nbytes)``."""
    hip = sub("_hip")
    lib = hip.load()
    B, ld = audio.shape
    stride = lib.mtts_flac_row_bytes(ld, bs)
    out = torch.full((B, stride), FILL, dtype=torch.uint8, device="cuda")
    nbytes = torch.full((B,), -7, dtype=torch.long, device="cuda")
    ws = torch.empty(lib.mtts_flac_workspace_bytes(B, ld, bs), dtype=torch.uint8, device="cuda")
    lengths = torch.tensor(lengths, dtype=torch.long, device="cuda")
    rates = torch.tensor(rates, dtype=torch.int32, device="cuda")
    keys = None if keys is None else torch.tensor(keys, dtype=torch.long, device="cuda")
    head = (hip.ptr(audio), ld, hip.ptr(lengths), hip.ptr(rates), hip.ptr(keys), B, bs)
    tail = (int(dither), seed, hip.ptr(out), stride, hip.ptr(nbytes), ws.data_ptr(), ws.numel(), hip.stream_ptr())
    hip.check(lib.mtts_flac_encode_lpc(*head, lpc, *tail) if entry == "mtts_flac_encode_lpc" else lib.mtts_flac_encode(*head, *tail))
    torch.cuda.synchronize()
    return out, host(out), nbytes.tolist()


@functools.lru_cache(maxsize=None)
def batch():
    """The case list as one ragged batch: every word exact in fp32, 0.77 behind a row's length (nothing there is read)."""
    rows = fl.cases()
    x = np.full((len(rows), LD), 0.77, dtype=np.float32)
    for b, (name, n, q, rate) in enumerate(rows):
        x[b, :n] = q.astype(np.float32) / np.float32(32768.0)
    return dict(rows=rows, audio=torch.from_numpy(x).cuda(), lengths=[n for _, n, _, _ in rows], rates=[r for _, _, _, r in rows],
                keys=[1000 + 3 * b for b in range(len(rows))])


@functools.lru_cache(maxsize=None)
def device_streams(bs, lpc):
    bt = batch()
    return raw_encode(bt["audio"], bt["lengths"], bt["rates"], bs, lpc)


def pcm_words(ac, bt, **kw):
    data, _ = ac.encode(bt["audio"], bt["lengths"], "pcm16", check=True, **kw)
    data = host(data)
    return [data[b, :2 * n].view("<i2").astype(np.int64) for b, n in enumerate(bt["lengths"])]


def check_rows(bt, bs, lpc, data, nbytes, words):
    """A batch against the restated encoder on ``words``: the bytes, the sentinels.  Returns the kinds written."""
    kinds = set()
    for b, (name, n, _, rate) in enumerate(bt["rows"]):
        info = []
        want = fl.encode(words[b], rate, bs, lpc, info)
        assert nbytes[b] == len(want), (name, n, nbytes[b], len(want), info)
        assert data[b, :nbytes[b]].tobytes() == want, (name, n, info)
        assert (data[b, nbytes[b]:] == FILL).all(), (name, n)                      # nothing at or beyond the stream
        kinds |= {(k, o) for k, o, _ in info}
    return kinds


@pytest.mark.parametrize("lpc", fl.MAX_ORDERS)
@pytest.mark.parametrize("bs", fl.BLOCK_SIZES)
def test_device_bytes_are_the_restated_encoder(ac, bs, lpc):
    bt = batch()
    words = pcm_words(ac, bt)
    for b, (name, n, q, _) in enumerate(bt["rows"]):                                # (the signals are exact in fp32: the words are the signals)
        assert np.array_equal(words[b], q), (name, n)
    _, data, nbytes = device_streams(bs, lpc)
    kinds = check_rows(bt, bs, lpc, data, nbytes, words)
    print(sorted(kinds))
    assert {k for k, _ in kinds} == {"CONSTANT", "FIXED", "VERBATIM", "LPC"}       # every kind was really written
    assert {o for k, o in kinds if k == "LPC"} <= set(fl.candidates(lpc, 4096))    # (the CPU tests see every candidate order win)
    # the wrapper: the same bytes
    d2, n2 = ac.encode_flac(bt["audio"], bt["lengths"], bt["rates"], block_size=bs, lpc_order=lpc, check=True)
    assert n2.tolist() == nbytes and d2.shape == data.shape
    d2 = host(d2)
    assert all(np.array_equal(d2[b, :nbytes[b]], data[b, :nbytes[b]]) for b in range(len(nbytes)))


@pytest.mark.parametrize("lpc", fl.MAX_ORDERS)
@pytest.mark.parametrize("bs", fl.BLOCK_SIZES)
def test_device_streams_decode_on_the_device_to_the_pcm16_words(ac, bs, lpc):
    bt = batch()
    dev, _, nbytes = device_streams(bs, lpc)
    audio, lengths, rates = ac.decode_flac(dev, nbytes, ld=LD, check=True)
    assert lengths.tolist() == bt["lengths"] and rates.tolist() == bt["rates"]
    pcm, _ = ac.encode(bt["audio"], bt["lengths"], "pcm16", check=True)
    want = pcm.view(torch.int16).to(torch.float32) / 32768.0                       # [B, LD] words as decode_flac scales them
    keep = torch.arange(LD, device="cuda")[None] < torch.tensor(bt["lengths"], device="cuda")[:, None]
    assert torch.equal(torch.where(keep, audio[:, :LD], torch.zeros_like(want)), torch.where(keep, want, torch.zeros_like(want)))
    assert not audio[~keep].any()                                                   # zeros from the length on


@pytest.mark.parametrize("bs", fl.BLOCK_SIZES)
def test_order_zero_is_the_old_entry(ac, bs):
    bt = batch()
    for kw in (dict(), dict(dither=True, seed=9, keys=bt["keys"])):
        new, _, n_new = raw_encode(bt["audio"], bt["lengths"], bt["rates"], bs, 0, **kw)
        old, _, n_old = raw_encode(bt["audio"], bt["lengths"], bt["rates"], bs, 0, entry="mtts_flac_encode", **kw)
        assert n_new == n_old and torch.equal(new, old)                            # (the sentinels too)
    d0, n0 = ac.encode_flac(bt["audio"], bt["lengths"], bt["rates"], block_size=bs, lpc_order=0, dither=True, seed=9, keys=bt["keys"])
    assert n0.tolist() == n_old and all(torch.equal(d0[b, :n], old[b, :n]) for b, n in enumerate(n_old))


@pytest.mark.parametrize("bs", fl.BLOCK_SIZES)
def test_dithered_streams_hold_the_dithered_pcm16_words(ac, bs):
    bt = batch()
    words = pcm_words(ac, bt, dither=True, seed=9, keys=bt["keys"])
    plain = pcm_words(ac, bt)
    assert any(not np.array_equal(a, b) for a, b in zip(words, plain))             # (the dither does something)
    _, data, nbytes = raw_encode(bt["audio"], bt["lengths"], bt["rates"], bs, 12, dither=True, seed=9, keys=bt["keys"])
    check_rows(bt, bs, 12, data, nbytes, words)
    for b in range(0, len(nbytes), 7):                                             # ... and the independent decoder reads them
        assert np.array_equal(fi.decode(data[b, :nbytes[b]].tobytes())["samples"][0], words[b]), b


@pytest.mark.parametrize("bs", fl.BLOCK_SIZES)
def test_a_row_does_not_depend_on_its_batch(ac, bs):
    bt = batch()
    _, data, nbytes = raw_encode(bt["audio"], bt["lengths"], bt["rates"], bs, 12, dither=True, seed=5, keys=bt["keys"])
    per = len(fl.LENGTHS)
    for b in sorted({0, len(nbytes) - 1, fl.LENGTHS.index(257), fl.LENGTHS.index(4096 + 5), per - 1, 5 * per + fl.LENGTHS.index(13)}):
        n = bt["lengths"][b]                                                       # alone, and at a narrower ld
        ld = max(4, (n + 3) // 4 * 4)
        alone = torch.zeros(1, ld, device="cuda")
        alone[0, :n] = bt["audio"][b, :n]
        _, d1, n1 = raw_encode(alone, [n], [bt["rates"][b]], bs, 12, dither=True, seed=5, keys=[bt["keys"][b]])
        assert n1 == [nbytes[b]] and np.array_equal(d1[0, :n1[0]], data[b, :nbytes[b]]), b


def test_refused_rows_are_untouched_and_their_neighbours_right(ac):
    bs, ld = 256, 600
    words = fl.speech_like(ld)[:519]
    x = torch.from_numpy((fl.speech_like(ld).astype(np.float32) / np.float32(32768.0))[None].repeat(7, 0)).cuda()
    lengths = [519, -1, 519, ld + 1, 519, 519, 519]
    rates = [24000, 24000, 8000, 24000, 0, 1048576, 1048575]
    _, data, nbytes = raw_encode(x, lengths, rates, bs, 12)
    for b in range(7):
        if b in (1, 3, 4, 5):
            assert nbytes[b] == -1 and (data[b] == FILL).all(), b
        else:
            info = []
            want = fl.encode(words, rates[b], bs, 12, info)
            assert nbytes[b] == len(want) and data[b, :nbytes[b]].tobytes() == want and (data[b, nbytes[b]:] == FILL).all(), b
            assert "LPC" in {k for k, _, _ in info}                                # (the neighbours are LPC frames, not the old kernel's)
    with pytest.raises(ValueError, match="row 1 was refused"):
        ac.encode_flac(x, lengths, rates, block_size=bs, lpc_order=12, check=True)


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
    got = fi.decode(stream.numpy().tobytes())
    want = words_of(pcm)
    assert (got["rate"], got["total"], got["channels"], got["bps"]) == (rate, want.size, 1, 16)
    assert np.array_equal(got["samples"][0], want)
    return [f["kinds"][0] for f in got["frames"]]


def test_tail_flac_lpc_rows_decode_to_the_pcm16_rows(ac, env, monkeypatch):
    inf, hp, model, vocos, mel, lengths = env
    rates = [24000, 8000, 24000, 24000]
    pcm = inf.to_waveforms(mel, lengths, vocos, encoding="pcm16", sample_rate=rates)
    fixed = inf.to_waveforms(mel, lengths, vocos, encoding="flac", sample_rate=rates)
    assert all(p.numel() > 0 for p in pcm)                                          # (nothing below is vacuous)
    calls, orders, real_flac = [], [], ac.encode_flac
    monkeypatch.setattr(ac, "encode_flac", lambda *a, **kw: (orders.append(kw.get("lpc_order")), real_flac(*a, **kw))[1])
    for name in ("cpu", "tolist", "item"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                calls.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    wf = sub("waveform")                                                            # (flac_lpc is an option of tail, which to_waveforms calls)
    streams = wf.tail(mel, lengths, vocos, encoding="flac", sample_rate=rates, flac_lpc=12).rows
    print(f"device reads with FLAC LPC rows: {calls}")
    assert calls == ["cpu", "cpu"]                                                  # the meta words (the one wait), then the copy of the bytes
    calls.clear()
    names = [None, "pcm16", "flac", "flac"]
    mixed = wf.tail(mel, lengths, vocos, encoding=names, sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8], flac_lpc=12).rows
    assert calls == ["cpu"] * 4                                                     # meta, then floats, samples and streams: copies behind the one wait
    calls.clear()
    each = wf.tail(mel, lengths, vocos, encoding=names, sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8], flac_lpc=[0, 0, 12, 0]).rows
    assert calls == ["cpu"] * 4                                                     # an order per row: two FLAC calls, still the one wait
    monkeypatch.undo()
    assert orders == [12, 12, None, 12]                                             # one FLAC call per distinct order, ascending; 0 is the call of before
    kinds = set()
    for b in range(4):
        kinds |= set(assert_stream(streams[b], pcm[b], rates[b]))
        assert streams[b].numel() <= fixed[b].numel()                               # (never longer: the contract)
    print(sorted(kinds), [s.numel() for s in streams], [s.numel() for s in fixed])
    # a mixed batch: the float and PCM rows keep their bits against the call without FLAC, the FLAC rows hold the dithered words
    without = inf.to_waveforms(mel, lengths, vocos, encoding=[None, "pcm16", None, None], sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8])
    dithered = inf.to_waveforms(mel, lengths, vocos, encoding="pcm16", sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8])
    mixed0 = inf.to_waveforms(mel, lengths, vocos, encoding=names, sample_rate=rates, dither=True, dither_keys=[5, 6, 7, 8])
    assert mixed[0].dtype == torch.float32 and torch.equal(mixed[0], without[0]) and torch.equal(mixed[1], without[1])
    assert_stream(mixed[2], dithered[2], rates[2])
    assert_stream(mixed[3], dithered[3], rates[3])
    # an order per row: each row is the row of the call that names its order for all
    assert torch.equal(each[2], mixed[2]) and torch.equal(each[3], mixed0[3]) and torch.equal(each[0], mixed[0]) and torch.equal(each[1], mixed[1])
    with pytest.raises(ValueError, match="flac_lpc"):
        wf.tail(mel, lengths, vocos, encoding=names, flac_lpc=[12, 0, 12, 0])


def test_service_batcher_and_per_request_tail_with_flac_lpc(ac, env, synthetic):
    inf, hp, model, vocos, mel, lengths = env
    bt, sv, wf = sub("batcher"), sub("serving"), sub("waveform")
    ids = synthetic.make_inputs(hp, 1, 20, seed=77)[0][0].tolist()
    common = dict(speaker=1, solver="midpoint", n_timesteps=2)
    with bt.FrameBudgetBatcher(model, max_batch=4, max_tokens=4096, max_wait_ms=1.0, vocoder=vocos) as q:
        pcm = q.submit(ids, encoding="pcm16", **common).result(timeout=120)
        plain = q.submit(ids, **common).result(timeout=120)
        flac0 = q.submit(ids, encoding="flac", **common).result(timeout=120)
        flac12 = q.submit(ids, encoding="flac", flac_lpc=12, **common).result(timeout=120)
        doc0 = q.submit_document([ids, ids[:9]], [30.0, 0.0], encoding="flac", **common).result(timeout=120)
        doc12 = q.submit_document([ids, ids[:9]], [30.0, 0.0], encoding="flac", flac_lpc=12, **common).result(timeout=120)
        body0 = asyncio.run(sv.SpeechService(q, phonemize=lambda text, lang: ids, flac=True).speak("ignored", voice=1, steps=2, response_format="flac"))
        body12 = asyncio.run(sv.SpeechService(q, phonemize=lambda text, lang: ids, flac=True, flac_lpc=12).speak("ignored", voice=1, steps=2,
                                                                                                                response_format="flac"))
    assert set(flac12) == {"mel", "mel_length", "audio", "encoding"} and flac12["encoding"] == "flac" and pcm["audio"].numel() > 0
    assert_stream(flac0["audio"], pcm["audio"], 24000)
    kinds = assert_stream(flac12["audio"], pcm["audio"], 24000)
    print(kinds, flac12["audio"].numel(), flac0["audio"].numel())
    assert flac12["audio"].numel() <= flac0["audio"].numel()
    assert body0 == flac0["audio"].numpy().tobytes() and body12 == flac12["audio"].numpy().tobytes()   # the service's choice reaches the request
    d0, d12 = fi.decode(doc0["audio"].numpy().tobytes()), fi.decode(doc12["audio"].numpy().tobytes())
    assert np.array_equal(d0["samples"], d12["samples"]) and d12["total"] > 0 and doc12["audio"].numel() <= doc0["audio"].numel()
    # the per-request tail: the batched row's stream from the batched row's floats
    again12, _ = wf.finish_request(plain["audio"].cuda(), encoding="flac", flac_lpc=12)
    again0, _ = wf.finish_request(plain["audio"].cuda(), encoding="flac")
    assert torch.equal(again12, flac12["audio"]) and torch.equal(again0, flac0["audio"])
    res, ref = [{"mel": pcm["mel"]}], [{"mel": pcm["mel"]}]
    unit = lambda encoding, **kw: bt.Request(ids=[1], sample_rate=8000, encoding=encoding, dither=True, dither_key=31, **kw)
    bt.waveforms_into(res, pcm["mel"][None], [pcm["mel_length"]], vocos, False, [unit("flac", flac_lpc=12)])
    bt.waveforms_into(ref, pcm["mel"][None], [pcm["mel_length"]], vocos, False, [unit("pcm16")])
    assert res[0]["encoding"] == "flac" and res[0]["sample_rate"] == 8000
    assert_stream(res[0]["audio"], ref[0]["audio"], 8000)
    empty, _ = wf.finish_request(torch.zeros(0, device="cuda"), encoding="flac", sample_rate=8000, flac_lpc=12)
    assert empty.numel() == 42 and fi.decode(empty.numpy().tobytes())["total"] == 0

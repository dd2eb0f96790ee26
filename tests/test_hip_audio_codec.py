"""Encoded audio on the GPU: mtts_pcm_encode / mtts_pcm_decode against the NumPy restatement (tests/audio_codec_restated.py), bit for
bit -- exhaustively over the 65536 words and the 256 codes, at the quantiser's edges, over ragged tails between canaries, and for the
dither's independence of the batch -- and the wiring into the waveform tail, the batchers, the service and the recording entries."""
import asyncio
import io
import wave

import numpy as np
import pytest
import torch

from conftest import sub
import audio_codec_restated as ar

pytestmark = pytest.mark.gpu

WORDS = np.arange(-32768, 32768, dtype=np.int32)
CODES = np.arange(256, dtype=np.uint8)
FILL = 0xA5


@pytest.fixture(scope="module")
def ac():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("audio_codec")


def host(t):
    return t.detach().cpu().contiguous().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ exhaustive
def test_every_word_through_the_three_encoders(ac):
    x = WORDS.astype(np.float32) / np.float32(32768.0)
    audio = torch.from_numpy(np.stack([x, x, x])).cuda()
    data, nbytes = ac.encode(audio, None, ["pcm16", "ulaw", "alaw"], check=True)
    assert data.shape == (3, 2 * 65536) and data.dtype == torch.uint8 and nbytes.tolist() == [131072, 65536, 65536]
    data = host(data)
    for b, fmt in enumerate((ar.PCM16, ar.ULAW, ar.ALAW)):
        want = ar.encode(x, fmt)
        assert np.array_equal(data[b, :want.size], want), fmt
    assert np.array_equal(data[0, :131072].view("<i2"), WORDS)               # v / 32768 comes back as v


def test_every_word_and_every_code_through_the_decoders(ac):
    pcm = WORDS.astype("<i2").view(np.uint8)
    data = np.zeros((3, pcm.size), dtype=np.uint8)
    data[0], data[1, :256], data[2, :256] = pcm, CODES, CODES
    out = host(ac.decode(torch.from_numpy(data).cuda(), [65536, 256, 256], ["pcm16", "ulaw", "alaw"], ld=65536))
    assert out.shape == (3, 65536) and out.dtype == np.float32
    assert np.array_equal(bits(out[0]), bits(ar.decode(pcm, ar.PCM16)))
    assert np.array_equal(bits(out[1, :256]), bits(ar.decode(CODES, ar.ULAW))) and not out[1, 256:].any()
    assert np.array_equal(bits(out[2, :256]), bits(ar.decode(CODES, ar.ALAW))) and not out[2, 256:].any()
    # decode then encode on the device: every word, every A-law code, and every mu-law code but the second zero
    back, _ = ac.encode(torch.from_numpy(out).cuda(), [65536, 256, 256], ["pcm16", "ulaw", "alaw"])
    back = host(back)
    assert np.array_equal(back[0, :131072], pcm) and np.array_equal(back[2, :256], CODES)
    assert np.nonzero(back[1, :256] != CODES)[0].tolist() == [0x7F] and back[1, 0x7F] == 0xFF


def test_edges_ties_to_even_and_saturation(ac):
    edge = [np.nan, np.inf, -np.inf, 1.0, -1.0, 1.0 - 2.0 ** -24, -0.0, 1e-42]
    ties = [(v + 0.5) / 32768.0 for v in range(-4, 5)]
    x = np.array(edge + ties, dtype=np.float32)
    assert x[5] < 1.0 and x[7] != 0.0                                        # the largest float below 1 and a denormal
    audio = torch.from_numpy(np.stack([x, x, x])).cuda()
    data, nbytes = ac.encode(audio, None, ["pcm16", "ulaw", "alaw"], check=True)
    data = host(data)
    q = data[0, :2 * x.size].view("<i2").tolist()
    assert q[:8] == [0, 32767, -32768, 32767, -32768, 32767, 0, 0]           # NaN -> 0, saturation at both ends
    assert q[8:] == [-4, -2, -2, 0, 0, 2, 2, 4, 4]                           # every tie goes to the even neighbour
    for b, fmt in enumerate((ar.PCM16, ar.ULAW, ar.ALAW)):
        want = ar.encode(x, fmt)
        assert np.array_equal(data[b, :want.size], want), fmt


# ------------------------------------------------------------------------------------------------ ragged tails
def tail_case(ac, rot):
    T = ac.TILE
    ld = T + 8
    lengths = [0, 1, 3, 5, T - 1, T, T + 5, ld, ld + 1]
    fmts = [(b + rot) % 3 for b in range(len(lengths))]
    rng = np.random.default_rng(700 + rot)
    x = rng.uniform(-1.2, 1.2, (len(lengths), ld)).astype(np.float32)
    return T, ld, lengths, fmts, x


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_ragged_tails_between_canaries_encode(ac, rot):
    hip = sub("_hip")
    lib = hip.load()
    T, ld, lengths, fmts, x = tail_case(ac, rot)
    B = len(lengths)
    audio = torch.from_numpy(x).cuda()
    d_len = torch.tensor(lengths, dtype=torch.long, device="cuda")
    d_fmt = torch.tensor(fmts, dtype=torch.int32, device="cuda")
    whole = torch.full((B + 2, 2 * ld), FILL, dtype=torch.uint8, device="cuda")     # canary row | B rows | canary row
    out = whole[1:B + 1]
    assert out.data_ptr() % 16 == 0 and audio.data_ptr() % 16 == 0
    nbytes = torch.full((B,), 12345, dtype=torch.long, device="cuda")
    hip.check(lib.mtts_pcm_encode(hip.ptr(audio), ld, hip.ptr(d_len), hip.ptr(d_fmt), None, B, 0, 0, hip.ptr(out), hip.ptr(nbytes),
                                  hip.stream_ptr()))
    with pytest.raises(ValueError, match=f"row {B - 1} was refused"):
        ac._status(lib, nbytes)
    got, nb = host(whole), nbytes.tolist()
    assert (got[0] == FILL).all() and (got[B + 1] == FILL).all()                    # both canaries
    for b, (L, fmt) in enumerate(zip(lengths, fmts)):
        row = got[1 + b]
        if L > ld:
            assert nb[b] == -1 and (row == FILL).all()                              # refused: no byte written
            continue
        want = ar.encode(x[b, :L], fmt)
        assert nb[b] == want.size == L * ar.BYTES[fmt]
        assert np.array_equal(row[:want.size], want), (b, L, fmt)
        assert (row[want.size:] == FILL).all(), (b, L, fmt)                         # nothing at or beyond the byte length
    # an unknown format and a length that already is -1: refused alone, the other rows as before
    fmts2, lengths2 = list(fmts), list(lengths)
    fmts2[2], lengths2[4] = 7, -1
    whole2 = torch.full((B + 2, 2 * ld), FILL, dtype=torch.uint8, device="cuda")
    d_len2 = torch.tensor(lengths2, dtype=torch.long, device="cuda")
    d_fmt2 = torch.tensor(fmts2, dtype=torch.int32, device="cuda")
    hip.check(lib.mtts_pcm_encode(hip.ptr(audio), ld, hip.ptr(d_len2), hip.ptr(d_fmt2), None, B, 0, 0, hip.ptr(whole2[1:B + 1]),
                                  hip.ptr(nbytes), hip.stream_ptr()))
    got2, nb2 = host(whole2), nbytes.tolist()
    for b in range(B):
        if b in (2, 4, B - 1):
            assert nb2[b] == -1 and (got2[1 + b] == FILL).all(), b
        else:
            assert nb2[b] == nb[b] and np.array_equal(got2[1 + b], got[1 + b]), b


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_ragged_tails_between_canaries_decode(ac, rot):
    hip = sub("_hip")
    lib = hip.load()
    T, ld, lengths, fmts, x = tail_case(ac, rot)
    B = len(lengths)
    ld_bytes = 2 * ld
    data = np.full((B, ld_bytes), 0x5A, dtype=np.uint8)                             # (bytes beyond a row's length are not zeros)
    for b, (L, fmt) in enumerate(zip(lengths, fmts)):
        enc = ar.encode(x[b, :min(L, ld)], fmt)
        data[b, :enc.size] = enc
    d_data = torch.from_numpy(data).cuda()
    d_len = torch.tensor(lengths, dtype=torch.long, device="cuda")
    d_fmt = torch.tensor(fmts, dtype=torch.int32, device="cuda")
    canary = np.frombuffer(bytes([FILL] * 4), dtype=np.float32)[0]
    whole = torch.full((B + 2, ld), float(canary), dtype=torch.float32, device="cuda")
    out_len = torch.full((B,), 12345, dtype=torch.long, device="cuda")
    hip.check(lib.mtts_pcm_decode(hip.ptr(d_data), ld_bytes, hip.ptr(d_len), hip.ptr(d_fmt), B, hip.ptr(whole[1:B + 1]), ld,
                                  hip.ptr(out_len), hip.stream_ptr()))
    got, n = host(whole), out_len.tolist()
    assert (bits(got[0]) == bits(canary)).all() and (bits(got[B + 1]) == bits(canary)).all()
    for b, (L, fmt) in enumerate(zip(lengths, fmts)):
        row = got[1 + b]
        if L > ld:
            assert n[b] == -1 and (bits(row) == bits(canary)).all()                 # refused: left unwritten
            continue
        assert n[b] == L
        assert np.array_equal(bits(row[:L]), bits(ar.decode(data[b, :L * ar.BYTES[fmt]], fmt))), (b, L, fmt)
        assert np.array_equal(bits(row[L:]), np.zeros(ld - L, dtype=np.uint32)), (b, L, fmt)      # +0.0 from the length on
    # a length whose bytes exceed the row is refused: the long PCM16 rows no longer fit rows of ld + 8 bytes
    short = torch.from_numpy(data[:, :ld + 8].copy()).cuda()
    hip.check(lib.mtts_pcm_decode(hip.ptr(short), ld + 8, hip.ptr(d_len), hip.ptr(d_fmt), B, hip.ptr(whole[1:B + 1]), ld, hip.ptr(out_len),
                                  hip.stream_ptr()))
    n = out_len.tolist()
    for b, (L, fmt) in enumerate(zip(lengths, fmts)):
        assert n[b] == (L if L <= ld and L * ar.BYTES[fmt] <= ld + 8 else -1), (b, L, fmt)


# ------------------------------------------------------------------------------------------------ dither
def test_dithered_rows_do_not_depend_on_their_batch(ac):
    T = ac.TILE
    L = T + 37
    rng = np.random.default_rng(11)
    x = (rng.uniform(-1, 1, (5, L)) * 2.0 ** -10).astype(np.float32)              # a few dozen LSB: the dither decides many samples
    keys = [3, -1, 1 << 40, 42, 0]
    audio = torch.from_numpy(x).cuda()
    data, nbytes = ac.encode(audio, None, "pcm16", dither=True, seed=9, keys=keys)
    alone, n_alone = ac.encode(audio[3:4].clone(), None, "pcm16", dither=True, seed=9, keys=[42])
    again, _ = ac.encode(audio, None, "pcm16", dither=True, seed=9, keys=keys)
    data, alone, again = host(data), host(alone), host(again)
    assert nbytes.tolist() == [2 * L] * 5 and n_alone.tolist() == [2 * L]
    assert np.array_equal(alone[0, :2 * L], data[3, :2 * L])                        # row 3 of 5 == the row alone, same key
    assert np.array_equal(again[:, :2 * L], data[:, :2 * L])                        # a second call: the same bits
    for b, key in enumerate(keys):
        assert np.array_equal(data[b, :2 * L], ar.encode(x[b], ar.PCM16, True, 9, key)), b
    assert not np.array_equal(data[3, :2 * L], ar.encode(x[3], ar.PCM16))          # and the dither did something
    # G.711 rows compand the undithered value; a per-row dither flag touches its own rows only
    mixed, _ = ac.encode(audio, None, ["pcm16", "ulaw", "pcm16", "alaw", "pcm16"], dither=[True, True, False, True, True], seed=9, keys=keys)
    mixed = host(mixed)
    want = [ar.encode(x[0], ar.PCM16, True, 9, keys[0]), ar.encode(x[1], ar.ULAW), ar.encode(x[2], ar.PCM16), ar.encode(x[3], ar.ALAW),
            ar.encode(x[4], ar.PCM16, True, 9, keys[4])]
    for b, w in enumerate(want):
        assert np.array_equal(mixed[b, :w.size], w), b


# ------------------------------------------------------------------------------------------------ through the interface
SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)             # tests/test_hip_vocos.py's second configuration


@pytest.fixture(scope="module")
def env(ac, hparams, synthetic):
    inf, voc, style = sub("inference"), sub("vocoder"), sub("style")
    hp = hparams.tiny(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to("cuda").eval()
    model.decoder.solver = "midpoint"
    vocos = voc.Vocos(**SMALL)
    vocos.load_state_dict(synthetic.make_vocos_state_dict(seed=23, **{k: v for k, v in SMALL.items() if k != "hop"}), strict=True)
    torch.manual_seed(21)
    enc = style.StyleEncoder(hp.n_feats, 32, 2, hp.spk_emb_dim).to("cuda").eval()
    return inf, hp, model, voc.VocosWrapper(vocos.to("cuda").eval()), enc


def test_to_waveforms_encoding_is_the_restatement_of_its_floats(ac, env):
    inf, hp, model, vocos, enc = env
    lengths = [40, 33, 25, 12]
    mel = (torch.randn(4, SMALL["n_mels"], 40, generator=torch.Generator().manual_seed(3)) * 2.0 - 4.0).cuda()
    rates = [24000, 8000, 24000, 8000]
    names = ["pcm16", "ulaw", "alaw", "pcm16"]
    floats = inf.to_waveforms(mel, lengths, vocos, sample_rate=rates)
    assert all(f.numel() > 0 for f in floats)                                       # (nothing below is vacuous)
    coded = inf.to_waveforms(mel, lengths, vocos, encoding=names, sample_rate=rates)
    for b, (f, c) in enumerate(zip(floats, coded)):
        assert c.dtype == torch.uint8 and c.dim() == 1 and c.device.type == "cpu"
        assert np.array_equal(c.numpy(), ar.encode(f.numpy(), ar.NAMES[names[b]])), b
    assert coded[0].untyped_storage().data_ptr() == coded[3].untyped_storage().data_ptr()      # views of one host buffer
    # one name for all rows; untrimmed rows; G.711 only (the copy is of the front half of the stride)
    for kw in (dict(encoding="pcm16"), dict(encoding="ulaw", trim=False), dict(encoding="alaw")):
        fl = inf.to_waveforms(mel, lengths, vocos, trim=kw.get("trim", True), sample_rate=rates)
        for b, c in enumerate(inf.to_waveforms(mel, lengths, vocos, sample_rate=rates, **kw)):
            assert np.array_equal(c.numpy(), ar.encode(fl[b].numpy(), ar.NAMES[kw["encoding"]])), (kw, b)
    # rows with None stay float, bit for bit; dither follows the row's key
    part = inf.to_waveforms(mel, lengths, vocos, encoding=[None, "ulaw", None, "pcm16"], dither=True, dither_keys=[5, 6, 7, 8], sample_rate=rates)
    assert part[0].dtype == torch.float32 and torch.equal(part[0], floats[0]) and torch.equal(part[2], floats[2])
    assert np.array_equal(part[1].numpy(), ar.encode(floats[1].numpy(), ar.ULAW))
    assert np.array_equal(part[3].numpy(), ar.encode(floats[3].numpy(), ar.PCM16, True, 0, 8))
    # no encoding named: the call made before there was a choice
    same = inf.to_waveforms(mel, lengths, vocos, encoding=[None] * 4, sample_rate=rates)
    assert all(torch.equal(a, b) for a, b in zip(same, floats))
    with pytest.raises(ValueError):
        inf.to_waveforms(mel, lengths, vocos, encoding="mp3")
    with pytest.raises(ValueError, match=r"mel_lengths\[1\] = 41"):
        inf.to_waveforms(mel, [40, 41, 25, 12], vocos, encoding="pcm16")


def test_batcher_request_and_service_return_encoded_audio(ac, env, synthetic):
    inf, hp, model, vocos, enc = env
    bt, sv = sub("batcher"), sub("serving")
    ids = synthetic.make_inputs(hp, 1, 20, seed=77)[0][0].tolist()
    common = dict(speaker=1, solver="midpoint", n_timesteps=2)
    with bt.FrameBudgetBatcher(model, max_batch=4, max_tokens=4096, max_wait_ms=1.0, vocoder=vocos) as q:
        plain8 = q.submit(ids, sample_rate=8000, **common).result(timeout=120)
        ulaw8 = q.submit(ids, sample_rate=8000, encoding="ulaw", **common).result(timeout=120)
        plain = q.submit(ids, **common).result(timeout=120)
        dith = q.submit(ids, encoding="pcm16", dither=True, dither_key=31, **common).result(timeout=120)
        svc = sv.SpeechService(q, phonemize=lambda text, lang: ids)
        body = asyncio.run(svc.speak("ignored", voice=1, steps=2, response_format="wav"))
        spoken = asyncio.run(svc.speak("ignored", voice=1, steps=2))
        leg = asyncio.run(svc.speak("ignored", voice=1, steps=2, sample_rate=8000, response_format="alaw"))
    assert set(plain) == {"mel", "mel_length", "audio"} and set(plain8) == {"mel", "mel_length", "audio", "sample_rate"}
    assert set(ulaw8) == {"mel", "mel_length", "audio", "sample_rate", "encoding"} and ulaw8["encoding"] == "ulaw"
    assert plain8["audio"].numel() > 0 and ulaw8["audio"].dtype == torch.uint8
    assert np.array_equal(ulaw8["audio"].numpy(), ar.encode(plain8["audio"].numpy(), ar.ULAW))
    assert dith["encoding"] == "pcm16" and np.array_equal(dith["audio"].numpy(), ar.encode(plain["audio"].numpy(), ar.PCM16, True, 0, 31))
    assert isinstance(body, bytes) and spoken.dtype == torch.float32 and spoken.numel() > 0
    with wave.open(io.BytesIO(body), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 24000, spoken.numel())
        assert w.readframes(w.getnframes()) == ar.encode(spoken.numpy(), ar.PCM16).tobytes()
    assert isinstance(leg, bytes) and len(leg) > 0
    # the per-request tail (MTTS_WAVE_BATCH=0) encodes too
    one, res = [{"mel": plain["mel"]}], [{"mel": plain["mel"]}]
    bt.waveforms_into(one, plain["mel"][None], [plain["mel_length"]], vocos, False, [bt.Request(ids=[1])])
    bt.waveforms_into(res, plain["mel"][None], [plain["mel_length"]], vocos, False, [bt.Request(ids=[1], encoding="alaw")])
    assert set(one[0]) == {"mel", "audio"} and one[0]["audio"].numel() > 0
    assert res[0]["encoding"] == "alaw" and np.array_equal(res[0]["audio"].numpy(), ar.encode(one[0]["audio"].numpy(), ar.ALAW))


def recorded(seconds, rate, i):
    t = torch.arange(int(seconds * rate), dtype=torch.float32) / rate
    g = torch.Generator().manual_seed(40 + i)
    return (0.4 * torch.sin(2 * np.pi * (120.0 + 20.0 * i) * t) + 0.05 * torch.randn(t.numel(), generator=g)).clamp(-1, 1)


def test_recordings_decode_encoded_clips_on_the_device(ac, env):
    inf, hp, model, vocos, enc = env
    clip8, clip24 = recorded(0.5, 8000, 0).numpy(), recorded(0.4, 24000, 1).numpy()
    ulaw, pcm = ar.encode(clip8, ar.ULAW), ar.encode(clip24, ar.PCM16)
    enc_clips = [ac.Encoded(ulaw.tobytes(), "ulaw", 8000), ac.Encoded(torch.from_numpy(pcm.copy()), "pcm16", 24000), torch.from_numpy(clip24)]
    flt_clips = [torch.from_numpy(ar.decode(ulaw, ar.ULAW)), torch.from_numpy(ar.decode(pcm, ar.PCM16)), torch.from_numpy(clip24)]
    want, want_len = inf.recordings(flt_clips, "cuda", [8000, 24000, 24000])
    for rate in (None, [None, None, 24000], [8000, 24000, 24000]):                 # Encoded.sample_rate where none is named
        got, got_len = inf.recordings(enc_clips, "cuda", rate)
        assert got_len == want_len == [12000, 9600, 9600]          # 4000 samples at 8 kHz; 9600 at 24 kHz
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), rate
    # a named rate wins over the clip's own
    as16, n16 = inf.recordings(enc_clips[:1], "cuda", 16000)
    ref16, m16 = inf.recordings(flt_clips[:1], "cuda", 16000)
    assert n16 == m16 == [6000] and torch.equal(as16, ref16)


def test_enroll_voice_from_a_mu_law_wav(ac, env, tmp_path):
    inf, hp, model, vocos, enc = env
    clips = [recorded(0.6, 8000, 2).numpy(), recorded(0.5, 8000, 3).numpy()]
    paths = []
    for i, c in enumerate(clips):
        paths.append(tmp_path / f"leg{i}.wav")
        paths[-1].write_bytes(ac.wav_bytes(ar.encode(c, ar.ULAW).tobytes(), "ulaw", 8000))
    read = [ac.read_wav(p) for p in paths]
    assert all(r.format == "ulaw" and r.sample_rate == 8000 for r in read)
    got = model.enroll_voice(read, enc, sample_rate=None)
    want = model.enroll_voice([torch.from_numpy(ar.decode(ar.encode(c, ar.ULAW), ar.ULAW)) for c in clips], enc, sample_rate=8000)
    assert got[0].shape == (1, hp.spk_emb_dim)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # align takes such a clip too (one clip, not in a list)
    x = torch.tensor([[3, 5, 7, 9, 11, 2]], device="cuda")
    x_len = torch.tensor([6], device="cuda")
    a = model.align(x, x_len, audio=read[0], sample_rate=None)
    b = model.align(x, x_len, audio=[torch.from_numpy(ar.decode(ar.encode(clips[0], ar.ULAW), ar.ULAW))], sample_rate=8000)
    assert torch.equal(a["durations"], b["durations"]) and torch.equal(a["score"], b["score"])

"""FLAC in on the GPU: mtts_flac_decode against the restated decoder (tests/flac_in_restated.py) on the case list and the refusal list of
tests/flac_in_cases.py -- integers to the bit, between sentinel words --, the round trip through the project's own encoder, a row's
independence of its batch, and the recording entries taking ``FlacClip`` files.  Every stream here first passes the CPU host-twin tests
of tests/test_flac_in_abi.py: these test the verdict and the samples, not the machine."""
import numpy as np
import pytest
import torch

from conftest import sub
import audio_codec_restated as ar
import flac_in_cases as fc
import flac_in_restated as fi

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e5)                   # no sample: |q / 2^(bps-1)| <= 1
GUARD = 64


@pytest.fixture(scope="module")
def ac():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("audio_codec")


def raw_decode(streams, ld, ld_bytes=None, max_block=4608):
    """mtts_flac_decode itself on rows whose bytes behind the stream are a run of valid frame headers, into sentinel-filled outputs with
    guard words around them: ``(audio [B, ld], lengths, rates)`` on the host."""
    hip = sub("_hip")
    lib = hip.load()
    B = len(streams)
    ld_bytes = ld_bytes or max(16, (max(len(s) for s in streams) + 15) // 16 * 16)
    junk = np.frombuffer((fc.small_frame() * (ld_bytes // 12 + 1))[:ld_bytes], dtype=np.uint8)
    rows = np.stack([np.r_[np.frombuffer(s, dtype=np.uint8), junk[len(s):]] for s in streams])
    data = torch.from_numpy(rows.copy()).cuda()
    nbytes = torch.tensor([len(s) for s in streams], dtype=torch.long, device="cuda")
    flat = torch.full((B * ld + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    out = flat[GUARD:GUARD + B * ld].view(B, ld)
    lengths = torch.full((B + 2,), -7, dtype=torch.long, device="cuda")
    rates = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(hip.size(lib.mtts_flac_decode_workspace_bytes(B, ld_bytes, ld, max_block)), dtype=torch.uint8, device="cuda")
    hip.check(lib.mtts_flac_decode(hip.ptr(data), ld_bytes, hip.ptr(nbytes), B, max_block, out.data_ptr(), ld, lengths[1:].data_ptr(),
                                   rates[1:].data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr()))
    torch.cuda.synchronize()
    flat, lengths, rates = flat.cpu().numpy(), lengths.tolist(), rates.tolist()
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "words outside d_out were written"
    assert lengths[0] == lengths[-1] == rates[0] == rates[-1] == -7
    assert lib.mtts_pcm_status(hip.ptr(torch.tensor(lengths[1:-1], device="cuda")), B, hip.stream_ptr()) == (-1 if -1 in lengths else 0)
    return flat[GUARD:-GUARD].reshape(B, ld), lengths[1:-1], rates[1:-1]


def assert_row(audio, length, rate, want, name):
    """One accepted row against the restated decoder: ``restated_int / 2^(bps-1)`` with ==, zeros behind the length."""
    x = want["samples"][0]
    assert (length, rate) == (len(x), want["rate"]), name
    assert np.array_equal(audio[:len(x)], (x / float(1 << (want["bps"] - 1))).astype(np.float32)), name
    assert x.size == 0 or np.abs(x).max() < 1 << 24                # (so the division above is exact in fp32 too)
    assert not audio[len(x):].any(), name


def test_case_list_equals_the_restated_decoder(ac):
    names = list(fc.good())
    assert len(names) <= 24
    audio, lengths, rates = raw_decode([fc.good()[n] for n in names], 8196)
    for b, name in enumerate(names):
        assert_row(audio[b], lengths[b], rates[b], fc.expected()[name], name)
    assert sorted(set(lengths))[0] == 0 and max(lengths) == 8193


@pytest.mark.parametrize("bs", [256, 4096])
def test_round_trip_with_the_projects_own_encoder(ac, bs):
    L = 2 * 4096 + 700
    rng, t = np.random.default_rng(bs), np.arange(L) / 24000.0
    speech = 0.3 * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * 180 * t) + 0.1 * np.sin(2 * np.pi * 1900 * t) + 0.002 * rng.standard_normal(L)
    noise = rng.uniform(-1.2, 1.2, L)                              # full scale and beyond: the VERBATIM path, with clamped words
    audio = torch.from_numpy(np.stack([speech, noise, speech, noise]).astype(np.float32)).cuda()
    lengths, keys = [L, L, 4096, 257], [3, 4, 5, 6]
    for dither in (False, True):
        data, nbytes = ac.encode_flac(audio, lengths, [24000, 8000, 11025, 100000], bs, dither=dither, seed=9, keys=keys, check=True)
        got, got_len, got_rates = ac.decode_flac(data, nbytes, ld=L)
        pcm, _ = ac.encode(audio, lengths, "pcm16", dither=dither, seed=9, keys=keys)
        want = ac.decode(pcm, lengths, "pcm16", ld=L)
        assert got_len.tolist() == lengths and got_rates.tolist() == [24000, 8000, 11025, 100000]
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), (bs, dither)
        assert got[0].abs().max() > 0.2 and got[1].abs().max() == 1.0


def test_a_row_does_not_depend_on_its_batch(ac):
    names = ["lpc_small", "stereo", "variable", "block_576", "lpc_wide", "metadata", "embedded", "empty", "numbers", "wasted"]
    good = [fc.good()[n] for n in names]
    bad = [fc.refused()[n][0] for n in ("crc16_flip", "zero_tail", "bytes_3", "partition_below_order")]
    audio, lengths, rates = raw_decode(good, 5040)
    for b, name in enumerate(names):
        assert_row(audio[b], lengths[b], rates[b], fc.expected()[name], name)
    rev = raw_decode(good[::-1], 6000, ld_bytes=8192)
    mixed = raw_decode([bad[0], good[0], bad[1], good[1], good[2], bad[2], bad[3]] + good[3:], 5040, ld_bytes=16384)
    at = [1, 3, 4] + list(range(7, 7 + len(good) - 3))
    for b, name in enumerate(names):
        n = lengths[b]
        alone = raw_decode([good[b]], max(4, (n + 3) // 4 * 4))
        for other, row in ((rev, len(names) - 1 - b), (mixed, at[b]), (alone, 0)):
            assert (other[1][row], other[2][row]) == (n, rates[b]), name
            assert np.array_equal(other[0][row, :n].view(np.uint32), audio[b, :n].view(np.uint32)) and not other[0][row, n:].any(), name
    assert [mixed[1][i] for i in (0, 2, 5, 6)] == [-1] * 4


def test_refusal_list_with_good_neighbours(ac):
    names = [n for n in fc.refused() if n != "total_above_ld"]
    good = [fc.good()[n] for n in ("lpc_small", "stereo", "rice_k", "escape")]
    wants = [fc.expected()[n] for n in ("lpc_small", "stereo", "rice_k", "escape")]
    seen = 0
    for i in range(0, len(names), 10):
        chunk = names[i:i + 10]
        streams = [good[0]]
        for j, name in enumerate(chunk):
            streams += [fc.refused()[name][0], good[(j + 1) % 4]]
        assert len(streams) <= 24
        audio, lengths, rates = raw_decode(streams, 260)
        for b in range(len(streams)):
            if b % 2 == 0:
                assert_row(audio[b], lengths[b], rates[b], wants[(b // 2) % 4], chunk[min(b // 2, len(chunk) - 1)])
            else:
                name = chunk[b // 2]
                assert (lengths[b], rates[b]) == (-1, 0), name
                assert (audio[b] == SENTINEL).all(), name           # no word of a refused row is written
                seen += 1
    assert seen == len(names) >= 24
    # the sample total above ld: the same stream is accepted where it fits
    stream, ld = fc.refused()["total_above_ld"]
    audio, lengths, rates = raw_decode([good[0], stream, good[1]], ld)
    assert lengths == [64, -1, 64] and rates[1] == 0 and (audio[1] == SENTINEL).all()
    assert_row(audio[0], lengths[0], rates[0], wants[0], "neighbour")
    assert_row(audio[2], lengths[2], rates[2], wants[1], "neighbour")
    assert raw_decode([stream], 256)[1] == [256]
    # a block size above the call's max_block, and an nbytes outside the row
    assert raw_decode([fc.good()["block_576"], good[0]], 1156, max_block=575)[1] == [-1, 64]
    assert raw_decode([fc.good()["block_576"], good[0]], 1156, max_block=576)[1] == [1153, 64]


# ------------------------------------------------------------------------------------------------ the recording entries
SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)


@pytest.fixture(scope="module")
def env(ac, hparams, synthetic):
    inf, style = sub("inference"), sub("style")
    hp = hparams.tiny(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to("cuda").eval()
    torch.manual_seed(21)
    enc = style.StyleEncoder(hp.n_feats, 32, 2, hp.spk_emb_dim).to("cuda").eval()
    return inf, hp, model, enc


def recorded(seconds, rate, i):
    t = torch.arange(int(seconds * rate), dtype=torch.float32) / rate
    g = torch.Generator().manual_seed(40 + i)
    return (0.4 * torch.sin(2 * np.pi * (120.0 + 20.0 * i) * t) + 0.05 * torch.randn(t.numel(), generator=g)).clamp(-1, 1)


def stereo_flac(seconds, rate, i, bs=1152):
    """A 16-bit stereo FLAC file (mid/side and left/side frames, FIXED and LPC subframes) and its left channel's words."""
    left = np.rint(recorded(seconds, rate, i).numpy() * 32767).astype(np.int64)
    right = np.rint(recorded(seconds, rate, i + 7).numpy() * 20000).astype(np.int64)
    lpc = {"kind": "lpc", "coefs": [1800, -700, 90], "precision": 12, "shift": 10, "po": 2}
    frames = [{"samples": [left[j:j + bs], right[j:j + bs]], "stereo": ("ms", "ls", "sr")[k % 3],
               "sub": [lpc, fc.FIX2] if len(left) - j >= bs else fc.FIX2} for k, j in enumerate(range(0, len(left), bs))]
    return fi.write_stream(frames, rate=rate, channels=2)[0], left


def test_recording_entries_take_flac_clips(ac, env, monkeypatch):
    inf, hp, model, enc = env
    data, left = stereo_flac(0.5, 16000, 0)
    clip8, clip24 = recorded(0.5, 8000, 1).numpy(), recorded(0.4, 24000, 2)
    ulaw = ar.encode(clip8, ar.ULAW)
    flac = ac.read_flac(data)
    assert (flac.sample_rate, flac.samples, flac.channels, flac.bits_per_sample, flac.max_block) == (16000, 8000, 2, 16, 1152)
    calls = []
    lib = sub("_hip").load()
    for name in ("mtts_pcm_decode", "mtts_flac_decode"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    clips = [flac, ac.Encoded(ulaw.tobytes(), "ulaw", 8000), clip24]
    plain = [torch.from_numpy((left / 32768.0).astype(np.float32)), torch.from_numpy(ar.decode(ulaw, ar.ULAW)), clip24]
    want, want_len = inf.recordings(plain, "cuda", [16000, 8000, 24000])
    assert calls == []                                              # waveforms: nothing is decoded
    for rate in (None, [None, None, 24000], [16000, 8000, 24000]):  # the clip's own rate where none is named
        calls.clear()
        got, got_len = inf.recordings(clips, "cuda", rate)
        assert sorted(calls) == ["mtts_flac_decode", "mtts_pcm_decode"]
        assert got_len == want_len == [12000, 12000, 9600]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), rate
    calls.clear()
    inf.recordings(clips[1:], "cuda", None)
    assert calls == ["mtts_pcm_decode"]                             # without a FlacClip: the launch sequence of before
    a = model.enroll_voice(clips, enc, sample_rate=None)
    b = model.enroll_voice(plain, enc, sample_rate=[16000, 8000, 24000])
    assert a[0].shape == (1, hp.spk_emb_dim) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    x, x_len = torch.tensor([[3, 5, 7, 9, 11, 2]], device="cuda"), torch.tensor([6], device="cuda")
    one = model.align(x, x_len, audio=flac, sample_rate=None)       # one clip, not in a list
    two = model.align(x, x_len, audio=[plain[0]], sample_rate=16000)
    assert torch.equal(one["durations"], two["durations"]) and torch.equal(one["score"], two["score"])
    # a file the device refuses is named, not read as silence
    bad = ac.read_flac(data[:-1])
    with pytest.raises(ValueError, match="refused"):
        inf.recordings([bad, clip24], "cuda", None)
    # decode_clips of FLAC files alone, a device tensor among them
    two_clips = [flac, ac.FlacClip(torch.frombuffer(bytearray(fc.good()["lpc_wide"]), dtype=torch.uint8).cuda(), 48000, 96, 1, 24, 96)]
    wave, counts = ac.decode_clips(two_clips, "cuda", check=True)
    assert counts == [8000, 96] and torch.equal(wave[0, :8000].cpu(), plain[0])
    assert np.array_equal(wave[1, :96].cpu().numpy() * float(1 << 23), fc.TRUTH["lpc_wide"][0].astype(np.float32))

"""Sample-rate conversion on the GPU: the kernel against the NumPy restatement (bit for bit in the documented order, and inside the
serial-sum bound of the dense fp64 evaluation), batch independence, the guarded lengths, two signal properties, and the wiring
into the recording entries (inbound) and the waveform tail (outbound)."""
import numpy as np
import pytest
import torch

from conftest import sub
import resample_restated as rr

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 24000), (44100, 24000), (16000, 24000), (24000, 8000), (24000, 44100)]
IDS = [f"{a}to{b}" for a, b in PAIRS]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def res():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("resample")


def tile_row_length(o, n, tile, longest):
    """A clip length whose out_len is one more than a multiple of the kernel's tile."""
    for m in range(1, 64):
        want = m * tile + 1
        L = want * o // n
        for cand in (L - 1, L, L + 1):
            if 0 < cand <= longest and rr.out_length(cand, o, n) == want:
                return cand
    raise AssertionError("no clip length gives out_len = multiple of the tile + 1")


_cases = {}


def case(res, pair):
    """Inputs, the device result and the two restated references of one rate pair: computed once, shared by the tests."""
    if pair in _cases:
        return _cases[pair]
    o, n, width, taps = rr.factors(*pair)
    K = rr.bank32(*pair)
    lengths = [0, 1, 5, 3 * o, 2531, 20000]
    lengths.append(tile_row_length(o, n, res.TILE, 20000))
    ld_in = (max(lengths) + 3) // 4 * 4
    rng = np.random.default_rng(1000 + pair[0] // 100 + pair[1] // 100)
    x = rng.uniform(-1, 1, (len(lengths), ld_in)).astype(np.float32)
    rs = res.Resampler(*pair)
    out, out_len = rs(torch.from_numpy(x).cuda(), lengths)
    want32 = [rr.resample32(x[b, :L], K, o, n, width) for b, L in enumerate(lengths)]
    want64 = [rr.resample64(x[b, :L], K, o, n, width) for b, L in enumerate(lengths)]
    _cases[pair] = dict(o=o, n=n, width=width, taps=taps, K=K, lengths=lengths, ld_in=ld_in, x=x, rs=rs, out=out.cpu(), out_len=out_len.cpu(),
                        want32=want32, want64=want64)
    return _cases[pair]


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_parity_with_the_restatement(res, pair):
    c = case(res, pair)
    rs, out, o, n = c["rs"], c["out"], c["o"], c["n"]
    assert (rs.o, rs.n, rs.width, rs.taps) == (o, n, c["width"], c["taps"]) and rs.band == rr.band_of(c["K"])
    assert out.shape[1] % 4 == 0 and out.shape[1] >= rr.out_length(c["ld_in"], o, n)
    assert c["out_len"].tolist() == [rr.out_length(L, o, n) for L in c["lengths"]] == [rs.out_length(L) for L in c["lengths"]]
    assert c["out_len"][-1] % res.TILE == 1                                    # the row that ends one sample into a tile
    worst = 0.0
    for b, L in enumerate(c["lengths"]):
        m = rr.out_length(L, o, n)
        got = out[b, :m]
        # (a) the documented order, bit for bit
        assert torch.equal(bits(got), bits(torch.from_numpy(c["want32"][b]))), (pair, b)
        # (b) the dense fp64 evaluation of the fp32 bank, inside the serial-sum bound
        ref, mag = c["want64"][b]
        err = np.abs(got.double().numpy() - ref)
        bound = (rs.band + 1) * 2.0 ** -24 * mag
        if m:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (pair, b, float((err - bound).max()))
        # (c) zeros from out_len to ld_out
        assert not out[b, m:].any(), (pair, b)
    print(f"{pair}: worst error / bound = {worst:.3f}")


def test_batch_independence_and_repeatability(res):
    pair = (44100, 24000)
    c = case(res, pair)
    rs = c["rs"]
    x = torch.from_numpy(c["x"]).cuda()
    lengths = c["lengths"]
    m = int(c["out_len"][4])
    alone, n_alone = rs(x[4:5].contiguous(), lengths[4:5])
    again, _ = rs(x, lengths)
    rev, n_rev = rs(x.flip(0).contiguous(), lengths[::-1])
    assert int(n_alone[0]) == m and n_rev.flip(0).tolist() == c["out_len"].tolist()
    assert torch.equal(bits(alone[0, :m]), bits(c["out"][4, :m])) and not alone[0, m:].any()
    assert torch.equal(bits(rev.flip(0)), bits(c["out"]))
    assert torch.equal(bits(again), bits(c["out"]))


@pytest.mark.parametrize("pair", [(44100, 24000), (24000, 44100)], ids=["44100to24000", "24000to44100"])
def test_guarded_lengths_and_poisoned_margins(res, pair):
    c = case(res, pair)
    rs, ld_in = c["rs"], c["ld_in"]
    B = len(c["lengths"])
    lengths = list(c["lengths"])
    lengths[3], lengths[5] = ld_in + 1, -3
    margin = 4096
    big = torch.full((B * ld_in + margin,), float("nan"), dtype=torch.float32)
    audio = big[:B * ld_in].view(B, ld_in)
    for b, L in enumerate(lengths):
        if 0 <= L <= ld_in:
            audio[b, :L] = torch.from_numpy(c["x"][b, :L])              # NaN from len_b to the end of the row, and after the buffer
    big = big.cuda()
    dev_audio = big[:B * ld_in].view(B, ld_in)
    assert dev_audio.data_ptr() % 16 == 0
    out, out_len = rs(dev_audio, lengths, check=False)
    with pytest.raises(ValueError, match=rf"row 3 has length {ld_in + 1}"):
        rs.status()
    out, out_len = out.cpu(), out_len.cpu()
    assert torch.isfinite(out).all()                                     # the margins were never read
    assert out_len[3] == -1 and out_len[5] == -1 and not out[3].any() and not out[5].any()
    for b in (0, 1, 2, 4, 6):
        assert out_len[b] == c["out_len"][b]
        assert torch.equal(bits(out[b]), bits(c["out"][b])), b
    # out_len larger than the output row: refused on the device too
    short, n_short = rs(dev_audio[:, :2532].contiguous(), [2531] * B, check=False, ld_out=64)
    assert n_short.tolist() == [-1] * B and not short.any()
    with pytest.raises(ValueError, match="row 0 has length 2531"):
        rs(dev_audio[:1, :2532].contiguous(), [2531], ld_out=64)


def test_signal_properties_48000_to_24000(res):
    t = np.arange(6000, dtype=np.float64)
    x = np.sin(2 * np.pi * 440.0 * t / 48000.0).astype(np.float32)
    y, n = res.resample(torch.from_numpy(x).cuda()[None], None, 48000, 24000)
    assert int(n[0]) == 3000
    want = np.sin(2 * np.pi * 440.0 * np.arange(3000, dtype=np.float64) / 24000.0)
    err = np.abs(y[0, :3000].cpu().double().numpy() - want)[200:-200].max()
    print(f"440 Hz sine: max error {err:.2e}")
    assert err < 1e-3
    t = np.arange(12000, dtype=np.float64)
    x = np.sin(2 * np.pi * 15000.0 * t / 48000.0).astype(np.float32)     # above the new Nyquist frequency
    y, n = res.resample(torch.from_numpy(x).cuda()[None], None, 48000, 24000)
    assert int(n[0]) == 6000
    peak = y[0, 750:5250].abs().max().item()
    print(f"15 kHz sine: residual peak {peak:.4f}")
    assert peak < 0.01


# ------------------------------------------------------------------------------------------------ wiring
@pytest.fixture(scope="module")
def voice_env(res, hparams, synthetic):
    """The synthetic model and style encoder of ``tools/enroll.py --synthetic``."""
    inf, style = sub("inference"), sub("style")
    hp = hparams.prod_v20(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to("cuda").eval()
    torch.manual_seed(0)
    enc = style.StyleEncoder(**style.DEFAULT_CFG).to("cuda").eval()
    return inf, hp, model, enc


def clip(rate, seconds, i):
    t = torch.arange(int(seconds * rate), dtype=torch.float32) / rate
    g = torch.Generator().manual_seed(40 + i)
    return (0.4 * torch.sin(2 * np.pi * (120.0 + 20.0 * i) * t) + 0.05 * torch.randn(t.numel(), generator=g)).clamp(-1, 1)


def converted(res, c, rate):
    out, n = res.resample(c.cuda()[None], None, rate, 24000)
    return out[0, :int(n[0])].clone()


def test_nothing_moves_at_24_khz(res, voice_env):
    inf, hp, model, enc = voice_env
    res.clear_cache()
    clips = [clip(24000, 1.0, i) for i in range(2)]
    a = model.enroll_voice(clips, enc)
    b = model.enroll_voice(clips, enc, sample_rate=24000)
    assert res.cached() == 0                                             # no resampler was ever built: no new launch
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_inbound_composition(res, voice_env, synthetic):
    inf, hp, model, enc = voice_env
    clips48 = [clip(48000, 1.0, i) for i in range(2)]
    got = model.enroll_voice(clips48, enc, sample_rate=48000)
    want = model.enroll_voice([converted(res, c, 48000) for c in clips48], enc)
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    assert res.cached() >= 1

    x, x_len, _ = synthetic.make_inputs(hp, 2, 12, seed=321, lengths=[12, 9])
    x, x_len = x.cuda(), x_len.cuda()
    mixed = [clip(44100, 1.0, 5), clip(24000, 1.0, 6)]
    a = model.align(x, x_len, audio=mixed, sample_rate=[44100, 24000])
    b = model.align(x, x_len, audio=[converted(res, mixed[0], 44100), mixed[1]])
    assert a["mel_fine_lengths"].tolist() == b["mel_fine_lengths"].tolist() == [24000 // 128 + 1] * 2
    for k in ("durations", "predicted_durations", "scale_correction", "score"):
        assert torch.equal(bits(a[k].float()), bits(b[k].float())), k

    s = model.score(x, x_len, audio=[clip(16000, 1.0, 7), clip(16000, 1.0, 8)], sample_rate=16000, t=torch.tensor([0.3, 0.6]))
    for k in ("dur_loss", "prior_loss", "diff_loss"):
        assert torch.isfinite(s[k]).all(), k
    with pytest.raises(ValueError):
        model.enroll_voice(clips48, enc, sample_rate=[48000])           # one rate per clip, or one int
    with pytest.raises(ValueError):
        model.enroll_voice(clips48, enc, sample_rate=1000)              # outside [4000, 384000]


def test_outbound(res, voice_env, synthetic):
    inf, hp, model, enc = voice_env
    wrapper = sub("vocoder").load_model("cuda", state_dict=synthetic.make_vocos_state_dict(seed=11))
    g = torch.Generator().manual_seed(3)
    lengths = [40, 33, 25]
    mel = (torch.randn(3, 100, 40, generator=g) * 2.0 - 4.0).cuda()
    base = inf.to_waveforms(mel, lengths, wrapper)
    rates = [24000, 8000, 48000]
    out = inf.to_waveforms(mel, lengths, wrapper, sample_rate=rates)
    assert torch.equal(bits(out[0]), bits(base[0]))
    for b in (1, 2):
        rs = res.resampler(24000, rates[b], "cuda")
        assert out[b].numel() == rs.out_length(base[b].numel())
        if base[b].numel():
            want, n = res.resample(base[b].cuda()[None], None, 24000, rates[b])
            assert int(n[0]) == out[b].numel()
            assert torch.equal(bits(out[b]), bits(want[0, :int(n[0])])), b
    assert any(base[b].numel() for b in (1, 2))
    # untrimmed rows convert their whole length
    raw = inf.to_waveforms(mel, lengths, wrapper, trim=False, sample_rate=rates)
    assert raw[0].numel() == 256 * 39 and raw[1].numel() == res.resampler(24000, 8000, "cuda").out_length(256 * 32)

    bt = sub("batcher")
    # the per-request tail (MTTS_WAVE_BATCH=0) converts too
    one24, one8 = [{"mel": mel[1, :, :33]}], [{"mel": mel[1, :, :33]}]
    bt.waveforms_into(one24, mel[1:2, :, :33], [33], wrapper, False, [bt.Request(ids=[1])])
    bt.waveforms_into(one8, mel[1:2, :, :33], [33], wrapper, False, [bt.Request(ids=[1], sample_rate=8000)])
    assert "sample_rate" not in one24[0] and one8[0]["sample_rate"] == 8000       # a 24 kHz result keeps the keys it always had
    assert one8[0]["audio"].numel() == res.resampler(24000, 8000, "cuda").out_length(one24[0]["audio"].numel())
    if one24[0]["audio"].numel():
        want, n = res.resample(one24[0]["audio"].cuda()[None], None, 24000, 8000)
        assert torch.equal(bits(one8[0]["audio"]), bits(want[0, :int(n[0])]))
    ids = synthetic.make_inputs(hp, 1, 20, seed=77)[0][0].tolist()
    with bt.FrameBudgetBatcher(model, max_batch=4, max_tokens=4096, max_wait_ms=1.0, vocoder=wrapper) as q:
        f16 = q.submit(ids, speaker=1, solver="midpoint", n_timesteps=2, sample_rate=16000)
        r16 = f16.result(timeout=120)
        f24 = q.submit(ids, speaker=1, solver="midpoint", n_timesteps=2)
        r24 = f24.result(timeout=120)
    assert r16["sample_rate"] == 16000 and set(r24) == {"mel", "mel_length", "audio"}
    assert r16["mel_length"] == r24["mel_length"]
    assert r16["audio"].numel() == res.resampler(24000, 16000, "cuda").out_length(r24["audio"].numel())

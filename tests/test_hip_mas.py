"""Forced alignment on the GPU: the search against the NumPy restatement bit for bit, the fp32 log-prior against fp64, planted
alignments, the device-side refusals, synthesis with given durations, and the loop audio -> align -> synthesise(durations=...)."""
import numpy as np
import pytest
import torch

from conftest import sub
import enroll_restated as E
import mas_restated as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 5), (64, 64), (65, 300), (130, 131), (128, 1500), (600, 2300), (1024, 1024)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def hip(dev, hparams):
    """A context only for its workspace cache and stream plumbing: the search needs no weights."""
    h = sub("_hip").HipModel(hparams.tiny(n_spks=2))
    h.device = dev
    return h


def ragged_lengths(rng, B, Tx, Tm):
    """Utterance 0 fills the padded shape; the others draw 1 <= Tx_b <= Tx and Tx_b <= Tm_b <= Tm (tight cases included)."""
    xl, yl = [Tx], [Tm]
    for b in range(1, B):
        x = int(rng.integers(1, Tx + 1))
        y = x if b % 5 == 1 else int(rng.integers(x, Tm + 1))
        xl.append(x)
        yl.append(y)
    return xl, yl


def check_against_restatement(lp, xl, yl, dur, score, path, rows=None):
    B, Tx, Tm = lp.shape
    for b in (range(B) if rows is None else rows):
        d, p, s = R.maximum_path(lp[b], xl[b], yl[b])
        assert np.array_equal(dur[b], d), (b, xl[b], yl[b])
        assert score[b] == s, (b, score[b], s)
        if path is not None:
            assert np.array_equal(path[b], p), b
        assert dur[b].sum() == yl[b] and (dur[b, :xl[b]] >= 1).all() and (dur[b, xl[b]:] == 0).all()


@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("Tx,Tm", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "integer"])
def test_search_equals_restatement_bitwise(hip, dev, Tx, Tm, B, kind):
    if B == 32 and Tx * Tm > 128 * 1500:
        B = 8                                   # (the host restatement is a Python loop over frames: keep the big shapes affordable)
    rng = np.random.default_rng(Tx * 7919 + Tm * 31 + B)
    if kind == "normal":
        lp = rng.standard_normal((B, Tx, Tm)).astype(np.float32) * 3.0
    else:
        lp = rng.integers(-3, 2, size=(B, Tx, Tm)).astype(np.float32)           # ties everywhere
    xl, yl = ragged_lengths(rng, B, Tx, Tm)
    d_lp = torch.from_numpy(lp).to(dev)
    d_xl, d_yl = torch.tensor(xl, device=dev), torch.tensor(yl, device=dev)
    want_path = Tx * Tm * B <= 8 * 600 * 2300
    dur, score, path = hip.mas(d_xl, d_yl, lp=d_lp, return_path=want_path)
    dur, score = dur.cpu().numpy(), score.cpu().numpy()
    path = path.cpu().numpy() if want_path else None
    assert dur.dtype == np.int32 and dur.shape == (B, Tx)
    rows = None if B * Tm <= 8 * 2300 else sorted({0, 1, B // 2, B - 1})
    check_against_restatement(lp, xl, yl, dur, score, path, rows)
    # an utterance's result does not depend on the batch it is in
    b = B - 1
    solo = hip.mas(d_xl[b:b + 1], d_yl[b:b + 1], lp=d_lp[b:b + 1].contiguous())
    assert np.array_equal(solo[0].cpu().numpy()[0], dur[b]) and solo[1].cpu().numpy()[0] == score[b]
    # two calls give the same bits
    again = hip.mas(d_xl, d_yl, lp=d_lp)
    assert np.array_equal(again[0].cpu().numpy(), dur) and np.array_equal(again[1].cpu().numpy(), score)


@pytest.mark.parametrize("Tx,Tm,B", [(5, 9, 3), (65, 300, 3), (130, 400, 4), (300, 700, 2)])
def test_padding_never_reaches_the_search(hip, dev, Tx, Tm, B):
    rng = np.random.default_rng(Tx + Tm)
    lp = rng.standard_normal((B, Tx, Tm)).astype(np.float32)
    xl, yl = ragged_lengths(rng, B, Tx, Tm)
    xl[0], yl[0] = max(Tx // 2, 1), Tm - 1
    poisoned = lp.copy()
    for b in range(B):
        poisoned[b, xl[b]:, :] = np.nan
        poisoned[b, :, yl[b]:] = np.nan
    d_xl, d_yl = torch.tensor(xl, device=dev), torch.tensor(yl, device=dev)
    clean = hip.mas(d_xl, d_yl, lp=torch.from_numpy(lp).to(dev), return_path=True)
    dirty = hip.mas(d_xl, d_yl, lp=torch.from_numpy(poisoned).to(dev), return_path=True)
    for a, c in zip(clean, dirty):
        assert torch.equal(a, c)
    check_against_restatement(lp, xl, yl, dirty[0].cpu().numpy(), dirty[1].cpu().numpy(), dirty[2].cpu().numpy())


@pytest.mark.parametrize("F,Tx,Tm,B", [(20, 12, 40, 2), (20, 70, 333, 3), (100, 128, 1500, 2), (100, 200, 641, 3)])
def test_log_prior_against_fp64(hip, dev, F, Tx, Tm, B):
    rng = np.random.default_rng(F + Tx)
    mu = rng.standard_normal((B, F, Tx)).astype(np.float32)
    y = (rng.standard_normal((B, F, Tm)) * 1.5 + 0.3).astype(np.float32)
    xl, yl = ragged_lengths(rng, B, Tx, Tm)
    lp = hip.mas_logprior(torch.from_numpy(mu).to(dev), torch.from_numpy(y).to(dev), torch.tensor(xl, device=dev),
                          torch.tensor(yl, device=dev)).cpu().numpy()
    assert lp.shape == (B, Tx, Tm) and lp.dtype == np.float32
    for b in range(B):
        ref = R.log_prior(mu[b, :, :xl[b]], y[b, :, :yl[b]])
        assert np.abs(lp[b, :xl[b], :yl[b]] - ref).max() <= 1e-5 * np.abs(ref).max()
        assert (lp[b, xl[b]:] == 0).all() and (lp[b, :, yl[b]:] == 0).all()


def planted(rng, B, F, Tx, sigma=0.0):
    xl = [Tx] + [int(rng.integers(1, Tx + 1)) for _ in range(B - 1)]
    mu = rng.standard_normal((B, F, Tx)).astype(np.float32)
    d = np.zeros((B, Tx), dtype=np.int32)
    for b in range(B):
        d[b, :xl[b]] = rng.integers(1, 13, size=xl[b])
    yl = d.sum(1).tolist()
    y = np.zeros((B, F, max(yl)), dtype=np.float32)
    for b in range(B):
        y[b, :, :yl[b]] = R.expand(mu[b, :, :xl[b]], d[b, :xl[b]])
        if sigma:
            y[b, :, :yl[b]] += (sigma * rng.standard_normal((F, yl[b]))).astype(np.float32)
    return mu, y, d, xl, yl


@pytest.mark.parametrize("F,Tx,B", [(20, 9, 3), (20, 100, 4), (100, 128, 32), (100, 300, 2)])
def test_planted_alignment_is_recovered(hip, dev, F, Tx, B):
    rng = np.random.default_rng(F * Tx + B)
    mu, y, d, xl, yl = planted(rng, B, F, Tx)
    dur, score, _ = hip.mas(torch.tensor(xl, device=dev), torch.tensor(yl, device=dev), mu_x=torch.from_numpy(mu).to(dev),
                            y=torch.from_numpy(y).to(dev))
    assert np.array_equal(dur.cpu().numpy(), d)
    assert (score.cpu().numpy() == 0).all()              # every frame of the true path scores -0.5 |y - mu|^2 = 0 exactly


@pytest.mark.parametrize("F,Tx,B", [(20, 30, 3), (100, 128, 4)])
def test_noisy_alignment_is_optimal_to_rounding(hip, dev, F, Tx, B):
    rng = np.random.default_rng(F + Tx + B)
    mu, y, d, xl, yl = planted(rng, B, F, Tx, sigma=0.3)
    dur, _, _ = hip.mas(torch.tensor(xl, device=dev), torch.tensor(yl, device=dev), mu_x=torch.from_numpy(mu).to(dev),
                        y=torch.from_numpy(y).to(dev))
    dur = dur.cpu().numpy()
    for b in range(B):
        lp64 = R.log_prior(mu[b, :, :xl[b]], y[b, :, :yl[b]])
        _, _, best = R.maximum_path(lp64)
        assert dur[b].sum() == yl[b] and (dur[b, :xl[b]] >= 1).all()
        starts = np.concatenate([[0], np.cumsum(dur[b, :xl[b]])])
        got = sum(lp64[x, starts[x]:starts[x + 1]].sum() for x in range(xl[b]))
        assert got <= best + 1e-9 and abs(got - best) <= 1e-5 * abs(best), (b, got, best)


def test_refusals(hip, dev):
    lib = hip.lib
    lp = torch.zeros(2, 4, 8, device=dev)
    xl, yl = torch.tensor([4, 3], device=dev), torch.tensor([8, 5], device=dev)
    with pytest.raises(RuntimeError, match="Tm < Tx"):
        hip.mas(xl, yl, lp=torch.zeros(2, 9, 8, device=dev))
    with pytest.raises(RuntimeError, match="1024"):
        hip.mas(torch.tensor([4], device=dev), torch.tensor([8], device=dev), lp=torch.zeros(1, 1025, 1030, device=dev))
    dur = torch.empty(2, 4, dtype=torch.int32, device=dev)
    ws = torch.empty(64, dtype=torch.uint8, device=dev)
    assert lib.mtts_mas(lp.data_ptr(), None, None, xl.data_ptr(), yl.data_ptr(), 2, 0, 4, 8, dur.data_ptr(), None, None, ws.data_ptr(), 64,
                        None) == -1 and b"workspace" in lib.mtts_last_error()
    assert lib.mtts_mas(lp.data_ptr(), None, None, None, yl.data_ptr(), 2, 0, 4, 8, dur.data_ptr(), None, None, ws.data_ptr(), 64,
                        None) == -1 and b"null" in lib.mtts_last_error()
    # one bad utterance in a batch: its row is zeroed, the status names it, the others are right
    rng = np.random.default_rng(3)
    B, Tx, Tm = 5, 70, 200
    lpn = rng.standard_normal((B, Tx, Tm)).astype(np.float32)
    for bad_row, (bx, by) in [(2, (40, 39)), (0, (71, 200)), (4, (10, 201)), (1, (0, 50)), (3, (-2, 7))]:
        xls, yls = [Tx, 33, 50, 1, 70], [Tm, 33, 120, 200, 70]
        xls[bad_row], yls[bad_row] = bx, by
        d_xl, d_yl = torch.tensor(xls, device=dev), torch.tensor(yls, device=dev)
        dur, score, path = hip.mas(d_xl, d_yl, lp=torch.from_numpy(lpn).to(dev), return_path=True, check_lengths=False)
        with pytest.raises(ValueError, match=f"utterance {bad_row} "):
            hip.mas_status()
        dur, score, path = dur.cpu().numpy(), score.cpu().numpy(), path.cpu().numpy()
        assert (dur[bad_row] == 0).all() and score[bad_row] == 0 and (path[bad_row] == 0).all()
        good = [b for b in range(B) if b != bad_row]
        check_against_restatement(lpn, xls, yls, dur, score, path, good)
        with pytest.raises(ValueError, match="x_length"):
            hip.mas(d_xl, d_yl, lp=torch.from_numpy(lpn).to(dev))
    # two bad utterances: the first is reported
    d_xl, d_yl = torch.tensor([70, 60, 50, 1, 70], device=dev), torch.tensor([200, 59, 49, 200, 70], device=dev)
    with pytest.raises(ValueError, match="utterance 1 "):
        hip.mas(d_xl, d_yl, lp=torch.from_numpy(lpn).to(dev))
    # and a clean call afterwards reports nothing
    hip.mas(torch.tensor([70] * 5, device=dev), torch.tensor([200] * 5, device=dev), lp=torch.from_numpy(lpn).to(dev))


@torch.inference_mode()          # (capture as the package does, modules.py: the device generator's graph state may be inference tensors)
def test_mas_replays_in_a_hip_graph(hip, dev):
    rng = np.random.default_rng(11)
    mu, y, d, xl, yl = planted(rng, 4, 20, 90)
    d_mu, d_y = torch.from_numpy(mu).to(dev), torch.from_numpy(y).to(dev)
    d_xl, d_yl = torch.tensor(xl, device=dev), torch.tensor(yl, device=dev)
    eager = hip.mas(d_xl, d_yl, mu_x=d_mu, y=d_y)                   # also sizes the cached workspace before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.mas(d_xl, d_yl, mu_x=d_mu, y=d_y)                       # this stream's workspace
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dur, score, _ = hip.mas(d_xl, d_yl, mu_x=d_mu, y=d_y, check_lengths=False)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        dur.zero_()
        score.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dur, eager[0]) and torch.equal(score, eager[1])
    assert np.array_equal(dur.cpu().numpy(), d)


# ------------------------------------------------------------------------------------------------ the model level
@pytest.fixture(scope="module", params=["tiny", "prod"])
def env(request, hparams, synthetic, dev):
    inf = sub("inference")
    hp = hparams.tiny(n_spks=3) if request.param == "tiny" else hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    m = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    m.decoder.solver = "midpoint"
    return hp, sd, m


def noise(synthetic, hp, B, dev):
    return lambda t_pad: synthetic.cpu_noise((B, hp.n_feats, t_pad)).to(dev)


def inputs(synthetic, hp, lengths, dev, seed=1234):
    x, x_len, spk = synthetic.make_inputs(hp, len(lengths), max(lengths), seed=seed, lengths=lengths)
    return x.to(dev), x_len.to(dev), spk.to(dev)


@pytest.mark.parametrize("lengths", [[12], [14, 9, 11]])
def test_own_durations_reproduce_the_default_call(env, synthetic, dev, lengths):
    hp, sd, model = env
    x, x_len, spk = inputs(synthetic, hp, lengths, dev)
    B = len(lengths)
    base = model.synthesise(x, x_len, 2, speaker=spk, scale_correction=1.07, length_scale=0.93, debug=True, z=noise(synthetic, hp, B, dev))
    again = model.synthesise(x, x_len, 2, speaker=spk, durations=base["phoneme_durations"], z=noise(synthetic, hp, B, dev))
    assert torch.equal(again["mel_lengths"], base["mel_lengths"]) and torch.equal(again["mel"], base["mel"])
    as_rows = model.synthesise(x, x_len, 2, speaker=spk, durations=[r[:n].tolist() for r, n in zip(base["phoneme_durations"], lengths)],
                               scale_correction=3.0, z=noise(synthetic, hp, B, dev))          # (scale_correction has no say here)
    assert torch.equal(as_rows["mel"], base["mel"])
    as_int = model.synthesise(x, x_len, 2, speaker=spk, durations=base["phoneme_durations"].to(torch.int32), z=noise(synthetic, hp, B, dev))
    assert torch.equal(as_int["mel"], base["mel"])


def test_given_durations_set_the_lengths(env, synthetic, dev):
    hp, sd, model = env
    lengths = [13, 7, 10]
    x, x_len, spk = inputs(synthetic, hp, lengths, dev)
    g = torch.Generator().manual_seed(5)
    d = (torch.rand(3, 13, generator=g) * 9.0).float()
    d[0, 3] = 0.0
    d[1, :2] = 0.0
    d[2, 4] = 2.5                                   # round half to even, as torch.round
    for ls in (1.0, 1.1, 0.5):
        out = model.synthesise(x, x_len, 2, speaker=spk, durations=d.to(dev), length_scale=ls, debug=True)
        mask = (torch.arange(13)[None] < torch.tensor(lengths)[:, None]).float()
        want = torch.round(d * torch.tensor(ls, dtype=torch.float32)).clamp(min=0) * mask
        assert torch.equal(out["phoneme_durations"].cpu(), want)
        assert out["mel_lengths"].tolist() == [max((int(s) + 1) // 2, 1) for s in want.sum(1).tolist()]
        assert out["mel"].shape[2] == max(out["mel_lengths"].tolist()) and torch.isfinite(out["mel"]).all()
    with pytest.raises(ValueError, match="shape"):
        model.synthesise(x, x_len, 2, speaker=spk, durations=d[:, :5].to(dev))
    with pytest.raises(ValueError, match="one row per utterance"):
        model.synthesise(x, x_len, 2, speaker=spk, durations=[None, None])


def test_batcher_mixes_given_and_predicted_durations(env, synthetic, dev):
    hp, sd, model = env
    bt = sub("batcher")
    lengths = [15, 11]
    ids = [synthetic.make_inputs(hp, 1, n, seed=90 + i)[0][0].tolist() for i, n in enumerate(lengths)]
    given = [float(3 + (i * 5) % 7) for i in range(lengths[0])]
    with bt.FrameBudgetBatcher(model, max_batch=4, max_tokens=1024, max_wait_ms=100.0) as q:
        futs = [q.submit(ids[0], speaker=1, solver="midpoint", n_timesteps=2, durations=given, length_scale=1.2),
                q.submit(ids[1], speaker=2, solver="midpoint", n_timesteps=2, scale_correction=1.05)]
        with pytest.raises(ValueError, match="durations"):
            q.submit(ids[1], durations=[1.0])
        res = [f.result(timeout=120) for f in futs]
        assert q.batches_run == 1
    solo = [model.synthesise(torch.tensor([ids[0]], device=dev), torch.tensor([lengths[0]], device=dev), 2, speaker=1,
                             durations=torch.tensor([given], device=dev), length_scale=1.2),
            model.synthesise(torch.tensor([ids[1]], device=dev), torch.tensor([lengths[1]], device=dev), 2, speaker=2,
                             scale_correction=1.05)]
    assert res[0]["mel_length"] == (int(torch.round(torch.tensor(given) * torch.tensor(1.2)).sum()) + 1) // 2
    for r, s in zip(res, solo):
        assert r["mel_length"] == int(s["mel_lengths"][0])
        assert (r["mel"][None] - s["mel"][:, :, :r["mel_length"]]).abs().max().item() < 5e-5


def test_align_on_the_models_own_mu_x(env, synthetic, dev):
    hp, sd, model = env
    lengths = [17, 9, 13]
    x, x_len, spk = inputs(synthetic, hp, lengths, dev, seed=77)
    dbg = model.synthesise(x, x_len, 2, speaker=spk, debug=True)
    mu = dbg["mu_x"].cpu().numpy()
    rng = np.random.default_rng(9)
    d = np.zeros((3, 17), dtype=np.int32)
    for b, n in enumerate(lengths):
        d[b, :n] = rng.integers(1, 13, size=n)
    yl = d.sum(1).tolist()
    y = np.zeros((3, hp.n_feats, max(yl)), dtype=np.float32)
    for b, n in enumerate(lengths):
        y[b, :, :yl[b]] = R.expand(mu[b, :, :n], d[b, :n]) + (0.05 * rng.standard_normal((hp.n_feats, yl[b]))).astype(np.float32)
    out = model.align(x, x_len, mel_fine=torch.from_numpy(y).to(dev), mel_fine_lengths=torch.tensor(yl, device=dev), speaker=spk,
                      return_path=True)
    lp = model.hip.mas_logprior(dbg["mu_x"], torch.from_numpy(y).to(dev), x_len, torch.tensor(yl, device=dev)).cpu().numpy()
    check_against_restatement(lp, lengths, yl, out["durations"].cpu().numpy(), out["score"].cpu().numpy(), out["path"].cpu().numpy())
    assert torch.equal(out["predicted_durations"], dbg["raw_phoneme_durations"])
    want = out["durations"].sum(1).float() / out["predicted_durations"].sum(1)
    assert torch.equal(out["scale_correction"], want) and out["scale_correction"].shape == (3,)
    assert out["mel_fine_lengths"].tolist() == yl
    # fewer frames than tokens: the device refuses that utterance and align names it
    with pytest.raises(ValueError, match="utterance 1 "):
        model.align(x, x_len, mel_fine=torch.from_numpy(y).to(dev), mel_fine_lengths=torch.tensor([yl[0], 8, yl[2]], device=dev), speaker=spk)
    with pytest.raises(ValueError, match="either"):
        model.align(x, x_len)


def test_align_from_audio_and_retime(env, synthetic, dev):
    hp, sd, model = env
    mel = sub("mel")
    clips = [E.synthetic_clip(n, 40 + i, "voiced") for i, n in enumerate([9000, 6100, 12345])]
    frames = [c.numel() // 128 + 1 for c in clips]
    lengths = [21, 12, 30]
    x, x_len, spk = inputs(synthetic, hp, lengths, dev, seed=55)
    out = model.align(x, x_len, audio=clips, speaker=spk)
    assert out["mel_fine_lengths"].tolist() == frames
    dur = out["durations"]
    assert dur.dtype == torch.int32 and dur.sum(1).tolist() == frames
    for b, n in enumerate(lengths):
        assert (dur[b, :n] >= 1).all() and (dur[b, n:] == 0).all()
    # device clips, a padded [B, L] tensor with lengths, and a given mel: all the same alignment; and a second call too
    on_dev = model.align(x, x_len, audio=[c.to(dev) for c in clips], speaker=spk)
    padded = torch.zeros(3, max(c.numel() for c in clips))
    for b, c in enumerate(clips):
        padded[b, :c.numel()] = c
    as_tensor = model.align(x, x_len, audio=padded.to(dev), audio_lengths=[c.numel() for c in clips], speaker=spk)
    wave = torch.zeros(3, (padded.shape[1] + 3) // 4 * 4, device=dev)
    wave[:, :padded.shape[1]] = padded.to(dev)
    m, ml = mel.extract(wave, [c.numel() for c in clips], 128, model._rt.mel_mean, model._rt.mel_std, n_mels=hp.n_feats)
    from_mel = model.align(x, x_len, mel_fine=m, mel_fine_lengths=ml, speaker=spk)
    for other in (on_dev, as_tensor, from_mel, model.align(x, x_len, audio=clips, speaker=spk)):
        assert torch.equal(other["durations"], dur) and torch.equal(other["score"], out["score"])
        assert torch.equal(other["scale_correction"], out["scale_correction"])
    # the loop the feature exists for: speak the same text with the recording's timing
    re = model.synthesise(x, x_len, 2, speaker=(spk + 1) % 3, durations=dur)
    assert re["mel_lengths"].tolist() == [(f + 1) // 2 for f in frames]
    assert re["mel"].shape[2] == max(re["mel_lengths"].tolist()) and torch.isfinite(re["mel"]).all()

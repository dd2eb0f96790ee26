"""GPU parity of the synthesis path (HIP library behind the reference's Python API) against
(a) the golden vectors recorded from the reference's own code and (b) the CPU oracle on the same seeded inputs.

Tolerance: 1e-3 max-abs on the denormalised mel (BASELINE.json north_star, fp32); intermediate tensors tighter."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN, sub

pytestmark = pytest.mark.gpu
MEL_TOL = 1e-3


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


def make_model(hp, sd, dev):
    inf = sub("inference")
    m = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def tiny(hparams, synthetic, dev):
    hp = hparams.tiny(n_spks=2)
    sd = synthetic.make_state_dict(hp, seed=7)
    return hp, sd, make_model(hp, sd, dev)


@pytest.fixture(scope="module")
def prod(hparams, synthetic, dev):
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    return hp, sd, make_model(hp, sd, dev)


def maxabs(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


# ------------------------------------------------------------------------------------------------ components, tiny
def test_tiny_encoder_vs_golden(tiny, dev):
    hp, sd, model = tiny
    g = np.load(GOLDEN / "tiny_encoder.npz")
    spk = _t(g["speakers"]).to(dev)
    e_enc = model.hip.speaker_embedding(0, spk)
    e_dur = model.hip.speaker_embedding(1, spk)
    assert torch.equal(e_enc.cpu(), sd["speaker_embeddings_enc.weight"][spk.cpu()])
    mu, logw, mask = model.encoder(_t(g["x"]).to(dev), _t(g["x_lengths"]).to(dev), e_enc, e_dur)
    assert torch.equal(mask.cpu(), _t(g["x_mask"]))
    assert maxabs(mu, _t(g["mu_x"])) < 2e-5
    assert maxabs(logw, _t(g["logw"])) < 2e-5


def test_tiny_decoder_vs_golden(tiny, synthetic, oracle, dev):
    hp, sd, model = tiny
    g = np.load(GOLDEN / "tiny_decoder.npz")
    T, nf = int(g["T"]), hp.n_feats
    x = _t(synthetic.portable_normal(11, 1, 2 * nf * T).reshape(2, nf, T))
    mu = _t(synthetic.portable_normal(11, 2, 2 * nf * T).reshape(2, nf, T))
    mask = oracle.sequence_mask(_t(g["lengths"]), T).unsqueeze(1).float()
    for tv in (0.0, 0.37):
        v = model.decoder.estimator(x.to(dev), mask.to(dev), mu.to(dev), torch.tensor(tv))
        assert v.shape == (2, nf, T)
        assert maxabs(v, _t(g[f"v_t{tv}"])) < 5e-5


@pytest.mark.parametrize("solver,steps", [("euler", 2), ("midpoint", 2), ("rk4", 1)])
def test_tiny_synthesise_vs_golden(tiny, synthetic, dev, solver, steps):
    hp, sd, model = tiny
    g = np.load(GOLDEN / "tiny_synth.npz")
    x, x_len, spk = synthetic.make_inputs(hp, 2, 12, seed=1234, lengths=[12, 9])
    model.decoder.solver = solver
    for b in range(2):
        n = int(x_len[b])
        ref = _t(g[f"mel_{solver}{steps}_b{b}"])
        out = model.synthesise(x[b:b + 1, :n].to(dev), x_len[b:b + 1].to(dev), steps, speaker=int(spk[b]), scale_correction=1.03,
                               length_scale=0.9, debug=True, z=_noise_for(model, synthetic, hp, n, dev))
        assert out["mel"].shape == ref.shape
        assert torch.equal(out["phoneme_durations"].cpu(), _t(g[f"dur_b{b}"]))
        assert maxabs(out["mel"], ref) < MEL_TOL


def _noise_for(model, synthetic, hp, n_tokens, dev, frames_per_token=5, batch=1):
    """CPU seed-42 stream for the decoder length the duration recipe produces: T_pad = roundup_even(5 * Tx)."""
    lf = frames_per_token * n_tokens
    t_pad = (lf + 1) // 2 * 2
    return synthetic.cpu_noise((batch, hp.n_feats, t_pad)).to(dev)


def test_tiny_voice_mix_vs_golden(tiny, synthetic, dev):
    hp, sd, model = tiny
    g = np.load(GOLDEN / "tiny_synth.npz")
    x, x_len, _ = synthetic.make_inputs(hp, 2, 12, seed=1234, lengths=[12, 9])
    model.decoder.solver = "euler"
    out = model.synthesise(x[:1].to(dev), x_len[:1].to(dev), 2, voice_mix=[(0, 0.7), (1, 0.3)], z=_noise_for(model, synthetic, hp, 12, dev))
    assert maxabs(out["mel"], _t(g["mel_mix"])) < MEL_TOL


def test_tiny_batched_ragged_vs_oracle(tiny, synthetic, oracle, dev):
    """B=2 with different lengths and speakers in ONE call (the batching extension) against the oracle."""
    hp, sd, model = tiny
    x, x_len, spk = synthetic.make_inputs(hp, 2, 12, seed=99, lengths=[12, 7])
    model.decoder.solver = "midpoint"
    with torch.inference_mode():
        ref = oracle.synthesise(sd, hp, x, x_len, 3, speaker=spk, solver="midpoint")
    z = synthetic.cpu_noise((2, hp.n_feats, ref["t_pad"])).to(dev)
    out = model.synthesise(x.to(dev), x_len.to(dev), 3, speaker=spk.to(dev), debug=True, z=z)
    assert torch.equal(out["mel_lengths"].cpu(), ref["mel_lengths"])
    assert maxabs(out["mu_y"], ref["mu_y"]) < 2e-5
    assert maxabs(out["mel"], ref["mel"]) < MEL_TOL


# ------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("lengths", [[1], [2, 1], [3, 12, 1]])
def test_tiny_minimal_lengths_vs_oracle(tiny, synthetic, oracle, dev, lengths):
    """One-token utterances: T_pad = 6 (3 frames at the coarse level), ragged against a full-length neighbour."""
    hp, sd, model = tiny
    B, Tx = len(lengths), max(lengths)
    x, x_len, spk = synthetic.make_inputs(hp, B, Tx, seed=5, lengths=lengths)
    model.decoder.solver = "euler"
    with torch.inference_mode():
        ref = oracle.synthesise(sd, hp, x, x_len, 2, speaker=spk, solver="euler")
    z = synthetic.cpu_noise((B, hp.n_feats, ref["t_pad"])).to(dev)
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), debug=True, z=z)
    assert out["mel"].shape == ref["mel"].shape
    assert torch.equal(out["mel_lengths"].cpu(), ref["mel_lengths"])
    assert maxabs(out["mel"], ref["mel"]) < MEL_TOL


def test_long_utterance_runs_and_matches_oracle_prefix_properties(prod, synthetic, dev):
    """Tx = 1500 tokens -> T_pad = 7500 decoder frames (the server's input cap gives <= ~3000 tokens): finite, deterministic,
    right shape.  (An oracle run at this length takes minutes of CPU; parity at length is covered by the 640-frame goldens.)"""
    hp, sd, model = prod
    x, x_len, _ = synthetic.make_inputs(hp, 1, 1500, seed=9)
    model.decoder.solver = "euler"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0)["mel"]
    assert out.shape == (1, 100, 3750) and torch.isfinite(out).all()
    assert torch.equal(out, model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0)["mel"])
    with pytest.raises(AssertionError):
        model.encoder(torch.zeros(1, 4001, dtype=torch.long, device=dev), torch.tensor([4001], device=dev),
                      torch.zeros(1, 96, device=dev), torch.zeros(1, 96, device=dev))   # reference RoPE cache limit


# ------------------------------------------------------------------------------------------------ glue kernels
def test_durations_and_alignment_vs_oracle(oracle, dev):
    """Ragged integer durations incl. zeros beyond x_len, odd total lengths, scale factors: bit-exact integer work,
    and the gather-based mu upsample+pool against the reference's one-hot matmul + avg_pool1d."""
    hipmod = sub("_hip")
    hp = sub("hparams").tiny()
    h = hipmod.HipModel(hp)   # durations/align need no weights
    g = torch.Generator().manual_seed(5)
    B, Tx, nf = 3, 37, 20
    d_int = torch.randint(1, 9, (B, Tx), generator=g).float()
    logw = torch.log(d_int + 2.0).unsqueeze(1)
    x_len = torch.tensor([37, 20, 1])
    x_mask = oracle.sequence_mask(x_len, Tx).unsqueeze(1).float()
    mu_x = torch.randn(B, nf, Tx, generator=g) * x_mask
    for sc, ls in ((1.0, 1.0), (1.08, 0.9), (1.03, 2.0)):
        ref_d = oracle.durations_from_logw(logw, x_mask, sc, ls)
        dur, cum, yfl = h.durations(logw.to(dev), x_mask.to(dev), sc, ls)
        assert torch.equal(dur.cpu(), ref_d)
        assert torch.equal(cum.cpu().long(), torch.cumsum(ref_d.long(), 1))
        mu_y_ref, y_mask_ref, y_len_ref, y_max, t_pad = oracle.align_and_pool(mu_x, ref_d, x_mask)
        mu_y, y_mask, y_len = h.align_pool(mu_x.to(dev), cum, yfl, t_pad)
        assert torch.equal(y_len.cpu(), y_len_ref) and torch.equal(y_mask.cpu(), y_mask_ref)
        assert maxabs(mu_y, mu_y_ref) < 1e-6


# ------------------------------------------------------------------------------------------------ prod shapes
def test_prod_single_utterance_vs_golden(prod, synthetic, dev):
    hp, sd, model = prod
    g = np.load(GOLDEN / "prod_synth.npz")
    x, x_len, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    z = synthetic.cpu_noise((1, 100, 640)).to(dev)
    model.decoder.solver = "euler"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, debug=True, z=z)
    assert out["mel"].shape == (1, 100, 320)
    assert maxabs(out["logw"], _t(g["logw"])) < 2e-5
    assert maxabs(out["mu_y"], _t(g["mu_y"])) < 2e-5
    assert maxabs(out["mel"], _t(g["mel_euler2"])) < MEL_TOL
    # one evaluation of the velocity field through the estimator API
    mu_y = _t(g["mu_y"]).to(dev)
    v = model.decoder.estimator(mu_y + z, out["y_mask"], mu_y, torch.tensor(0.5))
    assert maxabs(v, _t(g["v_t0.5"])) < 1e-4
    out10 = model.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)
    assert maxabs(out10["mel"], _t(g["mel_euler10"])) < MEL_TOL
    model.decoder.solver = "midpoint"
    out4 = model.synthesise(x.to(dev), x_len.to(dev), 4, speaker=0, z=z)
    assert maxabs(out4["mel"], _t(g["mel_midpoint4"])) < MEL_TOL


def test_prod_fp32_operand_path_vs_golden(prod, synthetic, dev, monkeypatch):
    """MTTS_P16=0 (read when the context is created) keeps activations in fp32 between kernels (gemm_f32.hip splits them in
    its loop): same golden, and within rounding of the default P16 flow."""
    hp, sd, model = prod
    g = np.load(GOLDEN / "prod_synth.npz")
    x, x_len, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    z = synthetic.cpu_noise((1, 100, 640)).to(dev)
    monkeypatch.setenv("MTTS_P16", "0")
    plain = make_model(hp, sd, dev)
    plain.decoder.solver = "euler"
    out = plain.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z)
    monkeypatch.delenv("MTTS_P16")
    assert maxabs(out["mel"], _t(g["mel_euler2"])) < MEL_TOL
    model.decoder.solver = "euler"
    ref = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z)
    assert maxabs(out["mel"], ref["mel"]) < 2e-4


@pytest.mark.parametrize("qb,ch", [("64", "128"), ("32", "128"), ("48", "256")])
def test_prod_chain_launch_vs_golden(prod, synthetic, dev, monkeypatch, qb, ch):
    """The transformer blocks' row-local part as ONE launch (csrc/tblock_chain.hip: out-projection, FeedForward, the next block's
    q|k|v).  The library takes it from MTTS_CHAIN_MIN_ROWS estimator rows on (large batches); forced here on one utterance: same
    goldens as the four-launch path, and within rounding of it; every workgroup shape."""
    hp, sd, model = prod
    g = np.load(GOLDEN / "prod_synth.npz")
    x, x_len, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    z = synthetic.cpu_noise((1, 100, 640)).to(dev)
    for k, v in (("MTTS_CHAIN_MIN_ROWS", "0"), ("MTTS_CHAIN_QB", qb), ("MTTS_CHAIN_CH", ch)):
        monkeypatch.setenv(k, v)
    fused = make_model(hp, sd, dev)
    fused.decoder.solver = "euler"
    out = fused.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z, debug=True)
    assert not bool(fused.hip.range_flags().any().item())
    for k in ("MTTS_CHAIN_MIN_ROWS", "MTTS_CHAIN_QB", "MTTS_CHAIN_CH"):
        monkeypatch.delenv(k)
    assert maxabs(out["mel"], _t(g["mel_euler2"])) < MEL_TOL
    mu_y = _t(g["mu_y"]).to(dev)
    v = fused.decoder.estimator(mu_y + z, out["y_mask"], mu_y, torch.tensor(0.5))
    assert maxabs(v, _t(g["v_t0.5"])) < 1e-4
    out10 = fused.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)
    assert maxabs(out10["mel"], _t(g["mel_euler10"])) < MEL_TOL
    model.decoder.solver = "euler"
    ref = model.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)       # one utterance: below the threshold, four launches
    assert maxabs(out10["mel"], ref["mel"]) < 2e-4


def test_chain_launch_ragged_batch_and_launch_count(hparams, synthetic, dev, monkeypatch):
    """Ragged production-width batch through the chain launch against the recorded reference batch, and the launch count per
    estimator evaluation: 12 blocks x (attention + chain) + 6 first q|k|v projections instead of 12 x 5."""
    hp = hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    monkeypatch.setenv("MTTS_CHAIN_MIN_ROWS", "0")
    fused = make_model(hp, sd, dev)
    fused.hip
    monkeypatch.setenv("MTTS_CHAIN", "0")
    plain = make_model(hp, sd, dev)
    plain.hip
    monkeypatch.delenv("MTTS_CHAIN")
    monkeypatch.delenv("MTTS_CHAIN_MIN_ROWS")
    g = np.load(GOLDEN / "prod_batch.npz")
    x, x_len, spk = synthetic.make_inputs(hp, 3, 128, seed=1234, lengths=[128, 100, 77])
    z = synthetic.cpu_noise((3, 100, 640)).to(dev)
    counts = {}
    for name, m in (("fused", fused), ("plain", plain)):
        m.decoder.solver = "euler"
        m.decoder.graph_mode = "0"                        # (the per-launch event pass does not run under graph capture)
        m.hip.prof_enable(True)
        m.hip.prof_reset()
        out = m.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), z=z)
        torch.cuda.synchronize()
        counts[name] = len(m.hip.prof_records())
        m.hip.prof_enable(False)
        assert maxabs(out["mel"], _t(g["mel"])) < MEL_TOL, name
    # two evaluations: each saves 12 * 3 - 6 launches (the chain replaces out-projection, FF1, FF2 and, for 6 blocks, q|k|v)
    assert counts["plain"] - counts["fused"] == 2 * 30, counts


def test_full_batch_estimator_is_bitwise_repeatable_over_many_launches(prod, dev):
    """B=32, T=320 (BASELINE configs[1]'s estimator shape; the chain launch runs at the fine level): 300 evaluations of the same
    inputs are bitwise equal.  Round 3's chain kernel failed this about once in 250 launches -- the compiler had copied weight-ring
    registers ahead of their inline-asm loads, which only shows when the weight stream misses the L2s (the build-time guard is
    tests/test_isa_guard.py; this is the run-time one)."""
    hp, sd, model = prod
    B, T = 32, 320
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, hp.n_feats, T, generator=g).to(dev)
    mu = torch.randn(B, hp.n_feats, T, generator=g).to(dev)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    mask = (torch.arange(T)[None, :] < lens[:, None]).float()[:, None, :].to(dev)
    first = model.hip.decoder_forward(x, mask, mu, 0.37).clone()
    assert torch.isfinite(first).all()
    differing = 0
    for _ in range(300):
        differing += int(not torch.equal(model.hip.decoder_forward(x, mask, mu, 0.37), first))
    assert differing == 0, f"{differing} of 300 evaluations differ from the first"


def test_prod_fp16_mode_is_opt_in_and_looser(prod, synthetic, dev, monkeypatch):
    """MTTS_GEMM_TERMS=1 (read when the context is created): the estimator multiplies only the fp16 head planes -- fp16 operand
    precision with fp32 accumulation, the arithmetic torch.autocast gives the reference on a GPU (reference inference.py:238).
    Opt-in: an order of magnitude looser than the default, so it must stay within 5e-2 of the fp32 golden (|mel| ~ 40) and the
    default must not be it."""
    hp, sd, model = prod
    g = np.load(GOLDEN / "prod_synth.npz")
    x, x_len, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    z = synthetic.cpu_noise((1, 100, 640)).to(dev)
    monkeypatch.setenv("MTTS_GEMM_TERMS", "1")
    fast = make_model(hp, sd, dev)
    fast.decoder.solver = "euler"
    out = fast.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)
    assert fast.hip.gemm_terms() == 1
    monkeypatch.delenv("MTTS_GEMM_TERMS")
    err = maxabs(out["mel"], _t(g["mel_euler10"]))
    assert MEL_TOL < err < 5e-2, err
    assert model.hip.gemm_terms() == 2


def test_prod_rk4_and_voice_mix_vs_oracle(hparams, synthetic, oracle, dev):
    """The solver and speaker paths the goldens do not cover at production shapes (P16 estimator): rk4 (3/8 rule, four
    evaluations per step through ode_combine) and a two-voice mix, against the oracle run here on the same inputs."""
    hp = hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    model = make_model(hp, sd, dev)
    x, x_len, _ = synthetic.make_inputs(hp, 1, 24, seed=77)
    z = synthetic.cpu_noise((1, 100, 120)).to(dev)
    mix = [(0, 0.25), (2, 0.75)]
    model.decoder.solver = "rk4"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, voice_mix=mix, z=z)
    ref = oracle.synthesise(sd, hp, x, x_len, 2, voice_mix=mix, solver="rk4", z=z.cpu())
    assert out["mel"].shape == ref["mel"].shape
    assert maxabs(out["mel"], ref["mel"]) < MEL_TOL


def test_prod_ragged_batch_vs_golden(hparams, synthetic, dev):
    hp = hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    model = make_model(hp, sd, dev)
    g = np.load(GOLDEN / "prod_batch.npz")
    x, x_len, spk = synthetic.make_inputs(hp, 3, 128, seed=1234, lengths=[128, 100, 77])
    z = synthetic.cpu_noise((3, 100, 640)).to(dev)
    model.decoder.solver = "euler"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), debug=True, z=z)
    assert torch.equal(out["mel_lengths"].cpu(), _t(g["y_lengths"]))
    assert maxabs(out["mel"], _t(g["mel"])) < MEL_TOL


@pytest.mark.parametrize("which,lengths,solver,steps", [("tiny", [12, 9, 5, 1], "midpoint", 2), ("prod", [128, 100, 77], "euler", 2)])
def test_per_request_padding_equals_batch_of_one(which, lengths, solver, steps, tiny, hparams, synthetic, dev):
    """per_request_padding: every utterance of a ragged batch gets the mel a batch-of-one call gives it (own padded length
    for GroupNorm statistics, attention keys and the seed-42 noise shape), unlike the reference-faithful default, whose
    result depends on the longest utterance in the call."""
    if which == "tiny":
        hp, sd, model = tiny
    else:
        hp = hparams.prod_v20(n_spks=3)
        sd = synthetic.make_state_dict(hp, seed=7)
        model = make_model(hp, sd, dev)
    B = len(lengths)
    x, x_len, spk = synthetic.make_inputs(hp, B, max(lengths), seed=99, lengths=lengths)
    model.decoder.solver = solver
    batched = model.synthesise(x.to(dev), x_len.to(dev), steps, speaker=spk.to(dev), per_request_padding=True)
    default = model.synthesise(x.to(dev), x_len.to(dev), steps, speaker=spk.to(dev))
    worst_default = 0.0
    for b, n in enumerate(lengths):
        alone = model.synthesise(x[b:b + 1, :n].to(dev), x_len[b:b + 1].to(dev), steps, speaker=spk[b:b + 1].to(dev))
        t = int(alone["mel_lengths"][0])
        assert int(batched["mel_lengths"][b]) == t
        # same arithmetic; only the summation order differs where the two grids pick different tile / MFMA shapes
        assert maxabs(batched["mel"][b, :, :t], alone["mel"][0, :, :t]) < 5e-5, f"utterance {b}"
        worst_default = max(worst_default, maxabs(default["mel"][b, :, :t], alone["mel"][0, :, :t]))
    assert worst_default > 1e-3        # the reference-faithful batch really does differ for the shorter utterances


@pytest.mark.parametrize("channels,n_blocks,heads", [((128, 128), 1, 2), ((256, 256), 2, 3), ((128, 256), 1, 2), ((96, 128), 1, 2)])
def test_small_p16_decoders_vs_oracle(channels, n_blocks, heads, hparams, synthetic, oracle, dev):
    """Narrow estimators that still qualify for the P16 flow (widths multiples of 64, 64-wide heads): groups of 16 / 32
    channels (GroupNorm statistics from the separate pass / from the conv epilogue with two groups per 64 columns), single-tile
    GEMMs, unequal level widths -- ragged batch, midpoint, against the oracle run here.  (96, 128) does not qualify (a width
    that is not a multiple of 64): the whole estimator runs on fp32 rows, with the row_stats kernel at width 96."""
    import dataclasses
    hp = hparams.tiny(n_spks=2)
    hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64,
                                                             n_blocks=n_blocks, num_mid_blocks=1, num_heads=heads))
    sd = synthetic.make_state_dict(hp, seed=21)
    model = make_model(hp, sd, dev)
    lengths = [14, 9, 3]
    x, x_len, spk = synthetic.make_inputs(hp, 3, max(lengths), seed=8, lengths=lengths)
    t_pad = 2 * ((5 * max(lengths) + 1) // 2)
    z = synthetic.cpu_noise((3, hp.n_feats, t_pad)).to(dev)
    model.decoder.solver = "midpoint"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), z=z)
    ref = oracle.synthesise(sd, hp, x, x_len, 2, speaker=spk, solver="midpoint", z=z.cpu())
    assert torch.equal(out["mel_lengths"].cpu(), ref["mel_lengths"])
    assert maxabs(out["mel"], ref["mel"]) < MEL_TOL


@pytest.mark.parametrize("channels,n_blocks,heads", [((128, 128), 2, 2), ((256, 256), 2, 3), ((128, 256), 1, 2)])
def test_small_p16_decoders_chain_launch_vs_oracle(channels, n_blocks, heads, hparams, synthetic, oracle, dev, monkeypatch):
    """The chain launch on the narrow estimators (one / two 16-channel tiles per wave, attention narrower than the stream, a
    q|k|v width that leaves the last pass partly empty), ragged, midpoint, against the oracle run here."""
    import dataclasses
    hp = hparams.tiny(n_spks=2)
    hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64,
                                                             n_blocks=n_blocks, num_mid_blocks=1, num_heads=heads))
    sd = synthetic.make_state_dict(hp, seed=21)
    monkeypatch.setenv("MTTS_CHAIN_MIN_ROWS", "0")
    model = make_model(hp, sd, dev)
    model.hip
    monkeypatch.delenv("MTTS_CHAIN_MIN_ROWS")
    lengths = [14, 9, 3]
    x, x_len, spk = synthetic.make_inputs(hp, 3, max(lengths), seed=8, lengths=lengths)
    t_pad = 2 * ((5 * max(lengths) + 1) // 2)
    z = synthetic.cpu_noise((3, hp.n_feats, t_pad)).to(dev)
    model.decoder.solver = "midpoint"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), z=z)
    ref = oracle.synthesise(sd, hp, x, x_len, 2, speaker=spk, solver="midpoint", z=z.cpu())
    assert torch.equal(out["mel_lengths"].cpu(), ref["mel_lengths"])
    assert maxabs(out["mel"], ref["mel"]) < MEL_TOL


@pytest.mark.parametrize("lengths", [[27], [13, 9], [31, 30, 29, 5, 1]])
def test_prod_odd_lengths_p16_vs_fp32_operand_path(lengths, prod, synthetic, dev, monkeypatch):
    """Padded lengths that are not multiples of the wave-tile height (T = 136, 66, 156: the GroupNorm statistics fall back from
    the conv epilogue to the separate pass, tail tiles are partly empty): the P16 flow must agree with the fp32-operand flow
    (MTTS_P16=0, independent kernels for every GEMM / attention / GroupNorm step) to rounding."""
    hp, sd, model = prod
    B = len(lengths)
    x, x_len, _ = synthetic.make_inputs(hp, B, max(lengths), seed=31, lengths=lengths)
    monkeypatch.setenv("MTTS_P16", "0")
    plain = make_model(hp, sd, dev)
    plain.decoder.solver = "euler"
    ref = plain.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0)
    monkeypatch.delenv("MTTS_P16")
    model.decoder.solver = "euler"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0)
    assert torch.equal(out["mel_lengths"], ref["mel_lengths"])
    assert torch.isfinite(out["mel"]).all()
    assert maxabs(out["mel"], ref["mel"]) < 2e-4


def test_config2_batch32_properties(prod, synthetic, oracle, dev):
    """BASELINE config #2 (B=32, Tx=128, euler/10) at full size: size-independent checks.
    All utterances of a batch are independent (per-sample norms and attention), so row b of the batched result must
    equal the same utterance synthesised alone with its slice of the noise; and the output must be deterministic."""
    hp, sd, model = prod
    x, x_len, _ = synthetic.make_inputs(hp, 32, 128, seed=1234)
    z = synthetic.cpu_noise((32, 100, 640)).to(dev)
    model.decoder.solver = "euler"
    out = model.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)["mel"]
    assert out.shape == (32, 100, 320) and torch.isfinite(out).all()
    again = model.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)["mel"]
    assert torch.equal(out, again)
    for b in (0, 17, 31):
        solo = model.synthesise(x[b:b + 1].to(dev), x_len[b:b + 1].to(dev), 10, speaker=0, z=z[b:b + 1])["mel"]
        assert maxabs(out[b:b + 1], solo) < 1e-4
    # rows other than the golden one against the oracle run here on the same ids and noise slice (utterances are independent)
    for b in (7, 19):
        with torch.inference_mode():
            ref = oracle.synthesise(sd, hp, x[b:b + 1], x_len[b:b + 1], 10, speaker=0, solver="euler", z=z[b:b + 1].cpu())
        assert maxabs(out[b:b + 1], ref["mel"]) < MEL_TOL, b
    g = np.load(GOLDEN / "prod_synth.npz")   # utterance 0 of the batch is the golden single utterance
    x1, _, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    if torch.equal(x1, x[:1]):
        assert maxabs(out[:1], _t(g["mel_euler10"])) < MEL_TOL


# ------------------------------------------------------------------------------------------------ folded padding
def _synth_both(model, x, x_len, steps, dev, align, **kw):
    """The same call on folded padding (rows per utterance from `align`) and on all T_pad reference frames."""
    dec = model.decoder
    keep = (dec.fold_padding, dec.fold_align)
    try:
        dec.fold_padding, dec.fold_align = True, align
        folded = model.synthesise(x.to(dev), x_len.to(dev), steps, **kw)
        dec.fold_padding = False
        full = model.synthesise(x.to(dev), x_len.to(dev), steps, **kw)
    finally:
        dec.fold_padding, dec.fold_align = keep
    return folded, full


@pytest.mark.parametrize("align", [1, 3, 8])
@pytest.mark.parametrize("lengths,solver,steps", [([12, 9], "euler", 2), ([12], "midpoint", 2), ([3, 12, 1], "rk4", 1), ([2, 1], "euler", 2),
                                                  ([1], "euler", 1), ([11, 12, 12, 5, 7], "midpoint", 3)])
def test_tiny_folded_padding_equals_full_padding(tiny, synthetic, oracle, dev, lengths, solver, steps, align):
    """include/mtts.h mtts_cfm_solve_folded on the tiny estimator (fp32-operand kernels, separate GroupNorm passes): valid rows
    + one row for all padded frames must reproduce the run over every reference frame -- incl. one-frame utterances (no padded
    frame at the coarse level), ragged batches (per-utterance multiplicities) and row counts that are not tile multiples -- and
    the oracle."""
    hp, sd, model = tiny
    B = len(lengths)
    x, x_len, spk = synthetic.make_inputs(hp, B, max(lengths), seed=41, lengths=lengths)
    model.decoder.solver = solver
    z = lambda t_pad: synthetic.cpu_noise((B, hp.n_feats, t_pad)).to(dev)
    folded, full = _synth_both(model, x, x_len, steps, dev, align, speaker=spk.to(dev), z=z)
    assert folded["mel"].shape == full["mel"].shape
    assert maxabs(folded["mel"], full["mel"]) < 5e-5
    with torch.inference_mode():
        ref = oracle.synthesise(sd, hp, x, x_len, steps, speaker=spk, solver=solver)
    assert maxabs(folded["mel"], ref["mel"]) < MEL_TOL


def test_folding_is_what_synthesise_runs_at_prod_shapes(prod, synthetic, dev):
    """The default plan at BASELINE config #2's shape: 320 valid of 640 frames -> 322 rows per utterance (160 + 1 at the
    coarse level, doubled); the golden tests above therefore already exercise the folded estimator.  Here:
    folded == unfolded at production width (P16 kernels), ragged, with whole wave tiles per utterance (align 32: GroupNorm
    statistics from the conv epilogues, fused ResNet tail) and without (statistics from the separate pass)."""
    hp, sd, model = prod
    assert model.decoder.fold_padding and model.decoder.fold_plan(640, 320) == 322
    assert model.decoder.fold_plan(640, 639) is None and model.decoder.fold_plan(2, 1) is None
    lengths = [128, 100, 77, 128]
    x, x_len, _ = synthetic.make_inputs(hp, 4, 128, seed=1234, lengths=lengths)
    z = synthetic.cpu_noise((4, 100, 640)).to(dev)
    model.decoder.solver = "euler"
    for align in (32, 8, 5):
        folded, full = _synth_both(model, x, x_len, 2, dev, align, speaker=0, z=z)
        assert torch.equal(folded["mel_lengths"], full["mel_lengths"])
        assert maxabs(folded["mel"], full["mel"]) < 1e-4, align


@pytest.mark.parametrize("channels,n_blocks,heads", [((128, 128), 1, 2), ((128, 256), 1, 2)])
def test_small_p16_decoders_folded_vs_full(channels, n_blocks, heads, hparams, synthetic, dev):
    """Narrow P16 estimators (16-channel groups: statistics from the separate pass; unequal level widths) folded vs full."""
    import dataclasses
    hp = hparams.tiny(n_spks=2)
    hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64,
                                                             n_blocks=n_blocks, num_mid_blocks=1, num_heads=heads))
    sd = synthetic.make_state_dict(hp, seed=21)
    model = make_model(hp, sd, dev)
    lengths = [14, 9, 3]
    x, x_len, spk = synthetic.make_inputs(hp, 3, max(lengths), seed=8, lengths=lengths)
    model.decoder.solver = "midpoint"
    for align in (1, 16):
        folded, full = _synth_both(model, x, x_len, 2, dev, align, speaker=spk.to(dev))
        assert maxabs(folded["mel"], full["mel"]) < 5e-5, align


def test_per_request_padding_on_folded_rows(tiny, prod, synthetic, dev):
    """per_request_padding composes with folding: utterance b's reference length is its own T_pad_b (mtts_set_frame_limits),
    the multiplicities follow it."""
    for (hp, sd, model), lengths, align in ((tiny, [12, 9, 5, 1], 1), (prod, [128, 60, 77], 32)):
        x, x_len, spk = synthetic.make_inputs(hp, len(lengths), max(lengths), seed=99, lengths=lengths)
        model.decoder.solver = "euler"
        spk = spk % hp.n_spks
        folded, full = _synth_both(model, x, x_len, 2, dev, align, speaker=spk.to(dev), per_request_padding=True)
        assert maxabs(folded["mel"], full["mel"]) < 1e-4


def test_graph_replay_with_both_chain_forms(prod, synthetic, dev):
    """B = 20, 128 tokens (6440 / 3220 estimator rows: the single-workgroup chain at the full-length level, the PAIR form at the
    half-length level) forced onto a captured HIP graph: the pair launches' flag values are baked into the graph, so every replay
    depends on the flags being zeroed inside it -- replay twice, compare with the direct launches and bit for bit with each other."""
    hp, sd, model = prod
    dec = model.decoder
    keep = dec.graph_mode, dec.solver, dec.graph_max_rows
    x, x_len, _ = synthetic.make_inputs(hp, 20, 128, seed=77)
    z = synthetic.cpu_noise((20, 100, 640)).to(dev)
    try:
        dec.solver = "euler"
        dec.graph_mode = "0"
        direct = model.synthesise(x.to(dev), x_len.to(dev), 3, speaker=0, z=z)["mel"]
        dec.graph_mode = "1"
        dec.graph_max_rows = 1 << 20
        first = model.synthesise(x.to(dev), x_len.to(dev), 3, speaker=0, z=z)["mel"]
        second = model.synthesise(x.to(dev), x_len.to(dev), 3, speaker=0, z=z)["mel"]
        assert torch.equal(first, second)
        assert maxabs(first, direct) < 1e-4
    finally:
        dec.graph_mode, dec.solver, dec.graph_max_rows = keep
        dec._graphs.clear()


# ------------------------------------------------------------------------------------------------ HIP graphs (small batches)
def test_graph_replay_equals_direct_launches(prod, tiny, synthetic, dev):
    """Launch-bound sizes run the ODE solve as one captured HIP graph per (batch, row bucket, solver, steps) (modules.CFM.
    _solve_on_graph): static buffers, the reference's padded length as device data.  Results equal the direct launches (only
    the bucketed row count, hence tile shapes, may differ: rounding level); requests whose lengths share a bucket replay the
    same graph; per-request padding and the reference's batch-wide padding both ride on it."""
    for (hp, sd, model), cases in ((prod, [([40], "euler", 3), ([47], "euler", 3), ([33, 47], "midpoint", 2), ([47, 20], "midpoint", 2)]),
                                   (tiny, [([12, 9, 5], "euler", 2), ([11, 12, 3], "euler", 2)])):
        dec = model.decoder
        keep = dec.graph_mode
        try:
            dec._graphs.clear()
            n_graphs = 0
            for lengths, solver, steps in cases:
                B = len(lengths)
                x, x_len, spk = synthetic.make_inputs(hp, B, max(lengths), seed=61, lengths=lengths)
                spk = spk % hp.n_spks
                dec.solver = solver
                for prp in (False, True):
                    dec.graph_mode = "0"
                    direct = model.synthesise(x.to(dev), x_len.to(dev), steps, speaker=spk.to(dev), per_request_padding=prp)
                    dec.graph_mode = "1"
                    before = dec.graph_replays
                    graphed = model.synthesise(x.to(dev), x_len.to(dev), steps, speaker=spk.to(dev), per_request_padding=prp)
                    assert dec.graph_replays == before + 1
                    assert torch.equal(graphed["mel_lengths"], direct["mel_lengths"])
                    assert graphed["mel"].shape == direct["mel"].shape
                    assert maxabs(graphed["mel"], direct["mel"]) < 5e-5, (lengths, solver, prp)
                    again = model.synthesise(x.to(dev), x_len.to(dev), steps, speaker=spk.to(dev), per_request_padding=prp)
                    assert torch.equal(again["mel"], graphed["mel"])
            # lengths 40 and 47 (and the two ragged pairs) share row buckets: fewer graphs than cases
            assert len(dec._graphs) < len(cases), (len(dec._graphs), len(cases))
        finally:
            dec.graph_mode = keep


def test_graph_cache_follows_weight_reload(hparams, synthetic, dev):
    """A captured graph bakes the packed weights' address into its kernel nodes.  Loading another state dict into a model that
    has already replayed a graph must not replay the old one (round-2 advisor finding): the second synthesis equals a fresh
    model's with the new weights, differs from the first, and the stale graph has left the cache."""
    hp = hparams.tiny(n_spks=2)
    sd_a, sd_b = synthetic.make_state_dict(hp, seed=7), synthetic.make_state_dict(hp, seed=8)
    model = make_model(hp, sd_a, dev)
    dec = model.decoder
    dec.graph_mode = "1"
    x, x_len, spk = synthetic.make_inputs(hp, 1, 12, seed=5, lengths=[12])
    args = (x.to(dev), x_len.to(dev), 2)
    first = model.synthesise(*args, speaker=spk.to(dev))["mel"].clone()
    assert dec.graph_replays == 1 and len(dec._graphs) == 1
    model.load_state_dict(sd_b, strict=True)
    second = model.synthesise(*args, speaker=spk.to(dev))["mel"].clone()
    assert dec.graph_replays == 2 and len(dec._graphs) == 1      # a new capture replaced the stale graph
    fresh = make_model(hp, sd_b, dev)
    fresh.decoder.graph_mode = "0"
    want = fresh.synthesise(*args, speaker=spk.to(dev))["mel"]
    assert maxabs(second, want) < 5e-5
    assert maxabs(second, first) > 1e-3


# ------------------------------------------------------------------------------------------------ 16-bit storage mode (config #3)
def _half_model(hp, sd, dev, monkeypatch, terms=16):
    monkeypatch.setenv("MTTS_GEMM_TERMS", str(terms))
    m = make_model(hp, sd, dev)
    m.hip                                   # the context reads the variable when it is created
    monkeypatch.delenv("MTTS_GEMM_TERMS")
    assert m.hip.gemm_terms() == terms
    return m


def test_half_storage_mode_small_estimators_vs_oracle(hparams, synthetic, oracle, dev, monkeypatch):
    """mtts_set_arithmetic 16 (BASELINE config #3's arithmetic; what torch.autocast gives the reference on its GPU, reference
    inference.py:238): H16 images (one fp16 plane, 2 B/element) between the estimator's kernels, one MFMA per MAC, fp32
    accumulation and statistics.  Narrow P16-capable estimators, ragged, midpoint, folded padding: the text encoder is untouched
    (same integer durations as the oracle), the mel agrees to fp16-operand precision (NOT the 1e-3 bar) and is not the default
    arithmetic's result."""
    import dataclasses
    for channels, heads in (((128, 128), 2), ((128, 256), 2)):
        hp = hparams.tiny(n_spks=2)
        hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64, n_blocks=1,
                                                                 num_mid_blocks=1, num_heads=heads))
        sd = synthetic.make_state_dict(hp, seed=21)
        half = _half_model(hp, sd, dev, monkeypatch)
        full = make_model(hp, sd, dev)
        lengths = [14, 9, 3]
        x, x_len, spk = synthetic.make_inputs(hp, 3, max(lengths), seed=8, lengths=lengths)
        t_pad = 2 * ((5 * max(lengths) + 1) // 2)
        z = synthetic.cpu_noise((3, hp.n_feats, t_pad)).to(dev)
        outs = {}
        for name, m in (("half", half), ("full", full)):
            m.decoder.solver = "midpoint"
            outs[name] = m.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), z=z, debug=True)
        ref = oracle.synthesise(sd, hp, x, x_len, 2, speaker=spk, solver="midpoint", z=z.cpu())
        assert torch.equal(outs["half"]["phoneme_durations"].cpu(), ref["durations"])
        scale = float(ref["mel"].abs().max())
        err = maxabs(outs["half"]["mel"], ref["mel"])
        assert err < 4e-3 * scale, (channels, err, scale)
        assert maxabs(outs["full"]["mel"], ref["mel"]) < MEL_TOL
        assert maxabs(outs["half"]["mel"], outs["full"]["mel"]) > 1e-5        # really another arithmetic


def test_config3_per_rank_shape_half_storage(prod, synthetic, dev, monkeypatch):
    """BASELINE config #3 at its per-rank shape (256 utterances 8-way = B=32 per GPU, Tx=128, euler/10) in the 16-bit storage
    mode: finite, deterministic, rows independent of the batch, durations those of the fp32 path, and the measured mel error
    against the fp32-equivalent path of this library reported (asserted loosely: the mode is outside the 1e-3 bar by design)."""
    hp, sd, model = prod
    half = _half_model(hp, sd, dev, monkeypatch)
    x, x_len, _ = synthetic.make_inputs(hp, 32, 128, seed=1234)
    z = synthetic.cpu_noise((32, 100, 640)).to(dev)
    half.decoder.solver = "euler"
    out = half.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z, debug=True)
    mel = out["mel"]
    assert mel.shape == (32, 100, 320) and torch.isfinite(mel).all()
    assert torch.equal(mel, half.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)["mel"])
    solo = half.synthesise(x[5:6].to(dev), x_len[5:6].to(dev), 10, speaker=0, z=z[5:6])["mel"]
    assert maxabs(mel[5:6], solo) < 2e-2                                     # tile shapes differ with the grid: fp16-level noise
    model.decoder.solver = "euler"
    ref = model.synthesise(x[:4].to(dev), x_len[:4].to(dev), 10, speaker=0, z=z[:4], debug=True)
    assert torch.equal(out["phoneme_durations"][:4], ref["phoneme_durations"])
    err = maxabs(mel[:4], ref["mel"])
    mean_err = float((mel[:4] - ref["mel"]).abs().mean())
    print(f"config #3 arithmetic: mel error vs the fp32-equivalent path max {err:.3e} mean {mean_err:.3e} (|mel| <= {float(ref['mel'].abs().max()):.1f})")
    # bounded by what the REFERENCE's own arithmetic does to its own mel under 16-bit autocast (tests/golden/prod_autocast.npz,
    # recorded from the reference on the utterance-0 inputs: fp16 max 3.7e-2 / mean 6.7e-3), times a small factor for the
    # other utterances of the batch -- not by a free-standing ceiling
    anchor = np.load(GOLDEN / "prod_autocast.npz")["err_fp16"]
    assert 1e-4 < err < 2.0 * anchor[0] and mean_err < 1.5 * anchor[1], (err, mean_err, anchor)


@pytest.mark.parametrize("terms,name", [(16, "fp16"), (17, "bf16")])
def test_half_storage_mode_vs_reference_autocast_anchor(prod, synthetic, dev, monkeypatch, terms, name):
    """The 16-bit storage modes (fp16 planes: terms 16; bfloat16 planes, the dtype BASELINE configs[2] names: terms 17) against
    the reference-derived anchor on the SAME inputs (prod_synth: Tx=128, euler/10, seed-42 noise): the reference's synthesise
    under torch.autocast(that dtype) -- what matcha/inference.py:238 runs -- deviates from its fp32 mel by err = (max, mean);
    the HIP mode (16-bit operands in HBM, one MFMA per MAC, fp32 accumulation, statistics and ODE state) must deviate from the
    same fp32 golden by no more than 1.5x that, and its result must be about as far from the autocast mel as that is from fp32
    (two different roundings of one computation, not a different function)."""
    hp, sd, model = prod
    g = np.load(GOLDEN / "prod_synth.npz")
    a = np.load(GOLDEN / "prod_autocast.npz")
    half = _half_model(hp, sd, dev, monkeypatch, terms)
    x, x_len, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    z = synthetic.cpu_noise((1, 100, 640)).to(dev)
    half.decoder.solver = "euler"
    mel = half.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z)["mel"].cpu()
    gold = _t(g["mel_euler10"])
    err_max, err_mean = maxabs(mel, gold), float((mel - gold).abs().mean())
    ref_max, ref_mean = (float(v) for v in a[f"err_{name}"])
    print(f"{name} storage mode vs fp32 golden: max {err_max:.3e} mean {err_mean:.3e}; reference {name} autocast: max {ref_max:.3e} mean {ref_mean:.3e}")
    assert 1e-4 < err_max <= 1.5 * ref_max, (err_max, ref_max)
    assert err_mean <= 1.5 * ref_mean, (err_mean, ref_mean)
    assert maxabs(mel, _t(a[f"mel_{name}"])) <= 2.5 * ref_max
    assert not bool(half.hip.range_flags().any().item())


# ------------------------------------------------------------------------------------------------ range guard
def test_range_guard_reruns_on_full_range_arithmetic(hparams, synthetic, oracle, dev):
    """The default arithmetic splits operands into fp16 terms and saturates beyond +-65504 (include/mtts.h "range guard").
    Weights scaled so that one FeedForward's hidden layer reaches ~1e5 (first projection x 4e4, second / 4e4: the network's
    function is otherwise ordinary): the sticky device flag must fire, `raise` must raise, `ignore` must produce the saturated
    (wrong) mel, and the default `rerun` must match the oracle on the same weights."""
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    k = "decoder.estimator.mid_blocks.0.1.0.ff.net."
    sd[k + "0.proj.weight"] = sd[k + "0.proj.weight"] * 4e4
    sd[k + "0.proj.bias"] = sd[k + "0.proj.bias"] * 4e4
    sd[k + "0.alpha"] = sd[k + "0.alpha"] - 10.0           # exp(alpha) small: the snake term stays a smooth function of the hidden value
    sd[k + "2.weight"] = sd[k + "2.weight"] / 4e4
    model = make_model(hp, sd, dev)
    x, x_len, _ = synthetic.make_inputs(hp, 1, 16, seed=77)
    z = synthetic.cpu_noise((1, 100, 80)).to(dev)
    model.decoder.solver = "euler"
    with torch.inference_mode():
        ref = oracle.synthesise(sd, hp, x, x_len, 2, speaker=0, solver="euler", z=z.cpu())
    model.range_policy = "ignore"
    bad = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z)
    assert bool(model.hip.range_flags().any().item())
    assert maxabs(bad["mel"], ref["mel"]) > 1e-2
    model.range_policy = "raise"
    with pytest.raises(FloatingPointError):
        model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z)
    model.range_policy = "rerun"
    out = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z)
    assert model.hip.gemm_terms() == 6                      # the runtime switched to the three-term bf16 context
    assert maxabs(out["mel"], ref["mel"]) < MEL_TOL
    again = model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0, z=z)
    assert torch.equal(out["mel"], again["mel"])


def test_range_guard_of_score_on_full_range_arithmetic(hparams, synthetic, dev):
    """``score`` under the three policies on the weights of the test above (the decoder FeedForward scaled by 4e4): its one
    estimator evaluation saturates, so `ignore` leaves the decoder's flag set, `raise` raises, and `rerun` switches the model to
    the three-term bf16 context and returns that run's figures, without the guard's private ``_flags`` entry."""
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    k = "decoder.estimator.mid_blocks.0.1.0.ff.net."
    sd[k + "0.proj.weight"] = sd[k + "0.proj.weight"] * 4e4
    sd[k + "0.proj.bias"] = sd[k + "0.proj.bias"] * 4e4
    sd[k + "0.alpha"] = sd[k + "0.alpha"] - 10.0
    sd[k + "2.weight"] = sd[k + "2.weight"] / 4e4
    model = make_model(hp, sd, dev)
    x, x_len, _ = synthetic.make_inputs(hp, 1, 16, seed=77)
    gen = torch.Generator().manual_seed(5)
    mel = torch.randn(1, hp.n_feats, 40, generator=gen).to(dev)
    mel_fine = torch.randn(1, hp.n_feats, 80, generator=gen).to(dev)
    noise = torch.randn(1, hp.n_feats, 40, generator=gen).to(dev)
    score = lambda: model.score(x.to(dev), x_len.to(dev), mel=mel, mel_fine=mel_fine, speaker=0, t=[0.5], noise=noise)
    model.range_policy = "ignore"
    assert "diff_loss" in score()
    assert bool(model.hip.range_flags()[1].item())
    model.range_policy = "raise"
    with pytest.raises(FloatingPointError):
        score()
    model.range_policy = "rerun"
    out = score()
    assert model.hip.gemm_terms() == 6                      # the runtime switched to the three-term bf16 context
    assert "_flags" not in out
    assert bool(torch.isfinite(out["diff_loss"]).all())
    assert torch.equal(out["diff_loss"], score()["diff_loss"])


def test_range_guard_is_quiet_on_ordinary_weights(prod, synthetic, dev):
    hp, sd, model = prod
    x, x_len, _ = synthetic.make_inputs(hp, 2, 40, seed=3)
    model.decoder.solver = "euler"
    model.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0)
    assert not bool(model.hip.range_flags().any().item()) and model.hip.gemm_terms() == 2 and not model.hip.weights_saturate()


# ------------------------------------------------------------------------------------------------ duration predictor live
@pytest.mark.parametrize("tag,which", [("dp_tiny", "tiny"), ("dp_prod", "prod")])
def test_duration_predictor_live_vs_golden(tag, which, hparams, synthetic, dev):
    """duration_recipe=False fixtures recorded from the reference (tests/golden/make_golden.py `dp_fixture`): the
    DurationPredictor's conv -> ReLU -> LN -> FiLM stack (reference text_encoder.py:64-112) decides logw, so durations vary
    per token (1..83 frames at prod shapes).  logw to 2e-5, the integer durations / lengths bit-equal (the fixture's seeds keep
    every exp(logw)-2 at least 5e-4 (relative) away from a rounding boundary), mu_y and the mel inside the path's tolerance."""
    g = np.load(GOLDEN / f"{tag}.npz")
    hp = hparams.tiny(n_spks=2) if which == "tiny" else hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=int(g["seed_w"]), duration_recipe=False)
    model = make_model(hp, sd, dev)
    lengths = [int(v) for v in g["x_lengths"]]
    x, x_len, spk = synthetic.make_inputs(hp, len(lengths), max(lengths), seed=int(g["seed_x"]), lengths=lengths)
    assert np.array_equal(x.numpy(), g["x"])
    sc, ls, steps = float(g["sc"]), float(g["ls"]), int(g["steps"])
    logw_g = _t(g["logw"])
    assert float(logw_g[:, 0, : min(lengths)].std()) > 0.3          # not the constant-duration recipe
    model.decoder.solver = "euler"
    z = lambda t_pad: synthetic.cpu_noise((len(lengths), hp.n_feats, t_pad)).to(dev)
    out = model.synthesise(x.to(dev), x_len.to(dev), steps, speaker=spk.to(dev), scale_correction=sc, length_scale=ls,
                           debug=True, z=z)
    assert maxabs(out["logw"], logw_g) < 2e-5
    assert maxabs(out["mu_x"], _t(g["mu_x"])) < 2e-5
    assert torch.equal(out["phoneme_durations"].cpu(), _t(g["durations"]))
    assert torch.equal(out["mel_lengths"].cpu(), _t(g["y_lengths"]))
    assert out["mu_y"].shape == g["mu_y"].shape and maxabs(out["mu_y"], _t(g["mu_y"])) < 2e-5
    assert out["mel"].shape == g["mel"].shape
    assert maxabs(out["mel"], _t(g["mel"])) < MEL_TOL
    # the reference's own batch-1 synthesise of utterance 0
    n0 = lengths[0]
    solo = model.synthesise(x[:1, :n0].to(dev), x_len[:1].to(dev), steps, speaker=int(spk[0]), scale_correction=sc,
                            length_scale=ls, debug=True, z=lambda t_pad: synthetic.cpu_noise((1, hp.n_feats, t_pad)).to(dev))
    assert torch.equal(solo["phoneme_durations"].cpu(), _t(g["solo_dur"]))
    assert maxabs(solo["mel"], _t(g["solo_mel"])) < MEL_TOL


# ------------------------------------------------------------------------------------------------ API behaviour
def test_api_surface(tiny, synthetic, dev):
    hp, sd, model = tiny
    inf = sub("inference")
    assert inf.SAMPLE_RATE == 24000 and inf.DEFAULT_ODE_SOLVER == "midpoint" and inf.DEFAULT_NUM_STEPS == 4
    assert len(inf.VOICES) == 15 and inf.VOICES[4]["lang"] == "en-gb"
    x, x_len, _ = synthetic.make_inputs(hp, 1, 12, seed=3)
    # the server wraps the estimator in torch.compile and pokes .solver per request (reference server.py:43-47,109)
    model.decoder.estimator = torch.compile(model.decoder.estimator)
    model.decoder.solver = "euler"
    a = model.synthesise(x.to(dev), x_len.to(dev), n_timesteps=2)["mel"]
    b = model.synthesise(x.to(dev), x_len.to(dev), n_timesteps=2)["mel"]
    assert torch.equal(a, b)          # device seed-42 generator => reproducible (reference flow_matching.py:43-44)
    # decoder(mu, mask, n) and solve()/solve_euler agree
    mu = torch.randn(1, hp.n_feats, 16, device=dev)
    mask = torch.ones(1, 1, 16, device=dev)
    zz = torch.randn(1, hp.n_feats, 16, device=dev)
    t_span = torch.linspace(0, 1, 3)
    s1 = model.decoder.solve(mu + zz, t_span, mu, mask)
    s2 = model.decoder.solve_euler(mu + zz, t_span, mu, mask)
    s3 = model.decoder(mu, mask, 2, z=zz)
    assert torch.equal(s1, s2) and torch.equal(s1, s3)
    with pytest.raises(RuntimeError):
        model.synthesise(x, x_len, 2)      # CPU tensors: no fallback
    with pytest.raises(ValueError):
        model.decoder.solver = "dopri5"
        model.synthesise(x.to(dev), x_len.to(dev), 2)
    model.decoder.solver = "euler"

"""GPU tests of the 16-bit storage modes (mtts_set_arithmetic 16 / 17) with the one-plane transformer-block chain launch
(csrc/tblock_chain_h16.hip) inside the estimator: against the tiled H16 launches (MTTS_CHAIN16=0), the oracle, the reference's own
autocast distance, launch counts, repeatability and graph replay."""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_hip_path import MEL_TOL, _t, make_model, maxabs

pytestmark = pytest.mark.gpu
H16_TAG = "tblock_h16_kernel"
# mel error of the narrow estimators against the fp32 oracle, relative to max |mel|: fp16 planes as the existing mode-16 test
# (4e-3); bfloat16 planes have 8 significand bits instead of 11, i.e. 8x the unit round-off
BOUND = {16: 4e-3, 17: 3.2e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


def model_with(monkeypatch, env, hp, sd, dev):
    """A model whose context was created under `env` (the library reads its switches at mtts_create only)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = make_model(hp, sd, dev)
    m.hip
    for k in env:
        monkeypatch.delenv(k)
    return m


def profiled(m, fn):
    """(result, per-launch tags) of fn() with the per-launch event pass on (eager launches)."""
    keep = m.decoder.graph_mode
    m.decoder.graph_mode = "0"
    m.hip.prof_enable(True)
    m.hip.prof_reset()
    try:
        out = fn()
        torch.cuda.synchronize()
        tags = m.hip.prof_tags()
        assert len(tags) == len(m.hip.prof_records())
    finally:
        m.hip.prof_enable(False)
        m.decoder.graph_mode = keep
    return out, tags


@pytest.mark.parametrize("terms", [16, 17])
@pytest.mark.parametrize("channels,n_blocks,heads", [((128, 128), 2, 2), ((256, 256), 2, 2), ((128, 256), 1, 2)])
def test_narrow_estimators_chain_vs_tiled_vs_oracle(channels, n_blocks, heads, terms, hparams, synthetic, oracle, dev, monkeypatch):
    hp = hparams.tiny(n_spks=2)
    hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64, n_blocks=n_blocks,
                                                             num_mid_blocks=1, num_heads=heads))
    sd = synthetic.make_state_dict(hp, seed=21)
    chained = model_with(monkeypatch, {"MTTS_GEMM_TERMS": str(terms), "MTTS_CHAIN16_MIN_ROWS": "0"}, hp, sd, dev)
    tiled = model_with(monkeypatch, {"MTTS_GEMM_TERMS": str(terms), "MTTS_CHAIN16": "0"}, hp, sd, dev)
    assert chained.hip.gemm_terms() == terms and tiled.hip.gemm_terms() == terms
    assert chained.hip.weights_signature() != tiled.hip.weights_signature()
    lengths = [14, 9, 3]
    x, x_len, spk = synthetic.make_inputs(hp, 3, max(lengths), seed=8, lengths=lengths)
    t_pad = 2 * ((5 * max(lengths) + 1) // 2)
    z = synthetic.cpu_noise((3, hp.n_feats, t_pad)).to(dev)
    outs, tags = {}, {}
    for name, m in (("chain", chained), ("tiled", tiled)):
        m.decoder.solver = "midpoint"
        outs[name], tags[name] = profiled(m, lambda: m.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev), z=z, debug=True))
    assert any(H16_TAG in t for t in tags["chain"]) and not any(H16_TAG in t for t in tags["tiled"])
    ref = oracle.synthesise(sd, hp, x, x_len, 2, speaker=spk, solver="midpoint", z=z.cpu())
    scale = float(ref["mel"].abs().max())
    for name in outs:
        assert torch.equal(outs[name]["phoneme_durations"].cpu(), ref["durations"]), name
        err = maxabs(outs[name]["mel"], ref["mel"])
        print(f"terms {terms} {channels} {name}: mel error vs oracle {err:.3e} (scale {scale:.2f})")
        assert err < BOUND[terms] * scale, (name, err, scale)
    assert maxabs(outs["chain"]["mel"], outs["tiled"]["mel"]) < BOUND[terms] * scale
    assert not bool(chained.hip.range_flags().any().item())


@pytest.mark.parametrize("terms,name", [(16, "fp16"), (17, "bf16")])
def test_prod_chain_forced_on_vs_reference_autocast_anchor(hparams, synthetic, dev, monkeypatch, terms, name):
    """Production shape, the reference-derived anchor of tests/test_hip_path.py::test_half_storage_mode_vs_reference_autocast_anchor
    with the one-plane chain forced on at every level (B = 1 is below the default threshold)."""
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    g = np.load(GOLDEN / "prod_synth.npz")
    a = np.load(GOLDEN / "prod_autocast.npz")
    half = model_with(monkeypatch, {"MTTS_GEMM_TERMS": str(terms), "MTTS_CHAIN16_MIN_ROWS": "0"}, hp, sd, dev)
    x, x_len, _ = synthetic.make_inputs(hp, 1, 128, seed=1234)
    z = synthetic.cpu_noise((1, 100, 640)).to(dev)
    half.decoder.solver = "euler"
    out, tags = profiled(half, lambda: half.synthesise(x.to(dev), x_len.to(dev), 10, speaker=0, z=z))
    assert sum(H16_TAG in t for t in tags) == 10 * 12            # every transformer block of every evaluation
    mel = out["mel"].cpu()
    gold = _t(g["mel_euler10"])
    err_max, err_mean = maxabs(mel, gold), float((mel - gold).abs().mean())
    ref_max, ref_mean = (float(v) for v in a[f"err_{name}"])
    print(f"{name} storage mode, chain on, vs fp32 golden: max {err_max:.3e} mean {err_mean:.3e}; reference autocast: max {ref_max:.3e} mean {ref_mean:.3e}")
    assert 1e-4 < err_max <= 1.5 * ref_max and err_mean <= 1.5 * ref_mean, (err_max, err_mean, ref_max, ref_mean)
    assert not bool(half.hip.range_flags().any().item())


def test_config3_shape_bf16_takes_the_chain_saves_launches_and_repeats_bitwise(hparams, synthetic, dev, monkeypatch):
    """B = 32, Tx = 128, euler, bfloat16 planes, DEFAULT threshold: the launch is taken at both levels (20608 / 10304 rows), an
    evaluation has 3 launches fewer per chained block that carries the next q|k|v (6 of 12) and 2 fewer per one that does not,
    repeated evaluations are bitwise equal and a captured-graph replay repeats itself bitwise and agrees with the eager run."""
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    chained = model_with(monkeypatch, {"MTTS_GEMM_TERMS": "17"}, hp, sd, dev)
    tiled = model_with(monkeypatch, {"MTTS_GEMM_TERMS": "17", "MTTS_CHAIN16": "0"}, hp, sd, dev)
    x, x_len, _ = synthetic.make_inputs(hp, 32, 128, seed=1234)
    z = synthetic.cpu_noise((32, 100, 640)).to(dev)
    steps, outs, tags = 2, {}, {}
    for name, m in (("chain", chained), ("tiled", tiled)):
        m.decoder.solver = "euler"
        outs[name], tags[name] = profiled(m, lambda: m.synthesise(x.to(dev), x_len.to(dev), steps, speaker=0, z=z)["mel"])
    n_h16 = sum(H16_TAG in t for t in tags["chain"])
    assert n_h16 == steps * 12 and all("true>" in t for t in tags["chain"] if H16_TAG in t), n_h16      # bfloat16 instantiations
    assert not any(H16_TAG in t for t in tags["tiled"])
    assert len(tags["tiled"]) - len(tags["chain"]) == steps * (6 * 3 + 6 * 2), (len(tags["tiled"]), len(tags["chain"]))
    assert torch.isfinite(outs["chain"]).all()
    # two bfloat16 roundings of one computation: each is ~0.25 from the fp32-equivalent mel at this shape (|mel| up to ~50, unit
    # round-off 2^-8), so they are at most about twice that apart
    assert maxabs(outs["chain"], outs["tiled"]) < 0.5
    # 100 evaluations of one estimator call at the same shape
    B, T = 32, 644
    g = torch.Generator().manual_seed(3)
    xs = torch.randn(B, hp.n_feats, T, generator=g).to(dev)
    mu = torch.randn(B, hp.n_feats, T, generator=g).to(dev)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    mask = (torch.arange(T)[None, :] < lens[:, None]).float()[:, None, :].to(dev)
    first = chained.hip.decoder_forward(xs, mask, mu, 0.37).clone()
    assert torch.isfinite(first).all()
    differing = sum(int(not torch.equal(chained.hip.decoder_forward(xs, mask, mu, 0.37), first)) for _ in range(100))
    assert differing == 0, f"{differing} of 100 evaluations differ from the first"
    # captured graph
    dec = chained.decoder
    keep = dec.graph_mode, dec.graph_max_rows
    try:
        dec.graph_mode = "0"
        direct = chained.synthesise(x.to(dev), x_len.to(dev), 3, speaker=0, z=z)["mel"]
        dec.graph_mode = "1"
        dec.graph_max_rows = 1 << 20
        one = chained.synthesise(x.to(dev), x_len.to(dev), 3, speaker=0, z=z)["mel"]
        two = chained.synthesise(x.to(dev), x_len.to(dev), 3, speaker=0, z=z)["mel"]
        assert dec.graph_replays >= 2
        assert torch.equal(one, two)
        assert maxabs(one, direct) < 0.5                         # (the bucketed row count changes the tiled kernels' tile shapes)
    finally:
        dec.graph_mode, dec.graph_max_rows = keep
        dec._graphs.clear()


def test_default_arithmetic_never_takes_the_h16_chain(hparams, synthetic, dev, monkeypatch):
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    m = model_with(monkeypatch, {"MTTS_CHAIN16_MIN_ROWS": "0"}, hp, sd, dev)
    x, x_len, _ = synthetic.make_inputs(hp, 2, 64, seed=5)
    m.decoder.solver = "euler"
    out, tags = profiled(m, lambda: m.synthesise(x.to(dev), x_len.to(dev), 2, speaker=0)["mel"])
    assert tags and not any(H16_TAG in t for t in tags)
    assert torch.isfinite(out).all()

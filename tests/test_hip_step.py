"""GPU tests of step-level batching: the one-step entry over a slot pool (include/mtts.h mtts_cfm_step), one time per utterance in
every ResNet block, and ``StepBatcher`` on the production synthetic model.

What must hold: n step calls on a uniform grid ARE the one-call solve; utterances at different times do not see each other's
time; a request's mel does not depend on who it shared its steps with."""
import time

import pytest
import torch

from conftest import sub

pytestmark = pytest.mark.gpu


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


def model_with_env(hp, sd, dev, monkeypatch, **env):
    """A model whose context was created under ``env`` (the switches are read once per context)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = make_model(hp, sd, dev)
    m.hip
    for k in env:
        monkeypatch.delenv(k)
    return m


@pytest.fixture(scope="module")
def tiny(hparams, synthetic, dev):
    hp = hparams.tiny(n_spks=2)
    sd = synthetic.make_state_dict(hp, seed=7)
    return hp, sd, make_model(hp, sd, dev)


@pytest.fixture(scope="module")
def prod(hparams, synthetic, dev):
    hp = hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    return hp, sd, make_model(hp, sd, dev)


def maxabs(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def state_inputs(synthetic, hp, y_lens, T, dev, seed=3):
    B, nf = len(y_lens), hp.n_feats
    z = torch.from_numpy(synthetic.portable_normal(seed, 1, B * nf * T).reshape(B, nf, T)).float().to(dev)
    mu = torch.from_numpy(synthetic.portable_normal(seed, 2, B * nf * T).reshape(B, nf, T)).float().to(dev)
    return z, mu, torch.tensor(y_lens, dtype=torch.int64, device=dev)


def pools_from(z, mu, slots, n_slots):
    B, nf, T = z.shape
    zp = torch.full((n_slots, nf, T), 7.5, device=z.device)          # (a recognisable filler in the slots nobody owns)
    mp = torch.full((n_slots, nf, T), -3.25, device=z.device)
    for b, s in enumerate(slots):
        zp[s].copy_(z[b])
        mp[s].copy_(mu[b])
    return zp, mp


# ------------------------------------------------------------------------------------------------ 1. uniform grid = the one-call solve
def solve_and_steps(model, hp, synthetic, dev, solver, n, y_lens, T):
    hip = model.hip
    z, mu, y_len = state_inputs(synthetic, hp, y_lens, T, dev)
    y_max = max(y_lens)
    t_fold = hip.fold_rows(y_max, 1)
    t_span = torch.linspace(0, 1, n + 1, dtype=torch.float32)
    ref = hip.cfm_solve(z, mu, None, t_span, solver, y_lengths=y_len, y_max=y_max, t_fold=t_fold, t_out=t_fold)
    B = len(y_lens)
    slots = [(3 * b + 1) % (B + 2) for b in range(B)]                # not the identity, not contiguous
    assert len(set(slots)) == B
    zp, mp = pools_from(z, mu, slots, B + 2)
    before = zp.clone()
    ts = t_span.tolist()
    for i in range(n):
        hip.cfm_step(zp, mp, slots, [ts[i]] * B, [ts[i + 1]] * B, y_len, y_max, t_fold, solver)
    got = torch.stack([zp[s, :, :t_fold] for s in slots])
    free = [s for s in range(B + 2) if s not in slots]
    assert torch.equal(zp[free], before[free])                       # slots outside the step are not touched
    assert torch.equal(zp[slots][:, :, t_fold:], before[slots][:, :, t_fold:])
    return ref, got


@pytest.mark.parametrize("solver,n", [("euler", 4), ("midpoint", 3), ("rk4", 2)])
def test_uniform_grid_steps_equal_one_call_solve_tiny(tiny, synthetic, dev, solver, n):
    hp, sd, model = tiny
    ref, got = solve_and_steps(model, hp, synthetic, dev, solver, n, [10, 7, 3], 24)
    assert torch.isfinite(got).all()
    assert maxabs(ref, got) <= 1e-5


@pytest.mark.parametrize("solver,n", [("euler", 3), ("midpoint", 2), ("rk4", 1)])
def test_uniform_grid_steps_equal_one_call_solve_prod(prod, synthetic, dev, solver, n):
    hp, sd, model = prod
    ref, got = solve_and_steps(model, hp, synthetic, dev, solver, n, [150, 97, 64], 320)
    assert torch.isfinite(got).all()
    assert maxabs(ref, got) <= 1e-5


def test_uniform_grid_steps_equal_one_call_solve_half_storage(hparams, synthetic, dev, monkeypatch):
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    model = model_with_env(hp, sd, dev, monkeypatch, MTTS_GEMM_TERMS="17")
    assert model.hip.gemm_terms() == 17
    ref, got = solve_and_steps(model, hp, synthetic, dev, "midpoint", 2, [150, 97, 64], 320)
    assert maxabs(ref, got) <= 1e-5


# ------------------------------------------------------------------------------------------------ 2. one time per utterance
def one_step(hip, z, mu, y_len_list, t0, t1, solver, t_len, dev, rows=None):
    """One step of a batch from pools that hold exactly (z, mu); returns the stepped states [B, n_feats, t_fold]."""
    B = z.shape[0]
    y_max = max(y_len_list)
    t_fold = hip.fold_rows(y_max, 1) if rows is None else rows
    zp, mp = z.clone(), mu.clone()
    hip.set_frame_limits(torch.tensor(t_len, dtype=torch.int32, device=dev))
    try:
        hip.cfm_step(zp, mp, list(range(B)), t0, t1, torch.tensor(y_len_list, dtype=torch.int64, device=dev), y_max, t_fold, solver)
    finally:
        hip.set_frame_limits(None)
    return zp, t_fold


def per_utterance_time(model, hp, synthetic, dev, solver, y_lens, T):
    hip = model.hip
    z, mu, _ = state_inputs(synthetic, hp, y_lens, T, dev, seed=5)
    B = len(y_lens)
    t_len = [2 * ((y + 1) // 2 * 2) for y in y_lens]                 # each utterance's own (even) padded length
    t0 = [0.0, 0.5, 0.9, 0.25][:B]
    t1 = [0.25, 0.6, 1.0, 0.75][:B]
    batch, _ = one_step(hip, z, mu, y_lens, t0, t1, solver, t_len, dev)
    worst = 0.0
    for b in range(B):
        solo, rows = one_step(hip, z[b:b + 1], mu[b:b + 1], y_lens[b:b + 1], t0[b:b + 1], t1[b:b + 1], solver, t_len[b:b + 1], dev)
        worst = max(worst, maxabs(batch[b, :, :y_lens[b]], solo[0, :, :y_lens[b]]))
    shared, _ = one_step(hip, z, mu, y_lens, [t0[0]] * B, [t1[0]] * B, solver, t_len, dev)
    apart = min(maxabs(batch[b, :, :y_lens[b]], shared[b, :, :y_lens[b]]) for b in range(1, B))
    return worst, apart


@pytest.mark.parametrize("flow,env", [("fused conv_gn", {"MTTS_RESNET_FUSE": "7"}), ("tiled conv + gn_apply", {"MTTS_RESNET_FUSE": "0"}),
                                      ("fp32 rows", {"MTTS_P16": "0"})])
@pytest.mark.parametrize("solver", ["euler", "rk4"])
def test_each_utterance_is_stepped_at_its_own_time_prod(hparams, synthetic, dev, monkeypatch, flow, env, solver):
    hp = hparams.prod_v20(n_spks=1)
    sd = synthetic.make_state_dict(hp, seed=7)
    model = model_with_env(hp, sd, dev, monkeypatch, **env)
    if flow == "fused conv_gn":
        hip = model.hip
        hip.prof_enable(True)
        hip.prof_reset()
    worst, apart = per_utterance_time(model, hp, synthetic, dev, solver, [150, 97, 120], 320)
    if flow == "fused conv_gn":
        tags = model.hip.prof_tags()
        model.hip.prof_enable(False)
        assert any("conv_gn_kernel" in t for t in tags), "the fused Block1D launch did not run"
    assert worst <= 2e-5, (flow, worst)
    assert apart > 100 * max(worst, 1e-6), (flow, worst, apart)     # a shared bias row or a shared dt would make these equal


@pytest.mark.parametrize("solver", ["euler", "midpoint", "rk4"])
def test_each_utterance_is_stepped_at_its_own_time_tiny(tiny, synthetic, dev, solver):
    hp, sd, model = tiny
    worst, apart = per_utterance_time(model, hp, synthetic, dev, solver, [10, 7, 3, 9], 24)
    assert worst <= 2e-5
    assert apart > 100 * max(worst, 1e-6)


# ------------------------------------------------------------------------------------------------ 3. the bias consumers alone
def test_conv_gn_bias_row_per_utterance(dev):
    hip = sub("_hip")
    g = torch.Generator().manual_seed(11)
    B, T, C, N = 3, 96, 128, 384
    x = torch.randn(B * T, C, generator=g).to(dev)
    w = (0.05 * torch.randn(N, C, 3, generator=g)).to(dev)
    bias, gamma, beta = (0.1 * torch.randn(N, generator=g)).to(dev), (1 + 0.1 * torch.randn(N, generator=g)).to(dev), (0.1 * torch.randn(N, generator=g)).to(dev)
    mask = torch.ones(B * T, device=dev)
    mask[T - 9:T] = 0
    rows = (0.3 * torch.randn(B, N + 64, generator=g)).to(dev)       # a stride larger than N, as in the model (tb_total)
    got = hip.conv_gn_rows(x, w, bias, gamma, beta, mask, rows, B=B, T=T)
    for b in range(B):
        solo = hip.conv_gn(x[b * T:(b + 1) * T], w, bias, gamma, beta, mask[b * T:(b + 1) * T], B=1, T=T, chbias=rows[b, :N].contiguous())
        assert torch.equal(got[b * T:(b + 1) * T], solo), b          # a workgroup per (utterance, group): bit for bit
    same = rows[:1].expand(B, -1).contiguous()
    assert torch.equal(hip.conv_gn_rows(x, w, bias, gamma, beta, mask, same, B=B, T=T),
                       hip.conv_gn(x, w, bias, gamma, beta, mask, B=B, T=T, chbias=rows[0, :N].contiguous()))


def test_groupnorm_mish_bias_row_per_utterance(dev):
    hip = sub("_hip")
    g = torch.Generator().manual_seed(12)
    B, T, C = 3, 50, 64
    y = torch.randn(B * T, C, generator=g).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    mask = torch.ones(B * T, device=dev)
    mask[2 * T - 5:2 * T] = 0
    rows = (0.3 * torch.randn(B, C + 32, generator=g)).to(dev)
    plain = hip.groupnorm_mish(y, gamma, beta, mask, B, T)
    want = (plain.view(B, T, C) + rows[:, None, :C]) * mask.view(B, T, 1)
    got = hip.groupnorm_mish_rows(y, gamma, beta, mask, rows, B, T)
    assert maxabs(got.view(B, T, C), want) <= 1e-6
    one = hip.groupnorm_mish_rows(y, gamma, beta, mask, rows[0, :C].contiguous(), B, T)       # stride 0: one row for the batch
    assert maxabs(one.view(B, T, C), (plain.view(B, T, C) + rows[0, :C]) * mask.view(B, T, 1)) <= 1e-6


# ------------------------------------------------------------------------------------------------ 4./5. the scheduler
def request_kwargs(i, n_tokens):
    steps = (2, 4, 10)[i % 3]
    kw = dict(speaker=i % 3, solver="midpoint" if i % 4 else "euler", n_timesteps=steps, length_scale=(1.0, 0.8, 1.3)[(i // 2) % 3],
              scale_correction=(1.0, 1.05)[i % 2])
    if i % 5 == 3:
        kw["durations"] = [float(1 + (j * 7 + i) % 4) for j in range(n_tokens)]
    return kw


def alone(model, ids, kw, dev):
    model.decoder.solver = kw["solver"]
    x = torch.tensor([ids], dtype=torch.long, device=dev)
    out = model.synthesise(x, torch.tensor([len(ids)], device=dev), kw["n_timesteps"], speaker=torch.tensor([kw["speaker"]], device=dev),
                           scale_correction=kw["scale_correction"], length_scale=kw["length_scale"], per_request_padding=True,
                           durations=None if "durations" not in kw else [kw["durations"]])
    t = int(out["mel_lengths"][0])
    return out["mel"][0, :, :t], t


def test_requests_are_unchanged_by_their_company(prod, synthetic, dev):
    hp, sd, model = prod
    bt, inf = sub("batcher"), sub("inference")
    vocoder = inf.load_vocoder("vocos", state_dict=synthetic.make_vocos_state_dict(seed=11))
    lengths = [40, 23, 61, 12, 35, 50, 8, 29, 44]
    x, _, _ = synthetic.make_inputs(hp, len(lengths), max(lengths), seed=17, lengths=lengths)
    reqs = [(x[b, :n].tolist(), request_kwargs(b, n)) for b, n in enumerate(lengths)]
    with bt.StepBatcher(model, max_batch=6, vocoder=vocoder) as q:
        futs = []
        for i, (ids, kw) in enumerate(reqs):
            futs.append(q.submit(ids, **kw))
            time.sleep(0.004 if i % 3 else 0.03)                     # staggered: some join while others are mid-solve
        res = [f.result(timeout=300) for f in futs]
        assert q.utterance_steps == sum(kw["n_timesteps"] for _, kw in reqs)
        assert q.utterance_steps > q.batches_run                     # steps were shared
        assert q.whole_solves == 0
    for (ids, kw), r in zip(reqs, res):
        mel, t = alone(model, ids, kw, dev)
        assert r["mel_length"] == t
        assert maxabs(r["mel"], mel) < 5e-5
        want = inf.to_waveforms(mel[None], torch.tensor([t]), vocoder)[0]
        assert r["audio"].shape == want.shape
        assert maxabs(r["audio"], want) < 2e-4


def test_a_recycled_slot_carries_nothing_over_and_long_requests_take_the_whole_solve(prod, synthetic, dev):
    hp, sd, model = prod
    bt = sub("batcher")
    x, _, _ = synthetic.make_inputs(hp, 2, 70, seed=23, lengths=[70, 9])
    long_ids, short_ids = x[0, :70].tolist(), x[1, :9].tolist()
    kw = dict(speaker=1, solver="euler", n_timesteps=3, length_scale=1.0, scale_correction=1.0)
    with bt.StepBatcher(model, max_batch=4, n_slots=1) as q:          # ONE slot: the short request inherits the long one's
        a = q.submit(long_ids, **kw).result(timeout=300)
        b = q.submit(short_ids, **kw).result(timeout=300)
        assert q.whole_solves == 0
    mel_a, t_a = alone(model, long_ids, kw, dev)
    mel_b, t_b = alone(model, short_ids, kw, dev)
    assert (a["mel_length"], b["mel_length"]) == (t_a, t_b)
    assert maxabs(a["mel"], mel_a) < 5e-5 and maxabs(b["mel"], mel_b) < 5e-5
    with bt.StepBatcher(model, max_batch=4, slot_frames=64) as q:     # slots too short for the long request
        a2, b2 = q.submit(long_ids, **kw), q.submit(short_ids, **kw)
        a2, b2 = a2.result(timeout=300), b2.result(timeout=300)
        assert q.whole_solves == 1
    assert maxabs(a2["mel"], mel_a) < 5e-5 and maxabs(b2["mel"], mel_b) < 5e-5


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_step_entry_refuses_bad_arguments_and_leaves_the_pools_alone(tiny, synthetic, dev):
    hp, sd, model = tiny
    hip = model.hip
    z, mu, y_len = state_inputs(synthetic, hp, [10, 7], 24, dev)
    zp, mp = pools_from(z, mu, [0, 2], 3)
    before = zp.clone()
    t_fold = hip.fold_rows(10, 1)
    good = dict(t0=[0.0, 0.5], t1=[0.5, 1.0], y_lengths=y_len, y_max=10, t_fold=t_fold, solver="euler")

    def refused(match, slots=(0, 2), **over):
        kw = dict(good, **over)
        with pytest.raises(RuntimeError, match=match):
            hip.cfm_step(zp, mp, list(slots), kw["t0"], kw["t1"], kw["y_lengths"], kw["y_max"], kw["t_fold"], kw["solver"])
        torch.cuda.synchronize()
        assert torch.equal(zp, before)

    refused("out of range", slots=(0, 3))
    refused("out of range", slots=(-1, 2))
    refused("twice", slots=(2, 2))
    refused("T_fold", t_fold=t_fold - 2)
    refused("T_fold", t_fold=26)                                     # beyond the slot's frames
    refused("multiple", t_fold=t_fold + 1) if t_fold + 1 <= 24 else None
    refused("does not fit", y_max=25)
    with pytest.raises(RuntimeError, match="B <= S"):
        hip.cfm_step(zp, mp, [0, 1, 2, 0], [0.0] * 4, [1.0] * 4, torch.tensor([3] * 4, dtype=torch.int64, device=dev), 3, hip.fold_rows(3, 1), "euler")
    assert torch.equal(zp, before)
    hip.cfm_step(zp, mp, [0, 2], **good)                             # and the well-formed call goes through
    torch.cuda.synchronize()
    assert not torch.equal(zp[0], before[0]) and torch.equal(zp[1], before[1])

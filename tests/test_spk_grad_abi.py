"""The speaker-row gradient without a GPU: the new C entries and every host-side refusal, and the yardstick itself -- the restated
fp64 autograd gradient (tests/spk_grad_restated.py) against central finite differences of the restated fp64 loss on the tiny model."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import spk_grad_restated as G


@pytest.fixture(scope="module")
def lib():
    return sub("_hip").load()


def test_symbols_declared_exported_and_bound(lib):
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    header = (ROOT / "include" / "mtts.h").read_text()
    hip = sub("_hip")
    assert "MTTS_ABI_VERSION 2" in header and "MTTS_IMAGE_REVISION 7" in header        # (spk_grad packs its own buffer: no ABI bump)
    assert "spk_grad.hip" in hip.SOURCES
    for method in ("speaker_grad", "spk_grad_status"):
        assert callable(getattr(hip.HipModel, method))
    inf = sub("inference").MatchaTTSInfer
    assert callable(inf.speaker_grad) and callable(inf.finetune_speaker)
    doc = inf.finetune_speaker.__doc__
    assert "dropout" in doc and "matcha_tts.py:154-162" in doc                         # the two stated deviations
    assert (ROOT / "tools" / "finetune_speaker.py").exists()


def test_host_visible_refusals_need_no_device(lib, hparams):
    """Every refusal the header lists, before anything is launched (a fake non-null pointer is never dereferenced)."""
    p = C.c_void_p(256)
    big = 1 << 40
    model = sub("_hip").HipModel(hparams.tiny(n_spks=2))          # a context without weights: enough for shapes and sizes
    ctx = model.ctx

    def grad(c=ctx, x=p, xl=p, ee=p, ed=p, y=p, yl=p, B=2, Tx=4, Tm=8, dp=0.15, dd=0.3, ge=p, gd=p, ps=p, ds=p, gb=p, ws=p, n=big):
        return lib.mtts_spk_grad(c, x, xl, ee, ed, y, yl, None, dp, dd, B, Tx, Tm, ge, gd, ps, ds, None, gb, ws, n, None)

    for kw in (dict(c=None), dict(x=None), dict(xl=None), dict(ee=None), dict(ed=None), dict(y=None), dict(yl=None), dict(ge=None),
               dict(gd=None), dict(ps=None), dict(ds=None), dict(gb=None), dict(ws=None)):
        assert grad(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
    assert grad(B=0) == -1 and b"B must be" in lib.mtts_last_error()
    assert grad(Tx=1025, Tm=2000) == -1 and b"1024" in lib.mtts_last_error()
    assert grad(Tx=9, Tm=8) == -1 and b"Tm < Tx" in lib.mtts_last_error()
    assert grad(dp=0.0) == -1 and b"threshold" in lib.mtts_last_error()
    assert grad(dd=-1.0) == -1 and b"threshold" in lib.mtts_last_error()
    need = lib.mtts_spk_grad_workspace_bytes(ctx, 2, 4, 8)
    assert need > 0
    assert grad(n=need - 512) == -1 and b"workspace" in lib.mtts_last_error()
    assert grad(n=need) == -1 and b"backward panels not uploaded" in lib.mtts_last_error()
    # sizes grow with every dimension; bad shapes and a null context are refused
    ws = lib.mtts_spk_grad_workspace_bytes
    sizes = [ws(ctx, B, Tx, Tm) for B, Tx, Tm in ((1, 8, 8), (1, 8, 2000), (4, 8, 2000), (4, 128, 2000))]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for bad in ((0, 4, 8), (1, 0, 8), (1, 1025, 2000), (1, 9, 8)):
        assert ws(ctx, *bad) < 0 and lib.mtts_last_error(), bad
    assert ws(None, 1, 4, 8) < 0 and lib.mtts_spk_grad_weights_bytes(None) < 0
    offs = [lib.mtts_spk_grad_tape_offset(ctx, 2, 4, 8, w) for w in range(3)]
    assert 0 < offs[0] < offs[1] < offs[2] < need and lib.mtts_spk_grad_tape_offset(ctx, 2, 4, 8, 3) < 0
    assert lib.mtts_spk_grad_weights_bytes(ctx) < 0 and b"missing tensor" in lib.mtts_last_error()      # nothing registered yet
    assert lib.mtts_spk_grad_upload_weights(ctx, None, 0) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_spk_grad_status(None, None) == -1
    # the unit entries
    assert lib.mtts_channel_layernorm_bwd(None, p, 1, 4, 8, p, p, 1e-5, 0, None, None, 0, p, None, None, None) == -1
    assert lib.mtts_channel_layernorm_bwd(p, p, 1, 4, 8, p, p, 1e-5, 1, None, None, 0, p, None, None, None) == -1 and b"act" in lib.mtts_last_error()
    assert lib.mtts_channel_layernorm_bwd(p, p, 1, 4, 8, p, p, 1e-5, 0, None, None, 0, p, p, None, None) == -1 and b"d_film" in lib.mtts_last_error()
    assert lib.mtts_attention_rope_bwd(p, p, p, None, 1, 4, 2, 24, 0.2, p, p, p, p, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_attention_rope_bwd(p, p, p, p, 1, 1025, 2, 24, 0.2, p, p, p, p, None) == -1 and b"1024" in lib.mtts_last_error()
    assert lib.mtts_attention_rope_bwd(p, p, p, p, 1, 4, 2, 20, 0.2, p, p, p, p, None) == -1 and b"multiple of 8" in lib.mtts_last_error()


def test_seed_gate_and_token_sum_entries_refuse_on_the_host(lib):
    """mtts_spk_grad_seeds, mtts_grad_gate and mtts_token_sums: null arguments, shapes, Tx > 1024, non-positive deltas, a bad mode --
    every refusal before anything is launched (a fake non-null pointer is never dereferenced)."""
    p = C.c_void_p(256)
    big = 1 << 40
    need = lib.mtts_spk_grad_seeds_scratch_bytes
    assert need(2, 8, 20) >= lib.mtts_score_workspace_bytes(2, 8, 20) + 2 * 2 * 4
    assert need(2, 8, 20) <= need(2, 8, 2000) < need(40, 8, 2000) < need(40, 8, 20000)     # (every part rounded to 256 bytes)
    for bad in ((0, 8, 20), (2, 0, 20), (2, 1025, 2000), (2, 9, 8)):
        assert need(*bad) < 0 and lib.mtts_last_error(), bad

    def seeds(mu=p, lw=p, du=p, y=p, xl=p, yl=p, w=p, B=2, F=20, Tx=8, Tm=20, Fd=5, dp=0.15, dd=0.3, sm=p, sl=p, sc=p, n=big):
        return lib.mtts_spk_grad_seeds(mu, lw, du, y, xl, yl, w, B, F, Tx, Tm, Fd, dp, dd, sm, sl, sc, n, None)

    for kw in (dict(mu=None), dict(lw=None), dict(du=None), dict(y=None), dict(xl=None), dict(yl=None), dict(w=None), dict(sm=None),
               dict(sl=None), dict(sc=None)):
        assert seeds(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
    assert seeds(B=0) == -1 and b"B must be" in lib.mtts_last_error()
    assert seeds(Tx=1025, Tm=2000) == -1 and b"1024" in lib.mtts_last_error()
    assert seeds(Tx=9, Tm=8) == -1 and b"Tm < Tx" in lib.mtts_last_error()
    assert seeds(F=0) == -1 and seeds(F=65536) == -1 and seeds(Fd=0) == -1 and b"Fd" in lib.mtts_last_error()
    for kw in (dict(dp=0.0), dict(dd=-1.0), dict(dp=float("nan"))):
        assert seeds(**kw) == -1 and b"threshold" in lib.mtts_last_error(), kw
    assert seeds(n=need(2, 8, 20) - 1) == -1 and b"scratch too small" in lib.mtts_last_error()
    assert seeds(sc=C.c_void_p(264)) == -1 and b"aligned" in lib.mtts_last_error()

    def gate(g=p, ldg=96, M=4, Cc=96, mode=1, ref=p, ldref=96, mask=None, sc=p):
        return lib.mtts_grad_gate(g, ldg, M, Cc, mode, ref, ldref, mask, sc, None)

    assert gate(g=None) == -1 and b"null" in lib.mtts_last_error()
    assert gate(ref=None) == -1 and b"null" in lib.mtts_last_error()
    for mode in (-1, 3):
        assert gate(mode=mode) == -1 and b"mode" in lib.mtts_last_error()
    for kw in (dict(M=0), dict(Cc=0), dict(ldg=95), dict(ldref=95)):
        assert gate(**kw) == -1 and b"ldg" in lib.mtts_last_error(), kw
    assert gate(mode=2, sc=None) == -1 and b"d_scratch" in lib.mtts_last_error()
    assert gate(mode=2, Cc=80, ldg=80, ldref=80) == -1 and b"multiple of 32" in lib.mtts_last_error()
    assert gate(mode=2, ldref=98) == -1 and b"multiple of 4" in lib.mtts_last_error()

    def sums(src=p, ld=40, col0=2, Cc=36, B=2, T=5, ln=None, vd=None, dst=p, ldd=40, dcol0=3, acc=0):
        return lib.mtts_token_sums(src, ld, col0, Cc, B, T, ln, vd, dst, ldd, dcol0, acc, None)

    assert sums(src=None) == -1 and b"null" in lib.mtts_last_error()
    assert sums(dst=None) == -1 and b"null" in lib.mtts_last_error()
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(Cc=0)):
        assert sums(**kw) == -1 and b"B <= 65535" in lib.mtts_last_error(), kw
    for kw in (dict(col0=-1), dict(dcol0=-1), dict(ld=37), dict(ldd=38)):
        assert sums(**kw) == -1 and b"col0" in lib.mtts_last_error(), kw
    assert sums(acc=2) == -1 and b"accumulate" in lib.mtts_last_error()


def seed_case(seed=11):
    """A small ragged case with zero durations, both Huber branches in either loss, and a refused utterance."""
    rng = np.random.default_rng(seed)
    B, F, Tx, Fd = 4, 6, 9, 5
    x_len = [9, 4, 1, 6]
    dur = np.zeros((B, Tx), dtype=np.int64)
    for b, n in enumerate(x_len):
        dur[b, :n] = rng.integers(0, 5, size=n)
        dur[b, 0] += 3
    y_len = dur.sum(1)
    y_len[3] += 1                                               # the durations do not sum to y_len: refused
    Tm = int(y_len.max()) + 2
    mu = rng.standard_normal((B, F, Tx))
    y = np.zeros((B, F, Tm))
    for b, n in enumerate(x_len):
        y[b, :, :dur[b].sum()] = np.repeat(mu[b, :, :n], dur[b, :n], axis=1) + 0.15 * rng.standard_normal((F, int(dur[b].sum())))
    logw = np.zeros((B, Tx))
    for b, n in enumerate(x_len):
        logw[b, :n] = np.log(2.0 + dur[b, :n]) + 0.3 * rng.standard_normal(n)
    return dict(mu=mu, logw=logw, dur=dur, y=y, x_len=x_len, y_len=y_len, w=rng.standard_normal(Fd), B=B, F=F, Tx=Tx, Tm=Tm, Fd=Fd)


def test_restated_seeds_are_the_autograd_of_the_restated_losses():
    """The yardstick of the seed kernels against what it must be the derivative of -- torch.autograd of score_restated.prior_loss with
    respect to mu_x and of score_restated.duration_loss with respect to logw, in fp64 -- so that neither is derived from the kernel's
    text.  The refused utterance's rows are zero; the fp32 order agrees with fp64 to fp32 accuracy."""
    import score_restated as S
    c = seed_case()
    ref = G.seeds(c["mu"], c["logw"], c["dur"], c["y"], c["x_len"], c["y_len"], c["w"], 0.15, 0.3)
    assert ref["verdict"] == [0, 0, 0, 2] and 0.1 < ref["clamped_mu"] < 0.9 and 0.1 < ref["clamped_logw"] < 0.9
    dp, dd = float(np.float32(0.15)), float(np.float32(0.3))
    ok = [0, 1, 2]
    mu = torch.tensor(c["mu"][ok], requires_grad=True)
    lw = torch.tensor(c["logw"][ok][:, None, :], requires_grad=True)
    dur, y = torch.tensor(c["dur"][ok]), torch.tensor(c["y"][ok])
    _, prior, _, _ = S.prior_loss(mu, dur, y, torch.tensor(c["y_len"][ok]), dp)
    g_mu, = torch.autograd.grad(prior.sum(), mu)
    _, dsum, _ = S.duration_loss(lw, dur, torch.tensor(c["x_len"])[ok], dd)
    g_lw, = torch.autograd.grad(dsum.sum(), lw)
    B, F, Tx, Fd = c["B"], c["F"], c["Tx"], c["Fd"]
    seed_mu = ref["seed_mu"].reshape(B, Tx, 8)
    assert (seed_mu[:, :, F:] == 0).all() and (seed_mu[3] == 0).all() and (ref["seed_logw"].reshape(B, Tx, Fd)[3] == 0).all()
    want_mu = g_mu.permute(0, 2, 1).numpy()                     # d prior_sum / d mu_x as channels-last rows
    scale = np.abs(want_mu).max()
    assert np.abs(seed_mu[:3, :, :F] - want_mu).max() <= 1e-13 * scale
    want_lw = g_lw[:, 0, :, None].numpy() * c["w"][None, None, :]
    live = (np.arange(Tx)[None, :] < np.array(c["x_len"])[ok, None])[:, :, None]
    got_lw = ref["seed_logw"].reshape(B, Tx, Fd)[:3]
    assert np.abs((got_lw - want_lw) * live).max() <= 1e-13 * np.abs(want_lw).max() and (got_lw * ~live == 0).all()
    assert (seed_mu[0, c["dur"][0] == 0] == 0).all()            # a token without frames: seed exactly 0
    ref32 = G.seeds(c["mu"].astype(np.float32), c["logw"].astype(np.float32), c["dur"], c["y"].astype(np.float32), c["x_len"], c["y_len"],
                    c["w"].astype(np.float32), 0.15, 0.3, dtype=np.float32)
    assert ref32["seed_mu"].dtype == np.float32 and np.abs(ref32["seed_mu"] - ref["seed_mu"]).max() <= 1e-5 * scale
    assert np.abs(ref32["seed_logw"] - ref["seed_logw"]).max() <= 1e-5 * np.abs(want_lw).max()


def test_restated_token_sums_and_gates():
    """Token sums: the fp32 phase order against a hand-worked case where the order shows, and against fp64.  Gate: the mode-2 rule on
    hand-picked values -- head rounded up (negative residual), head zero with a positive residual, flushed in both planes, zeros."""
    T, C_ = 9, 3
    src = np.zeros((2 * T, 5), dtype=np.float32)
    src[:T, 1] = [2.0 ** 24, 1, 1, 1, 1, 1, 1, 1, 1]            # phase 0: 2^24 + 1 + 1 = 2^24 (each 1 is lost); phases 1..3: 2 each
    src[:T, 2] = np.arange(T)
    src[T:, 1:4] = 1.0
    got, mag = G.token_sums(src, 1, C_, 2, T, lengths=[T, 4], verdict=None)
    assert got[0, 0] == np.float32(2.0 ** 24 + 6) and got[0, 1] == 36 and (got[1] == 4).all() and mag[0, 0] == 2.0 ** 24 + 8
    want, _ = G.token_sums(src, 1, C_, 2, T, lengths=[T, 4], dtype=np.float64)
    assert want[0, 0] == 2.0 ** 24 + 8
    assert (G.token_sums(src, 1, C_, 2, T, lengths=[T + 3, -2])[0] == np.stack([got[0], np.zeros(3, np.float32)])).all()
    assert (G.token_sums(src, 1, C_, 2, T, verdict=[1, 0])[0][0] == 0).all()
    x = torch.tensor([[0.0, -0.0, 2.0 ** -149, 2.0 ** -36, 2.0 ** -36 * 1.5, 2.0 ** -25, 2.0 ** -24, 1.0 + 2.0 ** -11 + 2.0 ** -13,
                       -(2.0 ** -30), -1.0, 3.0, 70000.0]], dtype=torch.float32)
    on1, _ = G.relu_gate(x, 1)
    on2, flushed = G.relu_gate(x, 2)
    assert on1[0].tolist() == [False, False, True, True, True, True, True, True, False, False, True, True]
    assert flushed[0].tolist() == [False, False, True, True] + [False] * 8        # 2^-36 * 2^11 = 2^-25 ties to the even 0
    assert torch.equal(on2, on1 & ~flushed)
    import p16_restated as P
    h, l = P.split(x)
    assert h[0, 7] > x[0, 7] and l[0, 7] < 0 and h[0, 4] == 0 and l[0, 4] > 0 and h[0, 5] == 0 and l[0, 5] > 0
    off, _ = G.relu_gate(x, 2, mask=torch.zeros(1))
    assert not off.any()
    z = torch.linspace(-8, 8, 33)
    d64 = G.silu_gate(torch.ones(33), z)
    zz = z.double().requires_grad_(True)
    auto, = torch.autograd.grad(torch.nn.functional.silu(zz).sum(), zz)
    assert (d64 - auto).abs().max() < 1e-14
    assert ((G.silu_gate(torch.ones(33), z, torch.float32).double() - d64).abs() <= G.silu_gate_floor(torch.ones(33), z)).all()


def test_backward_panels_pack_from_the_registered_tensors(lib, hparams, synthetic):
    """The on-demand pack needs no device: its size is stable, independent of the weight image, and a new tensor invalidates it."""
    hp = hparams.tiny(n_spks=2)
    model = sub("_hip").HipModel(hp)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    for k, v in sd.items():
        if k not in ("mel_mean", "mel_std"):
            model._set(k, v)
    n = lib.mtts_spk_grad_weights_bytes(model.ctx)
    assert n > 0 and lib.mtts_spk_grad_weights_bytes(model.ctx) == n
    e = hp.encoder
    H, F = e.n_channels + hp.spk_emb_dim, e.dp_filter_channels
    floats = (e.n_channels * hp.n_feats + H * e.n_channels + e.n_layers * (4 * H * H + 2 * e.kernel_size * H * e.filter_channels)
              + (e.dp_n_layers - 1) * e.dp_kernel_size * F * F + 2 * F * hp.spk_emb_dim + F)
    assert n >= 4 * floats                                        # at least every transposed weight once
    model._set("encoder.proj_m.2.weight", sd["encoder.proj_m.2.weight"] * 2)
    assert lib.mtts_spk_grad_weights_bytes(model.ctx) == n        # (repacked, same layout)


def tiny_case(hparams, synthetic, oracle):
    hp = dataclasses.replace(hparams.tiny(n_spks=3), prior_loss_threshold=0.15, duration_loss_threshold=0.3)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    lengths = [7, 4, 1]
    x, x_len, spk = synthetic.make_inputs(hp, 3, 7, seed=31, lengths=lengths)
    rng = np.random.default_rng(3)
    dur = torch.zeros(3, 7, dtype=torch.long)
    for b, n in enumerate(lengths):
        dur[b, :n] = torch.from_numpy(rng.integers(1, 6, size=n))
    y_len = dur.sum(1)
    Tm = int(y_len.max()) + 3
    with torch.inference_mode():
        mu_x, _, _ = oracle.text_encoder_forward(sd, hp, x, x_len, sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk])
    y = torch.zeros(3, hp.n_feats, Tm)
    for b, n in enumerate(lengths):
        y[b, :, :y_len[b]] = torch.repeat_interleave(mu_x[b, :, :n], dur[b, :n], dim=1) + 0.15 * torch.from_numpy(
            rng.standard_normal((hp.n_feats, int(y_len[b]))).astype(np.float32))
    return hp, sd, x, x_len, spk, dur, y, y_len


def test_restated_gradient_agrees_with_finite_differences(hparams, synthetic, oracle):
    hp, sd, x, x_len, spk, dur, y, y_len = tiny_case(hparams, synthetic, oracle)
    e_enc, e_dur = sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk]
    out = G.speaker_grad(oracle, sd, hp, x, x_len, e_enc, e_dur, y, y_len, dur, 0.15, 0.3)
    assert out["g_enc"].shape == (3, hp.spk_emb_dim) and out["g_dur"].abs().max() > 0 and out["g_enc"].abs().max() > 0
    sd64 = G.cast_state_dict(sd, torch.float64)
    h = 1e-6

    def total(which, b, j, step):
        ee, ed = e_enc.double().clone(), e_dur.double().clone()
        (ee if which == 0 else ed)[b, j] += step
        with torch.no_grad():
            prior, dsum, _, _ = G.sums(oracle, sd64, hp, x, x_len, ee, ed, y.double(), y_len, dur, 0.15, 0.3)
        return float(prior[b]) if which == 0 else float(dsum[b])

    worst = 0.0
    for which, g in ((0, out["g_enc"]), (1, out["g_dur"])):
        scale = float(g.abs().max())
        for b in range(3):
            for j in (0, 5, hp.spk_emb_dim - 1):
                fd = (total(which, b, j, h) - total(which, b, j, -h)) / (2 * h)
                worst = max(worst, abs(fd - float(g[b, j])) / scale)
    # central differences of a C1 function with step 1e-6 in fp64: truncation ~h^2, rounding ~1e-16 / h
    assert worst < 1e-6, worst
    # both Huber branches occur in this case
    d_prior = (y.double() - torch.matmul(out["mu_x"], __import__("score_restated").path_from_durations(dur, y.shape[2]).double()))
    m = __import__("score_restated").sequence_mask(y_len, y.shape[2])[:, None, :]
    inside = (d_prior.abs() < 0.15)[m.expand_as(d_prior)]
    assert 0.1 < inside.double().mean() < 0.9
    # and the fp32 loop is the same computation: it agrees with fp64 to fp32 accuracy
    out32 = G.speaker_grad(oracle, sd, hp, x, x_len, e_enc, e_dur, y, y_len, dur, 0.15, 0.3, dtype=torch.float32)
    assert float(G.row_error(out32["g_enc"], out["g_enc"]).max()) < 1e-4 and float(G.row_error(out32["g_dur"], out["g_dur"]).max()) < 1e-4


def test_fp64_finetune_loop_lowers_the_loss(hparams, synthetic, oracle):
    hp, sd, x, x_len, spk, dur, y, y_len = tiny_case(hparams, synthetic, oracle)
    # recordings were made with each utterance's own voice; start every utterance from voice 1 and train on the given durations
    e_enc, e_dur = sd["speaker_embeddings_enc.weight"][1], sd["speaker_embeddings_dur.weight"][1]
    trail, hist = G.finetune(oracle, sd, hp, x, x_len, y, y_len, e_enc, e_dur, steps=6, lr=1e-2, delta_prior=0.15, delta_dur=0.3, durations=dur)
    total = [d + p for d, p in hist]
    assert len(trail) == 7 and all(b < a for a, b in zip(total, total[1:])), total

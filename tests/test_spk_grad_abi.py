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

"""Duration-predictor training without a GPU: the yardstick itself -- the restated gradient (tests/dp_grad_restated.py) against
torch.autograd of the oracle's predictor in fp64, on the tiny and the production predictor shapes -- the parameter layout, every
host-side refusal of the new C entries, and the training component's round trip."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import dp_grad_restated as R

DELTA = 0.3


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def case(hp, B, T, lengths, seed):
    """Encoder rows at unit scale, speaker rows, durations that put the Huber terms on both branches."""
    g = torch.Generator().manual_seed(seed)
    Hd = hp.encoder.n_channels + hp.spk_emb_dim
    h = torch.randn(B, Hd, T, generator=g, dtype=torch.float64)
    e_dur = 0.5 * torch.randn(B, hp.spk_emb_dim, generator=g, dtype=torch.float64)
    dur = torch.randint(0, 9, (B, T), generator=g)
    return h, torch.tensor(lengths), e_dur, dur


@pytest.mark.parametrize("size,B,T,lengths", [("tiny", 3, 40, [40, 17, 1]), ("prod", 3, 40, [40, 17, 1]), ("tiny", 5, 300, [300, 299, 2, 150, 77]),
                                                 ("tiny", 5, 1024, [1024, 1000, 513, 1, 300])])
def test_restated_gradient_equals_fp64_autograd(hparams, synthetic, oracle, size, B, T, lengths):
    """Every parameter gradient, g_dur, the sums and logw: the formulas of include/mtts.h against autograd of the oracle's predictor.
    Both are fp64 and differ in the order of their sums alone: 1e-11 of each tensor's largest entry (fp64's 2^-53 times a few thousand
    terms is 1e-12).  This is the check of the yardstick itself: it runs no library code, so unlike the other tests of this file it
    does not depend on the feature being there.  Shapes: those of the GPU file (3 x 40, 5 x 1024) and one with two chunks of rows."""
    hp = hparams.tiny(n_spks=2) if size == "tiny" else hparams.prod_v20(n_spks=2)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    P = R.params_of(sd, hp)
    h, lens, e_dur, dur = case(hp, B, T, lengths, seed=5)
    G, g_dur, sums, logw = R.param_grads(P, hp, h, lens, e_dur, dur, DELTA)
    A, a_dur, a_sums, a_logw = R.autograd_grads(oracle, P, hp, h, lens, e_dur, dur, DELTA)
    d = (a_logw[:, 0] - torch.log(2 + dur.double()))[R.mask_of(lens, T, torch.float64)[:, 0] > 0]
    share = float((d.abs() < DELTA).double().mean())
    assert 0.02 <= share <= 0.98, share                     # both Huber branches occur
    assert torch.allclose(logw, a_logw, rtol=0, atol=1e-12) and torch.allclose(sums, a_sums, rtol=1e-12, atol=0)
    for k in P:
        assert G[k].shape == P[k].shape == A[k].shape, k
        top = A[k].abs().max().item()
        assert top > 0, k
        assert (G[k] - A[k]).abs().max().item() <= 1e-11 * top, k
    assert (g_dur - a_dur).abs().max().item() <= 1e-11 * a_dur.abs().max().item()


def test_parameter_layout_is_state_dict_order(lib, hparams, synthetic):
    hip = sub("_hip")
    for hp in (hparams.tiny(n_spks=2), hparams.prod_v20(n_spks=2)):
        sd = synthetic.make_state_dict(hp, seed=7)
        keys = [k[len(R.PREFIX):] for k in sd if k.startswith(R.PREFIX)]
        lay = R.layout(hp)
        assert [k for k, _, _ in lay] == keys                                      # state-dict order
        assert all(tuple(sd[R.PREFIX + k].shape) == shape for k, _, shape in lay)
        model = hip.HipModel(hp)                                                   # a context without a device
        assert lib.mtts_dp_param_count(model.ctx) == R.param_count(hp) == sum(sd[R.PREFIX + k].numel() for k in keys)
        for k, off, _ in lay:
            assert lib.mtts_dp_param_offset(model.ctx, k.encode()) == off, k
        assert model.dp_layout() == lay
        assert lib.mtts_dp_param_offset(model.ctx, b"conv_layers.99.weight") == -1 and b"no parameter" in lib.mtts_last_error()
    assert R.param_count(hparams.prod_v20()) > 250_000                             # (about 0.28 M floats at the production size)
    assert lib.mtts_dp_param_count(None) == -1 and lib.mtts_dp_param_offset(None, b"proj.bias") == -1


def test_host_visible_refusals_need_no_device(lib, hparams):
    """Every refusal the header lists, before anything is launched (a fake non-null pointer is never dereferenced)."""
    import dataclasses
    hip = sub("_hip")
    p = C.c_void_p(256)
    big = 1 << 40
    model = hip.HipModel(hparams.tiny(n_spks=2))
    ctx = model.ctx

    def grad(c=ctx, x=p, xl=p, ee=p, ed=p, du=p, dd=0.3, B=2, Tx=4, tb=p, g=p, gd=p, ds=p, lw=p, ws=p, n=big):
        return lib.mtts_dp_grad(c, x, xl, ee, ed, du, dd, B, Tx, tb, g, gd, ds, lw, ws, n, None)

    for kw in (dict(c=None), dict(x=None), dict(xl=None), dict(ee=None), dict(ed=None), dict(du=None), dict(tb=None), dict(g=None),
               dict(ds=None), dict(ws=None)):
        assert grad(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
    assert grad(B=0) == -1 and b"B must be" in lib.mtts_last_error()
    assert grad(Tx=1025) == -1 and b"1024" in lib.mtts_last_error()
    for dd in (0.0, -1.0, float("nan")):
        assert grad(dd=dd) == -1 and b"threshold" in lib.mtts_last_error()
    need = lib.mtts_dp_grad_workspace_bytes(ctx, 2, 4)
    assert need > 0
    assert grad(n=need - 512) == -1 and b"workspace" in lib.mtts_last_error()
    assert grad(ws=C.c_void_p(264)) == -1 and b"aligned" in lib.mtts_last_error()
    assert grad(n=need) == -1 and b"not uploaded" in lib.mtts_last_error()          # no mtts_dp_train_upload into d_train_buf yet
    assert grad(gd=None, lw=None, n=need) == -1 and b"not uploaded" in lib.mtts_last_error()   # (both optional)
    ws = lib.mtts_dp_grad_workspace_bytes
    sizes = [ws(ctx, B, Tx) for B, Tx in ((1, 8), (4, 8), (4, 128), (4, 1024))]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for bad in ((0, 4), (1, 0), (1, 1025)):
        assert ws(ctx, *bad) < 0 and lib.mtts_last_error(), bad
    assert ws(None, 1, 4) < 0
    offs = [lib.mtts_dp_grad_tape_offset(ctx, 2, 4, w) for w in range(2)]
    assert 0 < offs[0] < offs[1] < need and lib.mtts_dp_grad_tape_offset(ctx, 2, 4, 2) < 0
    assert lib.mtts_dp_grad_status(None, None) == -1
    rows = lib.mtts_spk_grad_rows_offset(ctx, 2, 4, 8)
    assert 0 < rows < lib.mtts_spk_grad_workspace_bytes(ctx, 2, 4, 8) and lib.mtts_spk_grad_rows_offset(None, 2, 4, 8) == -1
    assert lib.mtts_spk_grad_rows_offset(ctx, 2, 9, 8) == -1 and b"Tm < Tx" in lib.mtts_last_error()
    # the component: nothing registered yet, null arguments, a small buffer
    nb = lib.mtts_dp_train_weights_bytes(ctx)
    assert nb > 4 * R.param_count(hparams.tiny(n_spks=2))
    assert lib.mtts_dp_train_weights_bytes(None) == -1
    assert lib.mtts_dp_train_upload(ctx, None, None, nb) == -1 and b"null" in lib.mtts_last_error()
    host = np.zeros(nb, dtype=np.uint8)
    assert lib.mtts_dp_train_pack(ctx, None, host.ctypes.data, nb) == -1 and b"missing tensor" in lib.mtts_last_error()
    flat = np.zeros(R.param_count(hparams.tiny(n_spks=2)), dtype=np.float32)
    assert lib.mtts_dp_train_pack(ctx, flat.ctypes.data, host.ctypes.data, nb - 4) == -1 and b"too small" in lib.mtts_last_error()
    # dp_kernel != 5: the weight-gradient kernel has five taps
    hp3 = hparams.tiny(n_spks=2)
    hp3 = dataclasses.replace(hp3, encoder=dataclasses.replace(hp3.encoder, dp_kernel_size=3))
    m3 = hip.HipModel(hp3)
    assert lib.mtts_dp_grad(m3.ctx, p, p, p, p, p, 0.3, 2, 4, p, p, p, p, p, p, big, None) == -1 and b"dp_kernel" in lib.mtts_last_error()
    assert lib.mtts_dp_train_weights_bytes(m3.ctx) == -1 and b"dp_kernel" in lib.mtts_last_error()
    # the unit entries
    assert lib.mtts_dp_unit_workspace_bytes(2, 129, 32) == 4 * 2 * 64 and lib.mtts_dp_unit_workspace_bytes(0, 1, 1) < 0
    assert lib.mtts_ln_film_wgrad(None, p, p, p, 1, 4, 8, 1e-5, p, p, p, big, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_ln_film_wgrad(p, p, p, p, 1, 0, 8, 1e-5, p, p, p, big, None) == -1 and b"shape" in lib.mtts_last_error()
    assert lib.mtts_ln_film_wgrad(p, p, p, p, 1, 4, 8, 1e-5, p, p, p, 8, None) == -1 and b"workspace" in lib.mtts_last_error()
    assert lib.mtts_rows_wgrad(p, None, p, 1, 4, 8, p, p, p, big, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_rows_wgrad(p, p, p, 1, 4, 0, p, p, p, big, None) == -1 and b"shape" in lib.mtts_last_error()
    assert lib.mtts_rows_wgrad(p, p, p, 1, 4, 8, p, p, p, 8, None) == -1 and b"workspace" in lib.mtts_last_error()
    assert lib.mtts_outer_batch_sum(p, p, 1, 4, 8, None, p, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_outer_batch_sum(p, p, 0, 4, 8, p, p, None) == -1 and b"shape" in lib.mtts_last_error()


@pytest.mark.parametrize("size", ["tiny", "prod"])
def test_component_from_the_flat_vector_equals_the_one_from_registered_tensors(lib, hparams, synthetic, size):
    """Packing from h_params equal to the registered tensors gives the bytes of packing with h_params == NULL; other parameters give
    other bytes at the same size; and neither touches the model's own packed image."""
    hip = sub("_hip")
    hp = hparams.tiny(n_spks=2) if size == "tiny" else hparams.prod_v20(n_spks=2)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    model = hip.HipModel(hp)
    for k, v in sd.items():
        if k.startswith(R.PREFIX):
            model._set(k, v)
    flat = R.flatten(R.params_of(sd, hp, torch.float32), hp).numpy().copy()
    nb = lib.mtts_dp_train_weights_bytes(model.ctx)
    a, b, c = (np.full(nb, 0xA5, dtype=np.uint8) for _ in range(3))
    hip.check(lib.mtts_dp_train_pack(model.ctx, None, a.ctypes.data, nb))
    hip.check(lib.mtts_dp_train_pack(model.ctx, flat.ctypes.data, b.ctypes.data, nb))
    assert np.array_equal(a, b)
    assert lib.mtts_dp_train_weights_bytes(model.ctx) == nb
    flat[R.layout(hp)[2][1]] += 1.0                                                # one weight of conv_layers.0
    hip.check(lib.mtts_dp_train_pack(model.ctx, flat.ctypes.data, c.ctypes.data, nb))
    assert not np.array_equal(a, c)
    if size == "prod":
        assert nb < 4 * 1024 * 1024                                                # a small component of its own, not the model's image


def test_python_surface():
    header = (ROOT / "include" / "mtts.h").read_text()
    hip = sub("_hip")
    assert "dp_grad.hip" in hip.SOURCES and "NOT bit-equal" in header and "dropout-free" in header
    for method in ("dp_params", "dp_train_buffer", "dp_grad", "dp_grad_status", "update_tensors", "dp_layout"):
        assert callable(getattr(hip.HipModel, method)), method
    inf = sub("inference").MatchaTTSInfer
    assert callable(inf.duration_grad) and "dropout" in inf.duration_grad.__doc__
    D = sub("duration")
    for method in ("step", "fit", "commit", "save"):
        assert callable(getattr(D.DurationTrainer, method)), method
    assert D.is_decayed("conv_layers.0.weight") and D.is_decayed("spk_proj.weight") and D.is_decayed("proj.weight")
    assert not any(D.is_decayed(k) for k in ("conv_layers.0.bias", "norm_layers.1.gamma", "norm_layers.1.beta", "proj.bias", "spk_proj.bias"))
    assert (ROOT / "tools" / "finetune_durations.py").exists()

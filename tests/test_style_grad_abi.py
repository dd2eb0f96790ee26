"""The style encoder's parameter gradients without a GPU: the new C entries are bound, every host-side refusal, the flat parameter
layout, and the yardsticks themselves -- the restatements of tests/style_grad_restated.py against independent torch code."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, sub
import style_grad_restated as R

ENTRIES = ["mtts_style_param_count", "mtts_style_param_offset", "mtts_style_grad_weights_bytes", "mtts_style_grad_upload_weights",
           "mtts_style_grad_workspace_bytes", "mtts_style_grad_tape_offset", "mtts_style_forward_taped", "mtts_style_backward",
           "mtts_conv_wgrad_chunk_rows", "mtts_conv_wgrad_workspace_bytes", "mtts_conv_wgrad", "mtts_spk_grad_match_workspace_bytes",
           "mtts_spk_grad_match", "mtts_spk_grad_match_status", "mtts_match_seeds_scratch_bytes", "mtts_match_seeds"]


@pytest.fixture(scope="module")
def lib():
    return sub("_hip").load()


def make_ctx(lib, cfg):
    ctx = lib.mtts_style_create(*cfg)
    assert ctx
    return ctx


def test_entries_declared_bound_and_built(lib):
    # (arity and types: test_abi.py checks them for every entry of the header)
    header = (ROOT / "include" / "mtts.h").read_text()
    hip = sub("_hip")
    assert "MTTS_ABI_VERSION 2" in header and lib.mtts_abi_version() == 2          # additive: no bump
    assert "style_grad.hip" in hip.SOURCES
    for name in ENTRIES:
        assert name + "(" in header, name
        assert getattr(lib, name).argtypes is not None, name
    style = sub("style").StyleEncoder
    for method in ("forward_taped", "backward", "parameter_views", "parameter_layout", "mark_updated"):
        assert callable(getattr(style, method)), method
    for method in ("step", "fit", "save"):
        assert callable(getattr(sub("style").StyleTrainer, method)), method
    assert callable(hip.HipModel.speaker_grad_match) and callable(sub("inference").MatchaTTSInfer.style_match_grad)
    assert (ROOT / "tools" / "train_style_encoder.py").exists()
    assert "stays with the reference" not in sub("style").__doc__


def test_host_visible_refusals_need_no_device(lib):
    """Every refusal the header lists, before anything is launched (a fake non-null pointer is never dereferenced)."""
    p = C.c_void_p(256)
    big = 1 << 40
    ctx = make_ctx(lib, (20, 32, 2, 16))
    try:
        def wgrad(dz=p, x=p, B=2, T=8, cin=20, ldx=20, cout=32, dw=p, ws=p, n=big):
            return lib.mtts_conv_wgrad(dz, x, None, B, T, cin, ldx, cout, dw, None, ws, n, None)
        for kw in (dict(dz=None), dict(x=None), dict(dw=None), dict(ws=None)):
            assert wgrad(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
        for kw in (dict(B=0), dict(T=0), dict(cin=0), dict(cout=0), dict(ldx=19)):
            assert wgrad(**kw) == -1 and b"bad shape" in lib.mtts_last_error(), kw
        need = lib.mtts_conv_wgrad_workspace_bytes(2, 8, 20, 32)
        assert need == 4 * (5 * 20 * 32 + 32)                                          # one chunk
        assert wgrad(n=need - 4) == -1 and b"workspace" in lib.mtts_last_error()
        assert lib.mtts_conv_wgrad_workspace_bytes(0, 8, 20, 32) < 0

        def taped(c=ctx, mel=p, ln=p, B=2, T=8, ee=p, ed=p, ws=p, n=big):
            return lib.mtts_style_forward_taped(c, mel, ln, B, T, ee, ed, ws, n, None)
        for kw in (dict(c=None), dict(mel=None), dict(ln=None), dict(ee=None), dict(ed=None), dict(ws=None)):
            assert taped(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
        assert taped(B=0) == -1 and b"bad shape" in lib.mtts_last_error()
        assert taped(T=0) == -1 and b"bad shape" in lib.mtts_last_error()
        need = lib.mtts_style_grad_workspace_bytes(ctx, 2, 8)
        assert need > lib.mtts_style_workspace_bytes(ctx, 2, 8)                        # the tape and the backward's buffers
        assert taped(n=need - 512) == -1 and b"workspace" in lib.mtts_last_error()
        assert taped(n=need) == -1 and b"not uploaded" in lib.mtts_last_error()

        def back(c=ctx, ln=p, B=2, T=8, ge=p, gd=p, out=p, gb=p, ws=p, n=big):
            return lib.mtts_style_backward(c, ln, B, T, ge, gd, out, gb, ws, n, None)
        for kw in (dict(c=None), dict(ln=None), dict(ge=None), dict(gd=None), dict(out=None), dict(gb=None), dict(ws=None)):
            assert back(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
        assert back(B=0) == -1 and b"bad shape" in lib.mtts_last_error()
        assert back(n=need - 512) == -1 and b"workspace" in lib.mtts_last_error()
        assert back(n=need) == -1 and b"backward panels not uploaded" in lib.mtts_last_error()
        sizes = [lib.mtts_style_grad_workspace_bytes(ctx, B, T) for B, T in ((1, 8), (1, 300), (4, 300))]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        assert lib.mtts_style_grad_workspace_bytes(None, 1, 8) < 0 and lib.mtts_style_grad_workspace_bytes(ctx, 0, 8) < 0
        offs = [lib.mtts_style_grad_tape_offset(ctx, 2, 8, w) for w in range(5)]        # x, h0, h1, pooled, mask
        assert offs[0] < offs[4] < offs[1] < offs[2] < offs[3] < need
        assert lib.mtts_style_grad_tape_offset(ctx, 2, 8, 5) < 0 and lib.mtts_style_grad_tape_offset(ctx, 2, 8, -1) < 0
        assert lib.mtts_style_grad_weights_bytes(ctx) < 0 and b"missing tensor" in lib.mtts_last_error()     # nothing registered yet
        assert lib.mtts_style_grad_weights_bytes(None) < 0
        assert lib.mtts_style_grad_upload_weights(ctx, None, 0) == -1 and b"null" in lib.mtts_last_error()
        assert lib.mtts_style_param_count(None) < 0 and lib.mtts_style_param_offset(ctx, None) < 0
        assert lib.mtts_style_param_offset(ctx, b"convs.2.weight") < 0 and b"no parameter" in lib.mtts_last_error()
    finally:
        lib.mtts_style_destroy(ctx)


def test_matching_loss_refusals_need_no_device(lib, hparams):
    """mtts_spk_grad_match refuses what mtts_spk_grad refuses, before anything is launched."""
    p = C.c_void_p(256)
    big = 1 << 40
    ctx = sub("_hip").HipModel(hparams.tiny(n_spks=2)).ctx            # a context without weights: enough for shapes and sizes

    def match(c=ctx, x=p, xl=p, ee=p, ed=p, mr=p, lr=p, bm=0.002, bl=0.004, B=2, Tx=4, ge=p, gd=p, a=p, r=p, gb=p, ws=p, n=big):
        return lib.mtts_spk_grad_match(c, x, xl, ee, ed, mr, lr, bm, bl, B, Tx, ge, gd, a, r, gb, ws, n, None)

    for kw in (dict(c=None), dict(x=None), dict(xl=None), dict(ee=None), dict(ed=None), dict(mr=None), dict(lr=None), dict(ge=None),
               dict(gd=None), dict(a=None), dict(r=None), dict(gb=None), dict(ws=None)):
        assert match(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
    assert match(B=0) == -1 and b"B must be" in lib.mtts_last_error()
    assert match(Tx=1025) == -1 and b"1024" in lib.mtts_last_error()
    assert match(bm=0.0) == -1 and b"beta" in lib.mtts_last_error()
    assert match(bl=-1.0) == -1 and b"beta" in lib.mtts_last_error()
    need = lib.mtts_spk_grad_match_workspace_bytes(ctx, 2, 4)
    assert need > 0 and lib.mtts_spk_grad_match_workspace_bytes(ctx, 4, 4) > need
    assert match(n=need - 512) == -1 and b"workspace" in lib.mtts_last_error()
    assert match(n=need) == -1 and b"backward panels not uploaded" in lib.mtts_last_error()
    for bad in ((0, 4), (1, 0), (1, 1025)):
        assert lib.mtts_spk_grad_match_workspace_bytes(ctx, *bad) < 0, bad
    assert lib.mtts_spk_grad_match_workspace_bytes(None, 1, 4) < 0
    assert lib.mtts_spk_grad_match_status(None, None) == -1
    # the unit entry of its seed and sum kernels
    def seeds(mu=p, B=2, F=3, Tx=4, Fd=2, bm=0.002, sc=p):
        return lib.mtts_match_seeds(mu, p, p, p, p, p, B, F, Tx, Fd, bm, 0.004, p, p, p, p, sc, None)
    assert seeds(mu=None) == -1 and b"null" in lib.mtts_last_error()
    assert seeds(sc=None) == -1 and b"null" in lib.mtts_last_error()
    assert seeds(Tx=1025) == -1 and b"1024" in lib.mtts_last_error()
    assert seeds(B=0) == -1 and seeds(bm=0.0) == -1 and b"beta" in lib.mtts_last_error()
    assert lib.mtts_match_seeds_scratch_bytes(2, 3) >= 256 + 16 + 24 and lib.mtts_match_seeds_scratch_bytes(0, 3) < 0


@pytest.mark.parametrize("cfg", [(100, 256, 4, 96), (20, 32, 2, 16), (4, 4, 1, 8)])
def test_flat_parameter_layout_is_the_state_dict(lib, cfg):
    """mtts_style_param_offset walks the reference's state dict: names, order and sizes as torch's own module has them."""
    model = sub("style").StyleEncoder(*cfg)
    ctx = make_ctx(lib, cfg)
    try:
        off = 0
        assert list(model.state_dict()) == R.param_names(cfg[2])
        for k, v in model.state_dict().items():
            assert lib.mtts_style_param_offset(ctx, k.encode()) == off, k
            off += v.numel()
        assert lib.mtts_style_param_count(ctx) == off == sum(p.numel() for p in model.parameters())
    finally:
        lib.mtts_style_destroy(ctx)


def test_backward_panels_pack_from_the_registered_tensors(lib):
    """The on-demand pack needs no device: stable size, at least every transposed weight of layers >= 1 once, invalidated by a new tensor."""
    cfg = (20, 32, 3, 16)
    torch.manual_seed(1)
    model = sub("style").StyleEncoder(*cfg)
    ctx = make_ctx(lib, cfg)
    try:
        import numpy as np
        for k, v in model.state_dict().items():
            a = np.ascontiguousarray(v.numpy())
            assert lib.mtts_style_set_tensor(ctx, k.encode(), a.ctypes.data, a.size) == 0
        n = lib.mtts_style_grad_weights_bytes(ctx)
        assert n >= 4 * 2 * 5 * 32 * 32 and lib.mtts_style_grad_weights_bytes(ctx) == n
        a = np.zeros(7, dtype=np.float32)
        assert lib.mtts_style_set_tensor(ctx, b"convs.1.weight", a.ctypes.data, a.size) == 0
        assert lib.mtts_style_grad_weights_bytes(ctx) < 0 and b"unexpected size" in lib.mtts_last_error()      # repacked: sees the new tensor
    finally:
        lib.mtts_style_destroy(ctx)


def test_chunk_length_is_a_function_of_the_shape(lib):
    for B, T in ((1, 1), (3, 85), (4, 64), (1, 257), (5, 103), (16, 256), (1, 4097), (32, 600), (64, 1000)):
        ch = lib.mtts_conv_wgrad_chunk_rows(B, T)
        assert ch == R.chunk_rows(B, T) and ch % 256 == 0 and -(-(B * T) // ch) <= 16, (B, T)
    assert R.chunk_rows(4, 64) == 256 and R.chunk_rows(32, 600) == 1280
    assert R.wgrad_serial_run(5, 103) == 256 + 2 and R.bias_serial_run(5, 103) == 64 + 3 + 2


@pytest.mark.parametrize("rows,chunk,chunks", [(4096, 256, 16), (4097, 512, 9), (8192, 512, 16), (8193, 768, 11), (19200, 1280, 15)])
def test_chunk_length_at_the_training_row_counts(lib, rows, chunk, chunks):
    """The values the GPU cases beyond one chunk length are built on, and the serial runs their bounds use."""
    B, T, lengths = R.WGRAD_ROWS[rows]
    assert B * T == rows and len(lengths) == B and max(lengths) == T and lengths[-1] == T
    for b, t in ((B, T), (1, rows)):
        assert lib.mtts_conv_wgrad_chunk_rows(b, t) == R.chunk_rows(b, t) == chunk
        assert -(-rows // R.chunk_rows(b, t)) == chunks
        assert R.wgrad_serial_run(b, t) == chunk + chunks - 1 and R.bias_serial_run(b, t) == chunk // 4 + 3 + chunks - 1
    assert lib.mtts_conv_wgrad_workspace_bytes(B, T, 20, 32) == 4 * chunks * (5 * 20 * 32 + 32)


def test_one_training_case_has_a_clip_boundary_on_no_slab_or_chunk_boundary():
    for rows in (8193, 19200):
        B, T, lengths = R.WGRAD_ROWS[rows]
        inner = [b * T for b in range(1, B) if lengths[b - 1] == T and lengths[b] > 0]       # live rows on either side
        assert any(r % 32 and r % R.chunk_rows(B, T) for r in inner), rows


# ------------------------------------------------------------------------------------------------ the yardsticks
def test_integer_wgrad_cases_are_exact_in_fp32():
    """The precondition of every exact GPU case of the weight-gradient entry: integer operands in [-2, 2], NaN where nothing may be
    read, and no element's sum of absolute terms reaches 2^24.  The chunked form adds up to the whole, exactly."""
    cases = [(R.WGRAD_ROWS[rows] + (cin, cout, rows + cin)) for rows, cin, cout in R.WGRAD_CASES]            # (the GPU cases' seeds)
    cases += [(B, T, R.short_lengths(B, T), cin, cout, B) for B, T, cin, cout in R.SHORT_CASES]
    cases += [(B, T, [T] * B, cin, cout, B) for B, T, cin, cout in R.SHORT_CASES]
    for B, T, lengths, cin, cout, seed in cases:
        dz, x = R.integer_wgrad_case(B, T, lengths, cin, cout, seed)
        assert dz.shape == (B, T, cout) and x.shape == (B, T, cin + 4) and dz.dtype == x.dtype == torch.float32
        live = R.prefix_mask(lengths, T).bool()
        assert torch.isnan(x[:, :, cin:]).all() and torch.isnan(x[~live]).all() and torch.isnan(dz[~live]).all()
        assert not torch.isnan(x[live][:, :cin]).any() and not torch.isnan(dz[live]).any()
        assert x[live][:, :cin].abs().max() <= 2 and dz[live].abs().max() <= 2
        sums = R.wgrad_abs_sums(dz, x[:, :, :cin], lengths)
        assert R.fp32_is_exact_on(sums, dz, x) and sums["dW"] > 0, (B, T, cin, cout, sums)
        whole, _ = R.conv_wgrad(dz, x[:, :, :cin], lengths)
        val, mag, bias, _ = R.conv_wgrad_by_chunk(dz, x[:, :, :cin], lengths, R.chunk_rows(B, T))
        assert val.shape[0] == -(-(B * T) // R.chunk_rows(B, T)) and R.is_integer(val) and (mag >= val.abs()).all()
        assert torch.equal(val.sum(0), whole) and torch.equal(bias.sum(0), torch.nan_to_num(dz.double()).sum((0, 1)))
    for B, T in R.SHORT_CLIPS:
        assert set(R.short_lengths(B, T)) == set(range(T + 1))
    assert not R.fp32_is_exact_on({"x": 2.0 ** 24}, torch.ones(1)) and not R.fp32_is_exact_on({"x": 1.0}, torch.tensor([0.5]))


@pytest.mark.parametrize("T", [1, 2, 3])
def test_triple_loop_is_the_matrix_form_on_clips_shorter_than_the_tap_span(T):
    """Integer operands, clips of 0 .. T frames: the plain definition and the matrix form agree exactly, also chunk by chunk (chunks
    of 4 rows: a clip boundary inside a chunk, a tap across a chunk boundary)."""
    B, cin, cout = 11, 3, 5
    lengths = [b % (T + 1) for b in range(B)]
    dz, x = R.integer_wgrad_case(B, T, lengths, cin, cout, T)
    x = x[:, :, :cin]
    loops = R.conv_wgrad_loops(torch.nan_to_num(dz).double(), torch.nan_to_num(x).double(), lengths)
    fast, mag = R.conv_wgrad(dz, x, lengths)
    assert torch.equal(loops, fast) and R.is_integer(fast) and fast.abs().max() > 0
    taps_alive = [k for k in range(5) if (fast[:, :, k] != 0).any()]
    assert taps_alive == list(range(max(0, 3 - T), min(5, 2 + T)))              # a 1-frame clip has its centre tap alone
    val, _, _, _ = R.conv_wgrad_by_chunk(dz, x, lengths, 4)
    for c in range(val.shape[0]):
        only = torch.nan_to_num(dz).double().reshape(B * T, cout).clone()
        only[:4 * c] = 0
        only[4 * c + 4:] = 0
        assert torch.equal(val[c], R.conv_wgrad_loops(only.reshape(B, T, cout), torch.nan_to_num(x).double(), lengths)), c


def tape_chain_by_autograd(sd, x0, hs, pooled, lengths, g_enc, g_dur):
    """The chain of backward_from_tape with every step's derivative taken by torch autograd of the forward operation (F.linear,
    F.conv1d) at the tape's activations, fp64."""
    L = R.n_layers_of(sd)
    T = x0.shape[1]
    mask = R.prefix_mask(lengths, T)[:, :, None]
    n = torch.as_tensor(lengths).double().clamp(min=1)
    out = {}
    pooled_leaf = pooled.double().clone().requires_grad_(True)
    proj = {k: sd[k].double().clone().requires_grad_(True) for k in R.param_names(L)[2 * L:]}
    e_enc = F.linear(pooled_leaf, proj["proj_enc.weight"], proj["proj_enc.bias"])
    e_dur = F.linear(pooled_leaf, proj["proj_dur.weight"], proj["proj_dur.bias"])
    ((e_enc * g_enc.double()).sum() + (e_dur * g_dur.double()).sum()).backward()
    out.update({k: v.grad for k, v in proj.items()})
    dz = pooled_leaf.grad[:, None, :] / n[:, None, None] * (hs[L - 1] > 0) * mask               # the mean pool, the ReLU, the mask
    for l in range(L - 1, -1, -1):
        xin = (hs[l - 1] if l else x0).double().clone().requires_grad_(True)
        w = sd[f"convs.{l}.weight"].double().clone().requires_grad_(True)
        b = sd[f"convs.{l}.bias"].double().clone().requires_grad_(True)
        (F.conv1d(xin.transpose(1, 2), w, b, padding=2).transpose(1, 2) * dz).sum().backward()
        out[f"convs.{l}.weight"], out[f"convs.{l}.bias"] = w.grad, b.grad
        if l:
            dz = xin.grad * (hs[l - 1] > 0) * mask
    return out


@pytest.mark.parametrize("cfg,B,T,lengths", [R.TAPE_CASES["tiny"], ((100, 24, 4, 96), 5, 40, [32, 0, 1, 16, 2])], ids=["tiny", "four-layers"])
def test_backward_from_an_integer_tape_is_integer_and_autograd_exactly(cfg, B, T, lengths):
    """The restatement the exact GPU cases of the whole backward are held to: on a hand-written integer tape every gradient is an
    integer, equal to step-by-step autograd with no tolerance (the GPU's tiny case itself, and four layers at a small size)."""
    sd, x0, hs, pooled, g_enc, g_dur = R.integer_tape_case(cfg, B, T, lengths, 5)
    m = R.prefix_mask(lengths, T, torch.float32)[:, :, None]
    assert all(set(v.unique().tolist()) <= {-1.0, 0.0, 1.0} for v in sd.values())
    assert 0.2 < (sd["convs.1.weight"] != 0).float().mean() < 0.3
    assert torch.equal(x0, x0 * m) and x0.abs().max() == 2 and all(torch.equal(h, h * m) and h.min() == 0 for h in hs)
    assert all(0.4 < (h[m.expand_as(h) > 0] == 0).float().mean() < 0.6 for h in hs) and pooled.min() >= 0
    sums = R.tape_abs_sums(sd, x0, hs, pooled, lengths, g_enc, g_dur)
    assert len(sums) == 4 + 1 + 2 * cfg[2] + cfg[2] - 1
    assert R.fp32_is_exact_on(sums, *sd.values(), x0, *hs, pooled, g_enc, g_dur), sums
    got, _ = R.backward_from_tape(sd, x0, hs, pooled, lengths, g_enc, g_dur)
    want = tape_chain_by_autograd(sd, x0, hs, pooled, lengths, g_enc, g_dur)
    for k in R.param_names(cfg[2]):
        assert R.is_integer(got[k]) and got[k].abs().max() > 0 and got[k].abs().max() <= sums[k], k
        assert torch.equal(got[k], want[k]), k


def test_the_gpu_tape_cases_are_exact_in_fp32():
    for name, (cfg, B, T, lengths) in R.TAPE_CASES.items():
        assert B * T == 4800 and R.chunk_rows(B, T) == 512 and 0 in lengths and 2 in lengths
        sd, x0, hs, pooled, g_enc, g_dur = R.integer_tape_case(cfg, B, T, lengths, 5)
        sums = R.tape_abs_sums(sd, x0, hs, pooled, lengths, g_enc, g_dur)
        assert R.fp32_is_exact_on(sums, *sd.values(), x0, *hs, pooled, g_enc, g_dur), (name, sums)


@pytest.mark.parametrize("cin,cout,lengths,T", [(7, 5, [9, 0, 1, 2, 4], 9), (4, 4, [3], 3)])
def test_triple_loop_is_autograd_of_conv1d(cin, cout, lengths, T):
    """The plain definition, its matrix form, and autograd of F.conv1d on the masked input agree (fp64)."""
    g = torch.Generator().manual_seed(cin)
    B = len(lengths)
    m = R.prefix_mask(lengths, T)[:, :, None]
    x = torch.randn(B, T, cin, generator=g, dtype=torch.float64) * m
    dz = torch.randn(B, T, cout, generator=g, dtype=torch.float64) * m
    w = torch.zeros(cout, cin, 5, dtype=torch.float64, requires_grad=True)
    # each clip alone and cut to its length: what "zero frames around every clip" means
    loss = 0
    for b, n in enumerate(lengths):
        if n:
            loss = loss + (F.conv1d(x[b:b + 1, :n].transpose(1, 2), w, padding=2) * dz[b:b + 1, :n].transpose(1, 2)).sum()
    loss.backward()
    loops = R.conv_wgrad_loops(dz, x, lengths)
    fast, mag = R.conv_wgrad(dz, x, lengths)
    assert (loops - w.grad).abs().max() <= 1e-13 * max(1.0, w.grad.abs().max())
    assert (fast - w.grad).abs().max() <= 1e-13 * max(1.0, w.grad.abs().max())
    assert (mag >= fast.abs() - 1e-13).all()


def test_backward_from_tape_is_autograd():
    """backward_from_tape on the fp64 forward's own activations equals fp64 autograd from the inputs, and its bounds are positive
    where the gradient is not identically zero."""
    cfg = (12, 8, 3, 6)
    torch.manual_seed(2)
    sd = {k: v.double() for k, v in sub("style").StyleEncoder(*cfg).state_dict().items()}
    lengths, T = [11, 5, 0, 2], 11
    g = torch.Generator().manual_seed(3)
    mel = torch.randn(4, cfg[0], T, generator=g, dtype=torch.float64)
    g_enc, g_dur = torch.randn(4, cfg[3], generator=g, dtype=torch.float64), torch.randn(4, cfg[3], generator=g, dtype=torch.float64)
    want, _ = R.style_param_grads(sd, mel, lengths, g_enc, g_dur)
    mask = R.prefix_mask(lengths, T)[:, None, :]
    x, hs = mel * mask, []
    x0 = x.transpose(1, 2)
    for i in range(cfg[2]):
        x = torch.relu(F.conv1d(x * mask, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], padding=2)) * mask
        hs.append(x.transpose(1, 2))
    pooled = x.sum(2) / mask.sum(2).clamp(min=1)
    got, bounds = R.backward_from_tape(sd, x0, hs, pooled, lengths, g_enc, g_dur)
    for k in R.param_names(cfg[2]):
        assert got[k].shape == want[k].shape == bounds[k].shape, k
        assert (got[k] - want[k]).abs().max() <= 1e-12 * max(1.0, want[k].abs().max()), k
        assert (bounds[k] >= 0).all() and bounds[k].max() > 0 and bounds[k].max() < 1e-3 * want[k].abs().max(), k


@pytest.mark.parametrize("beta", [0.002, 0.004, 0.5])
def test_smooth_l1_restated_is_torch(beta):
    d = torch.tensor([0.0, 0.3 * beta, -0.3 * beta, beta, -beta, 3 * beta, -7.0], dtype=torch.float64, requires_grad=True)
    mine = R.smooth_l1_sum(d, beta)
    ref = F.smooth_l1_loss(d, torch.zeros_like(d), beta=beta, reduction="sum")
    assert abs(mine.item() - ref.item()) <= 1e-15 * max(1.0, abs(ref.item()))
    ref.backward()
    assert torch.equal(R.smooth_l1_seed(d.detach(), beta), d.grad) or (R.smooth_l1_seed(d.detach(), beta) - d.grad).abs().max() <= 1e-15


def test_adamw_restated_is_torch():
    torch.manual_seed(4)
    p0 = torch.randn(50, dtype=torch.float64)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4)
    q, m, v = p0.clone(), torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64)
    for step in range(1, 6):
        g = torch.randn(50, dtype=torch.float64)
        p.grad = g.clone()
        opt.step()
        q, m, v = R.adamw_step(q, g, m, v, step)
        assert (q - p.detach()).abs().max() <= 1e-14, step

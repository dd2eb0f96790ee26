"""GPU parity of the estimator's kernels in the DEFAULT arithmetic (P16 images: fp16 head + scaled fp16 residual, three products per
MAC), kernel by kernel through the C ABI: gemm_p16_kernel MODE 0 with every epilogue form the decoder uses (mtts_gemm_p16_args_run),
MODE 1 (fast16), the three two-plane instantiations of attention_f32_kernel (mtts_attention_p16_run), gn_apply_kernel's two-plane
store (mtts_groupnorm_mish_p16) and the fp32 <-> P16 conversions (mtts_to_p16_roundtrip).

The reference is fp64 PyTorch on operands ALREADY PASSED THROUGH THE SPLIT (tests/p16_restated.py p16(); weights too; biases,
affines, SnakeBeta constants and masks stay fp32), so kernel and reference differ only by the fp32 accumulation order, the dropped
l.l term (2^-22 relative per product) and the roundings the kernel itself performs: the 2^-22 representation error of the operands
is NOT inside the bars.  Where a launch writes fp32 rows and a P16 image of the same values, the decoded image must equal
p16(out * out16_mask, out_lscale) BIT FOR BIT: that one assertion pins the rounding of both planes, the mask order and the
lane-to-column mapping of the packed stores.  Every test asserts the instantiation the launcher reports, so the set of kernels
covered is part of the test.  MODE 1 multiplies the head planes alone: its reference is fp64 on operands rounded to fp16 heads.

Measured on an MI355X (worst case over the cases below; every bar is below twice its figure and none is above the bar
tests/test_hip_kernels.py holds for the operation: 2e-6 sqrt(K), 1e-5, 3e-6, 5e-6):
  GEMM fp32 rows, |err| / (sqrt(K) max(|ref|, 1))                       MODE 0 1.68e-8   MODE 1 1.40e-8 (products of fp16 planes are exact in fp32)
  LayerNorm in the epilogue + SnakeBeta, |err| / max(|ref|, 1)          MODE 0 5.16e-7   MODE 1 5.45e-7
  GroupNorm + Mish (+ time rows) fp32 rows, |err| / max(|ref|, 1)       1.70e-7;  through the Block1D tail 2.83e-7
  row moments beside the rows: mean 2.30e-7 absolute, M2 1.73e-7 relative
  attention, |err| / max(|ref|, 1)                                      MODE 0 9.19e-7   MODE 1 1.36e-4 (probabilities and values as
                                                                        single fp16 products: the fp16 unit round-off, as the
                                                                        H16 kernels; tests/test_hip_kernels.py holds no bar for it)
P16 images carry no figure of their own: each is bit for bit the split of fp32 rows that are bounded above."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import sub
from p16_restated import heads, image_bits, p16

pytestmark = pytest.mark.gpu

# ---- bars (the figure behind each is in the module docstring's table and beside the number)
GEMM_TOL = {0: 3e-8, 1: 2.5e-8}             # measured 1.68e-8, 1.40e-8
LN_TOL = {0: 1.0e-6, 1: 1.0e-6}             # measured 5.16e-7, 5.45e-7
GN_TOL, GNR_TOL = 3.3e-7, 5.5e-7            # measured 1.70e-7 (gn_apply), 2.83e-7 (Block1D tail)
STAT_MEAN_TOL, STAT_M2_TOL = 4.5e-7, 3.4e-7  # measured 2.30e-7 (absolute), 1.73e-7 (relative)
ATT_TOL = {0: 1.8e-6, 1: 2.7e-4}            # measured 9.19e-7, 1.36e-4
MEASURED = {}
SEEN = set()


def tag_is(o, want):
    SEEN.add(o["tag"])
    assert o["tag"] == want, (o["tag"], want)


def note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    yield sub("_hip")
    print("\np16 kernel tests, worst figures measured:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def act(*shape, seed=0):
    """activations: non-zero mean and a per-channel spread (cancellation-friendly noise hides mean / variance mistakes)"""
    g = torch.Generator().manual_seed(seed)
    spread = 0.5 + 1.5 * torch.rand(shape[-1], generator=g)
    return ((torch.randn(*shape, generator=g) * spread) * 2 + 0.3).cuda()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def image_is_split_rows(o, mask=None, lscale=2048.0):
    """out16 == p16(out * out16_mask, out_lscale), bit for bit"""
    rows = o["out"] if mask is None else o["out"] * mask[:, None]
    return same_bits(o["out16"], p16(rows, lscale))


def rel_err(out, ref):
    return (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)


def gemm_tag(bm, ln, nst, gn=False, ks=1, mode=0):
    m16 = not (bm == 64 and nst == 4)
    tf = lambda b: "true" if b else "false"
    return f"gemm_p16_kernel<{bm}, {tf(ln)}, {nst}, {mode}, {tf(m16)}, {tf(gn)}, {ks}>"


def ragged_mask(B, T, step=7):
    lens = torch.tensor([T - step * i for i in range(B)])
    return (torch.arange(T)[None] < lens[:, None]).float().reshape(-1).cuda(), lens


def conv_ref(a, w, bias, B, T, pad, stride=1):
    x = a.double().view(B, T, -1).transpose(1, 2)
    y = F.conv1d(x, w.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    return y.transpose(1, 2).reshape(-1, w.shape[0])


def operand(t, mode):
    """what the kernel multiplies of a P16 operand: head + residual (MODE 0) or the head alone (MODE 1)"""
    return heads(t) if mode else t


# ------------------------------------------------------------------------------------------------ conversions
HARD = [0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -22, 1 + 2.0 ** -11 - 2.0 ** -22,
        1 + 3 * 2.0 ** -11 - 2.0 ** -23, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -12, 2.0 ** -3 + 2.0 ** -15, 2.0 ** -3 + 2.0 ** -24,
        2.0 ** -3 + 2.0 ** -25, 2.0 ** -3 + 3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -15), 6.1e-5, 65504.0, -65504.0,
        65504.0 - 16.0 + 2.0 ** -7, 1.0e-40, 2.0 ** -14 + 2.0 ** -26]


@pytest.mark.parametrize("lscale", [2048.0, 1.0])
def test_image_equals_the_restated_split_bitwise_mask_first_and_padding_columns(hip, lscale):
    M, C, ld, ld16, C_valid = 37, 128, 136, 320, 64
    x = act(M, ld, seed=1)
    hard = torch.tensor(HARD)
    x[0, :len(HARD)] = hard.cuda()
    x[4, 64:64 + len(HARD)] = hard.cuda()
    x[9, 32:32 + len(HARD)] = -hard.cuda()
    mask = (torch.arange(M) % 4 != 1).float().cuda()
    mask[6] = 0.3                                      # a mask that is not 0 / 1 shows the order: applied BEFORE the split
    for cv in (C, C_valid):
        o = hip.to_p16_roundtrip(x, mask, C_valid=cv, ld16=ld16, lscale=lscale, Cc=C)
        want = torch.zeros(M, C, device="cuda")
        want[:, :cv] = x[:, :cv] * mask[:, None]
        assert torch.equal(o["bits"][:, :2 * C].cpu(), image_bits(want.cpu(), lscale)), cv        # both planes, on the CPU restatement
        img = o["bits"][:, :2 * C].reshape(M, C // 32, 2, 32)
        assert (img[:, cv // 32:] == 0).all()                                       # columns [C_valid, C): heads and residuals +0
        assert (o["bits"][:, 2 * C:] == 0x7e7e).all()                               # nothing written beyond 2 * C
        assert same_bits(o["out"].cpu(), p16(want.cpu(), lscale))
        assert o["flag"] == 0
    assert (o["bits"][:, :2 * C].reshape(M, C // 32, 2, 32)[:, :, 1] != 0).any()       # really two planes
    # (the other order, split then mask then split, gives another value on the 0.3 row: the assertion above can tell them apart)
    other = p16(p16(x[:, :C_valid], lscale) * mask[:, None], lscale)
    assert not torch.equal(other[6], o["out"][6, :C_valid]) and torch.equal(other[0], o["out"][0, :C_valid])


def test_out_of_range_elements_clamp_and_raise_the_flag(hip):
    M, C = 9, 64
    x = act(M, C, seed=2)
    mask = torch.ones(M, device="cuda")
    mask[3] = 0.0
    x[3, 5] = 1.0e6                                     # masked away: not "kept"
    x[4, 40] = -7.0e4                                   # beyond C_valid below: not kept either
    o = hip.to_p16_roundtrip(x, mask, C_valid=32)
    assert o["flag"] == 0
    assert (o["out"][3] == 0).all() and (o["out"][:, 32:] == 0).all()
    x[7, 3], x[8, 9] = 7.0e4, -1.0e9
    o = hip.to_p16_roundtrip(x, mask)
    assert o["flag"] == 1
    assert o["out"][7, 3].item() == 65504.0 and o["out"][8, 9].item() == -65504.0 and o["out"][4, 40].item() == -65504.0
    assert torch.isfinite(o["out"]).all() and same_bits(o["out"], p16(x * mask[:, None]))
    assert hip.to_p16_roundtrip(x, mask, lscale=1.0)["flag"] == 1


# ------------------------------------------------------------------------------------------------ GEMM
LINEAR = [
    # B, T, C, N, force_bm, (BM, stages, KS) the launcher must choose; a k line is 32 channels here
    (3, 100, 384, 384, 0, (64, 3, 2)),          # linear + bias + fp32 residual; 15 tiles, 12 lines: split-K
    (2, 77, 256, 100, 0, (64, 3, 2)),           # N not a multiple of 128 (no image: N % 32 != 0)
    (8, 1000, 128, 1152, 128, (128, 2, 1)),     # the 128-row tile
    (4, 160, 1536, 384, 64, (64, 2, 1)),        # the two-stage 64-row tile
    (1, 5, 64, 4, 0, (64, 4, 1)),               # tiny: two lines of K (fewer than four never split), the 4-stage ring
    (2, 100, 160, 256, 0, (64, 4, 1)),          # five 32-k lines on a one-round grid: 4-stage ring, odd line count, no split
    (10, 640, 128, 384, 0, (64, 3, 1)),         # 300 tiles: the 3-stage ring
    (5, 1000, 128, 640, 0, (64, 3, 1)),         # 395 tiles, a partly filled last row tile
]


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "fast16"])
@pytest.mark.parametrize("B,T,C,N,bm,form", LINEAR)
def test_linear_bias_residual_vs_fp64_and_image_bitwise(hip, mode, B, T, C, N, bm, form):
    a, w = p16(act(B * T, C, seed=1)), p16(rnd(N, C, seed=2, scale=C ** -0.5))
    b, r = rnd(N, seed=3), rnd(B * T, N, seed=4) * 2 + 0.5
    ref = F.linear(operand(a, mode).double(), operand(w, mode).double(), b.double()) + r.double()
    img = N % 32 == 0
    o = hip.gemm_p16_args(a, w, b, B=B, T_in=T, res=r, force_bm=bm, want_p16=img, fast16=bool(mode))
    tag_is(o, gemm_tag(form[0], False, form[1], ks=form[2], mode=mode))
    assert o["wave_rows"] == form[0] // 2 and o["flag"] == 0
    e = rel_err(o["out"], ref) / math.sqrt(C)
    note(f"gemm_mode{mode}", e)
    assert 0.0 < e <= GEMM_TOL[mode], e
    if img:
        assert image_is_split_rows(o)
        assert rel_err(o["out16"], ref) > 0.0
    if mode:                                            # really the heads alone: far from the two-plane product
        full = F.linear(a.double(), w.double(), b.double()) + r.double()
        assert rel_err(o["out"], full) > 20 * rel_err(o["out"], ref)


def test_image_only_launch_equals_the_two_output_launch(hip):
    """The model mostly writes the image alone: the same bits as beside fp32 rows, with the image mask applied to the image only;
    the same with the unscaled residual plane the attention kernel reads."""
    B, T, C, N = 3, 100, 384, 384
    a, w, b = p16(act(B * T, C, seed=5)), p16(rnd(N, C, seed=6, scale=C ** -0.5)), rnd(N, seed=7)
    mask, _ = ragged_mask(B, T, 9)
    for lscale in (2048.0, 1.0):
        both = hip.gemm_p16_args(a, w, b, B=B, T_in=T, want_p16=True, out16_mask=mask, out_lscale=lscale)
        only = hip.gemm_p16_args(a, w, b, B=B, T_in=T, want_f32=False, want_p16=True, out16_mask=mask, out_lscale=lscale)
        tag_is(both, gemm_tag(64, False, 3, ks=2))
        tag_is(only, gemm_tag(64, False, 3, ks=2))
        assert image_is_split_rows(both, mask, lscale)
        assert same_bits(both["out16"], only["out16"])
        assert (both["out16"][mask == 0] == 0).all() and (both["out"][mask == 0] != 0).any()      # `out` stays unmasked
    assert not same_bits(both["out16"], p16(both["out"] * mask[:, None], 2048.0))                 # (the two scales differ in bits)


@pytest.mark.parametrize("C,c1,N,B,T,gn", [(128, 0, 384, 2, 130, False), (384, 0, 384, 2, 100, False), (768, 384, 384, 2, 100, False),
                                           (384, 0, 384, 3, 77, True), (768, 384, 384, 2, 64, True)])
def test_conv_k3_same_with_folded_mask_split_k_one_and_two_segments(hip, C, c1, N, B, T, gn):
    """k3 "same" conv: tap shift and sequence-end padding are DMA source addresses, the ragged mask is folded into the image by its
    producer.  K = 3 * 384 and 3 * 768 (a second channel segment: the up path's skip concat) run split-K (<= 256 tiles); with the
    GroupNorm statistics in the epilogue (GN instantiations) the output rows must be the same bits."""
    a, w, b = p16(act(B * T, C, seed=5)), p16(rnd(N, C, 3, seed=6, scale=(3 * C) ** -0.5)), rnd(N, seed=7)
    mask, _ = ragged_mask(B, T)
    ref = conv_ref(a * mask[:, None], w, b, B, T, 1)
    o = hip.gemm_p16_args(a, w, b, B=B, T_in=T, c1=c1, a_mask=mask, want_p16=True, out16_mask=mask, gn_groups=8 if gn else 0)
    tag_is(o, gemm_tag(64, False, 3, gn=gn, ks=2))
    e = rel_err(o["out"], ref) / math.sqrt(3 * C)
    note("gemm_mode0", e)
    assert 0.0 < e <= GEMM_TOL[0], e
    assert image_is_split_rows(o, mask)
    if gn:
        plain = hip.gemm_p16_args(a, w, b, B=B, T_in=T, c1=c1, a_mask=mask)
        tag_is(plain, gemm_tag(64, False, 3, ks=2))
        assert same_bits(plain["out"], o["out"])


def test_conv_stride2_down(hip):
    B, T, C, N = 2, 50, 64, 64
    a, w, b = p16(act(B * T, C, seed=8)), p16(rnd(N, C, 3, seed=9, scale=(3 * C) ** -0.5)), rnd(N, seed=10)
    ref = conv_ref(a, w, b, B, T, 1, stride=2)
    o = hip.gemm_p16_args(a, w, b, B=B, T_in=T, T_out=25, in_stride=2, want_p16=True)
    tag_is(o, gemm_tag(64, False, 3, ks=2))             # six 32-k lines: split-K
    e = rel_err(o["out"], ref) / math.sqrt(3 * C)
    note("gemm_mode0", e)
    assert 0.0 < e <= GEMM_TOL[0], e
    assert image_is_split_rows(o)


def test_upsampling_conv_interleaves_both_phases_into_one_buffer(hip):
    """ConvTranspose1d(k4, s2, p1) as two phase GEMMs whose rows interleave in one [B, 2T] buffer (out_T / out_stride / out_off):
    out[2j] = W1.x[j] + W3.x[j-1], out[2j+1] = W0.x[j+1] + W2.x[j].  Each launch must leave the other phase's rows alone."""
    B, T, C = 3, 45, 128
    x, wt, b = p16(act(B * T, C, seed=11)), p16(rnd(C, C, 4, seed=12, scale=(2 * C) ** -0.5)), rnd(C, seed=13)
    mask2, _ = ragged_mask(B, 2 * T, 11)
    ref = F.conv_transpose1d(x.double().view(B, T, C).transpose(1, 2), wt.double(), b.double(), stride=2, padding=1)
    ref = ref.transpose(1, 2).reshape(B * 2 * T, C) * mask2[:, None].double()
    out = torch.full((B * 2 * T, C), 777.0, device="cuda")
    out16 = torch.full((B * 2 * T, C), 3.0, device="cuda")
    for ph, tsel, taps in ((0, (1, 3), (0, -1)), (1, (0, 2), (1, 0))):
        w = torch.stack([wt[:, :, tsel[0]].t(), wt[:, :, tsel[1]].t()], dim=2).contiguous()        # Conv1d layout [N, C, 2]
        o = hip.gemm_p16_args(x, w, b, B=B, T_in=T, tap_off=list(taps), out_mask=mask2, out=out, out16=out16, out_T=2 * T, out_stride=2,
                              out_off=ph)
        tag_is(o, gemm_tag(64, False, 3, ks=2))
        if ph == 0:                                     # the odd rows still hold what they held
            assert (out.view(B, T, 2, C)[:, :, 1] == 777.0).all() and (out16.view(B, T, 2, C)[:, :, 1] == 3.0).all()
        else:                                           # ... and the second launch left the even rows of the first alone
            assert same_bits(out.view(B, T, 2, C)[:, :, 0], even_rows) and same_bits(out16.view(B, T, 2, C)[:, :, 0], even_img)
        even_rows, even_img = out.view(B, T, 2, C)[:, :, 0].clone(), out16.view(B, T, 2, C)[:, :, 0].clone()
    e = rel_err(out, ref) / math.sqrt(2 * C)
    note("gemm_mode0", e)
    assert 0.0 < e <= GEMM_TOL[0], e
    assert same_bits(out16, p16(out))


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "fast16"])
@pytest.mark.parametrize("B,T,form", [(2, 90, (64, 3, 2)), (2, 800, (64, 3, 1)), (8, 1000, (64, 2, 1))])
def test_layernorm_in_epilogue_snake_and_image(hip, mode, B, T, form):
    """LayerNorm as rstd * (x.W' - mean * rowsum(W')) from the producer's partial moments or from mean / rstd arrays (the statistics
    of the image's rows, in fp32), SnakeBeta, the result as fp32 rows and as an image, C = 384 -> N = 1536.  MODE 1 multiplies the
    heads alone while moments and row sums stay those of the full values (what the model feeds it): its reference is that algebra
    in fp64."""
    C, N = 384, 1536
    a = p16(act(B * T, C, seed=11))
    w, b = p16(rnd(N, C, seed=12, scale=C ** -0.5)), rnd(N, seed=13)
    alpha, beta = rnd(N, seed=14, scale=0.2), rnd(N, seed=15, scale=0.2)
    ad = a.double()
    s = ad.view(-1, 6, 64)
    part = torch.stack([s.mean(-1), ((s - s.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).float().contiguous()
    mu = ad.mean(1)
    var = ((ad - mu[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    if mode == 0:
        h = F.linear((ad - mu[:, None]) * rstd[:, None], w.double(), b.double())
    else:
        h = rstd[:, None] * (F.linear(heads(a).double(), heads(w).double()) - mu[:, None] * w.double().sum(1)[None]) + b.double()
    ae, ib = torch.exp(alpha), 1.0 / (torch.exp(beta) + 1e-9)
    ref = h + ib.double() * torch.sin(h * ae.double()) ** 2
    o = hip.gemm_p16_args(a, w, b, B=B, T_in=T, a_part=part, act=3, p0=ae, p1=ib, want_p16=True, fast16=bool(mode))
    tag_is(o, gemm_tag(form[0], True, form[1], ks=form[2], mode=mode))
    e = rel_err(o["out"], ref)
    note(f"ln_snake_mode{mode}", e)
    assert 0.0 < e <= LN_TOL[mode], e
    assert image_is_split_rows(o)
    o2 = hip.gemm_p16_args(a, w, b, B=B, T_in=T, a_mean=mu.float(), a_rstd=rstd.float(), act=3, p0=ae, p1=ib, want_p16=True, fast16=bool(mode))
    tag_is(o2, gemm_tag(form[0], True, form[1], ks=form[2], mode=mode))
    e2 = rel_err(o2["out"], ref)
    note(f"ln_snake_mode{mode}", e2)
    assert 0.0 < e2 <= LN_TOL[mode], e2
    assert image_is_split_rows(o2)


@pytest.mark.parametrize("B,T,form", [(2, 100, (64, 3, 2)), (10, 640, (64, 3, 1))])
def test_residual_image_in_place_with_row_moments(hip, B, T, form):
    """The residual-stream update: the residual is read from the very image the result is written to (res16 == out16), and the
    LayerNorm moments that leave with it are those of the fp32 rows of the same launch.  Against a separate residual image: same bits."""
    C = 384
    a, x = p16(act(B * T, C, seed=51)), p16(act(B * T, C, seed=52))
    w, b = p16(rnd(C, C, seed=53, scale=C ** -0.5)), rnd(C, seed=54)
    ref = F.linear(a.double(), w.double(), b.double()) + x.double()
    o = hip.gemm_p16_args(a, w, b, B=B, T_in=T, inplace=x, stats_out=True)
    tag_is(o, gemm_tag(form[0], False, form[1], ks=form[2]))
    e = rel_err(o["out"], ref) / math.sqrt(C)
    note("gemm_mode0", e)
    assert 0.0 < e <= GEMM_TOL[0], e
    assert image_is_split_rows(o)
    sep = hip.gemm_p16_args(a, w, b, B=B, T_in=T, res16=x, want_p16=True)
    tag_is(sep, gemm_tag(form[0], False, form[1], ks=form[2]))
    assert same_bits(sep["out"], o["out"]) and same_bits(sep["out16"], o["out16"])
    # a residual that is NOT a fixed point of the split is read as its split (the image is all the kernel sees)
    raw = act(B * T, C, seed=55)
    o3 = hip.gemm_p16_args(a, w, b, B=B, T_in=T, res16=raw)
    o4 = hip.gemm_p16_args(a, w, b, B=B, T_in=T, res16=p16(raw))
    assert same_bits(o3["out"], o4["out"]) and not same_bits(raw, p16(raw))
    xd = o["out"].double().view(B * T, 6, 64)
    m2 = ((xd - xd.mean(-1, keepdim=True)) ** 2).sum(-1)
    em = (o["stats"][:, :, 0].double() - xd.mean(-1)).abs().max().item()
    eq = ((o["stats"][:, :, 1].double() - m2).abs() / m2).max().item()
    note("stats_mean", em)
    note("stats_m2_rel", eq)
    assert 0.0 < em <= STAT_MEAN_TOL and 0.0 < eq <= STAT_M2_TOL, (em, eq)


def test_rows_do_not_leak_linear(hip):
    """Rolling the rows by 19 rolls the result bit for bit (same tile shape), and what masked rows hold changes nothing."""
    B, T, C, N = 3, 100, 384, 384
    a, w, b = p16(act(B * T, C, seed=21)), p16(rnd(N, C, seed=22, scale=C ** -0.5)), rnd(N, seed=23)
    r = p16(act(B * T, N, seed=24))
    mask = (torch.arange(B * T) % 6 != 2).float().cuda()
    run = lambda a_, r_, m_: hip.gemm_p16_args(a_, w, b, B=B, T_in=T, a_mask=m_, res16=r_, out_mask=m_, want_p16=True, out16_mask=m_)
    base = run(a, r, mask)
    tag_is(base, gemm_tag(64, False, 3, ks=2))
    rolled = run(a.roll(19, 0), r.roll(19, 0), mask.roll(19, 0))
    assert same_bits(rolled["out"], base["out"].roll(19, 0)) and same_bits(rolled["out16"], base["out16"].roll(19, 0))
    a2 = a.clone()
    a2[mask == 0] = 1.0e4 * act(int((mask == 0).sum()), C, seed=25)
    other = run(a2, r, mask)
    assert same_bits(other["out"], base["out"]) and same_bits(other["out16"], base["out16"])
    again = run(a, r, mask)
    assert same_bits(again["out"], base["out"]) and same_bits(again["out16"], base["out16"])
    assert (base["out16"][mask == 0] == 0).all()


def test_rows_do_not_leak_conv(hip):
    """k3 conv over ragged utterances: rolling the batch moves the result with it bit for bit (utterances of 77 rows sit at other tile
    offsets then), frames beyond an utterance's length and the neighbouring utterance never reach it."""
    B, T, C, N = 4, 77, 128, 384
    a, w, b = p16(act(B * T, C, seed=31)), p16(rnd(N, C, 3, seed=32, scale=(3 * C) ** -0.5)), rnd(N, seed=33)
    mask, lens = ragged_mask(B, T, 9)
    run = lambda a_, m_: hip.gemm_p16_args(a_, w, b, B=B, T_in=T, a_mask=m_, out_mask=m_, want_p16=True, out16_mask=m_)
    base = run(a, mask)
    tag_is(base, gemm_tag(64, False, 3, ks=2))
    roll = lambda t: t.view(B, T, -1).roll(1, 0).reshape(B * T, -1)
    rolled = run(roll(a), roll(mask[:, None])[:, 0].contiguous())
    assert same_bits(rolled["out"], roll(base["out"])) and same_bits(rolled["out16"], roll(base["out16"]))
    a2 = a.clone()
    a2[mask == 0] = -50.0
    other = run(a2, mask)
    assert same_bits(other["out"], base["out"]) and same_bits(other["out16"], base["out16"])
    # an utterance alone gives the same rows as inside the batch (last frame of b and first of b + 1 are neighbours in memory only)
    solo = hip.gemm_p16_args(a[T:2 * T].contiguous(), w, b, B=1, T_in=T, a_mask=mask[T:2 * T].contiguous(), out_mask=mask[T:2 * T].contiguous())
    assert solo["tag"] == base["tag"]
    assert same_bits(solo["out"], base["out"][T:2 * T])


def test_epilogue_range_clamps_and_flags(hip):
    """An epilogue value beyond +-65504: the image stores the clamp +-65504 (split_pair clamps before converting, as split_f16) with
    a zero residual and the launch raises the range flag; the fp32 rows keep the value.  A masked image row cannot raise it."""
    B, T, C, N = 2, 70, 128, 128
    a, w = p16(act(B * T, C, seed=41)), p16(rnd(N, C, seed=42, scale=C ** -0.5))
    b = rnd(N, seed=43)
    b[17], b[90] = 1.0e5, -2.0e5
    keep = torch.ones(B * T, device="cuda")
    o = hip.gemm_p16_args(a, w, b, B=B, T_in=T, want_p16=True, out16_mask=keep)
    tag_is(o, gemm_tag(64, False, 3, ks=2))
    assert o["flag"] == 1
    assert torch.isfinite(o["out16"]).all() and (o["out"][:, 17] > 9.0e4).all()
    assert (o["out16"][:, 17] == 65504.0).all() and (o["out16"][:, 90] == -65504.0).all()
    assert image_is_split_rows(o)
    b2 = rnd(N, seed=43)
    ok = hip.gemm_p16_args(a, w, b2, B=B, T_in=T, want_p16=True)
    assert ok["flag"] == 0
    none = hip.gemm_p16_args(a, w, b, B=B, T_in=T, want_p16=True, out16_mask=torch.zeros(B * T, device="cuda"))
    assert none["flag"] == 0 and (none["out16"] == 0).all()


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_ref(y, B, T, gamma, beta, mask, chbias=None, nrows=None, extra=None, eps=1e-5, G=8):
    """fp64 GroupNorm(8) + Mish + mask [+ chbias rows + mask] over y [B*T, C]; statistics over the first nrows[b] frames plus
    extra = (bias row [C], copies [B]) rows that exist only in the count."""
    C = y.shape[1]
    yd = y.double().view(B, T, G, C // G)
    out = torch.empty(B, T, C, dtype=torch.float64, device=y.device)
    for i in range(B):
        n = T if nrows is None else int(nrows[i])
        rows = yd[i, :n]
        if extra is not None and int(extra[1][i]) > 0:
            rows = torch.cat([rows, extra[0].double().view(1, G, C // G).expand(int(extra[1][i]), G, C // G)], 0)
        mu = rows.mean((0, 2))
        var = ((rows - mu[None, :, None]) ** 2).mean((0, 2))
        z = ((yd[i] - mu[None, :, None]) / torch.sqrt(var + eps)[None, :, None]).reshape(T, C) * gamma.double() + beta.double()
        out[i] = F.mish(z)
    out = out * mask.double().view(B, T, 1)
    if chbias is not None:
        cb = chbias.double()[:, :C].reshape(-1, 1, C) if chbias.dim() == 2 else chbias.double().view(1, 1, C)
        out = (out + cb) * mask.double().view(B, T, 1)
    return out.reshape(B * T, C)


GN_CASES = [
    # B, T, nrows (None = T), force_bm, (BM, stages, KS) of the conv that leaves the statistics
    (2, 128, None, 0, (64, 3, 2)),          # T a multiple of the wave-tile rows (32)
    (3, 77, None, 0, (64, 3, 2)),           # not a multiple: wave tiles span two utterances
    (4, 45, None, 0, (64, 3, 2)),           # shorter than a 64-row workgroup tile
    (3, 100, (100, 61, 33), 0, (64, 3, 2)),  # nrows < T
    (10, 640, None, 0, (64, 3, 1)),         # 300 tiles: the GN epilogue OFF the split-K path (the large-grid form of the B = 32 headline)
    (4, 200, (200, 131, 64, 190), 128, (128, 2, 1)),      # 128-row tiles: wave tiles of 64 rows
    (7, 333, (333, 300, 17, 333, 1, 200, 333), 128, (128, 2, 1)),
]


@pytest.mark.parametrize("B,T,nrows,bm,form", GN_CASES)
def test_groupnorm_from_conv_epilogue_statistics_p16_store(hip, B, T, nrows, bm, form):
    """Block1D: conv (bias-only epilogue, GroupNorm statistics per wave tile, utterance part and group slice) -> gn_apply from those
    entries: Mish, mask, the per-utterance time-embedding rows, mask -- fp32 rows against fp64 (statistics of the conv's fp32 rows),
    the P16 image bit for bit the split of the fp32 rows times the image mask.  The statistics pass (no tile entries) must agree."""
    C = 384
    a, w, b = p16(act(B * T, C, seed=61)), p16(rnd(C, C, 3, seed=62, scale=(3 * C) ** -0.5) * 1.5), rnd(C, seed=63)
    g, be = 1 + 0.1 * rnd(C, seed=64), 0.1 * rnd(C, seed=65)
    mask, _ = ragged_mask(B, T, 5)
    chb = rnd(B, C + 8, seed=66).contiguous()
    m16 = (torch.arange(B * T) % 7 != 3).float().cuda()
    nr = None if nrows is None else torch.tensor(nrows, dtype=torch.int32).cuda()
    conv = hip.gemm_p16_args(a, w, b, B=B, T_in=T, a_mask=mask, gn_groups=8, gn_nrows=nr, force_bm=bm)
    tag_is(conv, gemm_tag(form[0], False, form[1], gn=True, ks=form[2]))
    assert conv["wave_rows"] == form[0] // 2
    y = conv["out"]
    e = rel_err(y, conv_ref(a * mask[:, None], w, b, B, T, 1)) / math.sqrt(3 * C)
    note("gemm_mode0", e)
    assert 0.0 < e <= GEMM_TOL[0], e
    ref = gn_ref(y, B, T, g, be, mask, chb, nrows)
    o = hip.groupnorm_mish_p16(y, g, be, mask, B, T, chbias=chb, tile_stats=conv["gn_stats"], tile_rows=conv["wave_rows"], out16_mask=m16)
    e = rel_err(o["out"], ref)
    note("gn", e)
    assert 0.0 < e <= GN_TOL, e
    assert same_bits(o["out16"], p16(o["out"] * m16[:, None])) and o["flag"] == 0
    assert (o["out16"][m16 == 0] == 0).all() and (o["out"][m16 == 0] != 0).any()
    p = hip.groupnorm_mish_p16(y, g, be, mask, B, T, chbias=chb, nrows=nr, out16_mask=m16)
    e = rel_err(p["out"], ref)
    note("gn", e)
    assert 0.0 < e <= GN_TOL, e
    assert same_bits(p["out16"], p16(p["out"] * m16[:, None]))
    only = hip.groupnorm_mish_p16(y, g, be, mask, B, T, chbias=chb, tile_stats=conv["gn_stats"], tile_rows=conv["wave_rows"], out16_mask=m16,
                                  want_f32=False)
    assert same_bits(only["out16"], o["out16"])


@pytest.mark.parametrize("B,T,nrows,bm,form", [(2, 128, None, 0, (64, 3, 2)), (3, 77, None, 0, (64, 3, 2)), (3, 100, (100, 61, 70), 0, (64, 3, 2)),
                                               (10, 640, None, 0, (64, 3, 1)), (4, 200, (200, 131, 64, 190), 128, (128, 2, 1))])
def test_resnet_second_half_through_the_block1d_tail(hip, B, T, nrows, bm, form):
    """The second half of a ResNet block in two launches: conv2 leaves fp32 rows y and their tile statistics; the 1x1 residual conv's
    epilogue adds Mish(GroupNorm(y)) * mask, and writes the block's output as fp32 rows, as an image and with its LayerNorm moments.
    Against fp64 (statistics of the kernel's y).  The producing conv runs split-K, the 3-stage ring or 128-row tiles (wave tiles of
    32 or 64 rows: gnr_tile_rows)."""
    C = 384
    h, x = p16(act(B * T, C, seed=71)), p16(act(B * T, C, seed=72))
    w2, b2 = p16(rnd(C, C, 3, seed=73, scale=(3 * C) ** -0.5) * 1.5), rnd(C, seed=74)
    wr, br = p16(rnd(C, C, seed=75, scale=C ** -0.5)), rnd(C, seed=76)
    g, be = 1 + 0.1 * rnd(C, seed=77), 0.1 * rnd(C, seed=78)
    mask, _ = ragged_mask(B, T, 5)
    nr = None if nrows is None else torch.tensor(nrows, dtype=torch.int32).cuda()
    conv = hip.gemm_p16_args(h, w2, b2, B=B, T_in=T, a_mask=mask, gn_groups=8, gn_nrows=nr, force_bm=bm)
    tag_is(conv, gemm_tag(form[0], False, form[1], gn=True, ks=form[2]))
    assert conv["wave_rows"] == form[0] // 2
    y = conv["out"]
    ref = F.linear(x.double(), wr.double(), br.double()) + gn_ref(y, B, T, g, be, mask, None, nrows)
    o = hip.gemm_p16_args(x, wr, br, B=B, T_in=T, want_p16=True, stats_out=True,
                          gnr=dict(y=y, stats=conv["gn_stats"], tile_rows=conv["wave_rows"], groups=8, gamma=g, beta=be, mask=mask))
    tag_is(o, gemm_tag(64, False, 3, ks=1 if B * T > 4096 else 2))
    e = rel_err(o["out"], ref)
    note("gnr", e)
    assert 0.0 < e <= GNR_TOL, e
    assert image_is_split_rows(o)
    xd = o["out"].double().view(B * T, 6, 64)
    em = (o["stats"][:, :, 0].double() - xd.mean(-1)).abs().max().item()
    note("stats_mean", em)
    assert 0.0 < em <= STAT_MEAN_TOL, em


def test_folded_padding_equals_the_explicit_padded_rows(hip):
    """Folded padding: beyond an utterance's first padded frame the conv output is exactly its bias row, so those frames enter the
    GroupNorm statistics in closed form (nextra copies, bias_stats) instead of existing.  Against the explicit padded rows, through
    gn_apply and through the Block1D tail."""
    B, T, C = 3, 96, 384
    lens = [96, 70, 41]
    a, w, b = p16(act(B * T, C, seed=81)), p16(rnd(C, C, 3, seed=82, scale=(3 * C) ** -0.5) * 1.5), rnd(C, seed=83) * 0.5
    g, be = 1 + 0.1 * rnd(C, seed=84), 0.1 * rnd(C, seed=85)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float().reshape(-1).cuda()
    nr = torch.tensor([min(T, n + 1) for n in lens], dtype=torch.int32).cuda()
    ne = torch.tensor([T - min(T, n + 1) for n in lens], dtype=torch.int32).cuda()
    bg = b.double().view(8, C // 8)
    bias_stats = torch.stack([bg.mean(1), ((bg - bg.mean(1, keepdim=True)) ** 2).sum(1)], 1).float().contiguous()
    explicit = hip.gemm_p16_args(a, w, b, B=B, T_in=T, a_mask=mask, gn_groups=8)
    tag_is(explicit, gemm_tag(64, False, 3, gn=True, ks=2))
    y = explicit["out"]
    assert same_bits(y.view(B, T, C)[1, 71:], b.expand(T - 71, C).contiguous())        # the premise: exactly the bias row
    ref = gn_ref(y, B, T, g, be, mask)
    folded = hip.gemm_p16_args(a, w, b, B=B, T_in=T, a_mask=mask, gn_groups=8, gn_nrows=nr)
    assert same_bits(folded["out"], y)
    kw = dict(out16_mask=mask)
    o_exp = hip.groupnorm_mish_p16(y, g, be, mask, B, T, tile_stats=explicit["gn_stats"], tile_rows=explicit["wave_rows"], **kw)
    o_fold = hip.groupnorm_mish_p16(y, g, be, mask, B, T, tile_stats=folded["gn_stats"], tile_rows=folded["wave_rows"], nextra=ne, bias_stats=bias_stats, **kw)
    o_pass = hip.groupnorm_mish_p16(y, g, be, mask, B, T, nrows=nr, nextra=ne, bias_stats=bias_stats, **kw)
    for o in (o_exp, o_fold, o_pass):
        e = rel_err(o["out"], ref)
        note("gn", e)
        assert 0.0 < e <= GN_TOL, e
        assert same_bits(o["out16"], p16(o["out"] * mask[:, None]))
    # without the closed-form rows the statistics are visibly different: the test can see the fold
    wrong = hip.groupnorm_mish_p16(y, g, be, mask, B, T, tile_stats=folded["gn_stats"], tile_rows=folded["wave_rows"], **kw)
    assert rel_err(wrong["out"], ref) > 1000 * GN_TOL
    x = p16(act(B * T, C, seed=86))
    wr, br = p16(rnd(C, C, seed=87, scale=C ** -0.5)), rnd(C, seed=88)
    ref2 = F.linear(x.double(), wr.double(), br.double()) + ref
    gnr = dict(y=y, stats=folded["gn_stats"], tile_rows=folded["wave_rows"], groups=8, gamma=g, beta=be, mask=mask)
    tail = hip.gemm_p16_args(x, wr, br, B=B, T_in=T, want_p16=True, gnr=dict(gnr, nextra=ne, bias_stats=bias_stats))
    tag_is(tail, gemm_tag(64, False, 3, ks=2))
    e = rel_err(tail["out"], ref2)
    note("gnr", e)
    assert 0.0 < e <= GNR_TOL, e
    assert image_is_split_rows(tail)
    wrong_tail = hip.gemm_p16_args(x, wr, br, B=B, T_in=T, gnr=gnr)
    assert rel_err(wrong_tail["out"], ref2) > 1000 * GN_TOL


def test_gn_apply_range_clamps_and_flags(hip):
    """gn_apply's image store goes through split_f16: beyond +-65504 the image holds the clamp and the flag is raised, unless the
    image mask removes the row."""
    B, T, C = 2, 40, 128
    y = act(B * T, C, seed=91)
    g, be = 1 + 0.1 * rnd(C, seed=92), 0.1 * rnd(C, seed=93)
    mask = torch.ones(B * T, device="cuda")
    chb = torch.zeros(C, device="cuda")
    chb[33] = 9.0e4
    o = hip.groupnorm_mish_p16(y, g, be, mask, B, T, chbias=chb)
    assert o["flag"] == 1 and torch.isfinite(o["out16"]).all()
    assert same_bits(o["out16"], p16(o["out"]))
    assert (o["out16"][:, 33] == 65504.0).all() and (o["out"][:, 33] > 8.0e4).all()
    m16 = torch.zeros(B * T, device="cuda")
    assert hip.groupnorm_mish_p16(y, g, be, mask, B, T, chbias=chb, out16_mask=m16)["flag"] == 0
    chb[33] = 0.5
    assert hip.groupnorm_mish_p16(y, g, be, mask, B, T, chbias=chb)["flag"] == 0


# ------------------------------------------------------------------------------------------------ attention
def att_tag(nw, mode=0):
    return f"attention_f32_kernel<{nw}, true, {'true' if mode else 'false'}, false, false, {192 if nw == 6 else 64}>"


def att_ref(qkv, bias, B, T, H, scale, klen=None):
    """fp64 softmax(q k^T * scale + bias[key]) v; keys of utterance b are rows [0, klen[b])"""
    q, k, v = (t.view(B, T, H, 64).transpose(1, 2) for t in qkv.double().view(B * T, 3, H * 64).unbind(1))
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double().view(B, 1, 1, T)
    if klen is not None:
        dead = torch.arange(T, device=qkv.device)[None] >= klen.view(B, 1)
        s = s.masked_fill(dead.view(B, 1, 1, T), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, H * 64)


def att_case(B, T, H, seed):
    """q|k|v as the image the attention kernel reads holds them: split with UNSCALED residuals"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g)
    qkv[:, 2 * H * 64:] = qkv[:, 2 * H * 64:] * 1.5 + 0.4          # values with a mean: a wrong normaliser shows
    qkv[:, :H * 64] *= 1.3                                         # sharper softmax rows
    return p16(qkv.cuda(), 1.0)


ATT = [(2, 320, 6, 2), (1, 640, 2, 2), (32, 640, 6, 4), (4, 161, 6, 6), (2, 192, 3, 6), (3, 65, 2, 6),
       (2, 64, 6, 2), (2, 65, 6, 6), (1, 193, 6, 2), (2, 257, 6, 2), (1, 385, 6, 2), (12, 513, 6, 2)]


@pytest.mark.parametrize("B,T,H,nw", ATT)
def test_attention_vs_fp64_with_ragged_key_mask(hip, B, T, H, nw):
    """Additive key bias of the decoder (1 valid / 0 padded, reference transformer.py) over ragged lengths, against fp64; the output
    image is a fixed point of the split with its residual scale, for both scales."""
    qkv = att_case(B, T, H, 200 + T)
    mask, _ = ragged_mask(B, T, 13 if T > 64 * B else 3)
    ref = att_ref(qkv, mask, B, T, H, 0.125)
    o = hip.attention_p16_run(qkv, mask, B, T, H, 64, 0.125, 0)
    tag_is(o, att_tag(nw))
    e = rel_err(o["out"], ref)
    note("att_mode0", e)
    assert 0.0 < e <= ATT_TOL[0], e
    assert same_bits(o["out"], p16(o["out"])) and o["flag"] == 0
    again = hip.attention_p16_run(qkv, mask, B, T, H, 64, 0.125, 0)
    assert same_bits(again["out"], o["out"])
    if B <= 4:                                         # the image with unscaled residuals: the same rows, split with lscale 1
        o1 = hip.attention_p16_run(qkv, mask, B, T, H, 64, 0.125, 0, out_lscale=1.0)
        assert same_bits(o1["out"], p16(o1["out"], 1.0)) and o1["tag"] == o["tag"]
        e1 = rel_err(o1["out"], ref)
        note("att_mode0", e1)
        assert 0.0 < e1 <= ATT_TOL[0], e1
        # both are splits of the same fp32 rows, each within 2^-22 of them (an fp16-subnormal unscaled residual: 2^-25 absolute)
        assert ((o1["out"] - o["out"]).abs() <= 2.0 ** -21 * o["out"].abs() + 2.0 ** -24).all() and not same_bits(o1["out"], o["out"])


@pytest.mark.parametrize("B,T,H,nw,Tf", [(3, 320, 6, 2, 900), (4, 161, 6, 6, 500), (32, 640, 6, 4, 1600), (2, 130, 2, 6, 400)])
def test_attention_folded_padding_vs_explicit_padded_keys(hip, B, T, H, nw, Tf):
    """Folded padding: utterance b has klen[b] keys, the last of which stands for n_pad identical padded frames and carries the key
    bias ln(n_pad) (the reference gives each of them bias +0).  Against fp64 attention over the explicitly padded keys; keys at or
    beyond klen[b] and other utterances' rows must not reach an utterance's output, bit for bit."""
    qkv = att_case(B, T, H, 300 + T)
    lens = [T - 1 - (17 * i) % (T // 2) for i in range(B)]              # valid frames; row lens[b] is the folded one
    klen = torch.tensor([n + 1 for n in lens], dtype=torch.int32).cuda()
    bias = torch.zeros(B, T, device="cuda")
    big = torch.empty(B, Tf, 3 * H * 64, device="cuda")
    bias_big = torch.zeros(B, Tf, device="cuda")
    for i, n in enumerate(lens):
        bias[i, :n] = 1.0
        bias[i, n] = math.log(Tf - n)
        big[i, :n] = qkv.view(B, T, -1)[i, :n]
        big[i, n:] = qkv.view(B, T, -1)[i, n]
        bias_big[i, :n] = 1.0
    ref = att_ref(big.reshape(B * Tf, -1), bias_big.reshape(-1), B, Tf, H, 0.125).view(B, Tf, -1)[:, :T]
    o = hip.attention_p16_run(qkv, bias.reshape(-1).contiguous(), B, T, H, 64, 0.125, 0, klen=klen)
    tag_is(o, att_tag(nw))
    live = (torch.arange(T, device="cuda")[None] < klen[:, None]).view(B, T, 1)
    mag = max((ref.abs() * live).max().item(), 1.0)
    e = ((o["out"].view(B, T, -1).double() - ref).abs() * live).max().item() / mag
    note("att_mode0", e)
    assert 0.0 < e <= ATT_TOL[0], e
    # the ln(n_pad) bias matters at this bar: without it the same launch is far off
    plain = bias.clone()
    for i, n in enumerate(lens):
        plain[i, n] = 0.0
    off = hip.attention_p16_run(qkv, plain.reshape(-1).contiguous(), B, T, H, 64, 0.125, 0, klen=klen)
    assert ((off["out"].view(B, T, -1).double() - ref).abs() * live).max().item() / mag > 100 * ATT_TOL[0]
    # dead keys and foreign rows: other values, other bias, same bits on the live rows
    q2, b2 = qkv.clone().view(B, T, -1), bias.clone()
    for i, n in enumerate(lens):
        q2[i, n + 1:] = 30.0
        b2[i, n + 1:] = 5.0
    o2 = hip.attention_p16_run(q2.reshape(B * T, -1), b2.reshape(-1).contiguous(), B, T, H, 64, 0.125, 0, klen=klen)
    assert same_bits(torch.where(live, o2["out"].view(B, T, -1), 0.0), torch.where(live, o["out"].view(B, T, -1), 0.0))
    solo = hip.attention_p16_run(qkv.view(B, T, -1)[1].contiguous(), bias[1].contiguous(), 1, T, H, 64, 0.125, 0, klen=klen[1:2].contiguous())
    if B * H * ((T + 127) // 128) < 512:              # (the same query-block form for one utterance as for the batch)
        assert solo["tag"] == o["tag"]
        assert same_bits(solo["out"][:lens[1] + 1], o["out"].view(B, T, -1)[1, :lens[1] + 1])


@pytest.mark.parametrize("B,T,H,nw", [(2, 320, 6, 2), (32, 640, 6, 4), (4, 161, 6, 6)])
def test_attention_fast16_vs_fp64_on_the_heads(hip, B, T, H, nw):
    """MODE 1 of the attention kernel: single fp16 products on the head planes, one shape per instantiation, with klen."""
    qkv = att_case(B, T, H, 400 + T)
    mask, lens = ragged_mask(B, T, 13 if T > 64 * B else 3)
    klen = lens.to(torch.int32).cuda()
    ref = att_ref(heads(qkv), mask, B, T, H, 0.125, klen=klen)
    o = hip.attention_p16_run(qkv, mask, B, T, H, 64, 0.125, 0, klen=klen, fast16=True)
    tag_is(o, att_tag(nw, 1))
    live = (torch.arange(T, device="cuda")[None] < klen[:, None]).view(B * T, 1)
    e = ((o["out"].double() - ref).abs() * live).max().item() / max((ref.abs() * live).max().item(), 1.0)
    note("att_mode1", e)
    assert 0.0 < e <= ATT_TOL[1], e
    assert same_bits(o["out"], p16(o["out"])) and o["flag"] == 0


REQUIRED_FORMS = [(128, False, 2, False, 1), (64, False, 2, False, 1), (64, False, 3, False, 1), (64, False, 4, False, 1), (64, False, 3, False, 2),
                  (64, True, 3, False, 2), (64, False, 3, True, 2), (64, True, 3, False, 1), (64, True, 2, False, 1),
                  (64, False, 3, True, 1), (128, False, 2, True, 1)]


def test_every_p16_instantiation_was_launched(request):
    """Coverage of the file, by the tags the launchers reported, MODE 0: the 128-row tile, the 64-row tile with 2, 3 and 4 stages,
    split-K without and with LayerNorm, the GroupNorm-statistics epilogue on split-K, LayerNorm on the 2- and 3-stage tiles (the nine
    forms of the H16 file), the GroupNorm-statistics epilogue at KS = 1 on the 3-stage 64-row tile and on the 128-row tile, and the
    three attention kernels.  Each case above asserts its own tag; when the whole file ran (no -k, no node ids) the set seen is
    asserted."""
    required = {gemm_tag(bm, ln, nst, gn=gn, ks=ks) for bm, ln, nst, gn, ks in REQUIRED_FORMS} | {att_tag(nw) for nw in (2, 4, 6)}
    assert len(required) == 14
    assert {f for *_, f in LINEAR} >= {(128, 2, 1), (64, 2, 1), (64, 3, 1), (64, 4, 1), (64, 3, 2)} and {nw for *_, nw in ATT} == {2, 4, 6}
    print("\nP16 instantiations launched:\n  " + "\n  ".join(sorted(SEEN)))
    whole_file = not request.config.getoption("keyword") and not any("::" in str(a) for a in request.config.args)
    if whole_file:
        assert required <= SEEN, sorted(required - SEEN)

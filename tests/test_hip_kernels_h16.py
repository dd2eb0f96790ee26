"""GPU parity of the estimator's kernels in the 16-bit storage modes (mtts_set_arithmetic 16: fp16 planes, 17: bfloat16 planes),
kernel by kernel through the C ABI: gemm_p16_kernel MODE 2 / 3 with every epilogue form the decoder uses (mtts_gemm_h16), the six
H16 instantiations of attention_f32_kernel (mtts_attention_h16), gn_apply_kernel's H16 store (mtts_groupnorm_mish_h16) and the
fp32 <-> H16 conversions (mtts_to_h16_roundtrip).

The reference is fp64 PyTorch on operands ALREADY ROUNDED to the 16-bit type (biases, affines, SnakeBeta constants and masks stay
fp32), so kernel and reference differ only by the fp32 accumulation order and by the roundings the kernel itself performs.  Where a
launch writes fp32 rows and an H16 image of the same values, the image must equal the rounded rows BIT FOR BIT: that one assertion
pins the rounding mode, the mask order and the lane-to-column mapping of the packed stores.  Every test asserts the instantiation
the launcher reports, so the set of kernels covered is part of the test.

Measured on an MI355X (worst case over the cases below and both dtypes; every bar is below twice its figure):
  GEMM fp32 rows, |err| / (sqrt(K) max(|ref|, 1))                       1.68e-8   (products of 16-bit operands are exact in fp32)
  LayerNorm in the epilogue + SnakeBeta, |err| / max(|ref|, 1)          6.67e-7
  GroupNorm + Mish (+ time rows) fp32 rows, |err| / max(|ref|, 1)       1.85e-7;  through the Block1D tail 1.65e-7
  row moments beside the rows: mean 2.49e-7 absolute, M2 1.82e-7 relative
  attention, |err| / max|v|                                             2.88e-4 fp16 (0.59 u), 2.22e-3 bfloat16 (0.57 u),
                                                                        u = 2^-11 / 2^-8: under one unit round-off of max|v|
H16 images carry no figure of their own: each is bit for bit the rounding of fp32 rows that are bounded above."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import sub

pytestmark = pytest.mark.gpu

BF = pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
DT = {False: torch.float16, True: torch.bfloat16}
MODE = {False: 2, True: 3}
# ---- bars (the figure behind each is in the module docstring's table and beside the number)
GEMM_TOL = 3e-8                             # measured 1.68e-8
LN_TOL = 1.2e-6                             # measured 6.67e-7
GN_TOL = 3.5e-7                             # measured 1.85e-7 (gn_apply), 1.65e-7 (Block1D tail)
STAT_MEAN_TOL, STAT_M2_TOL = 4.5e-7, 3.5e-7  # measured 2.49e-7 (absolute), 1.82e-7 (relative)
ATT_TOL = {False: 5.5e-4, True: 4.2e-3}     # measured 2.88e-4, 2.22e-3
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
    print("\nh16 kernel tests, worst figures measured:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def act(*shape, seed=0):
    """activations: non-zero mean and a per-channel spread (cancellation-friendly noise hides mean / variance mistakes)"""
    g = torch.Generator().manual_seed(seed)
    spread = 0.5 + 1.5 * torch.rand(shape[-1], generator=g)
    return ((torch.randn(*shape, generator=g) * spread) * 2 + 0.3).cuda()


def to16(t, bf16):
    """fp32 -> the 16-bit value the library stores: round to nearest even; fp16 clamps to +-65504 first (split_f16)"""
    return (t if bf16 else t.clamp(-65504.0, 65504.0)).to(DT[bf16])


def r16(t, bf16):
    return None if t is None else to16(t, bf16).float()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def image_is_rounded_rows(o, bf16, mask=None):
    """out16 == (out * out16_mask).to(dtype), bit for bit (both widened to fp32)"""
    rows = o["out"] if mask is None else o["out"] * mask[:, None]
    return same_bits(o["out16"], r16(rows, bf16))


def rel_err(out, ref):
    return (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)


def gemm_tag(bf16, bm, ln, nst, gn=False, ks=1):
    m16 = not (bm == 64 and nst == 4)
    tf = lambda b: "true" if b else "false"
    return f"gemm_p16_kernel<{bm}, {tf(ln)}, {nst}, {MODE[bf16]}, {tf(m16)}, {tf(gn)}, {ks}>"


def ragged_mask(B, T, step=7):
    lens = torch.tensor([T - step * i for i in range(B)])
    return (torch.arange(T)[None] < lens[:, None]).float().reshape(-1).cuda(), lens


def conv_ref(a, w, bias, B, T, pad, stride=1):
    x = a.double().view(B, T, -1).transpose(1, 2)
    y = F.conv1d(x, w.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    return y.transpose(1, 2).reshape(-1, w.shape[0])


# ------------------------------------------------------------------------------------------------ conversions
@BF
def test_image_equals_torch_rounding_bitwise_mask_first_and_padding_columns(hip, bf16):
    M, C, ld, ld16, C_valid = 37, 128, 136, 192, 64
    x = act(M, ld, seed=1)
    hard = torch.tensor([0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8),
                         2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -15), 6.1e-5, 65504.0, -65504.0, 1.0e-40])
    x[0, :16] = hard.cuda()
    x[4, 64:80] = hard.cuda()
    mask = (torch.arange(M) % 4 != 1).float().cuda()
    mask[6] = 0.3                                      # a mask that is not 0 / 1 shows the order: applied BEFORE the rounding
    for cv in (C, C_valid):
        o = hip.to_h16_roundtrip(x, mask, C_valid=cv, ld16=ld16, bf16=bf16, Cc=C)
        want = torch.zeros(M, C, device="cuda")
        want[:, :cv] = x[:, :cv] * mask[:, None]
        want16 = to16(want, bf16)
        assert torch.equal(o["bits"][:, :C], want16.view(torch.int16)), cv
        assert (o["bits"][:, cv:C] == 0).all()                                      # columns [C_valid, C) are +0
        assert (o["bits"][:, C:] == 0x7e7e).all()                                   # nothing written beyond C
        assert same_bits(o["out"], want16.float())
        assert o["flag"] == 0
    # (the other order, round then mask then round, gives other bits on the 0.3 row: the assertion above can tell them apart)
    other = to16(to16(x[:, :C_valid], bf16).float() * mask[:, None], bf16).view(torch.int16)
    assert not torch.equal(other[6], o["bits"][6, :C_valid]) and torch.equal(other[0], o["bits"][0, :C_valid])


@BF
def test_out_of_range_elements_clamp_and_raise_the_flag_for_fp16_only(hip, bf16):
    M, C = 9, 64
    x = act(M, C, seed=2)
    mask = torch.ones(M, device="cuda")
    mask[3] = 0.0
    x[3, 5] = 1.0e6                                     # masked away: not "kept"
    x[4, 40] = -7.0e4                                   # beyond C_valid below: not kept either
    o = hip.to_h16_roundtrip(x, mask, C_valid=32, bf16=bf16)
    assert o["flag"] == 0
    assert (o["out"][3] == 0).all() and (o["out"][:, 32:] == 0).all()
    x[7, 3], x[8, 9] = 7.0e4, -1.0e9
    o = hip.to_h16_roundtrip(x, mask, bf16=bf16)
    assert o["flag"] == (0 if bf16 else 1)
    if bf16:                                            # bfloat16 keeps the fp32 range
        assert same_bits(o["out"], (x * mask[:, None]).to(torch.bfloat16).float())
    else:                                               # the clamp, where torch alone gives inf
        assert o["out"][7, 3].item() == 65504.0 and o["out"][8, 9].item() == -65504.0 and o["out"][4, 40].item() == -65504.0
        assert torch.isinf((x * mask[:, None]).to(torch.float16)).sum().item() == 3
        assert torch.isfinite(o["out"]).all()


# ------------------------------------------------------------------------------------------------ GEMM
LINEAR = [
    # B, T, C, N, force_bm, (BM, stages, KS) the launcher must choose
    (3, 100, 384, 384, 0, (64, 3, 2)),          # linear + bias + fp32 residual; 15 tiles, 6 lines: split-K
    (2, 77, 256, 100, 0, (64, 3, 2)),           # N not a multiple of 128 (no image: N % 64 != 0)
    (8, 1000, 128, 1152, 128, (128, 2, 1)),     # the 128-row tile
    (4, 160, 1536, 384, 64, (64, 2, 1)),        # the two-stage 64-row tile
    (1, 5, 64, 4, 0, (64, 4, 1)),               # tiny: one line of K, the 4-stage ring
    (2, 100, 192, 256, 0, (64, 4, 1)),          # three 64-k lines on a one-round grid: 4-stage ring, odd line count, no split
    (10, 640, 128, 384, 0, (64, 3, 1)),         # 300 tiles: the 3-stage ring
    (5, 1000, 128, 640, 0, (64, 3, 1)),         # 395 tiles, a partly filled last row tile
]


@BF
@pytest.mark.parametrize("B,T,C,N,bm,form", LINEAR)
def test_linear_bias_residual_vs_fp64_and_image_bitwise(hip, bf16, B, T, C, N, bm, form):
    a, w = r16(act(B * T, C, seed=1), bf16), r16(rnd(N, C, seed=2, scale=C ** -0.5), bf16)
    b, r = rnd(N, seed=3), rnd(B * T, N, seed=4) * 2 + 0.5
    ref = F.linear(a.double(), w.double(), b.double()) + r.double()
    img = N % 64 == 0
    o = hip.gemm_h16(a, w, b, B=B, T_in=T, res=r, force_bm=bm, want_h16=img, bf16=bf16)
    tag_is(o, gemm_tag(bf16, form[0], False, form[1], ks=form[2]))
    assert o["wave_rows"] == form[0] // 2 and o["flag"] == 0
    e = rel_err(o["out"], ref) / math.sqrt(C)
    note("gemm", e)
    assert e <= GEMM_TOL, e
    if img:
        assert image_is_rounded_rows(o, bf16)
        assert rel_err(o["out16"], ref) > 0.0           # really 16-bit values


@BF
def test_image_only_launch_equals_the_two_output_launch(hip, bf16):
    """The model mostly writes the image alone: the same bits as beside fp32 rows, with the image mask applied to the image only."""
    B, T, C, N = 3, 100, 384, 384
    a, w, b = r16(act(B * T, C, seed=5), bf16), r16(rnd(N, C, seed=6, scale=C ** -0.5), bf16), rnd(N, seed=7)
    mask, _ = ragged_mask(B, T, 9)
    both = hip.gemm_h16(a, w, b, B=B, T_in=T, want_h16=True, out16_mask=mask, bf16=bf16)
    only = hip.gemm_h16(a, w, b, B=B, T_in=T, want_f32=False, want_h16=True, out16_mask=mask, bf16=bf16)
    assert image_is_rounded_rows(both, bf16, mask)
    assert same_bits(both["out16"], only["out16"])
    assert (both["out16"][mask == 0] == 0).all() and (both["out"][mask == 0] != 0).any()      # `out` stays unmasked


@BF
@pytest.mark.parametrize("C,c1,N,B,T,gn", [(128, 0, 384, 2, 130, False), (384, 0, 384, 2, 100, False), (768, 384, 384, 2, 100, False),
                                           (384, 0, 384, 3, 77, True), (768, 384, 384, 2, 64, True)])
def test_conv_k3_same_with_folded_mask_split_k_one_and_two_segments(hip, bf16, C, c1, N, B, T, gn):
    """k3 "same" conv: tap shift and sequence-end padding are DMA source addresses, the ragged mask is folded into the image by its
    producer.  K = 3 * 384 and 3 * 768 (a second channel segment: the up path's skip concat) run split-K (<= 256 tiles); with the
    GroupNorm statistics in the epilogue (GN instantiations) the output rows must be the same bits."""
    a, w, b = r16(act(B * T, C, seed=5), bf16), r16(rnd(N, C, 3, seed=6, scale=(3 * C) ** -0.5), bf16), rnd(N, seed=7)
    mask, _ = ragged_mask(B, T)
    ref = conv_ref(a * mask[:, None], w, b, B, T, 1)
    o = hip.gemm_h16(a, w, b, B=B, T_in=T, c1=c1, a_mask=mask, want_h16=True, out16_mask=mask, gn_groups=8 if gn else 0, bf16=bf16)
    tag_is(o, gemm_tag(bf16, 64, False, 3, gn=gn, ks=2))
    e = rel_err(o["out"], ref) / math.sqrt(3 * C)
    note("gemm", e)
    assert e <= GEMM_TOL, e
    assert image_is_rounded_rows(o, bf16, mask)
    if gn:
        plain = hip.gemm_h16(a, w, b, B=B, T_in=T, c1=c1, a_mask=mask, bf16=bf16)
        assert same_bits(plain["out"], o["out"])


@BF
def test_conv_stride2_down(hip, bf16):
    B, T, C, N = 2, 50, 64, 64
    a, w, b = r16(act(B * T, C, seed=8), bf16), r16(rnd(N, C, 3, seed=9, scale=(3 * C) ** -0.5), bf16), rnd(N, seed=10)
    ref = conv_ref(a, w, b, B, T, 1, stride=2)
    o = hip.gemm_h16(a, w, b, B=B, T_in=T, T_out=25, in_stride=2, want_h16=True, bf16=bf16)
    tag_is(o, gemm_tag(bf16, 64, False, 4))
    e = rel_err(o["out"], ref) / math.sqrt(3 * C)
    note("gemm", e)
    assert e <= GEMM_TOL, e
    assert image_is_rounded_rows(o, bf16)


@BF
def test_upsampling_conv_interleaves_both_phases_into_one_buffer(hip, bf16):
    """ConvTranspose1d(k4, s2, p1) as two phase GEMMs whose rows interleave in one [B, 2T] buffer (out_T / out_stride / out_off):
    out[2j] = W1.x[j] + W3.x[j-1], out[2j+1] = W0.x[j+1] + W2.x[j].  Each launch must leave the other phase's rows alone."""
    B, T, C = 3, 45, 128
    x, wt, b = r16(act(B * T, C, seed=11), bf16), r16(rnd(C, C, 4, seed=12, scale=(2 * C) ** -0.5), bf16), rnd(C, seed=13)
    mask2, _ = ragged_mask(B, 2 * T, 11)
    ref = F.conv_transpose1d(x.double().view(B, T, C).transpose(1, 2), wt.double(), b.double(), stride=2, padding=1)
    ref = ref.transpose(1, 2).reshape(B * 2 * T, C) * mask2[:, None].double()
    out = torch.full((B * 2 * T, C), 777.0, device="cuda")
    out16 = torch.full((B * 2 * T, C), 3.0, device="cuda")
    for ph, tsel, taps in ((0, (1, 3), (0, -1)), (1, (0, 2), (1, 0))):
        w = torch.stack([wt[:, :, tsel[0]].t(), wt[:, :, tsel[1]].t()], dim=2).contiguous()        # Conv1d layout [N, C, 2]
        o = hip.gemm_h16(x, w, b, B=B, T_in=T, tap_off=list(taps), out_mask=mask2, out=out, out16=out16, out_T=2 * T, out_stride=2,
                         out_off=ph, bf16=bf16)
        tag_is(o, gemm_tag(bf16, 64, False, 3, ks=2))
        if ph == 0:                                     # the odd rows still hold what they held
            assert (out.view(B, T, 2, C)[:, :, 1] == 777.0).all() and (out16.view(B, T, 2, C)[:, :, 1] == 3.0).all()
    e = rel_err(out, ref) / math.sqrt(2 * C)
    note("gemm", e)
    assert e <= GEMM_TOL, e
    assert same_bits(out16, r16(out, bf16))


@BF
@pytest.mark.parametrize("B,T,form", [(2, 90, (64, 3, 2)), (2, 800, (64, 3, 1)), (8, 1000, (64, 2, 1))])
def test_layernorm_in_epilogue_snake_and_image(hip, bf16, B, T, form):
    """LayerNorm as rstd * (x.W' - mean * rowsum(W')) from the producer's partial moments or from mean / rstd arrays (the statistics
    of the ROUNDED rows, in fp32), SnakeBeta, the result as fp32 rows and as an image, C = 384 -> N = 1536."""
    C, N = 384, 1536
    a = r16(act(B * T, C, seed=11), bf16)
    w, b = r16(rnd(N, C, seed=12, scale=C ** -0.5), bf16), rnd(N, seed=13)
    alpha, beta = rnd(N, seed=14, scale=0.2), rnd(N, seed=15, scale=0.2)
    ad = a.double()
    s = ad.view(-1, 6, 64)
    part = torch.stack([s.mean(-1), ((s - s.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).float().contiguous()
    mu = ad.mean(1)
    var = ((ad - mu[:, None]) ** 2).mean(1)
    h = F.linear((ad - mu[:, None]) / torch.sqrt(var + 1e-5)[:, None], w.double(), b.double())
    ae, ib = torch.exp(alpha), 1.0 / (torch.exp(beta) + 1e-9)
    ref = h + ib.double() * torch.sin(h * ae.double()) ** 2
    o = hip.gemm_h16(a, w, b, B=B, T_in=T, a_part=part, act=3, p0=ae, p1=ib, want_h16=True, bf16=bf16)
    tag_is(o, gemm_tag(bf16, form[0], True, form[1], ks=form[2]))
    e = rel_err(o["out"], ref)
    note("ln_snake", e)
    assert e <= LN_TOL, e
    assert image_is_rounded_rows(o, bf16)
    o2 = hip.gemm_h16(a, w, b, B=B, T_in=T, a_mean=mu.float(), a_rstd=(1.0 / torch.sqrt(var + 1e-5)).float(), act=3, p0=ae, p1=ib,
                      want_h16=True, bf16=bf16)
    e2 = rel_err(o2["out"], ref)
    note("ln_snake", e2)
    assert e2 <= LN_TOL, e2
    assert image_is_rounded_rows(o2, bf16)


@BF
@pytest.mark.parametrize("B,T,form", [(2, 100, (64, 3, 2)), (10, 640, (64, 3, 1))])
def test_residual_image_in_place_with_row_moments(hip, bf16, B, T, form):
    """The residual-stream update: the residual is read from the very image the result is written to (res16 == out16), and the
    LayerNorm moments that leave with it are those of the fp32 rows of the same launch.  Against a separate residual image: same bits."""
    C = 384
    a, x = r16(act(B * T, C, seed=51), bf16), r16(act(B * T, C, seed=52), bf16)
    w, b = r16(rnd(C, C, seed=53, scale=C ** -0.5), bf16), rnd(C, seed=54)
    ref = F.linear(a.double(), w.double(), b.double()) + x.double()
    o = hip.gemm_h16(a, w, b, B=B, T_in=T, inplace=x, stats_out=True, bf16=bf16)
    tag_is(o, gemm_tag(bf16, form[0], False, form[1], ks=form[2]))
    e = rel_err(o["out"], ref) / math.sqrt(C)
    note("gemm", e)
    assert e <= GEMM_TOL, e
    assert image_is_rounded_rows(o, bf16)
    sep = hip.gemm_h16(a, w, b, B=B, T_in=T, res16=x, want_h16=True, bf16=bf16)
    assert same_bits(sep["out"], o["out"]) and same_bits(sep["out16"], o["out16"])
    xd = o["out"].double().view(B * T, 6, 64)
    em = (o["stats"][:, :, 0].double() - xd.mean(-1)).abs().max().item()
    eq = ((o["stats"][:, :, 1].double() - ((xd - xd.mean(-1, keepdim=True)) ** 2).sum(-1)).abs() / ((xd - xd.mean(-1, keepdim=True)) ** 2).sum(-1)).max().item()
    note("stats_mean", em)
    note("stats_m2_rel", eq)
    assert em <= STAT_MEAN_TOL and eq <= STAT_M2_TOL, (em, eq)


@BF
def test_rows_do_not_leak_linear(hip, bf16):
    """Rolling the rows by 19 rolls the result bit for bit (same tile shape), and what masked rows hold changes nothing."""
    B, T, C, N = 3, 100, 384, 384
    a, w, b = r16(act(B * T, C, seed=21), bf16), r16(rnd(N, C, seed=22, scale=C ** -0.5), bf16), rnd(N, seed=23)
    r = r16(act(B * T, N, seed=24), bf16)
    mask = (torch.arange(B * T) % 6 != 2).float().cuda()
    run = lambda a_, r_, m_: hip.gemm_h16(a_, w, b, B=B, T_in=T, a_mask=m_, res16=r_, out_mask=m_, want_h16=True, out16_mask=m_, bf16=bf16)
    base = run(a, r, mask)
    rolled = run(a.roll(19, 0), r.roll(19, 0), mask.roll(19, 0))
    assert same_bits(rolled["out"], base["out"].roll(19, 0)) and same_bits(rolled["out16"], base["out16"].roll(19, 0))
    a2 = a.clone()
    a2[mask == 0] = 1.0e4 * act(int((mask == 0).sum()), C, seed=25)
    other = run(a2, r, mask)
    assert same_bits(other["out"], base["out"]) and same_bits(other["out16"], base["out16"])
    again = run(a, r, mask)
    assert same_bits(again["out"], base["out"]) and same_bits(again["out16"], base["out16"])
    assert (base["out16"][mask == 0] == 0).all()


@BF
def test_rows_do_not_leak_conv(hip, bf16):
    """k3 conv over ragged utterances: rolling the batch moves the result with it bit for bit (utterances of 77 rows sit at other tile
    offsets then), frames beyond an utterance's length and the neighbouring utterance never reach it."""
    B, T, C, N = 4, 77, 128, 384
    a, w, b = r16(act(B * T, C, seed=31), bf16), r16(rnd(N, C, 3, seed=32, scale=(3 * C) ** -0.5), bf16), rnd(N, seed=33)
    mask, lens = ragged_mask(B, T, 9)
    run = lambda a_, m_: hip.gemm_h16(a_, w, b, B=B, T_in=T, a_mask=m_, out_mask=m_, want_h16=True, out16_mask=m_, bf16=bf16)
    base = run(a, mask)
    roll = lambda t: t.view(B, T, -1).roll(1, 0).reshape(B * T, -1)
    rolled = run(roll(a), roll(mask[:, None])[:, 0].contiguous())
    assert same_bits(rolled["out"], roll(base["out"])) and same_bits(rolled["out16"], roll(base["out16"]))
    a2 = a.clone()
    a2[mask == 0] = -50.0
    other = run(a2, mask)
    assert same_bits(other["out"], base["out"]) and same_bits(other["out16"], base["out16"])
    # an utterance alone gives the same rows as inside the batch (last frame of b and first of b + 1 are neighbours in memory only)
    solo = hip.gemm_h16(a[T:2 * T].contiguous(), w, b, B=1, T_in=T, a_mask=mask[T:2 * T].contiguous(), out_mask=mask[T:2 * T].contiguous(), bf16=bf16)
    assert same_bits(solo["out"], base["out"][T:2 * T])


@BF
def test_epilogue_range_fp16_clamps_and_flags_bf16_rounds(hip, bf16):
    """An epilogue value beyond +-65504: the fp16 image stores the clamp +-65504 (split_pair clamps before converting, as split_f16)
    and the launch raises the range flag; the fp32 rows keep the value.  A masked image row cannot raise it.  bfloat16: no flag."""
    B, T, C, N = 2, 70, 128, 128
    a, w = r16(act(B * T, C, seed=41), bf16), r16(rnd(N, C, seed=42, scale=C ** -0.5), bf16)
    b = rnd(N, seed=43)
    b[17], b[90] = 1.0e5, -2.0e5
    keep = torch.ones(B * T, device="cuda")
    o = hip.gemm_h16(a, w, b, B=B, T_in=T, want_h16=True, out16_mask=keep, bf16=bf16)
    assert o["flag"] == (0 if bf16 else 1)
    assert torch.isfinite(o["out16"]).all() and (o["out"][:, 17] > 9.0e4).all()
    if bf16:
        assert same_bits(o["out16"], o["out"].to(torch.bfloat16).float())
    else:
        assert (o["out16"][:, 17] == 65504.0).all() and (o["out16"][:, 90] == -65504.0).all()
        assert image_is_rounded_rows(o, bf16)
    b2 = rnd(N, seed=43)
    ok = hip.gemm_h16(a, w, b2, B=B, T_in=T, want_h16=True, bf16=bf16)
    assert ok["flag"] == 0
    none = hip.gemm_h16(a, w, b, B=B, T_in=T, want_h16=True, out16_mask=torch.zeros(B * T, device="cuda"), bf16=bf16)
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
    # B, T, nrows (None = T), what
    (2, 128, None),          # T a multiple of the wave-tile rows (32)
    (3, 77, None),           # not a multiple: wave tiles span two utterances
    (4, 45, None),           # shorter than a 64-row workgroup tile
    (3, 100, (100, 61, 33)),  # nrows < T
]


@BF
@pytest.mark.parametrize("B,T,nrows", GN_CASES)
def test_groupnorm_from_conv_epilogue_statistics_h16_store(hip, bf16, B, T, nrows):
    """Block1D: conv (bias-only epilogue, GroupNorm statistics per wave tile, utterance part and group slice) -> gn_apply from those
    entries: Mish, mask, the per-utterance time-embedding rows, mask -- fp32 rows against fp64 (statistics of the conv's fp32 rows),
    the H16 image bit for bit the rounded fp32 rows times the image mask.  The statistics pass (no tile entries) must agree."""
    C = 384
    a, w, b = r16(act(B * T, C, seed=61), bf16), r16(rnd(C, C, 3, seed=62, scale=(3 * C) ** -0.5) * 1.5, bf16), rnd(C, seed=63)
    g, be = 1 + 0.1 * rnd(C, seed=64), 0.1 * rnd(C, seed=65)
    mask, _ = ragged_mask(B, T, 5)
    chb = rnd(B, C + 8, seed=66).contiguous()
    m16 = (torch.arange(B * T) % 7 != 3).float().cuda()
    nr = None if nrows is None else torch.tensor(nrows, dtype=torch.int32).cuda()
    conv = hip.gemm_h16(a, w, b, B=B, T_in=T, a_mask=mask, gn_groups=8, gn_nrows=nr, bf16=bf16)
    tag_is(conv, gemm_tag(bf16, 64, False, 3, gn=True, ks=2))
    y = conv["out"]
    e = rel_err(y, conv_ref(a * mask[:, None], w, b, B, T, 1)) / math.sqrt(3 * C)
    note("gemm", e)
    assert e <= GEMM_TOL, e
    ref = gn_ref(y, B, T, g, be, mask, chb, nrows)
    o = hip.groupnorm_mish_h16(y, g, be, mask, B, T, chbias=chb, tile_stats=conv["gn_stats"], tile_rows=conv["wave_rows"], out16_mask=m16, bf16=bf16)
    e = rel_err(o["out"], ref)
    note("gn", e)
    assert e <= GN_TOL, e
    assert same_bits(o["out16"], r16(o["out"] * m16[:, None], bf16)) and o["flag"] == 0
    p = hip.groupnorm_mish_h16(y, g, be, mask, B, T, chbias=chb, nrows=nr, out16_mask=m16, bf16=bf16)
    e = rel_err(p["out"], ref)
    note("gn", e)
    assert e <= GN_TOL, e
    assert same_bits(p["out16"], r16(p["out"] * m16[:, None], bf16))
    only = hip.groupnorm_mish_h16(y, g, be, mask, B, T, chbias=chb, tile_stats=conv["gn_stats"], tile_rows=conv["wave_rows"], out16_mask=m16,
                                  bf16=bf16, want_f32=False)
    assert same_bits(only["out16"], o["out16"])


@BF
@pytest.mark.parametrize("B,T,nrows", [(2, 128, None), (3, 77, None), (3, 100, (100, 61, 70))])
def test_resnet_second_half_through_the_block1d_tail(hip, bf16, B, T, nrows):
    """The second half of a ResNet block in two launches: conv2 leaves fp32 rows y and their tile statistics; the 1x1 residual conv's
    epilogue adds Mish(GroupNorm(y)) * mask, and writes the block's output as fp32 rows, as an image and with its LayerNorm moments.
    Against fp64 (statistics of the kernel's y)."""
    C = 384
    h, x = r16(act(B * T, C, seed=71), bf16), r16(act(B * T, C, seed=72), bf16)
    w2, b2 = r16(rnd(C, C, 3, seed=73, scale=(3 * C) ** -0.5) * 1.5, bf16), rnd(C, seed=74)
    wr, br = r16(rnd(C, C, seed=75, scale=C ** -0.5), bf16), rnd(C, seed=76)
    g, be = 1 + 0.1 * rnd(C, seed=77), 0.1 * rnd(C, seed=78)
    mask, _ = ragged_mask(B, T, 5)
    nr = None if nrows is None else torch.tensor(nrows, dtype=torch.int32).cuda()
    conv = hip.gemm_h16(h, w2, b2, B=B, T_in=T, a_mask=mask, gn_groups=8, gn_nrows=nr, bf16=bf16)
    y = conv["out"]
    ref = F.linear(x.double(), wr.double(), br.double()) + gn_ref(y, B, T, g, be, mask, None, nrows)
    o = hip.gemm_h16(x, wr, br, B=B, T_in=T, want_h16=True, stats_out=True, bf16=bf16,
                     gnr=dict(y=y, stats=conv["gn_stats"], tile_rows=conv["wave_rows"], groups=8, gamma=g, beta=be, mask=mask))
    tag_is(o, gemm_tag(bf16, 64, False, 3, ks=2))
    e = rel_err(o["out"], ref)
    note("gnr", e)
    assert e <= GN_TOL, e
    assert image_is_rounded_rows(o, bf16)
    xd = o["out"].double().view(B * T, 6, 64)
    em = (o["stats"][:, :, 0].double() - xd.mean(-1)).abs().max().item()
    note("stats_mean", em)
    assert em <= STAT_MEAN_TOL, em


@BF
def test_folded_padding_equals_the_explicit_padded_rows(hip, bf16):
    """Folded padding: beyond an utterance's first padded frame the conv output is exactly its bias row, so those frames enter the
    GroupNorm statistics in closed form (nextra copies, bias_stats) instead of existing.  Against the explicit padded rows, through
    gn_apply and through the Block1D tail."""
    B, T, C = 3, 96, 384
    lens = [96, 70, 41]
    a, w, b = r16(act(B * T, C, seed=81), bf16), r16(rnd(C, C, 3, seed=82, scale=(3 * C) ** -0.5) * 1.5, bf16), rnd(C, seed=83) * 0.5
    g, be = 1 + 0.1 * rnd(C, seed=84), 0.1 * rnd(C, seed=85)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float().reshape(-1).cuda()
    nr = torch.tensor([min(T, n + 1) for n in lens], dtype=torch.int32).cuda()
    ne = torch.tensor([T - min(T, n + 1) for n in lens], dtype=torch.int32).cuda()
    bg = b.double().view(8, C // 8)
    bias_stats = torch.stack([bg.mean(1), ((bg - bg.mean(1, keepdim=True)) ** 2).sum(1)], 1).float().contiguous()
    explicit = hip.gemm_h16(a, w, b, B=B, T_in=T, a_mask=mask, gn_groups=8, bf16=bf16)
    y = explicit["out"]
    assert same_bits(y.view(B, T, C)[1, 71:], b.expand(T - 71, C).contiguous())        # the premise: exactly the bias row
    ref = gn_ref(y, B, T, g, be, mask)
    folded = hip.gemm_h16(a, w, b, B=B, T_in=T, a_mask=mask, gn_groups=8, gn_nrows=nr, bf16=bf16)
    assert same_bits(folded["out"], y)
    kw = dict(out16_mask=mask, bf16=bf16)
    o_exp = hip.groupnorm_mish_h16(y, g, be, mask, B, T, tile_stats=explicit["gn_stats"], tile_rows=explicit["wave_rows"], **kw)
    o_fold = hip.groupnorm_mish_h16(y, g, be, mask, B, T, tile_stats=folded["gn_stats"], tile_rows=folded["wave_rows"], nextra=ne, bias_stats=bias_stats, **kw)
    o_pass = hip.groupnorm_mish_h16(y, g, be, mask, B, T, nrows=nr, nextra=ne, bias_stats=bias_stats, **kw)
    for o in (o_exp, o_fold, o_pass):
        e = rel_err(o["out"], ref)
        note("gn", e)
        assert e <= GN_TOL, e
        assert same_bits(o["out16"], r16(o["out"] * mask[:, None], bf16))
    # without the closed-form rows the statistics are visibly different: the test can see the fold
    wrong = hip.groupnorm_mish_h16(y, g, be, mask, B, T, tile_stats=folded["gn_stats"], tile_rows=folded["wave_rows"], **kw)
    assert rel_err(wrong["out"], ref) > 1000 * GN_TOL
    x = r16(act(B * T, C, seed=86), bf16)
    wr, br = r16(rnd(C, C, seed=87, scale=C ** -0.5), bf16), rnd(C, seed=88)
    ref2 = F.linear(x.double(), wr.double(), br.double()) + ref
    tail = hip.gemm_h16(x, wr, br, B=B, T_in=T, want_h16=True, bf16=bf16,
                        gnr=dict(y=y, stats=folded["gn_stats"], tile_rows=folded["wave_rows"], groups=8, gamma=g, beta=be, mask=mask, nextra=ne,
                                 bias_stats=bias_stats))
    e = rel_err(tail["out"], ref2)
    note("gnr", e)
    assert e <= GN_TOL, e
    assert image_is_rounded_rows(tail, bf16)


@BF
def test_gn_apply_range_fp16_clamps_and_flags_bf16_rounds(hip, bf16):
    """gn_apply's image store goes through split_f16: beyond +-65504 the fp16 image holds the clamp and the flag is raised, unless
    the image mask removes the row; bfloat16 rounds as usual and never flags."""
    B, T, C = 2, 40, 128
    y = act(B * T, C, seed=91)
    g, be = 1 + 0.1 * rnd(C, seed=92), 0.1 * rnd(C, seed=93)
    mask = torch.ones(B * T, device="cuda")
    chb = torch.zeros(C, device="cuda")
    chb[33] = 9.0e4
    o = hip.groupnorm_mish_h16(y, g, be, mask, B, T, chbias=chb, bf16=bf16)
    assert o["flag"] == (0 if bf16 else 1) and torch.isfinite(o["out16"]).all()
    assert same_bits(o["out16"], r16(o["out"], bf16))
    if not bf16:
        assert (o["out16"][:, 33] == 65504.0).all()
    m16 = torch.zeros(B * T, device="cuda")
    assert hip.groupnorm_mish_h16(y, g, be, mask, B, T, chbias=chb, out16_mask=m16, bf16=bf16)["flag"] == 0


# ------------------------------------------------------------------------------------------------ attention
def att_tag(bf16, nw):
    return f"attention_f32_kernel<{nw}, true, true, true, {'true' if bf16 else 'false'}, {192 if nw == 6 else 64}>"


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


def att_case(B, T, H, seed, bf16):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g)
    qkv[:, 2 * H * 64:] = qkv[:, 2 * H * 64:] * 1.5 + 0.4          # values with a mean: a wrong normaliser shows
    qkv[:, :H * 64] *= 1.3                                         # sharper softmax rows
    return r16(qkv.cuda(), bf16)


ATT = [(2, 320, 6, 2), (1, 640, 2, 2), (32, 640, 6, 4), (4, 161, 6, 6), (2, 192, 3, 6), (3, 65, 2, 6),
       (2, 64, 6, 2), (2, 65, 6, 6), (1, 193, 6, 2), (2, 257, 6, 2), (1, 385, 6, 2), (12, 513, 6, 2)]


@BF
@pytest.mark.parametrize("B,T,H,nw", ATT)
def test_attention_vs_fp64_with_ragged_key_mask(hip, bf16, B, T, H, nw):
    """Additive key bias of the decoder (1 valid / 0 padded, reference transformer.py) over ragged lengths.  The kernel rounds the
    probabilities (before P.V; the normaliser sums the unrounded ones) and the output to 16 bits: error of a few unit round-offs
    times max|v|."""
    qkv = att_case(B, T, H, 200 + T, bf16)
    mask, _ = ragged_mask(B, T, 13 if T > 64 * B else 3)
    ref = att_ref(qkv, mask, B, T, H, 0.125)
    o = hip.attention_h16(qkv, mask, B, T, H, 64, 0.125, 0, bf16=bf16)
    tag_is(o, att_tag(bf16, nw))
    vmax = qkv[:, 2 * H * 64:].abs().max().item()
    e = (o["out"].double() - ref).abs().max().item() / vmax
    note("att_bf16" if bf16 else "att_fp16", e)
    assert 0.0 < e <= ATT_TOL[bf16], e
    assert same_bits(o["out"], r16(o["out"], bf16)) and o["flag"] == 0
    again = hip.attention_h16(qkv, mask, B, T, H, 64, 0.125, 0, bf16=bf16)
    assert same_bits(again["out"], o["out"])


@BF
@pytest.mark.parametrize("B,T,H,nw,Tf", [(3, 320, 6, 2, 900), (4, 161, 6, 6, 500), (32, 640, 6, 4, 1600), (2, 130, 2, 6, 400)])
def test_attention_folded_padding_vs_explicit_padded_keys(hip, bf16, B, T, H, nw, Tf):
    """Folded padding: utterance b has klen[b] keys, the last of which stands for n_pad identical padded frames and carries the key
    bias ln(n_pad) (the reference gives each of them bias +0).  Against fp64 attention over the explicitly padded keys; keys at or
    beyond klen[b] and other utterances' rows must not reach an utterance's output, bit for bit."""
    qkv = att_case(B, T, H, 300 + T, bf16)
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
    o = hip.attention_h16(qkv, bias.reshape(-1).contiguous(), B, T, H, 64, 0.125, 0, klen=klen, bf16=bf16)
    tag_is(o, att_tag(bf16, nw))
    vmax = qkv[:, 2 * H * 64:].abs().max().item()
    live = (torch.arange(T, device="cuda")[None] < klen[:, None]).view(B, T, 1)
    e = ((o["out"].view(B, T, -1).double() - ref).abs() * live).max().item() / vmax
    note("att_bf16" if bf16 else "att_fp16", e)
    assert 0.0 < e <= ATT_TOL[bf16], e
    # the ln(n_pad) bias matters at this bar: without it the same launch is far off
    plain = bias.clone()
    for i, n in enumerate(lens):
        plain[i, n] = 0.0
    off = hip.attention_h16(qkv, plain.reshape(-1).contiguous(), B, T, H, 64, 0.125, 0, klen=klen, bf16=bf16)
    assert ((off["out"].view(B, T, -1).double() - ref).abs() * live).max().item() / vmax > 2 * ATT_TOL[bf16]
    # dead keys and foreign rows: other values, other bias, same bits on the live rows
    q2, b2 = qkv.clone().view(B, T, -1), bias.clone()
    for i, n in enumerate(lens):
        q2[i, n + 1:] = 30.0
        b2[i, n + 1:] = 5.0
    o2 = hip.attention_h16(q2.reshape(B * T, -1), b2.reshape(-1).contiguous(), B, T, H, 64, 0.125, 0, klen=klen, bf16=bf16)
    assert same_bits(torch.where(live, o2["out"].view(B, T, -1), 0.0), torch.where(live, o["out"].view(B, T, -1), 0.0))
    solo = hip.attention_h16(qkv.view(B, T, -1)[1].contiguous(), bias[1].contiguous(), 1, T, H, 64, 0.125, 0, klen=klen[1:2].contiguous(), bf16=bf16)
    if B * H * ((T + 127) // 128) < 512:              # (the same query-block form for one utterance as for the batch)
        assert solo["tag"] == o["tag"]
        assert same_bits(solo["out"][:lens[1] + 1], o["out"].view(B, T, -1)[1, :lens[1] + 1])


def test_every_h16_instantiation_was_launched(request):
    """Coverage of the file, by the tags the launchers reported: per dtype the 128-row tile, the 64-row tile with 2, 3 and 4
    stages, split-K without and with LayerNorm, the GroupNorm-statistics epilogue, LayerNorm on the 2- and 3-stage tiles, and the six
    attention kernels.  Each case above asserts its own tag; when the whole file ran (no -k, no node ids) the set seen is asserted."""
    required = set()
    for bf in (False, True):
        required |= {gemm_tag(bf, 128, False, 2), gemm_tag(bf, 64, False, 2), gemm_tag(bf, 64, False, 3), gemm_tag(bf, 64, False, 4),
                     gemm_tag(bf, 64, False, 3, ks=2), gemm_tag(bf, 64, True, 3, ks=2), gemm_tag(bf, 64, False, 3, gn=True, ks=2),
                     gemm_tag(bf, 64, True, 3), gemm_tag(bf, 64, True, 2)}
        required |= {att_tag(bf, nw) for nw in (2, 4, 6)}
    assert len(required) == 24
    assert {f for *_, f in LINEAR} >= {(128, 2, 1), (64, 2, 1), (64, 3, 1), (64, 4, 1), (64, 3, 2)} and {nw for *_, nw in ATT} == {2, 4, 6}
    print("\nH16 instantiations launched:\n  " + "\n  ".join(sorted(SEEN)))
    whole_file = not request.config.getoption("keyword") and not any("::" in str(a) for a in request.config.args)
    if whole_file:
        assert required <= SEEN, sorted(required - SEEN)

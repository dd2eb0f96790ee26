"""GPU parity of the fp32-ROW kernels (fp32 rows in, fp32 rows out), kernel by kernel through the C ABI: gemm_f32_kernel<BM, A_MASK,
A_NORM, TERMS> at terms 0 / 2 / 6 with every argument the text encoder, the duration predictor and the full-range estimator pass
(mtts_gemm_f32_args_run), attention_f32_kernel<2 | 4, false> with klen (mtts_attention_f32_run), gn_partial + gn_apply with the fp32
store (mtts_groupnorm_mish_f32_run), layernorm_kernel (mtts_channel_layernorm_ld) and row_stats_kernel (mtts_row_stats).

ONE RULE.  What must be bit-equal is compared bit for bit: products with an identity A at terms 0 / 6, rows under a 0 mask, the P16
copy of a launch against the restated split of the same launch's fp32 rows times out16_mask (both planes, out_lscale 2048 and 1),
repeated launches, row rolls of the batch, and the two upsampling phases interleaved into one buffer.  Everything else satisfies, per
element, with Bud the budget of tests/f32_restated.py in units of u = 2^-24,

    e_hip <= 8 e_cpu32 + floor          (e = max over the elements of |value - fp64 reference| / (u Bud), each in its own Bud)

where e_cpu32 is the error of the fp32 CPU twin against the same fp64 reference and floor is DERIVED (f32_restated.FLOOR):
  terms 0   1     the result's own rounding
  terms 2   1 + 4 the dropped l.l product: |l| / 2^11 <= 2^-11 |h| for either operand, so |l_a l_w| 2^-22 <= 4 u |a||w|, and
                  sum_k |a_k||w_k| <= Bud.  (A CPU simulation of the three products on pre-split N(0,1) operands gave at most 1.0 at
                  K = 32 and 0.2 at K = 384; the device's figure is recorded in profiles/r23_f32_parity.md, the floor is not lowered.)
  terms 6   1.25  the three dropped products of 8-bit terms, |m| <= 2^-9 |x|, |l| <= 2^-18 |x|: (2 2^-27 + 2^-36) |a||w| < u / 4 |a||w|
terms 2 operands (A and W) pass through tests/p16_restated.py's split BEFORE reference, twin and kernel.

ATTENTION is measured against A = sum_j p_j |v_j| per element.  Its allowance comes from the two figures the kernel header documents,
delta = 3e-8 absolute per split operand of size O(1) (taken as 3e-8 max(1, |x|): above 1 the residual's precision is relative) and
1e-6 relative of v_exp_f32, carried to the output:
  v split            sum_j p_j delta                                              = delta_v
  p split            the unnormalised weights e_j <= 1 are split: sum_j delta |v_j| / L,  L = sum_j e_j >= 1
  q, k split         a logit moves by ds <= scale (delta_k sum_d |q_d| + delta_q max_j sum_d |k_jd|); a softmax whose logits move by at
                     most ds moves the output by at most 2 ds A
  v_exp_f32          1e-6 on every weight, numerator and denominator:             2e-6 A
  own rounding       u A
The sum  W = (u + 2e-6 + 2 ds) A + delta_v + delta_p sum_j |v_j| / L  is the unit of an attention element: e = max |value - ref| / W and
e_hip <= 8 e_cpu32 + 1, the same rule with the derived allowance as its floor.  If the device needs more, that is a finding.  In mode 1 the rows left out are exactly those with mask 0 (their count is in the report line).

HARNESS.  Every output buffer is filled with a sentinel and has 64 guard floats behind it; where the entry allows the rows are wider
than N (ldc > N).  Columns [N, ldc), rows outside the launch's (strided) set and the guard must still hold the sentinel.  Every case
asserts the instantiation (tag); the closing test requires all 24 gemm_f32_kernel instantiations of terms 0 / 2 / 6 and both fp32-I/O
attention kernels.  With $MTTS_F32_REPORT set every assertion appends one line (case, e_hip, e_cpu32, floor, bar ratio) to that
file: profiles/r23_f32_parity.md.

Worst figures on one MI355X (profiles/r23_f32_parity.md; e_hip / (8 e_cpu32 + floor)): gemm terms 0 0.28, terms 2 0.12, terms 6 0.23
(LayerNorm from 16 partial moments), attention 0.29, gn_apply 0.13, layernorm 0.15, row_stats 0.12.  No terms 2 line needed the
dropped-product part of its floor (largest e_hip 2.91 at quiet rows x 2^-16 against e_cpu32 3.26): the fp16 MFMA keeps subnormal heads.
Each of eight one-line mutations of the kernels (scratch builds) fails this file; the table there names the tests and the factor."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import f32_restated as R
from conftest import sub
from p16_restated import p16

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("MTTS_F32_REPORT")
SEEN = set()
WORST = {}


def note(kernel, case, e_hip, e_cpu32, floor, worst, extra=""):
    line = f"| {kernel} | {case} | {e_hip:.4f} | {e_cpu32:.4f} | {floor} | {worst:.4f} |{extra}"
    print(line)
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    h = sub("_hip")
    yield h
    print("\nfp32-row kernels, worst ratio to the bar per kernel:", {k: f"{v:.3f}" for k, v in sorted(WORST.items())})


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return None if t is None else t.contiguous().cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def wide(t, ld, fill=3.0e30):
    """rows of t inside a wider device buffer (row stride ld); the pad columns hold a value no product survives"""
    buf = torch.full((t.shape[0], ld), fill, dtype=torch.float32)
    buf[:, :t.shape[1]] = t
    return buf.cuda()[:, :t.shape[1]]


def untouched(h, o, written_rows, rows, N):
    """sentinel everywhere a launch must not write: columns [N, ld), rows outside the written set, the guard"""
    buf, ld = o["buf"].cpu(), o["ld"]
    body = buf[:rows * ld].view(rows, ld)
    w = torch.zeros(rows, dtype=torch.bool)
    w[written_rows] = True
    ok = (body[:, N:] == h.F32_SENTINEL).all() and (body[~w] == h.F32_SENTINEL).all() and (buf[rows * ld:] == h.F32_SENTINEL).all()
    return bool(ok) and bool((body[w][:, :N] != h.F32_SENTINEL).all())


def gemm_tag(bm, mask, norm, terms):
    tf = lambda b: "true" if b else "false"
    return f"gemm_f32_kernel<{bm}, {tf(mask)}, {tf(norm)}, {terms}>"


def odd_x100(a, B, T):
    """odd utterances x100: a tap or a tile row that reads the neighbouring utterance is off by orders"""
    a = a.clone().view(B, T, -1)
    a[1::2] *= 100.0
    return a.reshape(B * T, -1)


def run_gemm(hip, name, a, w, bias=None, *, terms, B, T_in, T_out=None, bm=64, c1=0, sep_a1=False, lda_pad=4, a_mask=None, ln=None, act=0,
             p0=None, p1=None, res=None, ldr_pad=4, out_mask=None, out_scale=1.0, ldc=0, tap_off=None, in_stride=1, out_T=0, out_stride=1,
             out_off=0, stats_out=False, want_p16=False, out16_mask=None, out_lscale=2048.0, flag=0, into=None, presplit=True, judge=True):
    """One launch against the restatement under the module's rule.  a [B*T_in, C] and w on the CPU; terms 2: both pre-split here.
    ln: None, "arrays" or "parts" (partial moments of a's own 64-column slices).  Returns (device result, fp64 reference rows)."""
    T_out = T_in if T_out is None else T_out
    a_dev = a
    if terms == 2 and presplit:      # (an element beyond the fp16 range reaches the device as it is; the reference sees its clamp)
        a_dev, a, w = torch.where(a.abs() > 65504, a, p16(a)), p16(a), p16(w)
    C, N = a.shape[1], w.shape[0]
    kw = dict(B=B, T_in=T_in, T_out=T_out, tap_off=tap_off, in_stride=in_stride, a_mask=a_mask, act=act, p0=p0, p1=p1, out_scale=out_scale)
    dkw = {}
    if ln == "arrays":
        mean, rstd = R.row_stats(a)
        kw.update(a_mean=mean.float(), a_rstd=rstd.float())
        dkw.update(a_mean=dev(mean.float()), a_rstd=dev(rstd.float()))
    elif ln == "parts":
        part = R.row_moments(a).float()
        kw.update(a_part=part)
        dkw.update(a_part=dev(part))
    rows = B * (out_T if out_T else T_out)
    where = R.place_rows(rows, B, T_out, out_T if out_T else T_out, out_stride if out_T else 1, out_off if out_T else 0)
    kw.update(res=None if res is None else res[where], out_mask=None if out_mask is None else out_mask[where])
    ref, bud = R.gemm(a, w, bias, terms=terms, dtype=torch.float64, want_budget=True, **kw)
    twin = R.gemm(a, w, bias, terms=terms, dtype=torch.float32, **kw)
    c0 = C - c1
    if sep_a1:
        d_a, d_a1 = wide(a_dev[:, :c0], c0 + lda_pad), wide(a_dev[:, c0:], max(c0, c1) + lda_pad + 8)      # (lda1 > lda0)
    else:
        d_a, d_a1 = wide(a_dev, C + lda_pad), None
    d_res = None if res is None else (wide(res, N + ldr_pad) if ldr_pad else dev(res))
    o = hip.gemm_f32_args(d_a, w, dev(bias), terms=terms, B=B, T_in=T_in, T_out=T_out, tap_off=tap_off, in_stride=in_stride, c1=c1, a1=d_a1,
                          a_mask=dev(a_mask), act=act, p0=dev(p0), p1=dev(p1), res=d_res, out_mask=dev(out_mask), out_scale=out_scale,
                          out16_mask=dev(out16_mask), want_p16=want_p16, into=into, ldc=ldc, out_T=out_T, out_stride=out_stride, out_off=out_off,
                          stats_out=stats_out, force_bm=bm, out_lscale=out_lscale, **dkw)
    SEEN.add(o["tag"])
    assert o["tag"] == gemm_tag(bm, a_mask is not None, ln is not None, terms), o["tag"]
    assert o["flag"] == flag, o["flag"]
    if into is None:
        assert untouched(hip, o, where, rows, N), name
    out = o["out"].cpu()[where]
    assert torch.isfinite(out).all(), name
    if judge:
        ok, eh, ec, worst = R.judge(out, twin, ref, bud, R.FLOOR[terms])
        note(f"gemm terms {terms}", name, eh, ec, R.FLOOR[terms], worst)
        assert ok, (name, eh, ec, worst)
    if want_p16:
        m16 = torch.ones(rows) if out16_mask is None else out16_mask
        want = p16(o["out"].cpu()[where] * m16[where][:, None], out_lscale)
        assert same_bits(o["out16"].cpu()[where], want), name
        img = o["image"].cpu().view(rows + 64, N // 32, 2, 32)
        h16, l16 = img[:, :, 0].reshape(rows + 64, N).view(torch.float16), img[:, :, 1].reshape(rows + 64, N).view(torch.float16)
        assert same_bits(h16[where].float() + l16[where].float() / out_lscale, want), name
        masked = (o["out"].cpu()[where] * m16[where][:, None]).clamp(-65504, 65504).to(torch.float16)
        assert torch.equal(h16[where].view(torch.int16), masked.view(torch.int16)), name      # the head plane is the fp16 rounding of the row
        keep = torch.ones(rows + 64, dtype=torch.bool)
        keep[where] = False
        assert (o["image"].cpu()[keep] == 0x7e00).all(), name
    if stats_out:
        full = o["out"].cpu()[where].double().view(len(where), N // 64, 64)
        st = o["stats"].cpu()[where].double()
        mu = full.mean(2)
        m2 = ((full - mu[:, :, None]) ** 2).sum(2)
        # a 64-term fp32 sum by a tree of 2 + 4 levels, a multiply: 8 u mean|o|; M2 the same on the squares plus the mean's shift
        am = full.abs().mean(2)
        assert ((st[:, :, 0] - mu).abs() <= 8 * R.U * am + 1e-300).all(), name
        dev_abs = (full - mu[:, :, None]).abs().sum(2)
        assert ((st[:, :, 1] - m2).abs() <= R.U * (16 * m2 + 2 * dev_abs * 8 * am) + 1e-300).all(), name
        rest = torch.ones(rows, dtype=torch.bool)
        rest[where] = False
        if into is None:
            assert (o["stats_buf"].cpu()[:rows * 2 * (N // 64)].view(rows, -1)[rest] == hip.F32_SENTINEL).all()
        assert (o["stats_buf"].cpu()[rows * 2 * (N // 64):] == hip.F32_SENTINEL).all()
    return o, ref


TERMS = [0, 2, 6]


# ------------------------------------------------------------------------------------------------ GEMM: bit-equal
@pytest.mark.parametrize("terms", [0, 6])
@pytest.mark.parametrize("bm", [64, 128])
def test_identity_a_returns_the_panel_bit_for_bit(hip, terms, bm):
    K, N = 96, 132
    w = rnd(N, K, seed=1) * torch.exp(rnd(N, K, seed=2) * 3)
    o, _ = run_gemm(hip, f"identity bm {bm}", torch.eye(K), w, terms=terms, B=1, T_in=K, bm=bm, ldc=N + 4, judge=False)
    assert same_bits(o["out"], w.T)


@pytest.mark.parametrize("terms", TERMS)
def test_masked_rows_repeat_launches_and_row_rolls_are_bit_equal(hip, terms):
    B, T, C, N = 4, 33, 36, 100
    a, w, bias = odd_x100(rnd(B * T, C, seed=3), B, T), rnd(N, C, seed=4, scale=C ** -0.5), rnd(N, seed=5)
    am = (torch.arange(B * T) % 5 != 2).float()
    om = (torch.arange(B * T) % 7 != 3).float()
    res = rnd(B * T, N, seed=6)
    kw = dict(terms=terms, B=B, T_in=T, a_mask=am, ldc=N + 4)
    o, _ = run_gemm(hip, "a_mask rows", a, w, bias, act=R.ACT_RELU, **kw)
    assert same_bits(o["out"].cpu()[am == 0], torch.relu(bias).expand(int((am == 0).sum()), N))      # a 0 row is exactly act(bias)
    o2, _ = run_gemm(hip, "out_mask rows", a, w, bias, out_mask=om, res=res, **kw)
    assert same_bits(o2["out"].cpu()[om == 0], res[om == 0])                                       # out_mask 0: exactly the residual
    again, _ = run_gemm(hip, "repeat", a, w, bias, out_mask=om, res=res, **kw)
    assert same_bits(again["out"], o2["out"])
    roll = lambda t, k=1: t.view(B, T, *t.shape[1:]).roll(k, 0).reshape(t.shape)
    rolled, _ = run_gemm(hip, "rolled", roll(a), w, bias, out_mask=roll(om), res=roll(res), **dict(kw, a_mask=roll(am)))
    assert same_bits(roll(o2["out"].cpu().contiguous(), 1), rolled["out"])


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("lscale", [2048.0, 1.0])
def test_p16_copy_is_the_split_of_the_same_launchs_rows(hip, terms, lscale):
    """the encoder's FFN hand-over: the f32 kernel writes fp32 rows AND their image, the image times out16_mask"""
    B, T, C, N = 3, 43, 64, 96
    a, w, bias = rnd(B * T, C, seed=7) * 3 + 0.3, rnd(N, C, seed=8, scale=C ** -0.5), rnd(N, seed=9)
    m16 = (torch.arange(B * T) % 4 != 1).float()
    for bm in (64, 128):
        o, _ = run_gemm(hip, f"out16 lscale {lscale:g} bm {bm}", a, w, bias, terms=terms, B=B, T_in=T, bm=bm, act=R.ACT_RELU, want_p16=True,
                        out16_mask=m16, out_lscale=lscale, ldc=N + 8, res=rnd(B * T, N, seed=10))
        assert (o["out16"].cpu()[m16 == 0] == 0).all() and (o["out"].cpu()[m16 == 0] != 0).any()   # the mask touches the image only
        assert (o["image"].cpu()[:B * T].view(B * T, N // 32, 2, 32)[:, :, 1] != 0).any()          # really two planes


@pytest.mark.parametrize("terms", TERMS)
def test_two_upsampling_phases_interleave_into_one_buffer(hip, terms):
    """ConvTranspose1d(k4, s2, p1) as two phase GEMMs of two taps each, out_stride 2, out_off 0 / 1, against F.conv_transpose1d"""
    B, T, C, N = 3, 5, 32, 64
    x, wt, bias = odd_x100(rnd(B * T, C, seed=11), B, T), rnd(C, N, 4, seed=12, scale=(2 * C) ** -0.5), rnd(N, seed=13)
    if terms == 2:
        x, wt = p16(x), p16(wt)
    ph = [(wt[:, :, [1, 3]].permute(1, 0, 2).contiguous(), [0, -1], 0), (wt[:, :, [0, 2]].permute(1, 0, 2).contiguous(), [1, 0], 1)]
    o = None
    for w, taps, off in ph:
        o, _ = run_gemm(hip, f"phase {off}", x, w, bias, terms=terms, B=B, T_in=T, tap_off=taps, out_T=2 * T, out_stride=2, out_off=off, into=o,
                        ldc=N + 4, stats_out=True, presplit=False)
    full = F.conv_transpose1d(x.double().view(B, T, C).transpose(1, 2), wt.double(), bias.double(), stride=2, padding=1).transpose(1, 2).reshape(-1, N)
    alone = [run_gemm(hip, f"phase {off} alone", x, w, bias, terms=terms, B=B, T_in=T, tap_off=taps, out_T=2 * T, out_stride=2, out_off=off,
                      ldc=N + 4, presplit=False)[0]["out"].cpu() for w, taps, off in ph]
    out = o["out"].cpu()
    assert same_bits(out[0::2], alone[0][0::2]) and same_bits(out[1::2], alone[1][1::2])            # each phase's rows, bit for bit
    body = o["buf"].cpu()[:2 * B * T * (N + 4)].view(2 * B * T, N + 4)
    assert (body[:, N:] == hip.F32_SENTINEL).all() and (o["buf"].cpu()[2 * B * T * (N + 4):] == hip.F32_SENTINEL).all()
    assert (out.double() - full).abs().max().item() <= 1e-4 * full.abs().max().item()              # and the interleave is the transposed conv


# ------------------------------------------------------------------------------------------------ GEMM: the rule
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("bm", [64, 128])
@pytest.mark.parametrize("M", [1, 31, 33, 63, 64, 65, 127, 129, 130])
def test_rows_straddling_tiles_and_utterances(hip, terms, bm, M):
    B, C, N = 2, 28, 100
    a, w, bias = odd_x100(rnd(B * M, C, seed=20 + M), B, M), rnd(N, C, 3, seed=21, scale=(3 * C) ** -0.5), rnd(N, seed=22)
    run_gemm(hip, f"M {M} bm {bm} k3", a, w, bias, terms=terms, B=B, T_in=M, bm=bm, ldc=N + 4)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("N,ldc,ldr_pad", [(1, 1, 0), (4, 8, 4), (100, 104, 4), (100, 103, 4), (100, 104, 3), (101, 104, 4), (128, 132, 4), (132, 132, 0),
                                           (192, 200, 8)])
def test_columns_vector_and_scalar_epilogues(hip, terms, N, ldc, ldr_pad):
    B, T, C = 2, 37, 36
    a, w, bias = odd_x100(rnd(B * T, C, seed=30), B, T), rnd(N, C, seed=31 + N, scale=C ** -0.5), rnd(N, seed=32)
    res = rnd(B * T, N, seed=33)
    om = (torch.arange(B * T) % 6 != 1).float()
    run_gemm(hip, f"N {N} ldc {ldc} ldr +{ldr_pad}", a, w, bias, terms=terms, B=B, T_in=T, ldc=ldc, res=res, ldr_pad=ldr_pad, out_mask=om,
             out_scale=0.37, act=R.ACT_SILU)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("C,ntaps,T_in", [(4, 1, 5), (28, 3, 1), (32, 3, 2), (36, 5, 3), (200, 5, 5), (36, 5, 1), (32, 1, 3)])
def test_k_padding_and_taps_off_both_ends(hip, terms, C, ntaps, T_in):
    B, N = 3, 68
    a = odd_x100(rnd(B * T_in, C, seed=40 + C), B, T_in)
    w = rnd(N, C, ntaps, seed=41, scale=(ntaps * C) ** -0.5) if ntaps > 1 else rnd(N, C, seed=41, scale=C ** -0.5)
    run_gemm(hip, f"C {C} k{ntaps} T {T_in}", a, w, rnd(N, seed=42), terms=terms, B=B, T_in=T_in, ldc=N + 4)


@pytest.mark.parametrize("terms", TERMS)
def test_stride_2_with_odd_length_and_two_segments(hip, terms):
    B, T_in, N = 3, 7, 64
    T_out = (T_in + 2 - 3) // 2 + 1
    a = odd_x100(rnd(B * T_in, 36, seed=50), B, T_in)
    o, ref = run_gemm(hip, "k3 stride 2 T 7", a, rnd(N, 36, 3, seed=51, scale=0.1), rnd(N, seed=52), terms=terms, B=B, T_in=T_in, T_out=T_out,
                      in_stride=2, ldc=N + 4)
    for c0, c1 in ((32, 4), (64, 36)):
        B, T = 2, 33
        a = odd_x100(rnd(B * T, c0 + c1, seed=53), B, T)
        a[:, c0:] *= 7.0                                         # a segment read with the other's stride or offset is off by a factor
        am = (torch.arange(B * T) % 5 != 0).float()
        w, bias = rnd(N, c0 + c1, 3, seed=54, scale=0.05), rnd(N, seed=55)
        sep, _ = run_gemm(hip, f"segments {c0}+{c1} separate", a, w, bias, terms=terms, B=B, T_in=T, c1=c1, sep_a1=True, a_mask=am, ldc=N + 4)
        one, _ = run_gemm(hip, f"segments {c0}+{c1} adjacent", a, w, bias, terms=terms, B=B, T_in=T, c1=c1, a_mask=am, ldc=N + 4)
        assert same_bits(sep["out"], one["out"])


def hard_rows(M, C, seed):
    """LayerNorm rows: |mean| = 32 std, variance near eps, constant, all zero, one x100 row between unit rows"""
    a = rnd(M, C, seed=seed) + 0.3
    a[1] = 32.0 + rnd(C, seed=seed + 1)
    a[2] = 0.5 + rnd(C, seed=seed + 2) * 3e-3
    a[3] = 1.25
    a[4] = 0.0
    a[6] *= 100.0
    return a


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("ln,C", [("arrays", 36), ("arrays", 64), ("parts", 64), ("parts", 128), ("parts", 384), ("parts", 512), ("parts", 576),
                                  ("parts", 1024)])
def test_layernorm_prologue_arrays_and_partial_moments(hip, terms, ln, C):
    """a_nparts = C / 64 in {1, 2, 6, 8, 9, 16}: the merge of <= 8 parts in registers and the re-read loop beyond"""
    B, T, N = 2, 35, 64
    a = hard_rows(B * T, C, seed=60 + C)
    am = (torch.arange(B * T) % 9 != 5).float()
    for bm, mask in ((64, None), (128, am)):
        run_gemm(hip, f"LN {ln} C {C} bm {bm}{' masked' if mask is not None else ''}", a, rnd(N, C, seed=61, scale=C ** -0.5), rnd(N, seed=62),
                 terms=terms, B=B, T_in=T, bm=bm, ln=ln, a_mask=mask, ldc=N + 4)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_SILU, R.ACT_SNAKE])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_every_epilogue_form(hip, terms, act, res, masked):
    B, T, C, N = 2, 67, 64, 128
    a, w, bias = rnd(B * T, C, seed=70) * 2 + 0.2, rnd(N, C, seed=71, scale=C ** -0.5), rnd(N, seed=72)
    p0, p1 = torch.exp(rnd(N, seed=73) * 0.3), 1.0 / (torch.exp(rnd(N, seed=74) * 0.3) + 1e-9)
    om = (torch.arange(B * T) % 5 != 4).float() if masked else None
    for bm in (64, 128):
        run_gemm(hip, f"act {act} res {int(res)} mask {int(masked)} bm {bm}", a, w, bias, terms=terms, B=B, T_in=T, bm=bm, act=act,
                 p0=p0 if act == R.ACT_SNAKE else None, p1=p1 if act == R.ACT_SNAKE else None, res=rnd(B * T, N, seed=75) if res else None,
                 out_mask=om, out_scale=-1.7, ldc=N + 4, stats_out=True)
    run_gemm(hip, f"act {act} no bias", a, w, None, terms=terms, B=B, T_in=T, act=act, p0=p0 if act == R.ACT_SNAKE else None,
             p1=p1 if act == R.ACT_SNAKE else None, ldc=N + 4)


def test_range_flag_clamp_and_what_rerun_relies_on(hip):
    """terms 2 with one A element at 1e6: flag raised, result finite and equal to the reference on the CLAMPED operand.  terms 0 / 6 on
    the same input: flag untouched, the bar holds on the unclamped operand."""
    B, T, C, N = 2, 33, 64, 64
    a, w, bias = rnd(B * T, C, seed=80), rnd(N, C, seed=81, scale=C ** -0.5), rnd(N, seed=82)
    a[17, 5] = 1.0e6
    run_gemm(hip, "range terms 2 (clamped operand)", a, w, bias, terms=2, B=B, T_in=T, flag=1, ldc=N + 4)
    for terms in (0, 6):
        run_gemm(hip, "range unclamped", a, w, bias, terms=terms, B=B, T_in=T, flag=0, ldc=N + 4)
    # terms 6 has the fp32 exponent range: A x 2^40, W x 2^-40 gives the same error in units of Bud (bit-equal rows, in fact)
    a[17, 5] = 1.0
    plain, _ = run_gemm(hip, "terms 6 unscaled", a, w, None, terms=6, B=B, T_in=T, ldc=N + 4)
    scaled, _ = run_gemm(hip, "terms 6 A 2^40 W 2^-40", a * 2.0 ** 40, w * 2.0 ** -40, None, terms=6, B=B, T_in=T, ldc=N + 4)
    assert same_bits(plain["out"], scaled["out"])


@pytest.mark.parametrize("shift", [8, 16])
def test_quiet_rows_terms_2(hip, shift):
    """A rows x 2^-8 and x 2^-16, pre-split: the fp16 heads go subnormal (|h| < 2^-14).  The rule is the same."""
    B, T, C, N = 2, 33, 64, 64
    a = p16(rnd(B * T, C, seed=90)) * 2.0 ** -shift
    a = p16(a)
    assert (a.abs().to(torch.float16).float().abs() < 2.0 ** -14).float().mean().item() > (0.0 if shift == 8 else 0.5)
    run_gemm(hip, f"quiet rows 2^-{shift}", a, p16(rnd(N, C, seed=91, scale=C ** -0.5)), None, terms=2, B=B, T_in=T, ldc=N + 4, presplit=False)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("bm", [64, 128])
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("norm", [False, True])
def test_every_instantiation_once(hip, terms, bm, mask, norm):
    B, T, C, N = 2, 65, 64, 100
    a = hard_rows(B * T, C, seed=95)
    am = (torch.arange(B * T) % 4 != 3).float() if mask else None
    run_gemm(hip, f"<{bm}, {mask}, {norm}, {terms}>", a, rnd(N, C, seed=96, scale=C ** -0.5), rnd(N, seed=97), terms=terms, B=B, T_in=T, bm=bm,
             a_mask=am, ln="arrays" if norm else None, ldc=N + 4)


# ------------------------------------------------------------------------------------------------ attention
DELTA, EXP_REL = 3e-8, 1e-6


def run_attention(hip, name, qkv, mask, B, T, H, D, mode, klen=None, nw=2, scale=None):
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32)
    ref, A, aux = R.attention(qkv, mask, B, T, H, D, scale, mode, kl)
    twin, _, _ = R.attention(qkv, mask, B, T, H, D, scale, mode, kl, dtype=torch.float32)
    o = hip.attention_f32_run(dev(qkv), dev(mask), B, T, H, D, scale, mode, klen=dev(kl))
    SEEN.add(o["tag"])
    assert o["tag"] == f"attention_f32_kernel<{nw}, false, false, false, false, 64>", o["tag"]
    assert (o["buf"].cpu()[B * T * H * D:] == hip.F32_SENTINEL).all()
    out = o["out"].cpu()
    keep = torch.ones(B * T, dtype=torch.bool) if mode == 0 else mask != 0           # mode 1: exactly the rows with mask 0 are left out
    q, k, v = qkv.split(H * D, dim=1)
    dq, dk, dv = [DELTA * max(1.0, t.abs().max().item()) for t in (q, k, v)]
    ds = scale * (dk * aux["sq"] + dq * aux["sk"])
    unit = (R.U + EXP_REL * 2 + 2 * ds) * A + dv + DELTA * aux["sv"] / aux["L"]          # the derived allowance, per element
    nokey = (aux["sv"] == 0) & (A == 0) & keep[:, None]
    assert (bits(out[nokey]) == 0).all(), name                                             # a row without a key is exactly +0
    ok, eh, ec, worst = R.judge(out[keep], twin[keep], ref[keep], unit[keep] / R.U, 1.0)
    note("attention", name, eh, ec, 1, worst, f" excluded rows {int((~keep).sum())}")
    assert torch.isfinite(out[keep]).all() and ok, (name, eh, ec, worst)
    return o, ref


def ragged(B, T, step):
    lens = torch.tensor([max(1, T - step * i) for i in range(B)])
    return (torch.arange(T)[None] < lens[:, None]).float().reshape(-1)


@pytest.mark.parametrize("D", [4, 24, 48, 60, 64])
@pytest.mark.parametrize("T", [1, 31, 33, 63, 65, 129])
@pytest.mark.parametrize("mode", [0, 1])
def test_attention_head_dims_lengths_modes(hip, D, T, mode):
    B, H = 3, 2
    qkv = rnd(B * T, 3 * H * D, seed=100 + D + T)
    run_attention(hip, f"D {D} T {T} mode {mode}", qkv, ragged(B, T, 11), B, T, H, D, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_attention_klen_and_foreign_utterances(hip, mode):
    B, T, H, D = 4, 65, 2, 48
    qkv = rnd(B * T, 3 * H * D, seed=110)
    qkv.view(B, T, -1)[1::2, :, 2 * H * D:] *= 100.0                      # odd utterances' values x100: a key of the neighbour shows
    klen = [65, 40, 0, 1]
    o, _ = run_attention(hip, f"klen mode {mode}", qkv, ragged(B, T, 3), B, T, H, D, mode, klen=klen)
    assert (bits(o["out"].cpu().view(B, T, -1)[2]) == 0).all()           # klen = 0: exactly +0
    free, _ = run_attention(hip, f"no klen mode {mode}", qkv, ragged(B, T, 3), B, T, H, D, mode)
    assert not same_bits(free["out"].view(B, T, -1)[1], o["out"].view(B, T, -1)[1])      # klen < T really removed keys


@pytest.mark.parametrize("what", ["rescale", "quiet", "loud"])
def test_attention_forced_rescale_and_operand_scales(hip, what):
    B, T, H, D = 1, 256, 1, 64
    qkv = rnd(B * T, 3 * D, seed=120, scale=0.5)
    if what == "rescale":      # one key per tile dominates: the running maximum jumps at every tile boundary
        for tile in range(4):
            qkv[tile * 64 + 13, D:2 * D] = qkv[5, :D] * (4.0 + 3.0 * tile)
    elif what == "quiet":      # q, k at 2^-6: every unscaled residual is an fp16 subnormal
        qkv[:, :2 * D] *= 2.0 ** -6 / 0.5
    else:                      # q, k at 8: logits of +-60 scale
        qkv[:, :2 * D] *= 8.0 / 0.5
    run_attention(hip, what, qkv, torch.ones(B * T), B, T, H, D, 0)


def test_attention_128_query_form_at_its_smallest_grid(hip):
    B, H, T, D = 32, 12, 250, 8                                          # B H ceil(T / 128) = 768 blocks, waste 2.3 %
    qkv = rnd(B * T, 3 * H * D, seed=130)
    for mode in (0, 1):
        run_attention(hip, f"128-query mode {mode}", qkv, ragged(B, T, 5), B, T, H, D, mode, nw=4, klen=[T - (i % 7) for i in range(B)])


# ------------------------------------------------------------------------------------------------ GroupNorm + Mish, fp32 store
def run_gn(hip, name, y, B, T, *, chbias=None, res=None, nrows=None, nextra=None, bias_row=None, stats_out=False, seed=0, ref_kw=None):
    C = y.shape[1]
    g, be = 1 + 0.1 * rnd(C, seed=seed + 1), 0.1 * rnd(C, seed=seed + 2)
    mask = ragged(B, T, 2)
    i32 = lambda t: None if t is None else torch.tensor(t, dtype=torch.int32)
    kw = dict(chbias=chbias, res=res, nrows=i32(nrows), nextra=i32(nextra), bias_row=bias_row) if ref_kw is None else ref_kw
    ref, bud = R.groupnorm_mish(y, g, be, mask, B, T, want_budget=True, **kw)
    twin = R.groupnorm_mish(y, g, be, mask, B, T, dtype=torch.float32, **kw)
    d_cb = None if chbias is None else (dev(chbias) if chbias.dim() == 1 else wide(chbias, C + 8))
    o = hip.groupnorm_mish_f32_run(dev(y), dev(g), dev(be), dev(mask), B, T, chbias=d_cb, res=None if res is None else wide(res, C + 12),
                                   nrows=dev(i32(nrows)), nextra=dev(i32(nextra)), bias_stats=None if bias_row is None else dev(R.gn_bias_stats(bias_row)),
                                   stats_out=stats_out)
    assert (o["buf"].cpu()[B * T * C:] == hip.F32_SENTINEL).all() and (o["out"].cpu() != hip.F32_SENTINEL).all(), name
    ok, eh, ec, worst = R.judge(o["out"].cpu(), twin, ref, bud, 1.0)
    note("gn_apply", name, eh, ec, 1, worst)
    assert ok, (name, eh, ec, worst)
    if stats_out:
        full = o["out"].cpu().double().view(B * T, C // 64, 64)
        mu = full.mean(2)
        assert ((o["stats"].cpu()[:, :, 0].double() - mu).abs() <= 8 * R.U * full.abs().mean(2) + 1e-300).all(), name
        m2 = ((full - mu[:, :, None]) ** 2).sum(2)
        assert ((o["stats"].cpu()[:, :, 1].double() - m2).abs() <= R.U * (16 * m2 + 16 * (full - mu[:, :, None]).abs().sum(2) * full.abs().mean(2)) + 1e-300).all(), name
        assert (o["stats_buf"].cpu()[B * T * 2 * (C // 64):] == hip.F32_SENTINEL).all()
    return o


@pytest.mark.parametrize("C", [32, 64, 96, 384])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 33])
def test_groupnorm_chunk_heights_and_widths(hip, C, T):
    B = 3
    y = odd_x100(rnd(B * T, C, seed=140 + C + T) * 1.5 + 0.2, B, T)
    run_gn(hip, f"C {C} T {T}", y, B, T, seed=141)
    run_gn(hip, f"C {C} T {T} rows + res", y, B, T, chbias=rnd(B, C, seed=142), res=rnd(B * T, C, seed=143), stats_out=C % 64 == 0, seed=141)
    run_gn(hip, f"C {C} T {T} one row", y, B, T, chbias=rnd(C, seed=144), seed=141)


def test_groupnorm_nrows_nextra_and_a_large_group_mean(hip):
    B, T, C = 3, 33, 96
    y = rnd(B * T, C, seed=150) * 1.5 + 0.2
    y[:, :12] += 1.0e3                                                    # a group mean of 1e3 on unit variance
    bias_row = rnd(C, seed=151) * 0.5
    run_gn(hip, "nrows < T", y, B, T, nrows=[33, 20, 1], seed=152)
    run_gn(hip, "nrows 0 with nextra", y, B, T, nrows=[33, 0, 9], nextra=[0, 5, 24], bias_row=bias_row, seed=152)
    # folded padding against the explicit padded rows: rows [n, T) of y hold the bias row, the statistics count them in closed form
    lens = [33, 21, 8]
    yp = y.clone().view(B, T, C)
    for b, n in enumerate(lens):
        yp[b, n:] = bias_row
    yp = yp.reshape(B * T, C)
    explicit = run_gn(hip, "explicit padded rows", yp, B, T, seed=152)
    folded = run_gn(hip, "nextra folded", yp, B, T, nrows=lens, nextra=[T - n for n in lens], bias_row=bias_row, seed=152, ref_kw={})
    assert (folded["out"] - explicit["out"]).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------------------------ channel LayerNorm, row statistics
@pytest.mark.parametrize("C", [4, 252, 256, 260, 2048])
@pytest.mark.parametrize("act,film,masked", [(0, False, False), (0, True, True), (2, False, True), (2, True, False)])
def test_channel_layernorm_widths_and_forms(hip, C, act, film, masked):
    B, T = 3, 7                                                           # M = 21: not a multiple of the 4 rows of a workgroup
    x = hard_rows(B * T, C, seed=160 + C) if C > 4 else rnd(B * T, C, seed=160) + 0.3
    g, be = 1 + 0.1 * rnd(C, seed=161), 0.1 * rnd(C, seed=162)
    fl = rnd(B, 2 * C, seed=163) if film else None
    mk = ragged(B, T, 2) if masked else None
    kw = dict(act=act, film=fl, mask=mk)
    ref, bud = R.channel_layernorm(x, B, T, g, be, want_budget=True, **kw)
    twin = R.channel_layernorm(x, B, T, g, be, dtype=torch.float32, **kw)
    o = hip.channel_layernorm_ld(wide(x, C + 8), B, T, C, dev(g), dev(be), act=act, film=dev(fl), mask=dev(mk), ldy=C + 4)
    body = o["buf"].cpu()[:B * T * (C + 4)].view(B * T, C + 4)
    assert (body[:, C:] == hip.F32_SENTINEL).all() and (o["buf"].cpu()[B * T * (C + 4):] == hip.F32_SENTINEL).all()
    ok, eh, ec, worst = R.judge(o["out"].cpu(), twin, ref, bud, 1.0)
    note("layernorm", f"C {C} act {act} film {int(film)} mask {int(masked)}", eh, ec, 1, worst)
    assert ok, (C, eh, ec, worst)


def test_channel_layernorm_film_with_one_frame_per_utterance(hip):
    B, T, C = 5, 1, 96
    x, g, be, fl = rnd(B, C, seed=170) + 0.7, 1 + 0.1 * rnd(C, seed=171), 0.1 * rnd(C, seed=172), rnd(B, 2 * C, seed=173)
    ref, bud = R.channel_layernorm(x, B, T, g, be, film=fl, want_budget=True)
    twin = R.channel_layernorm(x, B, T, g, be, film=fl, dtype=torch.float32)
    o = hip.channel_layernorm_ld(wide(x, C + 4), B, T, C, dev(g), dev(be), film=dev(fl), ldy=C + 4)
    ok, eh, ec, worst = R.judge(o["out"].cpu(), twin, ref, bud, 1.0)
    note("layernorm", "FiLM T 1 B 5", eh, ec, 1, worst)
    assert ok, (eh, ec, worst)


@pytest.mark.parametrize("C", [4, 252, 256, 260, 2048])
def test_row_stats(hip, C):
    """mean: a C-term fp32 sum and a division, |err| <= u (log2 C + 2) mean|x|; rstd relative: the same on the squares, root, division"""
    M = 21
    x = hard_rows(M, C, seed=180 + C) if C > 4 else rnd(M, C, seed=180) + 0.3
    lib = hip.load()
    mean, rstd = hip.guarded(M, 1, "cuda"), hip.guarded(M, 1, "cuda")
    xd = wide(x, C + 8)
    hip.check(lib.mtts_row_stats(xd.data_ptr(), M, C, C + 8, 1e-5, mean.data_ptr(), rstd.data_ptr(), hip.stream_ptr()))
    assert (mean.cpu()[M:] == hip.F32_SENTINEL).all() and (rstd.cpu()[M:] == hip.F32_SENTINEL).all()
    mu, rs = R.row_stats(x)
    mu32, rs32 = R.row_stats(x, dtype=torch.float32)
    depth = math.log2(C) + 2
    bud_mu = depth * x.double().abs().mean(1)
    var = ((x.double() - mu[:, None]) ** 2).mean(1)
    # d var <= u (depth var + 2 mean|x - mu| (|mu| u-shift ...)): the shift of the mean moves var only in second order
    bud_rs = rs * (0.5 * (depth * var + 2 * (x.double() - mu[:, None]).abs().mean(1) * bud_mu) / (var + 1e-5) + 3)
    for nm, got, twin, ref, bud in (("mean", mean, mu32, mu, bud_mu), ("rstd", rstd, rs32, rs, bud_rs)):
        ok, eh, ec, worst = R.judge(got.cpu()[:M], twin, ref, bud, 1.0)
        note("row_stats", f"{nm} C {C}", eh, ec, 1, worst)
        assert ok, (nm, C, eh, ec, worst)


# ------------------------------------------------------------------------------------------------ the set of kernels covered
def test_every_fp32_row_instantiation_was_launched(hip):
    want = {gemm_tag(bm, m, n, t) for bm in (64, 128) for m in (False, True) for n in (False, True) for t in TERMS}
    want |= {f"attention_f32_kernel<{nw}, false, false, false, false, 64>" for nw in (2, 4)}
    assert len(want) == 26 and want <= SEEN, sorted(want - SEEN)

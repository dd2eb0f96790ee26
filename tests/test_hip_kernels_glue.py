"""Kernel-level parity of the kernels that are not GEMMs, through their unit entries (csrc/unit_entries.hip): the Vocos tail
(csrc/vocos.hip: dwconv7_ln, spec_polar, istft_ola) and the solver / layout glue (csrc/norm_glue.hip: ode_combine, step_tables,
time_sinusoid, rope, the four layout moves, durations / durations_given / align_pool).

One tolerance rule.  Where the operation is exact in fp32 (the moves, products with a 0/1 mask, the step tables, the combine stages:
the build keeps every rounding point, -ffp-contract=off) the result is bit-equal to fp32 torch on the CPU.  Elsewhere the arbiter is
the fp64 restatement (tests/glue_restated.py, checked against independent torch code in tests/test_glue_abi.py) on the same fp32
inputs and the bound is measured here: e_hip <= 8 * e_cpu32 + floor, e_cpu32 the error of fp32 torch on the CPU against the same
reference, floor one fp32 ulp of the output's largest magnitude.  The 8 covers a different summation order (64-lane butterfly against
a sequential sum) and device expf / sinf / cosf at a couple of ulp against libm's half ulp; a wrong tap, divisor, coefficient or
index is off by orders of magnitude more.

Every output buffer is filled with a sentinel first and must be unchanged outside the documented region; inputs that must not be
read as data hold NaN.  Measured (e_hip, e_cpu32) pairs: profiles/r13_glue_parity.md."""
import math

import pytest
import torch
import torch.nn.functional as F

import glue_restated as G
from conftest import sub

pytestmark = pytest.mark.gpu
SENT = -12345.0
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    h = sub("_hip")
    h.build()
    h.load()
    return h


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp32(m):
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 2.0 ** -149


def measured(name, out, ref64, cpu32, scale=None, floor_at=None):
    """e_hip <= 8 * e_cpu32 + floor against the fp64 reference; `scale` divides the errors (a relative bound), floor_at is the
    largest magnitude of the (scaled) output."""
    d_hip, d_cpu = (out.double() - ref64).abs(), (cpu32.double() - ref64).abs()
    if scale is not None:
        d_hip, d_cpu = d_hip / scale, d_cpu / scale
    e_hip, e_cpu = d_hip.max().item(), d_cpu.max().item()
    floor = ulp32(ref64.abs().max().item() if floor_at is None else floor_at)
    print(f"GLUE-PARITY {name}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} floor {floor:.3e}")
    assert math.isfinite(e_hip) and e_hip <= 8 * e_cpu + floor, f"{name}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} floor {floor:.3e}"
    return e_hip, e_cpu


def guarded(shape, fill=SENT, guard=64):
    """A device buffer of `shape` filled with `fill`, followed by `guard` sentinel floats that nothing may touch."""
    n = int(torch.tensor(shape).prod())
    flat = torch.full((n + guard,), fill, dtype=torch.float32, device="cuda")
    flat[n:] = SENT
    return flat[:n].view(*shape), flat[n:]


def untouched(tail):
    return bool((tail == SENT).all().item())


# ------------------------------------------------------------------------------------------------ depthwise k7 conv + LayerNorm
BT = [(1, 1), (3, 2), (2, 3), (3, 5), (2, 7), (1, 9)]


def dw_inputs(B, T, C, seed, mean=0.0):
    g = gen(seed)
    x = torch.randn(B, T, C, generator=g)
    for b in range(1, B, 2):
        x[b] *= 100.0                                   # the neighbours of a unit-scale utterance are 100 times larger
    w7 = torch.randn(7, C, generator=g)                 # a different weight per tap
    bias = torch.randn(C, generator=g) * 0.1 + mean
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return x, w7, bias, gamma, beta


def dw_cpu32(x, w7, bias, gamma, beta):
    C = x.shape[2]
    y = F.conv1d(x.transpose(1, 2), w7.t().reshape(C, 1, 7).contiguous(), bias, padding=3, groups=C).transpose(1, 2)
    return F.layer_norm(y, (C,), gamma, beta, eps=1e-6)


def dw_run(hip, x, w7, bias, gamma, beta, lengths=None):
    B, T, C = x.shape
    y, tail = guarded((B * T, C))
    dev = lambda t: t.cuda().contiguous()
    hip.dwconv7_ln(dev(x.view(B * T, C)), dev(w7), dev(bias), dev(gamma), dev(beta), B, T, eps=1e-6,
                   lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda"), out=y)
    torch.cuda.synchronize()
    assert untouched(tail)
    return y.cpu().view(B, T, C)


@pytest.mark.parametrize("C", [4, 68, 256, 260, 512, 2048])
def test_dwconv7_ln_plain(hip, C):
    """One lane active, a partly used wave, exactly one slot, a partly used second slot, the production size, all eight slots; B*T
    mostly no multiple of the 4 rows of a workgroup; T < 7: taps fall off both ends."""
    for B, T in BT:
        p = dw_inputs(B, T, C, seed=C * 100 + B * 10 + T)
        out = dw_run(hip, *p)
        ref = G.dwconv7_ln(*[t.double() for t in p], 1e-6)
        measured(f"dwconv7_ln C={C} B={B} T={T}", out, ref, dw_cpu32(*p))


def test_dwconv7_ln_row_mean_1e3_on_unit_variance(hip):
    """A one-pass variance (E[x^2] - E[x]^2) loses every digit here: 1e6 against 1."""
    B, T, C = 2, 7, 512
    g = gen(77)
    x, w7 = torch.randn(B, T, C, generator=g), torch.randn(7, C, generator=g) * (1.0 / math.sqrt(7.0))
    bias, gamma, beta = torch.full((C,), 1000.0), torch.ones(C), torch.zeros(C)
    ref = G.dwconv7_ln(x.double(), w7.double(), bias.double(), gamma.double(), beta.double(), 1e-6)
    pre = G.dwconv7_ln(x.double(), w7.double(), bias.double(), gamma.double(), beta.double(), 1e30)     # ~ (acc - mean) * 1e-15
    assert 0.3e-15 < pre.std().item() < 3e-15                                                            # unit variance before the norm
    measured("dwconv7_ln mean 1e3", dw_run(hip, x, w7, bias, gamma, beta), ref, dw_cpu32(x, w7, bias, gamma, beta))


@pytest.mark.parametrize("C", [68, 512])
def test_dwconv7_ln_ragged(hip, C):
    """Rows t < clamp(len, 0, T) equal the reference on x[b, :len] alone and are finite although every row beyond is NaN."""
    B, T, lengths = 6, 9, [9, 3, 1, 0, 14, -2]
    x, w7, bias, gamma, beta = dw_inputs(B, T, C, seed=C + 1)
    ns = [G.clamp_len(n, T) for n in lengths]
    for b, n in enumerate(ns):
        x[b, n:] = NAN
    out = dw_run(hip, x, w7, bias, gamma, beta, lengths)
    ref = G.dwconv7_ln(x.double(), w7.double(), bias.double(), gamma.double(), beta.double(), 1e-6, lengths)
    valid = torch.zeros(B, T, dtype=torch.bool)
    cpu = torch.zeros(B, T, C)
    for b, n in enumerate(ns):
        valid[b, :n] = True
        if n:
            cpu[b, :n] = dw_cpu32(x[b:b + 1, :n], w7, bias, gamma, beta)[0]
    assert valid.sum().item() == 9 + 3 + 1 + 9 and torch.isfinite(out[valid]).all() and torch.isfinite(ref[valid]).all()
    measured(f"dwconv7_ln ragged C={C}", out[valid], ref[valid], cpu[valid])


# ------------------------------------------------------------------------------------------------ polar spectrum
@pytest.mark.parametrize("M,nbins,off,ld", [(7, 33, 36, 72), (3, 513, 516, 1032)])
def test_spec_polar(hip, M, nbins, off, ld):
    """Log-magnitudes on both sides of the clip, phases of tens of radians (a real checkpoint's) and the exact quadrant points; the
    error is taken relative to the magnitude."""
    g = gen(M)
    x = torch.full((M, ld), SENT)
    x[:, :nbins] = torch.rand(M, nbins, generator=g) * 13.0 - 7.0
    x[:, off:off + nbins] = torch.rand(M, nbins, generator=g) * 120.0 - 60.0
    x[0, off:off + 5] = torch.tensor([0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi])
    clipped = (torch.exp(x[:, :nbins].double()) > 100.0).float().mean().item()
    assert clipped >= 0.05 and 1.0 - clipped >= 0.5, clipped
    dx, tail = guarded((M, ld))
    dx.copy_(x)
    hip.spec_polar(dx, nbins, off, 1e2)
    torch.cuda.synchronize()
    out = dx.cpu()
    assert untouched(tail) and (out[:, nbins:off] == SENT).all() and (out[:, off + nbins:] == SENT).all()
    ref, cpu = G.spec_polar(x.double(), nbins, off), G.spec_polar(x, nbins, off)
    mag = torch.clamp(torch.exp(x[:, :nbins].double()), max=100.0)
    cols = torch.cat([torch.arange(nbins), off + torch.arange(nbins)])
    measured(f"spec_polar M={M} nbins={nbins}", out[:, cols], ref[:, cols], cpu[:, cols], scale=torch.cat([mag, mag], dim=1), floor_at=1.0)


# ------------------------------------------------------------------------------------------------ overlap-add
OLA = [(16, 4, 2), (16, 4, 9), (32, 8, 7), (64, 32, 5), (64, 16, 3), (16, 8, 2), (16, 16, 4), (1024, 256, 3)]


def ola_run(hip, frames, window, hop, lengths=None):
    B, T, n_fft = frames.shape
    audio, tail = guarded((B, hop * (T - 1)))
    hip.istft_ola(frames.view(B * T, n_fft).cuda().contiguous(), window.cuda(), B, T, hop,
                  lengths=None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda"), out=audio)
    torch.cuda.synchronize()
    assert untouched(tail)
    return audio.cpu()


@pytest.mark.parametrize("n_fft,hop,T", OLA)
def test_istft_ola_plain(hip, n_fft, hop, T):
    """hop ratios 1, 2, 4; random frames (not the output of a DFT), so that an indexing error cannot cancel."""
    frames = torch.randn(2, T, n_fft, generator=gen(n_fft + hop + T))
    window = torch.hann_window(n_fft)
    out = ola_run(hip, frames, window, hop)
    ref, env = G.istft_ola(frames.double(), window.double(), hop)
    cpu, env32 = G.istft_ola(frames, window, hop)
    if hop == n_fft:
        assert (env32 <= 1e-11).sum().item() == 2 * (T - 1)          # the undivided branch is reached: pos a multiple of n_fft
        keep = env32 <= 1e-11
        assert torch.equal(out[keep], cpu[keep])
    else:
        assert (env32 > 1e-11).all()
    measured(f"istft_ola n_fft={n_fft} hop={hop} T={T}", out, ref, cpu)


def test_istft_ola_ragged(hip):
    """Each row is the plain result of its own frames (the frames beyond are NaN), then exact zeros up to hop * (T - 1)."""
    n_fft, hop, T, lengths = 32, 8, 7, [7, 4, 2, 1, 0, 9]
    frames = torch.randn(6, T, n_fft, generator=gen(9))
    for b, n in enumerate(lengths):
        frames[b, G.clamp_len(n, T):] = NAN
    window = torch.hann_window(n_fft)
    out = ola_run(hip, frames, window, hop, lengths)
    ref = torch.zeros(6, hop * (T - 1), dtype=torch.float64)
    cpu = torch.zeros(6, hop * (T - 1))
    for b, n in enumerate(lengths):
        n = G.clamp_len(n, T)
        Lb = hop * max(n - 1, 0)
        if n >= 2:
            ref[b, :Lb] = G.istft_ola(frames[b:b + 1, :n].double(), window.double(), hop)[0][0]
            cpu[b, :Lb] = G.istft_ola(frames[b:b + 1, :n], window, hop)[0][0]
        assert (out[b, Lb:] == 0).all(), b
    assert torch.isfinite(out).all()
    measured("istft_ola ragged", out, ref, cpu)


# ------------------------------------------------------------------------------------------------ rk4 stage combinations
def combine_case(M, C, ldy, ldk, ldo, seed):
    g = gen(seed)
    pad = lambda ld: torch.cat([torch.randn(M, C, generator=g), torch.full((M, ld - C), NAN)], dim=1)      # columns >= C are never read
    return pad(ldy), [pad(ldk) for _ in range(4)]


@pytest.mark.parametrize("per_utt", [False, True])
@pytest.mark.parametrize("stage", [0, 1, 2, 3, 4])
def test_ode_combine_bit_equal(hip, stage, per_utt):
    """Bit-equal to fp32 torch in torchdiffeq's operation order; three different leading dimensions, all larger than C; one dt, or one
    per utterance.  The grid-stride loop's second trip at M * C > 2048 * 256."""
    for (B, T, C, ldy, ldk, ldo) in [(2, 5, 37, 40, 48, 44), (2, 550, 480, 484, 488, 492)]:
        M = B * T
        y, ks = combine_case(M, C, ldy, ldk, ldo, seed=stage + 10 * per_utt + C)
        dts = torch.tensor([0.1, -0.25])
        dt_cpu = dts.repeat_interleave(T)[:, None] if per_utt else dts[0]
        ref = G.ode_combine(stage, dt_cpu, y[:, :C], *[k[:, :C] for k in ks])
        assert torch.isfinite(ref).all()
        out, tail = guarded((M, ldo))
        hip.ode_combine(stage, dts.cuda() if per_utt else 0.1, y.cuda(), *[k.cuda() for k in ks], C=C, out=out, T=T)
        torch.cuda.synchronize()
        got = out.cpu()
        assert untouched(tail) and (got[:, C:] == SENT).all()
        assert torch.equal(got[:, :C], ref), (stage, per_utt, M, (got[:, :C] - ref).abs().max().item())


@pytest.mark.parametrize("per_utt", [False, True])
@pytest.mark.parametrize("stage", [0, 4])
def test_ode_combine_in_place(hip, stage, per_utt):
    """out = y with ldo = ldy: the aliasing of the solver's call sites (decoder.hip: the last rk4 stage writes the state it read;
    stages 1..3 write the second state buffer); stage 0, the plain axpy, is held to the same."""
    B, T, C, ldy, ldk = 2, 5, 37, 40, 48
    y, ks = combine_case(B * T, C, ldy, ldk, ldy, seed=50 + stage)
    dts = torch.tensor([0.1, -0.25])
    ref = G.ode_combine(stage, dts.repeat_interleave(T)[:, None] if per_utt else dts[0], y[:, :C], *[k[:, :C] for k in ks])
    dy = y.cuda()
    hip.ode_combine(stage, dts.cuda() if per_utt else 0.1, dy, *[k.cuda() for k in ks], C=C, out=dy, T=T)
    torch.cuda.synchronize()
    assert torch.equal(dy.cpu()[:, :C], ref) and torch.isnan(dy.cpu()[:, C:]).all()


# ------------------------------------------------------------------------------------------------ step tables
@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("stages", [1, 2, 4])
def test_step_tables_bit_equal(hip, stages, T):
    B = 3
    t0, t1 = torch.tensor([0.0, 0.3, 0.9]), torch.tensor([1.0, 0.4, 1.0])
    mask = (torch.arange(T)[None, :] < torch.tensor([T, (T + 1) // 2, 0 if T > 1 else 1])[:, None]).float()
    tv, tail_tv = guarded((stages * B,))
    dt_b, tail_dt = guarded((B,))
    rf, tail_rf = guarded((B * T,))
    rh, tail_rh = guarded((B * T,))
    hip.step_tables(t0.cuda(), t1.cuda(), mask.cuda(), stages, out=(tv, dt_b, rf, rh))
    torch.cuda.synchronize()
    assert all(untouched(t) for t in (tail_tv, tail_dt, tail_rf, tail_rh))
    r_tv, r_dt, r_rf, r_rh = G.step_tables(t0, t1, mask, stages)
    assert torch.equal(tv.cpu(), r_tv) and torch.equal(dt_b.cpu(), r_dt) and torch.equal(rf.cpu(), r_rf) and torch.equal(rh.cpu(), r_rh)
    if stages == 4:                                         # t0 + dt * fp32(1/3), t0 + dt * fp32(2/3), written out
        dt = t1 - t0
        third, two_thirds = torch.tensor(1.0 / 3.0), torch.tensor(2.0 / 3.0)
        assert third.item() == 0.3333333432674408 and two_thirds.item() == 0.6666666865348816
        assert torch.equal(tv.cpu()[B:2 * B], t0 + dt * third) and torch.equal(tv.cpu()[2 * B:3 * B], t0 + dt * two_thirds)
        assert torch.equal(tv.cpu()[3 * B:], t1)


# ------------------------------------------------------------------------------------------------ time sinusoid
TIMES = [0.0, 1e-4, 0.37, 0.5, 0.999, 1.0]


def times(nt, seed):
    t = torch.rand(nt, generator=gen(seed))
    k = min(nt, len(TIMES))
    t[:k] = torch.tensor(TIMES[-k:] if nt < len(TIMES) else TIMES)
    return t


@pytest.mark.parametrize("half", [1, 64, 129])
def test_time_sinusoid_both_forms(hip, half):
    """The argument (scale * t) * f is the fp32 product formed on the CPU, bit for bit: the reference is sin / cos in fp64 OF THAT fp32
    argument, and an argument formed in another order is off by an ulp of 1000, a hundred times the bound.  More than one trip of the
    128-thread loop at half = 129; host and device forms give the same bits."""
    freqs = hip.time_freqs(2 * half) if half > 1 else torch.ones(1)
    for nt, dev_form in ((1, False), (5, False), (256, False), (256, True), (300, True)):
        t = times(nt, seed=half + nt)
        out, tail = guarded((nt, 2 * half))
        hip.time_sinusoid(freqs.cuda(), t.cuda() if dev_form else t, 1000.0, out=out)
        torch.cuda.synchronize()
        assert untouched(tail)
        arg = G.sinusoid_arg(freqs, t, 1000.0)
        got = out.cpu()
        measured(f"time_sinusoid half={half} nt={nt} {'dev' if dev_form else 'host'}", got, G.sinusoid(arg.double()), G.sinusoid(arg), floor_at=1.0)
        if nt == 256 and not dev_form:
            host256 = got
        if nt == 256 and dev_form:
            assert torch.equal(got, host256)


def test_time_sinusoid_argument_is_scale_times_t_in_fp32(hip):
    """half = 1, f = 1: the kernel's argument is fp32(1000 * t); sin of the fp64 product would differ by up to 3e-5."""
    t = times(256, seed=3)
    out = hip.time_sinusoid(torch.ones(1).cuda(), t, 1000.0).cpu()
    arg32 = (1000.0 * t).double()
    assert (torch.sin(arg32) - torch.sin(1000.0 * t.double())).abs().max().item() > 1e-5
    measured("time_sinusoid argument", out, torch.stack([torch.sin(arg32), torch.cos(arg32)], dim=1), G.sinusoid((1000.0 * t)[:, None]), floor_at=1.0)


# ------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("B,T,H,D,d", [(2, 5, 2, 8, 4), (1, 70, 3, 64, 32), (2, 9, 1, 6, 6)])
def test_rope(hip, B, T, H, D, d):
    """A different table row per position, B*T rows of them so that a `row` in place of `row % T` reads other positions' values; the
    value section and each head's dims >= d_rope keep their bits."""
    qkv = torch.randn(B * T, 3 * H * D, generator=gen(T))
    cos, sin = hip.rope_tables(d, B * T)
    buf, tail = guarded((B * T, 3 * H * D))
    buf.copy_(qkv)
    hip.rope(buf, B, T, H, D, d, cos.cuda(), sin.cuda())
    torch.cuda.synchronize()
    out = buf.cpu()
    assert untouched(tail)
    o5, q5 = out.view(B, T, 3, H, D), qkv.view(B, T, 3, H, D)
    assert torch.equal(o5[:, :, 2], q5[:, :, 2]) and torch.equal(o5[..., d:], q5[..., d:])
    assert not torch.equal(o5[:, 1:, :2, :, :d], q5[:, 1:, :2, :, :d]) or T == 1
    measured(f"rope B={B} T={T} H={H} D={D} d={d}", out, G.rope(qkv.double(), B, T, H, D, d, cos.double(), sin.double()),
             G.rope(qkv, B, T, H, D, d, cos, sin))


# ------------------------------------------------------------------------------------------------ layout moves
CT = [(1, 1), (31, 33), (32, 32), (33, 31), (80, 70)]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("C,T", CT)
def test_cf_to_cl(hip, C, T, with_add, ragged):
    B, ld, off = 3, C + 8, 4
    g = gen(C * T)
    src, add = torch.randn(B, C, T + 3, generator=g), torch.randn(B, C, T + 3, generator=g)
    lengths = [T, T // 2, 1] if ragged else None
    for b in range(B):
        n = lengths[b] if ragged else T
        src[b, :, n:] = NAN                                 # past the length (and past T): never read as data
        add[b, :, n:] = NAN
    dst, tail = guarded((B * T, ld))
    hip.cf_to_cl(src.cuda(), dst, T=T, col_off=off, add=add.cuda() if with_add else None,
                 lengths=torch.tensor(lengths, dtype=torch.int64, device="cuda") if ragged else None)
    torch.cuda.synchronize()
    ref = G.cf_to_cl(src, torch.full((B * T, ld), SENT), T, off, add if with_add else None, lengths)
    out = dst.cpu()
    assert untouched(tail) and torch.isfinite(out).all() and torch.equal(out, ref)
    if ragged:
        assert (out.view(B, T, ld)[1, T // 2:, off:off + C] == 0).all() and (out.view(B, T, ld)[2, 1:, off:off + C] == 0).all()


@pytest.mark.parametrize("C,T", CT)
def test_cl_to_cf_and_round_trip(hip, C, T):
    B, ld = 3, C + 8
    T_out = T - 2 if T > 2 else T
    src = torch.randn(B * T, ld, generator=gen(C + T))
    src[:, C:] = NAN
    src.view(B, T, ld)[:, T_out:] = NAN
    dst, tail = guarded((B, C, T_out))
    hip.cl_to_cf(src.cuda(), dst, T=T, scale=2.5, shift=-5.5)
    torch.cuda.synchronize()
    ref = G.cl_to_cf(src, B, C, T, T_out) * torch.tensor(2.5) + torch.tensor(-5.5)
    assert untouched(tail) and torch.equal(dst.cpu(), ref)
    # cf_to_cl then cl_to_cf (scale 1, shift 0) is the identity
    x = torch.randn(B, C, T, generator=gen(C)).cuda()
    rows, _ = guarded((B * T, ld))
    back, _ = guarded((B, C, T))
    hip.cf_to_cl(x, rows, col_off=0)
    hip.cl_to_cf(rows, back, T=T)
    assert torch.equal(back, x)
    # and the other way round on the C columns
    rows2, _ = guarded((B * T, ld))
    hip.cf_to_cl(back, rows2, col_off=0)
    assert torch.equal(rows2[:, :C], rows[:, :C])


@pytest.mark.parametrize("C,T", CT)
def test_slot_moves(hip, C, T):
    """One live slot, two out of range: the load writes zero rows for the dead ones, the store leaves the whole pool outside slot 3's
    [C, :T] region bit-identical to its fill."""
    B, S, T_pool, ld, off = 3, 5, T + 2, C + 8, 4
    slots = [3, -1, 5]
    d_slots = torch.tensor(slots, dtype=torch.int32, device="cuda")
    pool = torch.randn(S, C, T_pool, generator=gen(C + 2 * T))
    pool[:, :, T:] = NAN
    dst, tail = guarded((B * T, ld))
    hip.slots_to_cl(pool.cuda(), d_slots, dst, T=T, col_off=off)
    torch.cuda.synchronize()
    ref = G.slots_to_cl(pool, slots, torch.full((B * T, ld), SENT), T, off)
    assert untouched(tail) and torch.equal(dst.cpu(), ref) and (dst.cpu().view(B, T, ld)[1:, :, off:off + C] == 0).all()
    src = torch.randn(B * T, ld, generator=gen(C + 3 * T))
    src[:, C:] = NAN
    dpool, ptail = guarded((S, C, T_pool))
    hip.cl_to_slots(src.cuda(), dpool, d_slots, T=T)
    torch.cuda.synchronize()
    want = G.cl_to_slots(src, torch.full((S, C, T_pool), SENT), slots, T)
    assert untouched(ptail) and torch.equal(dpool.cpu(), want)
    assert (dpool.cpu()[[0, 1, 2, 4]] == SENT).all() and (dpool.cpu()[3, :, T:] == SENT).all()
    # load then store into a fresh pool gives back slot 3
    rows, _ = guarded((B * T, ld))
    hip.slots_to_cl(pool.cuda(), d_slots, rows, T=T, col_off=0)
    again, _ = guarded((S, C, T_pool))
    hip.cl_to_slots(rows, again, d_slots, T=T)
    assert torch.equal(again.cpu()[3, :, :T], pool[3, :, :T])


# ------------------------------------------------------------------------------------------------ durations, alignment
@pytest.fixture(scope="module")
def model(hip):
    return hip.HipModel(sub("hparams").tiny())              # durations / alignment need no weights


def x_lengths(Tx):
    return torch.tensor([Tx, max(1, (2 * Tx) // 3), 1])


@pytest.mark.parametrize("Tx", [1, 256, 257, 600])
def test_durations_scan_against_cumsum(model, oracle, Tx):
    """At most one element per scanning thread (Tx <= 256) and the chunked scan (per = 2 at 257, 3 at 600); scalar and per-utterance
    factors; bit-equal to the oracle and an int64 cumsum."""
    B = 3
    g = gen(Tx)
    d_int = torch.randint(1, 9, (B, Tx), generator=g).float()
    logw = torch.log(d_int + 2.0).unsqueeze(1)
    x_mask = oracle.sequence_mask(x_lengths(Tx), Tx).unsqueeze(1).float()
    col = lambda v: torch.tensor(v)[:, None]
    for sc, ls in ((1.0, 1.0), (1.08, 0.9), ([1.0, 1.08, 1.03], [1.0, 0.9, 2.0])):
        per_utt = isinstance(sc, list)
        ref = oracle.durations_from_logw(logw, x_mask, col(sc) if per_utt else sc, col(ls) if per_utt else ls)
        dur, cum, yfl = model.durations(logw.cuda(), x_mask.cuda(), sc, ls)
        assert torch.equal(dur.cpu(), ref), (Tx, sc, ls)
        assert torch.equal(cum.cpu().long(), torch.cumsum(ref.long(), 1)), (Tx, sc, ls)
        assert torch.equal(yfl.cpu(), ref.long().sum(1).clamp_min(1))


def given_case(Tx, oracle):
    B = 3
    g = gen(1000 + Tx)
    x_mask = oracle.sequence_mask(x_lengths(Tx), Tx).unsqueeze(1).float()
    given = torch.randint(0, 5, (B, Tx), generator=g).float()
    given[torch.rand(B, Tx, generator=g) < 0.3] = 0.0                          # runs of tokens without frames
    ties = torch.tensor([0.5, 1.5, 2.5, 3.5, -1.0, 0.0, 0.0, 0.0, 2.0, -0.5])
    k = min(Tx, ties.numel())
    given[0, :k] = ties[:k]
    if Tx > 20:
        given[1, 5:12] = 0.0
    return given, x_mask


@pytest.mark.parametrize("Tx", [1, 256, 257, 600])
def test_durations_given_rows_and_alignment(model, oracle, Tx):
    """Zeros, .5 ties (to even), a negative value; given_rows = [1, 0, 1]: the middle row keeps what dur held and is scanned again;
    then align_pool on those durations: runs of empty tokens make ties in the search for the first cumulative value above a frame."""
    B, nf = 3, 20
    given, x_mask = given_case(Tx, oracle)
    m = x_mask.squeeze(1)
    for ls in (1.0, [1.0, 2.0, 0.5]):
        lsc = torch.tensor(ls)[:, None] if isinstance(ls, list) else ls
        ref = torch.clamp_min(torch.round(given * lsc), 0.0) * m
        dur, cum, yfl = model.durations_given(given.cuda(), x_mask.cuda(), ls)
        assert torch.equal(dur.cpu(), ref) and torch.equal(cum.cpu().long(), torch.cumsum(ref.long(), 1))
        assert torch.equal(yfl.cpu(), ref.long().sum(1).clamp_min(1))
    if Tx >= 10:
        assert (ref == 0)[m > 0].any() and ((given * 2) % 2 == 1).any() and (given < 0).any()
    # a mixed batch: the predictor's durations first, then rows 0 and 2 replaced
    d_int = torch.randint(1, 9, (B, Tx), generator=gen(Tx + 7)).float()
    pred, _, _ = model.durations(torch.log(d_int + 2.0).unsqueeze(1).cuda(), x_mask.cuda(), 1.0, 1.0)
    kept = pred.cpu().clone()
    dur, cum, yfl = model.durations_given(given.cuda(), x_mask.cuda(), 1.0, given_rows=[1, 0, 1], out=pred)
    ref = torch.clamp_min(torch.round(given), 0.0) * m
    ref[1] = kept[1]
    assert dur.data_ptr() == pred.data_ptr() and torch.equal(dur.cpu(), ref)
    assert torch.equal(cum.cpu().long(), torch.cumsum(ref.long(), 1)) and torch.equal(yfl.cpu(), ref.long().sum(1).clamp_min(1))
    # alignment + pooling on these durations, a few frames beyond the longest utterance
    mu_x = torch.randn(B, nf, Tx, generator=gen(Tx + 9)) * x_mask
    t_pad = int((yfl.max().item() + 1) // 2) + 3
    mu_y, y_mask, y_len = model.align_pool(mu_x.cuda(), cum, yfl, t_pad)
    r_mu, r_mask, r_len = G.align_pool(mu_x.double(), ref.double(), t_pad)
    c_mu, _, _ = G.align_pool(mu_x, ref, t_pad)
    assert torch.equal(y_len.cpu(), r_len) and torch.equal(y_mask.cpu().double(), r_mask)
    measured(f"align_pool Tx={Tx}", mu_y.cpu(), r_mu, c_mu)
    o_mu, o_mask, o_len, _, o_pad = oracle.align_and_pool(mu_x.double(), ref.double(), x_mask.double())
    n = min(o_pad, t_pad)
    assert torch.equal(o_len, r_len) and (o_mu[:, :, :n] - r_mu[:, :, :n]).abs().max().item() < 1e-13

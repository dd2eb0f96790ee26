"""CPU checks of the unit entries of the default arithmetic's two-plane (P16) kernels (csrc/unit_entries.hip: mtts_gemm_p16_args_run,
mtts_attention_p16_run, mtts_groupnorm_mish_p16, mtts_to_p16_roundtrip; nothing runs on a GPU): the binding itself is checked for every
entry in test_abi.py; here: every refusal that can be decided on the host
returns -1 with a message before anything is launched (the buffers named here are never touched); and the restatement of the
split the GPU file measures against (tests/p16_restated.py) gives the hand-worked values: ties, 1 + 2^-11, subnormal residuals at
lscale 1, +-65504, values beyond the range, signed zeros, and is value-idempotent."""
import ctypes as C

import pytest
import torch

from conftest import sub
from p16_restated import heads, image_bits, p16, split

FAKE = 0x1000          # a non-null "pointer" for buffers a refused call must not touch


@pytest.fixture(scope="module")
def hip():
    h = sub("_hip")
    h.build()
    h.load()
    return h


@pytest.fixture(scope="module")
def lib(hip):
    return hip.load()


def test_new_entries_are_declared_exported_and_bound_with_matching_arity_and_types(hip, lib):
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_abi_version() == 2
    for wrapper in ("gemm_p16_args", "attention_p16_run", "groupnorm_mish_p16", "to_p16_roundtrip", "tblock_chain_args", "conv_gn_args"):
        assert callable(getattr(hip, wrapper))


def gemm_block(hip, **kw):
    g = hip.MttsGemmH16Args()
    base = dict(d_a=FAKE, lda=128, C=128, B=1, T_in=64, T_out=64, ntaps=1, in_stride=1, h_w=FAKE, N=128, out_scale=1.0, d_out=FAKE,
                wave_rows=77)
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("kw,fast16,lscale,needle", [
    (dict(half16=1), 0, 2048.0, "two-plane"),
    (dict(bf16=1), 0, 2048.0, "two-plane"),
    (dict(half16=1, bf16=1), 0, 2048.0, "two-plane"),
    (dict(C=80, lda=80), 0, 2048.0, "C % 32"),
    (dict(C=128, c1=48), 0, 2048.0, "C % 32"),
    (dict(C=128, c1=128), 0, 2048.0, "c1 < C"),
    (dict(d_gn_stats=FAKE, gn_groups=4), 1, 2048.0, "gn_stats with fast16"),
    (dict(d_gn_stats=FAKE, gn_groups=4, act=3, d_p0=FAKE, d_p1=FAKE), 0, 2048.0, "gn_stats with an activation"),
    (dict(d_gn_stats=FAKE, gn_groups=4, d_a_part=FAKE, a_nparts=2), 0, 2048.0, "gn_stats with an activation"),
    (dict(res16_mode=1, d_res16_f32=FAKE, d_res=FAKE, ldr=128), 0, 2048.0, "res16 together with res"),
    (dict(res16_mode=2), 0, 2048.0, "in place"),
    (dict(res16_mode=2, d_out16_f32=FAKE, out16_preload=1), 0, 1.0, "in place"),
    (dict(res16_mode=1), 0, 2048.0, "d_res16_f32"),
    (dict(d_a=None), 0, 2048.0, "null buffer"),
    (dict(h_w=None), 0, 2048.0, "null buffer"),
    (dict(d_out=None), 0, 2048.0, "null buffer"),
    (dict(d_out16_f32=FAKE, N=100), 0, 2048.0, "N % 32"),
    (dict(ntaps=9), 0, 2048.0, "ntaps"),
    (dict(ntaps=3), 0, 2048.0, "tap offsets"),
    (dict(out_T=64, out_stride=2, out_off=0), 0, 2048.0, "output rows"),
    (dict(lda=100), 0, 2048.0, "lda"),
    (dict(), 2, 2048.0, "fast16 is 0 or 1"),
    (dict(), 0, 1024.0, "out_lscale"),
])
def test_gemm_refusals_before_any_launch(hip, lib, kw, fast16, lscale, needle):
    g = gemm_block(hip, **kw)
    assert lib.mtts_gemm_p16_args_run(C.byref(g), fast16, lscale, FAKE, None) == -1
    assert needle.encode() in lib.mtts_last_error(), lib.mtts_last_error()
    assert g.wave_rows == 0 and g.tag == b""                 # the block's last fields sit where the library writes them


def test_gemm_null_scratch_and_block(hip, lib):
    assert lib.mtts_gemm_p16_args_run(C.byref(gemm_block(hip)), 0, 2048.0, None, None) == -1
    assert b"null buffer" in lib.mtts_last_error()
    assert lib.mtts_gemm_p16_args_run(None, 0, 2048.0, FAKE, None) == -1
    assert lib.mtts_gemm_p16_args_scratch_bytes(None) == -1
    g = gemm_block(hip, d_out16_f32=FAKE)
    need = lib.mtts_gemm_p16_args_scratch_bytes(C.byref(g))
    # A image, output and residual images (4 bytes per element each), fp32 panel, its two planes, row sums
    assert need >= 64 * 128 * 4 + 2 * 64 * 128 * 4 + 2 * 128 * 128 * 4 + 128 * 4
    # the existing entry still refuses the two-plane request (tests/test_h16_abi.py), the new one the one-plane request
    assert lib.mtts_gemm_h16(C.byref(gemm_block(hip)), FAKE, None) == -1 and b"half16" in lib.mtts_last_error()


def test_other_entries_refuse_on_the_host(lib):
    # conversions: C % 32, null buffers, C_valid beyond C, an image row shorter than 2 * C, a scale that no image uses
    rt = lambda x=FAKE, ld=64, M=4, Cc=64, cv=64, ld16=128, ls=2048.0, img=FAKE: lib.mtts_to_p16_roundtrip(x, ld, None, M, Cc, cv, ld16, ls, img, FAKE, None, None)
    assert rt(Cc=48, ld=48, cv=48, ld16=96) == -1 and b"C % 32" in lib.mtts_last_error()
    assert rt(x=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert rt(img=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert rt(cv=68) == -1 and b"C_valid" in lib.mtts_last_error()
    assert rt(ld16=64) == -1 and b"stride" in lib.mtts_last_error()           # ld16 < 2 * C: one plane's worth
    assert rt(ls=4096.0) == -1 and b"lscale" in lib.mtts_last_error()
    assert rt(M=0) == -1
    # attention: head dim 64 only, null buffers, boolean mode without a mask, fast16 and out_lscale values
    at = lambda **k: lib.mtts_attention_p16_run(k.get("q", FAKE), k.get("mask"), None, 1, 64, 2, k.get("D", 64), 0.125, k.get("mode", 0),
                                                k.get("fast", 0), k.get("ls", 2048.0), FAKE, None, k.get("scratch", FAKE), None)
    assert at(D=48) == -1 and b"D == 64" in lib.mtts_last_error()
    assert at(scratch=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert at(q=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert at(mode=1) == -1 and b"needs a mask" in lib.mtts_last_error()
    assert at(fast=3) == -1 and b"fast16" in lib.mtts_last_error()
    assert at(ls=2.0) == -1 and b"out_lscale" in lib.mtts_last_error()
    # GroupNorm: C % 32, null buffers, folded padding needs both of its arrays, tile statistics need their tile height
    gn = lambda **k: lib.mtts_groupnorm_mish_p16(k.get("y", FAKE), FAKE, FAKE, FAKE, k.get("chb"), k.get("cs", 0), 2, 64, k.get("C", 384), 8, 1e-5,
                                                 k.get("ts"), k.get("tr", 0), None, k.get("nextra"), k.get("bs"), None, None,
                                                 k.get("o16", FAKE), None, FAKE, None)
    assert gn(C=80) == -1 and b"C % 32" in lib.mtts_last_error()
    assert gn(y=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(o16=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(nextra=FAKE) == -1 and b"nextra" in lib.mtts_last_error()
    assert gn(bs=FAKE) == -1 and b"nextra" in lib.mtts_last_error()
    assert gn(ts=FAKE, tr=0) == -1 and b"tile_rows" in lib.mtts_last_error()
    assert gn(chb=FAKE, cs=380) == -1 and b"bias row" in lib.mtts_last_error()
    assert lib.mtts_groupnorm_p16_scratch_bytes(2, 64, 384, 8) >= 2 * 64 * 384 * 4
    assert lib.mtts_groupnorm_p16_scratch_bytes(0, 64, 384, 8) == -1


# ------------------------------------------------------------------------------------------------ the restated split
def bits16(t):
    return [int(v) & 0xffff for v in t.view(torch.int16).tolist()]


def test_split_on_hand_worked_values_scale_2048():
    u = 2.0 ** -11                                       # half an ulp of fp16 at 1
    x = torch.tensor([1.0, 1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u), 1 + u + 2.0 ** -22, 1 + u - 2.0 ** -22, 1 + 2.0 ** -22, 1 + 2.0 ** -23])
    h, l = split(x)
    #            1       tie -> even (1)  tie -> even (1 + 2^-9)  and their mirror images   just above / below the tie        22 bits kept, the 23rd lost
    assert bits16(h) == [0x3C00, 0x3C00, 0x3C02, 0xBC00, 0xBC02, 0x3C01, 0x3C00, 0x3C00, 0x3C00]
    # residuals times 2048: 0, +1 (2^-11 * 2^11), -1, -1, +1, -(1 - 2^-11), 1 - 2^-11, 2^-11, 2^-12
    assert l.tolist() == [0.0, 1.0, -1.0, -1.0, 1.0, -(1 - 2.0 ** -11), 1 - 2.0 ** -11, 2.0 ** -11, 2.0 ** -12]
    v = p16(x)
    assert torch.equal(v[:8], x[:8])                     # every value with <= 22 significant bits is held exactly
    assert v[8].item() == 1 + 2.0 ** -23                 # (so is this one: the residual has its own exponent)
    y = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -23])      # 13 significant residual bits: the residual rounds to 11
    assert p16(y).item() == 1 + 2.0 ** -11 and p16(y).item() != y.item()


def test_split_range_zeros_and_subnormal_residuals():
    x = torch.tensor([65504.0, -65504.0, 65519.9, 65520.0, -70000.0, 1.0e9, -3.0e38, 0.0, -0.0])
    h, l = split(x)
    assert bits16(h) == [0x7BFF, 0xFBFF, 0x7BFF, 0x7BFF, 0xFBFF, 0x7BFF, 0xFBFF, 0x0000, 0x8000]      # the clamp, never inf
    assert (l == 0).all()                                # the residual is taken from the CLAMPED value
    assert p16(x).tolist() == [65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0, 0.0, 0.0]
    assert torch.isinf(x.to(torch.float16)).sum().item() == 4          # where torch's own conversion overflows
    # the largest residual: just below 65504's upper neighbour's tie, (16 - eps) * 2048 still fits fp16
    big = torch.tensor([65504.0 - 16.0 + 2.0 ** -7])
    assert torch.isfinite(split(big)[1]).all() and p16(big).item() == big.item()
    # lscale 1 (the attention's q|k|v image): residuals below 2^-14 are fp16 subnormals, below 2^-25 they vanish
    s = torch.tensor([1 + 2.0 ** -12, 2.0 ** -3 + 2.0 ** -15, 2.0 ** -3 + 2.0 ** -24, 2.0 ** -3 + 2.0 ** -25, 2.0 ** -3 + 3 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -26])
    h1, l1 = split(s, 1.0)
    assert bits16(l1) == [0x0C00, 0x0200, 0x0001, 0x0000, 0x0002, 0x0000]      # 2^-12; subnormals 2^-15, 2^-24; tie to zero; tie to even; lost
    assert p16(s, 1.0).tolist() == [1 + 2.0 ** -12, 2.0 ** -3 + 2.0 ** -15, 2.0 ** -3 + 2.0 ** -24, 2.0 ** -3, 2.0 ** -3 + 2.0 ** -24 * 2, 2.0 ** -14]
    # ... the scaled residual keeps them all (why GEMM operands use 2048)
    assert torch.equal(p16(s[:5]), s[:5])
    # fp16-subnormal heads
    t = torch.tensor([2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1.0e-40])
    assert bits16(split(t)[0]) == [0x0001, 0x0000, 0x0002, 0x0000]
    assert p16(t).tolist()[:3] == [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25]      # the residual brings back what the head lost
    assert heads(t).tolist() == [2.0 ** -24, 0.0, 2.0 ** -23, 0.0]


def test_split_is_value_idempotent_and_22_bits_wide():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1 << 16, generator=g) * torch.exp(torch.empty(1 << 16).uniform_(-12, 11, generator=g))
    u = 2.0 ** -11
    x[:6] = torch.tensor([1 + 3 * u - 2.0 ** -23, 1 + u - 2.0 ** -23, -(1 + 3 * u - 2.0 ** -23), 65504.0, -1.0e6, 2.0 ** -20])
    for ls in (2048.0, 1.0):
        v = p16(x, ls)
        again = p16(v, ls)
        nz = v != 0
        assert torch.equal(again.view(torch.int32)[nz], v.view(torch.int32)[nz]), ls
        # the one exception is the sign of zero: a negative value too small for either plane is held as -0 + -0 = -0, and -0 as -0 + +0 = +0
        assert (again[~nz].view(torch.int32) == 0).all()
        assert (v[~nz].view(torch.int32) < 0).any() == (ls == 1.0)      # (with the scaled residual nothing of this sample is that small)
    # (the PAIR is not a fixed point: a value that rounds onto a tie of the head splits differently the second time, same sum)
    v = p16(x[:1])
    assert v.item() == 1 + 3 * u and bits16(split(x[:1])[0]) == [0x3C01] and bits16(split(v)[0]) == [0x3C02]
    inside = (x.abs() < 65504.0) & (x.abs() > 1.0e-3)      # (below, the scaled residual itself becomes an fp16 subnormal)
    rel = ((p16(x).double() - x.double()).abs() / x.double().abs())[inside]
    assert 0.0 < rel.max().item() <= 2.0 ** -22
    assert ((heads(x).double() - x.double()).abs() / x.double().abs())[inside].max().item() > 2.0 ** -12.1


def test_image_layout_is_heads_then_residuals_per_32_channels():
    x = torch.arange(2 * 64, dtype=torch.float32).view(2, 64) + 2.0 ** -12
    img = image_bits(x)
    assert img.shape == (2, 128)
    h, l = split(x)
    assert torch.equal(img[:, 0:32], h[:, 0:32].view(torch.int16)) and torch.equal(img[:, 32:64], l[:, 0:32].view(torch.int16))
    assert torch.equal(img[:, 64:96], h[:, 32:64].view(torch.int16)) and torch.equal(img[:, 96:128], l[:, 32:64].view(torch.int16))

"""CPU checks of the unit entries of the fp32-row flow (csrc/unit_entries.hip: mtts_gemm_f32_args_run, mtts_attention_f32_run,
mtts_groupnorm_mish_f32_run, mtts_channel_layernorm_ld; nothing runs on a GPU): the binding itself is checked for every entry in
test_abi.py; here: every refusal that can be decided on the host returns -1 with a message before
anything is launched (the buffers named here are never touched); the restatement the GPU file measures against
(tests/f32_restated.py) agrees with independent torch code -- F.conv1d, F.conv_transpose1d for the two-phase interleave,
F.group_norm + F.mish on explicitly padded rows for nextra, F.layer_norm, the oracle's sdpa_reference -- and the input classes the
GPU file's cases claim are really present in what it launches."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import f32_restated as R
from conftest import ROOT, sub
from p16_restated import p16, split

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
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    for wrapper in ("gemm_f32_args", "attention_f32_run", "groupnorm_mish_f32_run", "channel_layernorm_ld", "guarded", "rows_ptr"):
        assert callable(getattr(hip, wrapper))
    assert lib.mtts_last_kernel_tag() == b""           # no launcher ran on this thread


def gemm_block(hip, **kw):
    g = hip.MttsGemmH16Args()
    base = dict(d_a=FAKE, lda=128, C=128, B=1, T_in=64, T_out=64, ntaps=1, in_stride=1, h_w=FAKE, N=128, out_scale=1.0, d_out=FAKE, wave_rows=77)
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


TAPS = (C.c_int32 * 3)(1, 0, -1)
@pytest.mark.parametrize("kw,call,needle", [
    (dict(d_a=None), {}, "null buffer"),
    (dict(h_w=None), {}, "null buffer"),
    (dict(d_out=None), {}, "null buffer"),
    (dict(half16=1), {}, "fp32-row"),
    (dict(bf16=1), {}, "fp32-row"),
    (dict(), dict(terms=3), "terms must be 0, 2 or 6"),
    (dict(), dict(terms=1), "terms must be 0, 2 or 6"),
    (dict(), dict(out_lscale=1024.0), "out_lscale"),
    (dict(res16_mode=1), {}, "res16"),
    (dict(d_res16_f32=FAKE), {}, "res16"),
    (dict(out16_preload=1), {}, "res16"),
    (dict(d_gn_stats=FAKE, gn_groups=8), {}, "gn_stats"),
    (dict(d_gnr_y=FAKE), {}, "gnr"),
    (dict(ntaps=9), {}, "ntaps"),
    (dict(ntaps=0), {}, "ntaps"),
    (dict(N=0), {}, "bad shape"),
    (dict(T_in=0), {}, "bad shape"),
    (dict(C=130, lda=132), {}, "multiples of 4"),
    (dict(c1=6), {}, "multiples of 4"),
    (dict(c1=128), {}, "c1 < C"),
    (dict(c1=28), {}, "% 32"),                               # c0 = 100
    (dict(), dict(d_a1=FAKE, lda1=32), "d_a1 without c1"),
    (dict(lda=100), {}, "lda"),
    (dict(lda=130), {}, "lda"),
    (dict(c1=32, lda=96), {}, "lda"),                        # both segments from d_a need lda >= C
    (dict(c1=32, lda=96), dict(d_a1=FAKE, lda1=28), "lda1"),
    (dict(c1=32, lda=96), dict(d_a1=FAKE, lda1=34), "lda1"),
    (dict(), dict(ldc=100), "ldc"),
    (dict(d_res=FAKE, ldr=100), {}, "ldr"),
    (dict(d_out16_f32=FAKE, N=100), {}, "N % 32"),
    (dict(d_out16_f32=FAKE), dict(ldc=130), "N % 32"),
    (dict(d_out16_f32=FAKE, d_res=FAKE, ldr=130), {}, "N % 32"),
    (dict(d_a_mean=FAKE), {}, "come together"),
    (dict(d_a_rstd=FAKE), {}, "come together"),
    (dict(d_a_part=FAKE, a_nparts=0), {}, "a_part"),
    (dict(d_a_part=FAKE, a_nparts=2, d_a_mean=FAKE, d_a_rstd=FAKE), {}, "a_part"),
    (dict(d_a_part=FAKE, a_nparts=2, ntaps=3, h_tap_off=C.cast(TAPS, C.c_void_p)), {}, "plain Linear"),
    (dict(d_a_mean=FAKE, d_a_rstd=FAKE, in_stride=2), {}, "plain Linear"),
    (dict(d_a_mean=FAKE, d_a_rstd=FAKE, h_tap_off=C.cast(TAPS, C.c_void_p)), {}, "plain Linear"),
    (dict(d_stats_out=FAKE, N=96), {}, "stats_out"),
    (dict(d_stats_out=FAKE), dict(ldc=130), "stats_out"),
    (dict(act=3), {}, "SnakeBeta"),
    (dict(act=7), {}, "act"),
    (dict(force_bm=32), {}, "force_bm"),
    (dict(out_T=64, out_stride=2, out_off=0), {}, "output rows"),
    (dict(out_T=128, out_stride=2, out_off=2), {}, "output rows"),
    (dict(out_T=128, out_stride=0), {}, "output rows"),
    (dict(ntaps=3), {}, "tap offsets"),
])
def test_gemm_refusals_before_any_launch(hip, lib, kw, call, needle):
    g = gemm_block(hip, **kw)
    c = dict(terms=0, d_a1=None, lda1=0, ldc=0, out_lscale=2048.0)
    c.update(call)
    assert lib.mtts_gemm_f32_args_run(C.byref(g), c["terms"], c["d_a1"], c["lda1"], c["ldc"], c["out_lscale"], FAKE, None) == -1
    assert needle.encode() in lib.mtts_last_error(), lib.mtts_last_error()
    assert g.wave_rows == 0 and g.tag == b""


def test_gemm_null_scratch_block_and_sizes(hip, lib):
    assert lib.mtts_gemm_f32_args_run(C.byref(gemm_block(hip)), 0, None, 0, 0, 2048.0, None, None) == -1
    assert b"null buffer" in lib.mtts_last_error()
    assert lib.mtts_gemm_f32_args_run(None, 0, None, 0, 0, 2048.0, FAKE, None) == -1 and b"null argument block" in lib.mtts_last_error()
    assert lib.mtts_gemm_f32_args_scratch_bytes(None) == -1
    plain = lib.mtts_gemm_f32_args_scratch_bytes(C.byref(gemm_block(hip)))
    assert plain >= 128 * 128 * 4 + 128 * 128 * 6                                  # fp32 panel, three bf16 planes
    with16 = lib.mtts_gemm_f32_args_scratch_bytes(C.byref(gemm_block(hip, d_out16_f32=FAKE)))
    assert with16 - plain >= (64 + 64) * 2 * 128 * 2                               # the raw image and its guard rows
    # the existing entries are as they were: the P16 entry takes the same block, the H16 entry still wants half16
    assert lib.mtts_gemm_h16(C.byref(gemm_block(hip)), FAKE, None) == -1 and b"half16" in lib.mtts_last_error()


def test_other_entries_refuse_on_the_host(lib):
    at = lambda **k: lib.mtts_attention_f32_run(k.get("q", FAKE), k.get("mask"), None, k.get("B", 1), 64, 2, k.get("D", 48), 0.125, k.get("mode", 0),
                                                k.get("out", FAKE), None)
    assert at(q=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert at(out=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert at(B=0) == -1 and b"empty batch" in lib.mtts_last_error()
    for D in (0, 68, 50):
        assert at(D=D) == -1 and b"head dim" in lib.mtts_last_error()
    assert at(mode=1) == -1 and b"needs a mask" in lib.mtts_last_error()
    assert at(mode=2) == -1 and b"mask_mode" in lib.mtts_last_error()
    gn = lambda **k: lib.mtts_groupnorm_mish_f32_run(k.get("y", FAKE), FAKE, FAKE, k.get("mask", FAKE), k.get("chb"), k.get("cs", 0), k.get("res"),
                                                     k.get("ldr", 0), 2, k.get("T", 64), k.get("C", 384), k.get("G", 8), 1e-5, None, k.get("nextra"),
                                                     k.get("bs"), k.get("out", FAKE), k.get("st"), k.get("scratch", FAKE), None)
    assert gn(y=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(out=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(mask=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(scratch=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(C=100) == -1 and b"C % G" in lib.mtts_last_error()
    assert gn(C=40, G=20) == -1 and b"C % G" in lib.mtts_last_error()             # 2 channels per group
    assert gn(T=0) == -1
    assert gn(chb=FAKE, cs=380) == -1 and b"bias row" in lib.mtts_last_error()
    assert gn(chb=FAKE, cs=386) == -1 and b"bias row" in lib.mtts_last_error()
    assert gn(nextra=FAKE) == -1 and b"nextra" in lib.mtts_last_error()
    assert gn(bs=FAKE) == -1 and b"nextra" in lib.mtts_last_error()
    assert gn(res=FAKE, ldr=380) == -1 and b"ldr" in lib.mtts_last_error()
    assert gn(res=FAKE, ldr=386) == -1 and b"ldr" in lib.mtts_last_error()
    assert gn(st=FAKE, C=96) == -1 and b"stats_out" in lib.mtts_last_error()
    ln = lambda **k: lib.mtts_channel_layernorm_ld(k.get("x", FAKE), k.get("ldx", 96), 2, k.get("T", 8), k.get("C", 96), FAKE, FAKE, 1e-5, k.get("act", 0),
                                                   None, None, k.get("y", FAKE), k.get("ldy", 96), None)
    assert ln(x=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert ln(y=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert ln(T=0) == -1 and b"empty batch" in lib.mtts_last_error()
    assert ln(C=98) == -1 and b"multiple of 4" in lib.mtts_last_error()
    assert ln(C=2052, ldx=2052, ldy=2052) == -1 and b"at most 2048" in lib.mtts_last_error()
    assert ln(ldx=92) == -1 and b"leading dimension" in lib.mtts_last_error()
    assert ln(ldy=98) == -1 and b"leading dimension" in lib.mtts_last_error()
    assert ln(act=1) == -1 and b"act" in lib.mtts_last_error()


# ------------------------------------------------------------------------------------------------ the restatement against independent torch
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("C,k,T,stride", [(28, 3, 5, 1), (36, 5, 3, 1), (32, 3, 1, 1), (36, 3, 7, 2), (4, 1, 5, 1), (200, 5, 2, 1)])
def test_gemm_restated_is_conv1d(C, k, T, stride):
    B, N = 3, 20
    a, w, bias = rnd(B * T, C, seed=1), rnd(N, C, k, seed=2), rnd(N, seed=3)
    am = (torch.arange(B * T) % 3 != 1).float()
    T_out = (T + 2 * (k // 2) - k) // stride + 1
    got = R.gemm(a, w if k > 1 else w[:, :, 0], bias, B=B, T_in=T, T_out=T_out, in_stride=stride, a_mask=am)
    x = (a * am[:, None]).double().view(B, T, C).transpose(1, 2)
    want = F.conv1d(x, w.double(), bias.double(), stride=stride, padding=k // 2).transpose(1, 2).reshape(-1, N)
    assert close(got, want)
    twin = R.gemm(a, w if k > 1 else w[:, :, 0], bias, B=B, T_in=T, T_out=T_out, in_stride=stride, a_mask=am, dtype=torch.float32)
    assert twin.dtype == torch.float32 and close(twin.double(), want, 1e-5) and not torch.equal(twin.double(), want)


def test_two_phase_interleave_is_conv_transpose1d():
    B, T, C, N = 3, 5, 32, 24
    x, wt, bias = rnd(B * T, C, seed=4), rnd(C, N, 4, seed=5), rnd(N, seed=6)
    out = torch.zeros(B * 2 * T, N, dtype=torch.float64)
    for sel, taps, off in (([1, 3], [0, -1], 0), ([0, 2], [1, 0], 1)):
        w = wt[:, :, sel].permute(1, 0, 2).contiguous()
        rows = R.place_rows(B * 2 * T, B, T, 2 * T, 2, off)
        out[rows] = R.gemm(x, w, bias, B=B, T_in=T, tap_off=taps)
    want = F.conv_transpose1d(x.double().view(B, T, C).transpose(1, 2), wt.double(), bias.double(), stride=2, padding=1).transpose(1, 2).reshape(-1, N)
    assert close(out, want)
    assert sorted(R.place_rows(0, 2, 3, 6, 2, 1).tolist()) == [1, 3, 5, 7, 9, 11]


def test_layernorm_prologue_epilogue_and_moments():
    M, C, N = 9, 128, 12
    a, w, bias = rnd(M, C, seed=7) * 2 + 0.4, rnd(N, C, seed=8), rnd(N, seed=9)
    res, om = rnd(M, N, seed=10), (torch.arange(M) % 2).float()
    mean, rstd = R.row_stats(a)
    want = F.linear(F.layer_norm(a.double(), (C,), eps=1e-5), w.double(), bias.double())
    assert close(R.gemm(a, w, bias, B=1, T_in=M, a_mean=mean, a_rstd=rstd), want)
    part = R.row_moments(a)
    assert close(R.gemm(a, w, bias, B=1, T_in=M, a_part=part), want, 1e-11)        # the equal-count merge of 64-column moments is LayerNorm
    twin = R.gemm(a, w, bias, B=1, T_in=M, a_part=part.float(), dtype=torch.float32)
    assert twin.dtype == torch.float32 and close(twin.double(), want, 1e-5)
    for act, fn in ((1, torch.relu), (2, F.silu)):
        got = R.gemm(a, w, bias, B=1, T_in=M, act=act, out_mask=om, out_scale=-1.7, res=res)
        assert close(got, fn(F.linear(a.double(), w.double(), bias.double())) * om[:, None].double() * -1.7 + res.double())
    p0, p1 = torch.exp(rnd(N, seed=11)), torch.exp(rnd(N, seed=12))
    z = F.linear(a.double(), w.double(), bias.double())
    assert close(R.gemm(a, w, bias, B=1, T_in=M, act=3, p0=p0, p1=p1), z + p1.double() * torch.sin(z * p0.double()) ** 2)
    o, bud = R.gemm(a, w, bias, B=1, T_in=M, act=3, p0=p0, p1=p1, want_budget=True)
    assert (bud > 0).all() and (bud >= (a.double().abs() @ w.double().abs().T)).all()
    # the budget is the unit, not the bound: an fp32 chain of K terms may lose up to K u Bud (and loses ~sqrt(K) u Bud), which is why the
    # rule measures the device against the twin's own error
    twin = R.gemm(a, w, bias, B=1, T_in=M, dtype=torch.float32)
    ref, bud = R.gemm(a, w, bias, B=1, T_in=M, want_budget=True)
    e = (twin.double() - ref).abs() / (R.U * bud)
    assert (e <= C).all() and e.max().item() > 0.05
    st = R.row_moments(a)
    assert close(st[:, :, 0], a.double().view(M, 2, 64).mean(2)) and close(st[:, :, 1], a.double().view(M, 2, 64).var(2, unbiased=False) * 64)


def test_attention_restated_is_sdpa_reference():
    import matcha_oracle as O
    B, T, H, D = 2, 19, 2, 12
    qkv = rnd(B * T, 3 * H * D, seed=13)
    mask = (torch.arange(T)[None] < torch.tensor([19, 11])[:, None]).float().reshape(-1)
    q, k, v = [z.view(B, T, H, D).transpose(1, 2).double() for z in qkv.split(H * D, dim=1)]
    m2 = mask.view(B, T)
    for mode, am in ((0, m2.double().view(B, 1, 1, T).expand(B, H, 1, T)), (1, (m2[:, None, :, None] * m2[:, None, None, :]).bool())):
        want = O.sdpa_reference(q, k, v, am, 0.3).transpose(1, 2).reshape(B * T, H * D)
        got, A, aux = R.attention(qkv, mask, B, T, H, D, 0.3, mode)
        assert close(got, want) and (A >= got.abs() - 1e-12).all() and ((aux["L"] >= 1 - 1e-12) | (aux["L"] <= 1e-38)).all()
    # klen: the keys beyond it are gone (the same as cutting the utterance), klen 0 gives exactly 0
    got, _, _ = R.attention(qkv, mask, B, T, H, D, 0.3, 0, klen=torch.tensor([7, 0]))
    cut = O.sdpa_reference(q[:1, :, :, :], k[:1, :, :7], v[:1, :, :7], m2[:1, :7].double().view(1, 1, 1, 7), 0.3).transpose(1, 2).reshape(T, H * D)
    assert close(got[:T], cut) and (got[T:] == 0).all()


def test_groupnorm_restated_is_group_norm_mish_on_explicit_rows():
    B, T, C = 3, 9, 96
    y, g, be = rnd(B * T, C, seed=14) * 1.5 + 0.2, 1 + 0.1 * rnd(C, seed=15), 0.1 * rnd(C, seed=16)
    mask = (torch.arange(T)[None] < torch.tensor([9, 6, 2])[:, None]).float().reshape(-1)
    want = (F.mish(F.group_norm(y.double().view(B, T, C).transpose(1, 2), 8, g.double(), be.double(), eps=1e-5)) * mask.view(B, 1, T).double())
    want = want.transpose(1, 2).reshape(-1, C)
    assert close(R.groupnorm_mish(y, g, be, mask, B, T), want)
    assert close(R.groupnorm_mish(y, g, be, mask, B, T, dtype=torch.float32).double(), want, 1e-5)
    # nextra: n extra copies of the bias row in the statistics == the utterance padded with those rows explicitly
    bias_row, lens = rnd(C, seed=17) * 0.5, [9, 6, 2]
    yp = y.clone().view(B, T, C)
    for b, n in enumerate(lens):
        yp[b, n:] = bias_row
    yp = yp.reshape(B * T, C)
    folded = R.groupnorm_mish(yp, g, be, mask, B, T, nrows=torch.tensor(lens), nextra=torch.tensor([T - n for n in lens]), bias_row=bias_row)
    explicit = (F.mish(F.group_norm(yp.double().view(B, T, C).transpose(1, 2), 8, g.double(), be.double(), eps=1e-5)) * mask.view(B, 1, T).double())
    assert close(folded, explicit.transpose(1, 2).reshape(-1, C))
    # ... and the closed form the kernel is given: per group the mean of the bias row and the squared deviations of ONE copy
    bs = R.gn_bias_stats(bias_row)
    assert close(bs[:, 0].double(), bias_row.double().view(8, 12).mean(1), 1e-6) and close(bs[:, 1].double(), bias_row.double().view(8, 12).var(1, unbiased=False) * 12, 1e-6)
    cb, res = rnd(B, C + 8, seed=18), rnd(B * T, C, seed=19)
    got = R.groupnorm_mish(y, g, be, mask, B, T, chbias=cb, res=res)
    assert close(got, (want + cb[:, :C].double().repeat_interleave(T, 0)) * mask[:, None].double() + res.double())


def test_channel_layernorm_restated_is_layer_norm():
    B, T, C = 3, 5, 252
    x, g, be, fl = rnd(B * T, C, seed=20) * 3 + 0.7, 1 + 0.1 * rnd(C, seed=21), 0.1 * rnd(C, seed=22), rnd(B, 2 * C, seed=23)
    mask = (torch.arange(B * T) % 4 != 0).float()
    base = F.layer_norm(x.double(), (C,), g.double(), be.double(), 1e-5)
    assert close(R.channel_layernorm(x, B, T, g, be), base)
    want = (F.silu(base) * fl[:, :C].double().repeat_interleave(T, 0) + fl[:, C:].double().repeat_interleave(T, 0)) * mask[:, None].double()
    assert close(R.channel_layernorm(x, B, T, g, be, act=2, film=fl, mask=mask), want)
    mu, rs = R.row_stats(x)
    assert close(mu, x.double().mean(1)) and close(rs, 1 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5))


# ------------------------------------------------------------------------------------------------ the input classes are present
def test_the_gpu_files_input_classes_are_present():
    import test_hip_kernels_f32 as G
    a = G.hard_rows(70, 128, seed=60)
    mu, rs = R.row_stats(a)
    std = (a.double() - mu[:, None]).pow(2).mean(1).sqrt()
    assert 25 < (mu[1].abs() / std[1]).item() < 40                                  # |mean| = 32 std
    assert std[2].item() ** 2 < 2e-5 and std[2].item() > 0                          # variance near eps
    assert std[3].item() == 0 and a[3, 0].item() == 1.25 and (a[4] == 0).all()      # constant, all zero
    assert std[6].item() > 50 * std[5].item() and std[6].item() > 50 * std[7].item()   # one x100 row between unit rows
    x = G.odd_x100(torch.ones(4 * 3, 2), 4, 3).view(4, 3, 2)
    assert (x[0] == 1).all() and (x[1] == 100).all() and (x[3] == 100).all()
    # quiet rows: at 2^-16 most heads are fp16 subnormals, at 2^-8 some are; the restated split still holds the value to 2^-22
    for shift, least in ((8, 0.002), (16, 0.9)):
        q = p16(p16(rnd(66, 64, seed=90)) * 2.0 ** -shift)
        h, _ = split(q)
        sub_heads = (h.float().abs() < 2.0 ** -14) & (h.float() != 0)
        assert sub_heads.float().mean().item() > least
        assert ((p16(q).double() - q.double()).abs() <= 2.0 ** -22 * q.double().abs()).all()
    # the a_nparts values of the LayerNorm cases reach both merge branches
    parts = sorted({C // 64 for ln, C in [("parts", 64), ("parts", 128), ("parts", 384), ("parts", 512), ("parts", 576), ("parts", 1024)]})
    assert parts == [1, 2, 6, 8, 9, 16]
    # the 128-query attention grid is the launcher's smallest: B H ceil(T / 128) >= 768 with waste < 0.1
    B, H, T = 32, 12, 250
    assert B * H * math.ceil(T / 128) == 768 and 1 - T / (math.ceil(T / 128) * 128) < 0.1
    # ragged masks really are ragged, and mode 1 leaves out exactly the mask-0 rows
    m = G.ragged(3, 33, 11).view(3, 33)
    assert m.sum(1).tolist() == [33, 22, 11]
    # attention operand scales: residuals of q, k at 2^-6 are all fp16 subnormals or zero at lscale 1
    qk = rnd(256, 128, seed=120, scale=0.5) * 2.0 ** -6 / 0.5
    _, l = split(qk, 1.0)
    assert (l.float().abs() < 2.0 ** -14).all() and (l.float() != 0).any()

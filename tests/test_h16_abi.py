"""CPU checks of the unit entries of the 16-bit storage modes' kernels (csrc/unit_entries.hip: mtts_gemm_h16, mtts_attention_h16,
mtts_groupnorm_mish_h16, mtts_to_h16_roundtrip and the host-only helpers; nothing runs on a GPU): the binding itself (declared, exported,
arity, types, the argument block field for field) is checked for every entry in test_abi.py; here: every
refusal that can be decided on the host returns -1 with a message before anything is launched (the buffers named here are never
touched); and the 16-bit weight plane equals torch's rounding bit for bit, ties, subnormals and the fp16 clamp included."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import sub

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


def test_new_entries_are_declared_exported_and_bound_with_matching_arity(hip, lib):
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_abi_version() == 2
    for wrapper in ("gemm_h16", "attention_h16", "groupnorm_mish_h16", "to_h16_roundtrip", "panel_h16_host", "last_kernel_tag"):
        assert callable(getattr(hip, wrapper))
    assert lib.mtts_last_kernel_tag() == b""           # no launcher ran on this thread


def gemm_block(hip, **kw):
    g = hip.MttsGemmH16Args()
    base = dict(d_a=FAKE, lda=128, C=128, B=1, T_in=64, T_out=64, ntaps=1, in_stride=1, h_w=FAKE, N=128, out_scale=1.0, d_out=FAKE,
                half16=1, wave_rows=77)
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("kw,needle", [
    (dict(C=96, lda=96), "C % 64"),
    (dict(C=128, c1=32), "C % 64"),
    (dict(half16=0, bf16=1), "half16"),
    (dict(half16=0), "half16"),
    (dict(res16_mode=1, d_res16_f32=FAKE, d_res=FAKE, ldr=128), "res16 together with res"),
    (dict(d_gn_stats=FAKE, gn_groups=4, act=3, d_p0=FAKE, d_p1=FAKE), "gn_stats with an activation"),
    (dict(d_a=None), "null buffer"),
    (dict(h_w=None), "null buffer"),
    (dict(d_out=None), "null buffer"),
    (dict(res16_mode=2), "in place"),
    (dict(d_out16_f32=FAKE, N=100), "N % 64"),
    (dict(ntaps=9), "ntaps"),
])
def test_gemm_refusals_before_any_launch(hip, lib, kw, needle):
    g = gemm_block(hip, **kw)
    assert lib.mtts_gemm_h16(C.byref(g), FAKE, None) == -1
    assert needle.encode() in lib.mtts_last_error(), lib.mtts_last_error()
    assert g.wave_rows == 0 and g.tag == b""                 # the block's last fields sit where the library writes them
    assert lib.mtts_last_kernel_tag() == b""


def test_gemm_null_scratch_and_block(hip, lib):
    assert lib.mtts_gemm_h16(C.byref(gemm_block(hip)), None, None) == -1
    assert b"null buffer" in lib.mtts_last_error()
    assert lib.mtts_gemm_h16(None, FAKE, None) == -1
    assert lib.mtts_gemm_h16_scratch_bytes(None) == -1
    g = gemm_block(hip, d_out16_f32=FAKE)
    need = lib.mtts_gemm_h16_scratch_bytes(C.byref(g))
    assert need >= 64 * 128 * 2 + 2 * 64 * 128 * 2 + 128 * 128 * 2 + 128 * 4


def test_wave_rows_follow_the_tile_choice(lib):
    assert lib.mtts_gemm_h16_wave_rows(3, 100, 384, 0) == 32            # 15 tiles: the 64-row ring
    assert lib.mtts_gemm_h16_wave_rows(8, 1000, 1152, 128) == 64
    assert lib.mtts_gemm_h16_wave_rows(4, 160, 384, 64) == 32
    assert lib.mtts_gemm_h16_wave_rows(0, 160, 384, 0) == -1
    assert lib.mtts_gemm_h16_wave_rows(1, 160, 384, 96) == -1


def test_other_entries_refuse_on_the_host(lib):
    # conversions: C % 64, null buffers, C_valid beyond C
    assert lib.mtts_to_h16_roundtrip(FAKE, 96, None, 4, 96, 96, 96, 0, FAKE, FAKE, None, None) == -1
    assert b"C % 64" in lib.mtts_last_error()
    assert lib.mtts_to_h16_roundtrip(None, 64, None, 4, 64, 64, 64, 0, FAKE, FAKE, None, None) == -1
    assert b"null buffer" in lib.mtts_last_error()
    assert lib.mtts_to_h16_roundtrip(FAKE, 64, None, 4, 64, 68, 64, 1, FAKE, FAKE, None, None) == -1
    assert lib.mtts_to_h16_roundtrip(FAKE, 64, None, 4, 64, 64, 60, 1, FAKE, FAKE, None, None) == -1      # ld16 < C
    # attention: head dim 64 only, null buffers
    assert lib.mtts_attention_h16(FAKE, None, None, 1, 64, 2, 48, 0.125, 0, 0, FAKE, None, FAKE, None) == -1
    assert b"D == 64" in lib.mtts_last_error()
    assert lib.mtts_attention_h16(FAKE, None, None, 1, 64, 2, 64, 0.125, 0, 1, FAKE, None, None, None) == -1
    assert b"null buffer" in lib.mtts_last_error()
    assert lib.mtts_attention_h16(FAKE, None, None, 1, 64, 2, 64, 0.125, 1, 1, FAKE, None, FAKE, None) == -1      # boolean mode without a mask
    # GroupNorm: C % 64, null buffers, folded padding needs both of its arrays, tile statistics need their tile height
    gn = lambda **k: lib.mtts_groupnorm_mish_h16(k.get("y", FAKE), FAKE, FAKE, FAKE, None, 0, 2, 64, k.get("C", 384), 8, 1e-5,
                                                 k.get("ts"), k.get("tr", 0), None, k.get("nextra"), None, None, 0, None,
                                                 k.get("o16", FAKE), None, FAKE, None)
    assert gn(C=96) == -1 and b"C % 64" in lib.mtts_last_error()
    assert gn(y=None) == -1 and b"null buffer" in lib.mtts_last_error()
    assert gn(o16=None) == -1
    assert gn(nextra=FAKE) == -1 and b"nextra" in lib.mtts_last_error()
    assert gn(ts=FAKE, tr=0) == -1 and b"tile_rows" in lib.mtts_last_error()
    assert lib.mtts_groupnorm_h16_scratch_bytes(2, 64, 384, 8) >= 2 * 64 * 384 * 2
    assert lib.mtts_panel_h16_host(None, 4, 0, FAKE) == -1


def hard_panel():
    """Values where a 16-bit rounding can go wrong: exact ties of both types (to even, up and down), values just beside a tie, the
    largest finite fp16 and beyond, fp16 subnormals and values that round to them or to zero, signed zeros."""
    rng = np.random.default_rng(11)
    v = [0.0, -0.0, 1.0, -1.0,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),            # fp16 ties: down to even, up to even
         1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20,
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),                # bfloat16 ties
         1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20,
         65504.0, -65504.0, 65519.9, 65520.0, -65520.0, 70000.0, -70000.0, 1.0e6, -1.0e9, 3.0e38, -3.0e38,
         2.0 ** -14, 2.0 ** -15, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 6.1e-5, 5.97e-8, 1.0e-40]
    return np.concatenate([np.array(v, dtype=np.float32), (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 12, 4096))).astype(np.float32)])


def test_fp16_plane_equals_torch_on_the_clamped_panel_bit_for_bit(hip):
    x = hard_panel()
    got = hip.panel_h16_host(x, bf16=False)
    t = torch.from_numpy(x)
    want = t.clamp(-65504.0, 65504.0).to(torch.float16)
    assert np.array_equal(got, want.view(torch.int16).numpy().view(np.uint16))
    # beyond the range: the clamp, where torch alone gives +-inf
    big = np.abs(x) > 65504.0
    assert big.sum() >= 9 and torch.isinf(t.to(torch.float16)[torch.from_numpy(big)]).any()
    assert set(got[big]) == {0x7BFF, 0xFBFF}
    # inside the range torch's own conversion is the same thing
    assert np.array_equal(got[~big], t.to(torch.float16).view(torch.int16).numpy().view(np.uint16)[~big])
    assert got[0] == 0x0000 and got[1] == 0x8000
    assert list(got[4:8]) == [0x3C00, 0x3C02, 0xBC00, 0xBC02]            # ties go to even
    assert got[29] == 0x0001 and got[31] == 0x0000 and got[33] == 0x0002   # 2^-24; 2^-25 ties to zero; 3 * 2^-25 ties to even (2)


def test_bf16_plane_equals_torch_bit_for_bit(hip):
    x = hard_panel()
    got = hip.panel_h16_host(x, bf16=True)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert list(got[10:14]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82]          # ties go to even
    assert got[21] == 0x4789 and got[25] == 0x7F62                        # 70000 and 3e38 keep the fp32 range

"""CPU checks of the one-plane transformer-block chain's boundary (csrc/tblock_chain_h16.hip; nothing runs on a GPU): the
binding itself is checked for every entry in test_abi.py; here: fragment counts for a table of shapes; the
packed stream of a small random block equals a Python restatement of the layout, for fp16 (a weight beyond +-65504 saturates and
sets the flag) and for bfloat16 (round to nearest even, ties included)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ROOT, sub


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def test_new_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_abi_version() == 2
    assert callable(sub("_hip").tblock_chain_h16)


def frags(Cc, inner, ch, n_qkv):
    """Restatement: per wave, C/128 fragments per k-step of a C-wide product, ch/128 per k-step of FF1, ring padding 4 * C/128."""
    NT, NT1 = Cc // 128, ch // 128
    passes = -(-(n_qkv // 16) // (8 * NT)) if n_qkv else 0
    return (inner // 32) * NT + (4 * Cc // ch) * ((Cc // 32) * NT1 + (ch // 32) * NT) + passes * (Cc // 32) * NT + 4 * NT


@pytest.mark.parametrize("Cc,inner,ch,n_qkv,expect", [
    (384, 384, 256, 1152, 36 + 6 * 48 + 3 * 36 + 12),
    (384, 384, 256, 0, 36 + 6 * 48 + 12),
    (384, 384, 128, 1152, 36 + 12 * 24 + 3 * 36 + 12),
    (384, 0, 256, 0, 6 * 48 + 12),
    (256, 128, 128, 384, 8 + 8 * 16 + 2 * 16 + 8),
    (256, 256, 128, 768, 16 + 8 * 16 + 3 * 16 + 8),
    (128, 128, 128, 384, 4 + 4 * 8 + 3 * 4 + 4),
    (128, 128, 128, 0, 4 + 4 * 8 + 4),
])
def test_fragment_counts(lib, Cc, inner, ch, n_qkv, expect):
    assert frags(Cc, inner, ch, n_qkv) == expect
    assert lib.mtts_chain_stream_frags_h16(Cc, inner, ch, n_qkv) == expect
    # one plane: half of the two-plane stream's tiles (that stream pads with its own ring depth)
    assert lib.mtts_tblock_chain_h16_scratch_bytes(100, Cc, inner, n_qkv, ch) > expect * 8 * 1024


def test_unsupported_shapes_are_refused(lib):
    assert lib.mtts_chain_stream_frags_h16(192, 128, 128, 0) == -1
    assert lib.mtts_chain_stream_frags_h16(256, 192, 128, 576) == -1      # attention width not a whole ring period of line steps
    assert lib.mtts_chain_stream_frags_h16(256, 128, 256, 0) == -1        # 256-wide chunks at width 384 only
    assert lib.mtts_chain_stream_frags_h16(128, 128, 128, 40) == -1
    assert b"mtts_chain_stream_frags_h16" in lib.mtts_last_error()
    assert lib.mtts_tblock_chain_h16_scratch_bytes(0, 128, 128, 0, 128) == -1


def to16(w, bf16):
    """fp32 -> the 16 bits the stream holds (numpy / torch do the rounding: nearest even; fp16 saturating)."""
    t = torch.from_numpy(np.ascontiguousarray(w))
    if bf16:
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return t.clamp(-65504.0, 65504.0).to(torch.float16).view(torch.int16).numpy().view(np.uint16)


def restate(Cc, inner, ch, n_qkv, w_out, w1, w2, w_qkv, bf16):
    NT, NT1, KG, KG2, NCH = Cc // 128, ch // 128, Cc // 32, ch // 32, 4 * Cc // ch
    per_wave = frags(Cc, inner, ch, n_qkv)
    out = np.zeros((8, per_wave, 64, 8), dtype=np.uint16)
    lane = np.arange(64)
    r, q = lane & 15, lane >> 4

    def frag(w, n0, n_valid, k0):
        f = np.zeros((64, 8), dtype=np.float32)
        rows = n0 + r
        ok = rows < n_valid
        cols = k0 + 8 * q[:, None] + np.arange(8)[None, :]
        f[ok] = w[rows[ok][:, None], cols[ok]]
        return to16(f, bf16)

    passes = -(-(n_qkv // 16) // (8 * NT)) if n_qkv else 0
    for wv in range(8):
        o = 0
        for s in range(inner // 32):
            for t in range(NT):
                out[wv, o] = frag(w_out, 16 * (wv * NT + t), Cc, 32 * s); o += 1
        for j in range(NCH):
            for s in range(KG):
                for t in range(NT1):
                    out[wv, o] = frag(w1, j * ch + 16 * (wv * NT1 + t), 4 * Cc, 32 * s); o += 1
            for s in range(KG2):
                for t in range(NT):
                    out[wv, o] = frag(w2, 16 * (wv * NT + t), Cc, j * ch + 32 * s); o += 1
        for ps in range(passes):
            for s in range(KG):
                for t in range(NT):
                    out[wv, o] = frag(w_qkv, 16 * (ps * 8 * NT + wv * NT + t), n_qkv, 32 * s); o += 1
        assert o + 4 * NT == per_wave
    return out


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("Cc,inner,ch,n_qkv", [(128, 128, 128, 352), (256, 128, 128, 0)])
def test_packed_stream_equals_the_layout_restated(lib, bf16, Cc, inner, ch, n_qkv):
    rng = np.random.default_rng(5)
    w_out = rng.standard_normal((Cc, inner)).astype(np.float32)
    w1 = rng.standard_normal((4 * Cc, Cc)).astype(np.float32)
    w2 = rng.standard_normal((Cc, 4 * Cc)).astype(np.float32)
    w_qkv = rng.standard_normal((n_qkv, Cc)).astype(np.float32) if n_qkv else None
    # exact ties of the bfloat16 rounding (8 significand bits): 1 + 2^-8 -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6 (even)
    w1[0, 0], w1[0, 1], w1[0, 2] = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)
    n = lib.mtts_chain_stream_frags_h16(Cc, inner, ch, n_qkv)
    dst = np.full(n * 8 * 512, 0xFFFF, dtype=np.uint16)
    sat = C.c_int(0)
    p = lambda a: None if a is None else a.ctypes.data
    assert lib.mtts_chain_stream_pack_h16(Cc, inner, ch, n_qkv, p(w_out), p(w1), p(w2), p(w_qkv), int(bf16), dst.ctypes.data, C.byref(sat)) == 0
    assert sat.value == 0
    want = restate(Cc, inner, ch, n_qkv, w_out, w1, w2, w_qkv, bf16)
    assert np.array_equal(dst.reshape(want.shape), want)
    if bf16:
        first = dst.reshape(want.shape)[0, inner // 32 * (Cc // 128), 0, :3]       # wave 0's first FF1 fragment, lane 0
        assert list(first) == [0x3F80, 0x3F82, 0xBF80]
    # a weight beyond the fp16 range: saturates to +-65504 and is reported -- for fp16 planes only
    w2[3, 7] = -1.0e6
    sat = C.c_int(0)
    assert lib.mtts_chain_stream_pack_h16(Cc, inner, ch, n_qkv, p(w_out), p(w1), p(w2), p(w_qkv), int(bf16), dst.ctypes.data, C.byref(sat)) == 0
    assert sat.value == (0 if bf16 else 1)
    assert np.array_equal(dst.reshape(want.shape), restate(Cc, inner, ch, n_qkv, w_out, w1, w2, w_qkv, bf16))
    if not bf16:
        assert 0xFBFF in dst                                               # -65504

"""CPU checks of tests/fused_restated.py, the yardstick of tests/test_hip_kernels_fused.py (nothing here runs on a GPU):
  * the restatement agrees with the independent plain fp64 code of the old tests (test_hip_chain.chain_ref,
    test_resnet_conv.block1d_fp64, on UNSPLIT operands) to within the representation and re-split terms of its own budget;
  * the fp32 twin's error e_cpu32 = max |twin - fp64| / (u B) is finite on every case (printed: run with -s for the table);
  * every input condition the GPU file relies on holds for exactly the operands it launches: the row classes of the hard tile,
    the spread of the weight rows, the all-zero rows, 8 <= max |p0 z| < 64, nothing beyond 65504 outside the range test and
    something beyond it inside, the constant and the offset GroupNorm group, the ragged frame counts;
  * the argument-block entries refuse on the host what they must."""
import ctypes as C
import math

import pytest
import torch

import fused_restated as R
from conftest import ROOT, sub
from p16_restated import p16
from test_hip_chain import chain_ref
from test_resnet_conv import block1d_fp64

CHAIN_KEYS = sorted({c[0] for c in R.chain_case_list()}, key=str)
CONV_KEYS = R.conv_case_list()
FAKE = 0x1000


def finite(r):
    return all(torch.isfinite(v).all().item() for v in r.values() if isinstance(v, torch.Tensor))


@pytest.mark.parametrize("key", CHAIN_KEYS, ids=lambda k: "-".join(str(v) for v in k if v != ""))
def test_chain_restatement_against_plain_fp64_and_its_twin(key):
    case = R.chain_case(*key)
    ops, r64, r32, B = case["ops"], case["r64"], case["r32"], case["B"]
    x1, x2, qkv = chain_ref(*ops)
    rep = R.chain_budget(r64, *ops, rounding=False, operands=True)
    d_x2 = R.measure(r64["x2"], x2, rep["x2"])
    d_q = R.measure(r64["qkv"], qkv, rep["qkv"]) if qkv is not None else 0.0
    assert finite(r64) and finite(r32)
    e_x = R.measure(r32["x_out"], r64["x_out"], B["x_out"])
    e_q = R.measure(r32["qkv"], r64["qkv"], B["qkv"]) if qkv is not None else 0.0
    print(f"chain {key}: restated - plain fp64 = {d_x2:.3f} / {d_q:.3f} of the representation budget; e_cpu32 x_out {e_x:.4f} qkv {e_q:.4f}; "
          f"cos allowance x_out {R.cos_term(B['cos_x_out'], B['x_out']):.3f}" + (f" qkv {R.cos_term(B['cos_qkv'], B['qkv']):.3f}" if qkv is not None else ""))
    assert d_x2 <= 1.0 and d_q <= 1.0
    assert math.isfinite(e_x) and math.isfinite(e_q) and e_x > 0.0
    # inputs: nothing leaves the fp16 range, and the SnakeBeta argument reaches 8 but stays below 64
    for name in ("x1", "z", "h", "x2_raw", "qkv_raw"):
        if name in r64:
            assert r64[name].abs().max().item() < R.F16_MAX, name
    pz = (r64["z"] * ops[6].double()).abs().max().item()
    assert 8.0 <= pz < 64.0, pz
    # every image value is a fixed point of the split it was stored with
    assert torch.equal(p16(r64["x_out"].float()), r64["x_out"].float())
    if qkv is not None:
        assert torch.equal(p16(r64["qkv"].float(), 1.0), r64["qkv"].float())


@pytest.mark.parametrize("C", [384, 256, 128])
def test_hard_columns(C):
    inner, n_qkv = R.FULL[C]
    w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv, b_qkv = R.chain_weights(C, inner, n_qkv, 1)
    for w, K in ((w_out, inner), (w1, C), (w2, 4 * C), (w_qkv, C)):
        norm = w.double().norm(dim=1)
        assert (norm == 0).sum().item() == 1                                   # one all-zero output row per panel
        lg = torch.log2(norm[norm > 0])
        assert lg.min().item() < -5.0 and lg.max().item() > 1.0 and len(set(lg.round().tolist())) >= 8      # spread over 2^-6 .. 2^2
    for p in (p0, p1):
        assert math.exp(-1.4) <= p.min().item() < 0.35 and 3.0 < p.max().item() <= math.exp(1.4)


@pytest.mark.parametrize("C,inner", [(384, 384), (256, 256), (128, 128), (256, 0)])
def test_hard_rows_hold_every_class(C, inner):
    key = ("hard", C, inner, R.FULL[C][1] if inner else 0, "b_out" if inner else "")
    case = R.chain_case(*key)
    r64, r32 = case["r64"], case["r32"]
    ratio = (r64["mean1"].abs() * r64["rstd1"]).flatten()                      # |mean| / sqrt(var + eps) of what LayerNorm sees
    std = (1.0 / r64["rstd1"] ** 2 - R.EPS).clamp_min(0).sqrt().flatten()
    cls = R.HARD_CLASSES
    assert all(0.05 < ratio[i] < 0.5 for i in cls["m0.15"]) and all(2.0 < ratio[i] < 8.0 for i in cls["m4"])
    assert all(16.0 < ratio[i] < 64.0 for i in cls["m32"])
    assert all(0.03 * R.EPS < std[i] ** 2 < 3 * R.EPS for i in cls["x1e-3"])  # variance (1e-6) within reach of eps (1e-5)
    assert all(std[i] == 0 and r64["x1"][i].abs().max() == 3.0 for i in cls["const"])
    assert all(r64["x1"][i].abs().max() == 0 for i in cls["zero"])
    i = cls["x100"][0]
    assert std[i] > 50 * std[i - 1] and std[i] > 50 * std[i + 1] and 0.5 < std[i - 1] < 2 and 0.5 < std[i + 1] < 2
    assert sorted(sum(cls.values(), [])) == list(range(R.HARD_M))
    masked = [i for i in range(R.HARD_M) if case["mask"][i] == 0]
    assert masked == R.HARD_MASKED and all(any(i in rows for i in masked) for name, rows in cls.items() if len(rows) > 1)
    for name, rows in cls.items():                                            # the twin stays finite on each class, with a finite measure
        for out in ("x_out", "qkv"):
            if out in r64:
                e = R.measure(r32[out][rows], r64[out][rows], case["B"][out][rows])
                print(f"hard rows C={C} inner={inner} class {name}: e_cpu32 {out} {e:.4f}")
                assert math.isfinite(e)
    assert (r64["x_out"][masked] == 0).all()
    # the loud twin of the tile shares the kept rows bit for bit (fp64 restatement: rows are independent)
    loud = R.chain_case("loud", *key[1:])
    assert torch.equal(loud["ops"][1][R.HARD_KEPT], case["ops"][1][R.HARD_KEPT])
    assert torch.equal(loud["r64"]["x_out"][R.HARD_KEPT], r64["x_out"][R.HARD_KEPT])
    other = [i for i in range(R.HARD_M) if i not in R.HARD_KEPT]
    assert loud["ops"][1][other].abs().mean() > 30 * case["ops"][1][other].abs().mean()
    assert loud["r64"]["x2_raw"].abs().max() < R.F16_MAX


def test_case_list_reaches_every_instantiation_and_edge():
    cases = R.chain_case_list()
    for shape in R.CHAIN_SHAPES:
        for pair in (False, True):
            assert any((k[1], qb, ch) == shape and p == pair for k, qb, ch, M, p in cases), (shape, pair)
    for C, qb, ch in R.SWEEP_SHAPES:
        ms = {M for k, q, c, M, p in cases if (k[1], q, c) == (C, qb, ch) and k[0] == "plain" and k[2] == C}
        assert {1, 15, 17, qb - 1, qb, qb + 1, 2 * qb + 1} <= ms
    assert {C for C, _, _ in R.SWEEP_SHAPES} == {384, 256, 128}
    for k, qb, ch, M, p in cases:
        assert M <= (R.HARD_M if k[0] != "plain" else R.POOL)
        if k[0] == "plain" and M not in R.sweep_ms(qb):
            assert M % qb                                                      # the last tile is partly filled
        if p:
            assert ((M + qb - 1) // qb) % 8 and k[2] > 0                       # the pair grid holds idle workgroups
    inners = {(k[1], k[2]) for k, *_ in cases}
    assert {(384, 0), (384, 128), (384, 384), (256, 0), (256, 128), (256, 256), (128, 0), (128, 128)} <= inners
    for C, n_qkv in ((384, 1088), (256, 576), (128, 352)):                     # the last q|k|v pass is partly empty
        assert any(k[1] == C and k[3] == n_qkv for k, *_ in cases) and (n_qkv // 16) % (8 * C // 128)
    assert {"b_out", "b1", "b2", "b_qkv"} <= {k[4] for k, *_ in cases}


def test_chain_range_case_leaves_the_range_in_one_row_only():
    c = R.chain_range_case()
    ok, bad = c["r_ok"], c["r_bad"]
    assert ok["x2_raw"].abs().max() < R.F16_MAX and ok["x1"].abs().max() < R.F16_MAX
    over = bad["x2_raw"].abs() > R.F16_MAX
    assert over[R.RANGE_ROW].sum() >= 2 and not over[[i for i in range(40) if i != R.RANGE_ROW]].any()
    assert set(torch.nonzero(over[R.RANGE_ROW]).flatten().tolist()) <= set(R.RANGE_COLS)
    assert (bad["x2"][over].abs() == R.F16_MAX).all()                          # the image saturates: heads +-65504, residual 0
    rest = [i for i in range(40) if i != R.RANGE_ROW]
    assert torch.equal(bad["x_out"][rest], ok["x_out"][rest]) and torch.equal(bad["qkv"][rest], ok["qkv"][rest])
    assert c["bad"].abs().max() <= R.F16_MAX                                   # the INPUT image is in range: the flag is the kernel's own


@pytest.mark.parametrize("key", CONV_KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_conv_gn_restatement_against_plain_fp64_and_its_twin(key):
    kind, T, Cc, c1 = key
    case = R.conv_case(*key)
    ops, kw, B, r64, r32 = case["ops"], case["kw"], case["B"], case["r64"], case["r32"]
    x, w, bias, gamma, beta, mask = ops
    assert torch.isfinite(r64["out"]).all() and torch.isfinite(r32["out"]).all()
    if "nextra" not in kw and (kw.get("chbias") is None or kw["chbias"].dim() == 1):       # (what the plain code can express)
        ref = block1d_fp64(x, w, bias, gamma, beta, mask, B, T, kw.get("chbias"), kw["nrows"])
        rep = R.conv_gn_budget(r64, *ops, B, T, **kw, rounding=False, operands=True)
        d = R.measure(r64["out"], ref, rep)
        print(f"conv_gn {key}: restated - plain fp64 = {d:.3f} of the representation budget")
        assert d <= 1.0
    e = R.measure(r32["out"], r64["out"], case["budget"])
    print(f"conv_gn {key}: e_cpu32 {e:.4f}")
    assert math.isfinite(e) and e > 0.0
    assert r64["out_raw"].abs().max() < R.F16_MAX
    assert torch.equal(p16(r64["out"].float()), r64["out"].float())
    assert (r64["out"][mask == 0] == 0).all() and (mask == 0).any() and (case["budget"][mask == 0] == 0).all()
    # the constant group has variance 0, the offset group its mean at about 8 standard deviations, in every utterance with frames enough
    std = (1.0 / r64["rs"] ** 2 - R.EPS).clamp_min(0).sqrt()
    assert (std[:, R.CONST_GROUP] == 0).all() and (r64["mean"][:, R.CONST_GROUP] == 0.75).all()
    full = [b for b in range(B) if int(kw["nrows"][b]) >= 20 and not (kind == "loud" and b == 1)]
    assert full and all(4.0 < (r64["mean"][b, R.OFFSET_GROUP] / std[b, R.OFFSET_GROUP]).abs() < 16.0 for b in full)
    if kind == "ragged":
        assert kw["nrows"].tolist() == [T, 1, T - 37]                        # one full utterance, one of a single frame
    if kind == "loud":
        quiet = R.conv_case("quiet", T, Cc, c1)
        rows = torch.cat([torch.arange(0, T), torch.arange(2 * T, 3 * T)])
        assert torch.equal(quiet["ops"][0][rows], x[rows]) and torch.equal(quiet["r64"]["out"][rows], r64["out"][rows])
        assert x[T:2 * T].abs().mean() > 50 * quiet["ops"][0][T:2 * T].abs().mean()
    if kind == "extra":
        assert kw["nextra"].tolist() == [30, 0, 17] and kw["nrows"].tolist() == [72, 42, 3]


def test_conv_range_case_leaves_the_range_in_one_utterance_only():
    c = R.conv_range_case()
    T = 66
    over = c["r_bad"]["out_raw"].abs() > R.F16_MAX
    rows = torch.arange(R.RANGE_UTT * T, (R.RANGE_UTT + 1) * T)
    assert over[rows].any() and not over[:R.RANGE_UTT * T].any() and not over[(R.RANGE_UTT + 1) * T:].any()
    assert set(torch.nonzero(over.any(0)).flatten().tolist()) == set(R.RANGE_CHANNELS)
    assert c["r_ok"]["out_raw"].abs().max() < R.F16_MAX
    keep = torch.ones(3 * T, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(c["r_bad"]["out"][keep], c["r_ok"]["out"][keep])
    assert (c["r_bad"]["out"][over].abs() == R.F16_MAX).all()


# ------------------------------------------------------------------------------------------------ the argument-block entries, on the host
@pytest.fixture(scope="module")
def hip():
    h = sub("_hip")
    h.build()
    h.load()
    return h


def chain_block(hip, **kw):
    g = hip.MttsChainArgs()
    base = dict(d_att=FAKE, d_x=FAKE, M=40, C=128, inner=128, h_w_out=FAKE, h_w1=FAKE, h_p0=FAKE, h_p1=FAKE, h_w2=FAKE, h_w_qkv=FAKE, n_qkv=384,
                qb=64, ch=128, d_x_out=FAKE, d_qkv_out=FAKE, tag=b"untouched")
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("kw,needle", [
    (dict(C=192), "unsupported shape"), (dict(M=0), "unsupported shape"), (dict(inner=96), "unsupported shape"), (dict(ch=64), "unsupported shape"),
    (dict(inner=0, d_att=None, h_w_out=None, h_w_qkv=None, pair=1), "pair form"),
    (dict(pad_x=4), "row pad"), (dict(pad_qkv=-8), "row pad"), (dict(pad_out=8192), "row pad"), (dict(pad_att=12), "row pad"),
    (dict(sentinel=0x10000), "16-bit"),
    (dict(d_x=None), "null buffer"), (dict(h_w1=None), "null buffer"), (dict(h_p0=None), "null buffer"), (dict(d_x_out=None), "null buffer"),
    (dict(d_qkv_out=None), "null buffer"), (dict(d_att=None), "null buffer"),
])
def test_chain_args_refusals_before_any_launch(hip, kw, needle):
    lib = hip.load()
    g = chain_block(hip, **kw)
    assert lib.mtts_tblock_chain_args_run(C.byref(g), FAKE, None) == -1
    assert needle.encode() in lib.mtts_last_error(), lib.mtts_last_error()
    assert lib.mtts_tblock_chain_args_run(None, FAKE, None) == -1 and lib.mtts_tblock_chain_args_scratch_bytes(None) == -1
    assert lib.mtts_tblock_chain_args_run(C.byref(chain_block(hip)), None, None) == -1 and b"null buffer" in lib.mtts_last_error()


def test_chain_args_scratch_grows_with_pads_and_guard_rows(hip):
    lib = hip.load()
    plain = lib.mtts_tblock_chain_args_scratch_bytes(C.byref(chain_block(hip)))
    padded = lib.mtts_tblock_chain_args_scratch_bytes(C.byref(chain_block(hip, pad_att=8, pad_x=16, pad_out=24, pad_qkv=32)))
    guard = hip.ENTRY_GUARD_ROWS
    assert guard == 64 and "#define MTTS_ENTRY_GUARD_ROWS 64" in (ROOT / "include" / "mtts.h").read_text()
    assert plain >= 40 * 256 * 2 * 2 + (40 + guard) * (256 + 768) * 2 + 4 * (18 * 128 + 2 * 384)
    assert padded - plain >= 2 * (40 * (8 + 16) + (40 + guard) * (24 + 32)) - 4 * 256
    assert lib.mtts_tblock_chain_args_scratch_bytes(C.byref(chain_block(hip, pair=1))) >= plain


def conv_block(hip, **kw):
    g = hip.MttsConvGnArgs()
    base = dict(d_x=FAKE, B=2, T=66, C=96, N=384, d_w=FAKE, d_wpacked=FAKE, d_bias=FAKE, d_gamma=FAKE, d_beta=FAKE, d_mask=FAKE, eps=1e-5,
                d_out=FAKE, tag=b"untouched")
    base.update(kw)
    for k, v in base.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("kw,needle", [
    (dict(C=80), "multiples of 32"), (dict(c1=96), "c1 < C"), (dict(T=64), "unsupported shape"), (dict(T=385), "unsupported shape"),
    (dict(N=256), "unsupported shape"), (dict(B=0), "multiples of 32"),
    (dict(pad_x=4), "row pad"), (dict(pad_out=-8), "row pad"), (dict(sentinel=0x10000), "16-bit"),
    (dict(d_chbias=FAKE, chbias_stride=100), "bias row"), (dict(d_nextra=FAKE), "come together"),
    (dict(d_x=None), "null buffer"), (dict(d_mask=None), "null buffer"), (dict(d_out=None), "null buffer"),
])
def test_conv_gn_args_refusals_before_any_launch(hip, kw, needle):
    lib = hip.load()
    g = conv_block(hip, **kw)
    assert lib.mtts_conv_gn_args_run(C.byref(g), FAKE, None) == -1
    assert needle.encode() in lib.mtts_last_error(), lib.mtts_last_error()
    assert lib.mtts_conv_gn_args_run(None, FAKE, None) == -1 and lib.mtts_conv_gn_args_scratch_bytes(None) == -1
    need = lib.mtts_conv_gn_args_scratch_bytes(C.byref(conv_block(hip, pad_x=8, pad_out=16)))
    assert need >= 2 * 66 * (192 + 8) * 2 + (2 * 66 + hip.ENTRY_GUARD_ROWS) * (768 + 16) * 2

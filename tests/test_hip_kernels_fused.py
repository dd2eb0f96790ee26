"""Kernel-level parity of the two fused P16 kernels -- tblock_chain_kernel (csrc/tblock_chain.hip, single and pair form, all eight
instantiations) and conv_gn_kernel (csrc/resnet_conv.hip, both wave layouts) -- through the argument-block entries
(include/mtts.h mtts_tblock_chain_args_run, mtts_conv_gn_args_run) against the fp64 restatement of tests/fused_restated.py.

Measure and bar.  e = max over elements of |out - restated| / (u B), u = 2^-24, B the per-element budget derived in
fused_restated.py; per output (x_out, qkv; conv_gn: out).  The device must hold
    e_hip <= 8 e_cpu32 + cos
with e_cpu32 the same measure of the fp32 CPU twin (computed here, never from the device), 8 = 4 (22-bit products against fp32's
24 bits) x 2 (another summation order), and cos the hardware-cosine allowance: (p1 / 2) delta_cos per hidden element with
delta_cos = 1e-6 (csrc/device_utils.h), carried to the outputs like B_h and expressed in the same units, max over elements of
cos_abs / (u B).  conv_gn has no cosine: e_hip <= 8 e_cpu32.  Every (case, e_hip, e_cpu32, cos) is printed and, with
$MTTS_FUSED_REPORT set, appended to the file that became profiles/r20_fused_parity.md; the worst figures measured there are
quoted at the end of this docstring.

Beside the bar, every launch asserts: the instantiation (tag), range flag 0, the decoded images are bitwise fixed points of the
split they were stored with (p16(x_out, 2048), p16(qkv, 1)), the raw image decodes to them in the image layout and its head plane
holds the fp16 roundings (both planes' packed stores, the lane-to-channel map), every payload element was written, and the pad columns and the 64 guard rows behind
row M still hold the sentinel.  Further: strided images give the bits of packed ones; a row's bits do not depend on its tile
neighbours (x100 rows), on its position (rolled by 19) or, in the pair form, on the launch; the range test (x2, or the Block1D
output, beyond 65504 in one row / utterance: flag raised, heads +-65504, every other row unchanged); masked rows exactly 0.
The closing test fails if one of the 8 x 2 chain instantiations-and-forms or one of the two conv_gn layouts was never launched.

Worst figures (profiles/r20_fused_parity.md):
  x_out    e_hip 0.2416 against a bar of 0.8255 (ratio 0.29; C 384, qb 48, ch 256, M 15 / 17), largest e_hip 0.5658 against 4.55
  qkv      e_hip 0.0098 against a bar of 0.0782 (ratio 0.13; C 128, qb 32, n_qkv 352), largest e_hip 0.0139 against 0.125
  conv_gn  e_hip 0.1998 against a bar of 2.2171 (ratio 0.09; T 65, C 96), largest e_hip 0.3243 against 3.63
  The cosine allowance was never needed (every line also holds e_hip <= 8 e_cpu32); the single and the pair form measure the same.
Each of six one-line mutations of the kernels (scratch builds) fails this file; the table there names the test and the factor."""
import os

import pytest
import torch

import fused_restated as R
from conftest import sub
from p16_restated import p16

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MTTS_FUSED_REPORT")
SENTINEL = 0x7e00                      # an fp16 NaN: poisons whatever reads a pad column, and no finite image holds it
LAUNCHED = set()
CHAIN_CASES = R.chain_case_list()
CONV_CASES = R.conv_case_list()


def note(case, e_hip, e_cpu32, cos):
    line = f"| {case} | {e_hip:.4f} | {e_cpu32:.4f} | {cos:.4f} | {8 * e_cpu32 + cos:.4f} |"
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("_hip")


def dev(t):
    return None if t is None else t.contiguous().cuda()


def decode(bits, lscale):
    """int16 image bits [M, 2 C] -> fp32 [M, C]: per 32-channel group 32 heads then 32 residuals, value h + l / lscale.  (The pair is not
    unique at a tie -- a residual of exactly half an ulp of the head -- so images are compared by value, not re-split.)"""
    v = bits.contiguous().view(torch.float16).float().view(bits.shape[0], -1, 2, 32)
    return (v[:, :, 0] + v[:, :, 1] / lscale).reshape(bits.shape[0], -1)


def heads_are_roundings(bits, lscale):
    """every head is the fp16 rounding of its value: the residual is at most half an ulp of the head (which plane is which)"""
    v = bits.contiguous().view(torch.float16).float().view(bits.shape[0], -1, 2, 32)
    h, l = v[:, :, 0], v[:, :, 1] / lscale
    ulp = torch.where(h == 0, torch.tensor(2.0 ** -24), 2.0 ** (torch.clamp(torch.frexp(h.abs())[1] - 1, min=-14) - 10).float())
    return (l.abs() <= ulp / 2).all().item()


def sent(t):
    return (t.cpu() == torch.tensor(SENTINEL, dtype=torch.int16)).all().item()


def run_chain(hip, ops, M, qb, ch, pair, mask=None, expect_flag=0, **pads):
    """One launch through the argument block, with every assertion that holds for EVERY launch; returns the entry's dict (on the CPU)."""
    att, x, w = ops[0], ops[1], ops[2:]
    Cc, n_qkv = x.shape[1], (w[8].shape[0] if w[8] is not None else 0)
    res = hip.tblock_chain_args(dev(None if att is None else att[:M]), dev(x[:M]), *w[:8], w_qkv=w[8], b_qkv=w[9],
                                out_mask=dev(None if mask is None else mask[:M]), qb=qb, ch=ch, pair=pair, sentinel=SENTINEL, **pads)
    assert res["tag"] == f"tblock_chain_kernel<{Cc}, {qb}, {ch}>" and hip.last_kernel_tag() == res["tag"]
    LAUNCHED.add((Cc, qb, ch, bool(pair)))
    res = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    assert res["flag"].tolist() == [expect_flag, 0]                    # (second word: a pair-form workgroup gave up waiting)
    for name, width, ls, pad in (("x_out", Cc, 2048.0, pads.get("pad_out", 0)), ("qkv", n_qkv, 1.0, pads.get("pad_qkv", 0))):
        if not width:
            continue
        out, img = res[name], res[name + "_image"]
        assert img.shape == (M + hip.ENTRY_GUARD_ROWS, 2 * width + pad)
        assert sent(img[M:]) and sent(img[:M, 2 * width:]), f"{name}: the kernel wrote outside its rows"
        assert torch.isfinite(out).all()
        assert torch.equal(p16(out, ls), out), f"{name}: not a fixed point of its split"
        assert torch.equal(decode(img[:M, :2 * width], ls), out), f"{name}: the raw image does not hold the decoded values"
        assert heads_are_roundings(img[:M, :2 * width], ls), f"{name}: a head plane that is not the rounding of its values"
    return res


def chain_bar(case_name, res, case, M):
    r64, r32, B = case["r64"], case["r32"], case["B"]
    for name in ("x_out", "qkv"):
        if res.get(name) is None:
            continue
        b = B[name][:M]
        e_hip = R.measure(res[name], r64[name][:M], b)
        e_cpu = R.measure(r32[name][:M], r64[name][:M], b)
        cos = R.cos_term(B["cos_" + name][:M], b)
        note(f"{case_name} {name}", e_hip, e_cpu, cos)
        assert e_hip <= 8 * e_cpu + cos, (case_name, name, e_hip, e_cpu, cos)


def chain_id(c):
    key, qb, ch, M, pair = c
    kind, Cc, inner, n_qkv, none = key
    return f"{kind}-C{Cc}-qb{qb}-ch{ch}-inner{inner}-nqkv{n_qkv}-M{M}-{'pair' if pair else 'single'}" + (f"-no_{none.replace(',', '_')}" if none else "")


@pytest.mark.parametrize("c", CHAIN_CASES, ids=chain_id)
def test_chain_parity(hip, c):
    key, qb, ch, M, pair = c
    case = R.chain_case(*key)
    res = run_chain(hip, case["ops"], M, qb, ch, pair, mask=case["mask"])
    chain_bar(chain_id(c), res, case, M)
    if case["mask"] is not None:
        gone = case["mask"][:M] == 0
        assert gone.any() and (res["x_out"][gone] == 0).all() and (res["x_out_image"][:M, :2 * key[1]][gone] == 0).all()
    if (key[1], qb, ch) in R.SWEEP_SHAPES and key[0] == "plain":
        # image rows longer than their payload: the same bits, and nothing in the pad columns
        strided = run_chain(hip, case["ops"], M, qb, ch, pair, pad_att=8, pad_x=16, pad_out=24, pad_qkv=40)
        assert torch.equal(strided["x_out"], res["x_out"]) and (res["qkv"] is None or torch.equal(strided["qkv"], res["qkv"]))
    if pair:
        again = run_chain(hip, case["ops"], M, qb, ch, pair, mask=case["mask"])
        assert torch.equal(again["x_out_image"], res["x_out_image"])
        assert res["qkv_image"] is None or torch.equal(again["qkv_image"], res["qkv_image"])


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("Cc", [384, 128])
def test_chain_rows_do_not_depend_on_neighbours_or_position(hip, Cc, pair):
    inner, n_qkv = R.FULL[Cc]
    key = ("hard", Cc, inner, n_qkv, "b_out")
    case, loud = R.chain_case(*key), R.chain_case("loud", *key[1:])
    M, kept = R.HARD_M, R.HARD_KEPT
    base = run_chain(hip, case["ops"], M, 64, 128, pair, mask=case["mask"])
    other = run_chain(hip, loud["ops"], M, 64, 128, pair, mask=loud["mask"])
    chain_bar(f"loud-C{Cc}-{'pair' if pair else 'single'}", other, loud, M)
    assert torch.equal(other["x_out_image"][kept], base["x_out_image"][kept]) and torch.equal(other["qkv_image"][kept], base["qkv_image"][kept])
    assert not torch.equal(other["x_out"], base["x_out"])
    roll = lambda t: None if t is None else torch.roll(t, 19, 0)
    ops = [roll(case["ops"][0]), roll(case["ops"][1])] + case["ops"][2:]
    rolled = run_chain(hip, ops, M, 64, 128, pair, mask=roll(case["mask"]))
    assert torch.equal(torch.roll(rolled["x_out"], -19, 0), base["x_out"]) and torch.equal(torch.roll(rolled["qkv"], -19, 0), base["qkv"])
    # the same rows in 32-row tiles (two workgroups, other lanes) hold the same bits
    small = run_chain(hip, case["ops"], M, 32, 128, pair, mask=case["mask"])
    assert torch.equal(small["x_out"], base["x_out"]) and torch.equal(small["qkv"], base["qkv"])


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
def test_chain_range_flag_and_saturation(hip, pair):
    c = R.chain_range_case()
    M, row = 40, R.RANGE_ROW
    ok = run_chain(hip, [c["att"], c["x"]] + c["w"], M, 64, 128, pair)
    bad = run_chain(hip, [c["att"], c["bad"]] + c["w"], M, 64, 128, pair, expect_flag=1)
    rest = [i for i in range(M) if i != row]
    assert torch.equal(bad["x_out_image"][rest], ok["x_out_image"][rest]) and torch.equal(bad["qkv_image"][rest], ok["qkv_image"][rest])
    raw = c["r_bad"]["x2_raw"][row]
    over = raw.abs() > R.F16_MAX
    assert over.sum() >= 2
    got = bad["x_out"][row][over]
    assert torch.equal(got, torch.sign(raw[over]).float() * 65504.0), got
    img = bad["x_out_image"][row].view(-1, 2, 32)                               # [group][head | residual][32]
    idx = torch.nonzero(over).flatten()
    hb = img[idx // 32, 0, idx % 32]
    assert hb.tolist() == [0x7bff if v > 0 else 0xfbff - 0x10000 for v in raw[over].tolist()]
    assert (img[idx // 32, 1, idx % 32] == 0).all()


def test_every_chain_instantiation_was_launched_in_both_forms():
    want = {(Cc, qb, ch, pair) for Cc, qb, ch in R.CHAIN_SHAPES for pair in (False, True)}
    assert want <= LAUNCHED, sorted(want - LAUNCHED)


# ------------------------------------------------------------------------------------------------ conv_gn
def run_conv(hip, case, T, c1=0, chbias="case", expect_flag=0, **pads):
    ops, kw, B = case["ops"], dict(case["kw"]), case["B"]
    if not isinstance(chbias, str):
        kw["chbias"] = chbias
    if "nextra" in kw:
        kw["bias_stats"] = R.bias_stats(ops[2])
    N = ops[1].shape[0]
    res = hip.conv_gn_args(*[dev(t) for t in ops], B=B, T=T, c1=c1, sentinel=SENTINEL, **{k: dev(v) for k, v in kw.items()}, **pads)
    tag = "conv_gn_kernel<2>" if T <= 192 else "conv_gn_kernel<1>"
    assert res["tag"] == tag and hip.last_kernel_tag() == tag
    LAUNCHED.add(tag)
    res = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    assert res["flag"].tolist() == [expect_flag]
    out, img, pad = res["out"], res["image"], pads.get("pad_out", 0)
    assert img.shape == (B * T + hip.ENTRY_GUARD_ROWS, 2 * N + pad)
    assert sent(img[B * T:]) and sent(img[:B * T, 2 * N:]), "the kernel wrote outside its rows"
    assert torch.isfinite(out).all() and torch.equal(p16(out), out) and torch.equal(decode(img[:B * T, :2 * N], 2048.0), out) and heads_are_roundings(img[:B * T, :2 * N], 2048.0)
    gone = ops[5] == 0
    assert (out[gone] == 0).all()                                              # masked frames are exactly 0
    return res


def conv_bar(name, res, case):
    e_hip = R.measure(res["out"], case["r64"]["out"], case["budget"])
    e_cpu = R.measure(case["r32"]["out"], case["r64"]["out"], case["budget"])
    note(name, e_hip, e_cpu, 0.0)
    assert e_hip <= 8 * e_cpu, (name, e_hip, e_cpu)


@pytest.mark.parametrize("key", CONV_CASES, ids=lambda k: "-".join(str(v) for v in k))
def test_conv_gn_parity(hip, key):
    kind, T, Cc, c1 = key
    case = R.conv_case(*key)
    chbias = "case"
    if kind == "rows":                                                         # a row stride above N, NaN in the tail no launch may read
        cb = case["kw"]["chbias"]
        chbias = torch.full((cb.shape[0], cb.shape[1] + 16), float("nan"))
        chbias[:, :cb.shape[1]] = cb
    res = run_conv(hip, case, T, c1, chbias=chbias)
    conv_bar("conv_gn " + "-".join(str(v) for v in key), res, case)
    strided = run_conv(hip, case, T, c1, chbias=chbias, pad_x=8, pad_out=24)
    assert torch.equal(strided["out"], res["out"])
    if kind == "loud":                                                         # a x100 utterance: its neighbours do not change by a bit
        quiet = run_conv(hip, R.conv_case("quiet", T, Cc, c1), T, c1)
        rows = torch.cat([torch.arange(0, T), torch.arange(2 * T, 3 * T)])
        assert torch.equal(quiet["image"][rows], res["image"][rows]) and not torch.equal(quiet["out"][T:2 * T], res["out"][T:2 * T])


def test_conv_gn_range_flag_and_saturation(hip):
    c = R.conv_range_case()
    T, utt = 66, R.RANGE_UTT
    case = {"ops": c["ops"], "kw": c["kw"], "B": c["B"]}
    ok = run_conv(hip, case, T, chbias=c["ok"])
    bad = run_conv(hip, case, T, chbias=c["bad"], expect_flag=1)
    keep = torch.ones(3 * T, dtype=torch.bool)
    keep[utt * T:(utt + 1) * T] = False
    assert torch.equal(bad["image"][:3 * T][keep], ok["image"][:3 * T][keep])
    raw = c["r_bad"]["out_raw"]
    over = raw.abs() > R.F16_MAX
    assert over.any() and torch.equal(bad["out"][over], torch.sign(raw[over]).float() * 65504.0)


def test_both_conv_gn_layouts_were_launched():
    assert {"conv_gn_kernel<2>", "conv_gn_kernel<1>"} <= LAUNCHED

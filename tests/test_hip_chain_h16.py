"""GPU parity of the one-plane transformer-block chain kernel (csrc/tblock_chain_h16.hip) through the C ABI (mtts_tblock_chain_h16)
against fp64 PyTorch on operands pre-rounded to the 16-bit type, for fp16 and bfloat16 planes; masked rows, row independence,
prefetch workgroups and repeat launches bitwise."""
import pytest
import torch

from conftest import sub
from test_hip_chain import chain_ref, make_case

pytestmark = pytest.mark.gpu

# max |error| / max(|reference|, 1) against fp64 on pre-rounded operands.  What remains are the roundings INSIDE the chain (x1, the
# hidden layer, x2 and the outputs themselves: four 16-bit roundings at unit round-off 2^-11 / 2^-8, amplified by the FeedForward).
# Measured on an MI355X over the cases below: at most 6.4e-4 (fp16) and 4.8e-3 (bfloat16); the bars are below twice that.
TOL = {False: 1.2e-3, True: 9e-3}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("_hip")


def r16(t, bf16):
    return None if t is None else t.to(torch.bfloat16 if bf16 else torch.float16).float()


def rounded_case(M, C, inner, n_qkv, seed, bf16):
    """make_case with every 16-bit operand (activations, panels) pre-rounded; biases and SnakeBeta constants stay fp32."""
    att, x, w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv, b_qkv = make_case(M, C, inner, n_qkv, seed)
    return (r16(att, bf16), r16(x, bf16), r16(w_out, bf16), b_out, r16(w1, bf16), b1, p0, p1, r16(w2, bf16), b2, r16(w_qkv, bf16), b_qkv)


def run(hip, case, dev, **kw):
    att = case[0]
    return hip.tblock_chain_h16(None if att is None else att.to(dev), case[1].to(dev), *case[2:10], w_qkv=case[10], b_qkv=case[11], **kw)


CASES = [
    # M, C, inner, n_qkv, qb, ch
    (200, 384, 384, 1152, 64, 256),       # production width, a partly filled last workgroup
    (250, 384, 384, 1152, 96, 256),       # 96-row workgroups (two staging passes)
    (97, 384, 384, 1152, 32, 256),
    (130, 384, 384, 1152, 64, 128),
    (100, 384, 384, 0, 96, 256),          # last block of a run: no q|k|v
    (70, 384, 0, 0, 64, 256),             # FeedForward alone
    (75, 128, 128, 384, 64, 128),         # narrow estimators of the test suite
    (33, 128, 128, 352, 32, 128),         # q|k|v width that leaves the last pass partly empty
    (90, 256, 256, 768, 64, 128),
    (50, 256, 128, 384, 32, 128),
    (40, 256, 0, 0, 32, 128),
]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,C,inner,n_qkv,qb,ch", CASES)
def test_chain_h16_vs_fp64_on_rounded_operands(hip, M, C, inner, n_qkv, qb, ch, bf16):
    case = rounded_case(M, C, inner, n_qkv, 100 + M, bf16)
    _, x2, qkv = chain_ref(*case)
    x_out, qkv_out = run(hip, case, torch.device("cuda"), bf16=bf16, qb=qb, ch=ch)
    worst = {}
    for what, out, ref in (("x_out", x_out, x2), ("qkv", qkv_out, qkv)):
        if ref is None:
            continue
        assert torch.isfinite(out).all()
        worst[what] = (out.cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1.0)
    print(f"h16 chain {'bf16' if bf16 else 'fp16'} M={M} C={C} inner={inner} n_qkv={n_qkv} qb={qb} ch={ch}: relative error {worst}")
    for what, e in worst.items():
        assert e <= TOL[bf16], (what, e)
        assert e > 0.0                    # really 16-bit arithmetic


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_masked_rows_are_zero_and_rows_are_independent(hip, bf16):
    M, C = 230, 384
    case = rounded_case(M, C, 384, 1152, 7, bf16)
    dev = torch.device("cuda")
    mask = (torch.arange(M) % 5 != 0).float()
    plain, q_plain = run(hip, case, dev, bf16=bf16, qb=64, ch=256)
    masked, q_masked = run(hip, case, dev, bf16=bf16, qb=64, ch=256, out_mask=mask.to(dev))
    keep = mask.bool().to(dev)
    assert torch.equal(masked[keep], plain[keep])
    assert masked[~keep].abs().max().item() == 0.0
    assert torch.equal(q_masked, q_plain)
    # the same rows shifted by 19 positions: other row tiles, other lanes, other neighbours in the tile
    shifted = list(case)
    shifted[0], shifted[1] = torch.roll(case[0], 19, 0), torch.roll(case[1], 19, 0)
    rolled, q_rolled = run(hip, shifted, dev, bf16=bf16, qb=64, ch=256)
    assert torch.equal(torch.roll(rolled, -19, 0), plain) and torch.equal(torch.roll(q_rolled, -19, 0), q_plain)
    # other workgroup heights: the same accumulation order per row
    for qb in (32, 96):
        other, q_other = run(hip, case, dev, bf16=bf16, qb=qb, ch=256)
        assert torch.equal(other, plain) and torch.equal(q_other, q_plain), qb


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
def test_prefetch_workgroups_and_repeat_launches_are_bitwise_equal(hip, bf16):
    M, C = 300, 384
    case = rounded_case(M, C, 384, 1152, 11, bf16)
    dev = torch.device("cuda")
    base, q_base = run(hip, case, dev, bf16=bf16, qb=64, ch=256, pf_wgs=0)
    for pf in (0, 8, 16):
        out, q = run(hip, case, dev, bf16=bf16, qb=64, ch=256, pf_wgs=pf)
        assert torch.equal(out, base) and torch.equal(q, q_base), pf


def test_pair_form_and_bad_shapes_are_refused(hip):
    dev = torch.device("cuda")
    case = rounded_case(64, 256, 192, 0, 3, False)            # attention width 192: not a whole ring period
    with pytest.raises(RuntimeError):
        run(hip, case, dev, qb=64, ch=128)
    case = rounded_case(64, 128, 128, 0, 3, False)
    with pytest.raises(RuntimeError):
        run(hip, case, dev, qb=96, ch=128)                    # 96-row workgroups exist at width 384 only

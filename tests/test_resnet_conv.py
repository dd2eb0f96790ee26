"""The one-launch Block1D (csrc/resnet_conv.hip, conv_gn_kernel): the kernel alone through the C ABI against fp64 PyTorch, the
model with the launch switched on and off (MTTS_RESNET_FUSE), and static checks of its LDS-DMA ring's instruction stream."""
import re
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

from conftest import sub



def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def block1d_fp64(x, w, bias, gamma, beta, mask, B, T, chbias, nrows):
    """Block1D of the reference decoder on channels-last rows, statistics over the first nrows[b] frames of utterance b."""
    xd = x.double().view(B, T, -1).transpose(1, 2)
    y = F.conv1d(xd, w.double(), bias.double(), padding=1)
    out = torch.empty_like(y)
    for b in range(B):
        n = int(nrows[b]) if nrows is not None else T
        g = y[b].view(8, -1, T)
        mean = g[:, :, :n].mean(dim=(1, 2), keepdim=True)
        var = ((g[:, :, :n] - mean) ** 2).mean(dim=(1, 2), keepdim=True)
        out[b] = ((g - mean) / torch.sqrt(var + 1e-5)).view(-1, T) * gamma.double()[:, None] + beta.double()[:, None]
    m = mask.double().view(B, 1, T)
    out = F.mish(out) * m
    if chbias is not None:
        out = (out + chbias.double()[None, :, None]) * m
    return out.transpose(1, 2).reshape(B * T, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,C,c1,ragged,tb", [(2, 65, 384, 0, False, True), (3, 161, 384, 0, True, True), (2, 176, 768, 384, True, False),
                                                (2, 192, 96, 32, True, True), (5, 100, 384, 0, True, False), (2, 193, 384, 0, True, True),
                                                (3, 322, 384, 0, True, True), (2, 384, 768, 384, False, False)])
def test_conv_gn_kernel_vs_fp64(B, T, C, c1, ragged, tb):
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    hip = sub("_hip")
    N = 384
    x = rnd(B * T, C, seed=1) * 1.3 + 0.1
    w = rnd(N, C, 3, seed=2) / (3 * C) ** 0.5
    bias, gamma, beta = 0.2 * rnd(N, seed=3), 1 + 0.1 * rnd(N, seed=4), 0.1 * rnd(N, seed=5)
    chbias = 0.3 * rnd(N, seed=6) if tb else None
    lens = torch.tensor([max(1, T - 37 * i) if i + 1 < B else 1 for i in range(B)]) if ragged else torch.full((B,), T)
    mask = (torch.arange(T)[None] < lens[:, None]).float().reshape(-1)
    x = x * mask[:, None]                     # images reach the conv already masked
    nrows = lens.to(torch.int32) if ragged else None
    ref = block1d_fp64(x, w, bias, gamma, beta, mask, B, T, chbias, nrows)
    dev = torch.device("cuda")
    out = hip.conv_gn(x.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), beta.to(dev), mask.to(dev), B=B, T=T, c1=c1,
                      chbias=chbias.to(dev) if tb else None, nrows=nrows.to(dev) if ragged else None)
    out2 = hip.conv_gn(x.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), beta.to(dev), mask.to(dev), B=B, T=T, c1=c1,
                       chbias=chbias.to(dev) if tb else None, nrows=nrows.to(dev) if ragged else None)
    assert torch.equal(out, out2)             # fixed reduction order: run-to-run identical
    err = (out.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5 * max(ref.abs().max().item(), 1.0), err


@pytest.mark.gpu
def test_conv_gn_closed_form_rows_match_explicit_rows():
    """nextra copies of the conv's bias row enter the statistics in closed form (folded padding): the same numbers as a longer
    utterance whose extra rows ARE the bias row."""
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    hip = sub("_hip")
    dev = torch.device("cuda")
    B, T, C, N, L, extra = 2, 120, 384, 384, 70, 30
    x = rnd(B * T, C, seed=11)
    w = rnd(N, C, 3, seed=12) / (3 * C) ** 0.5
    bias, gamma, beta = 0.2 * rnd(N, seed=13), 1 + 0.1 * rnd(N, seed=14), 0.1 * rnd(N, seed=15)
    mask = (torch.arange(T)[None] < torch.tensor([L, L])[:, None]).float().reshape(-1)
    x = x * mask[:, None]
    # rows L+1 .. see zero input on all three taps: their conv output is the bias row
    gb = bias.double().view(8, -1)
    bstats = torch.stack([gb.mean(1), ((gb - gb.mean(1, keepdim=True)) ** 2).sum(1)], 1).float().contiguous()
    a = hip.conv_gn(x.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), beta.to(dev), mask.to(dev), B=B, T=T,
                    nrows=torch.tensor([L + 2, L + 2], dtype=torch.int32, device=dev),
                    nextra=torch.tensor([extra, extra], dtype=torch.int32, device=dev), bias_stats=bstats.to(dev))
    b = hip.conv_gn(x.to(dev), w.to(dev), bias.to(dev), gamma.to(dev), beta.to(dev), mask.to(dev), B=B, T=T,
                    nrows=torch.tensor([L + 2 + extra, L + 2 + extra], dtype=torch.int32, device=dev))
    assert (a - b).abs().max().item() <= 2e-6


@pytest.mark.gpu
def test_model_resnet_fuse_switch_agrees_and_repeats(hparams, synthetic, monkeypatch):
    """Short ragged utterances (both levels within the kernel's 65..384 rows): MTTS_RESNET_FUSE=0 (tiled launches), 5 (first
    Block1D and the final one) and 7 (both Block1Ds) -- bit 2 lifts the batch gate, the model takes the launch from B = 16 -- give
    the same mel to reordered-sum accuracy, and two runs of each are bit-identical."""
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    dev = torch.device("cuda")
    inf = sub("inference")
    hp = hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    x, x_len, spk = synthetic.make_inputs(hp, 3, 48, seed=99, lengths=[48, 40, 29])
    mels = {}
    for flag in ("7", "5", "0"):
        monkeypatch.setenv("MTTS_RESNET_FUSE", flag)
        m = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        m.decoder.solver = "euler"
        runs = [m.synthesise(x.to(dev), x_len.to(dev), 2, speaker=spk.to(dev))["mel"].clone() for _ in range(2)]
        assert torch.equal(runs[0], runs[1])
        mels[flag] = runs[0]
    scale = max(1.0, mels["0"].abs().max().item())
    assert not torch.equal(mels["7"], mels["0"])          # (the launch was taken: reordered sums differ in the last bits)
    assert (mels["5"] - mels["0"]).abs().max().item() <= 2e-5 * scale
    assert (mels["7"] - mels["0"]).abs().max().item() <= 2e-5 * scale


def test_conv_gn_ring_is_not_spilled_and_waits_are_the_written_ones(tmp_path_factory):
    """conv_gn_kernel<KS> counts its LDS-DMA pieces by hand (KS = 2: 5 or 6 per wave and stage, one stage in flight across the
    barrier; KS = 1: every stage drained).  A spill would put scratch loads into those counts: no scratch traffic anywhere in
    the kernel, the DMA requests are exactly the written issue sites (a wave's 6 / 9 pieces, two / one prologue stages + the
    loop), and the ring's `s_waitcnt vmcnt(N) lgkmcnt(0)` + `s_barrier` pairs carry only the written constants."""
    from test_isa_guard import disassemble
    isa = disassemble("resnet_conv", tmp_path_factory)
    names = {int(re.search(r"conv_gn_kernelILi(\d)E", n).group(1)): n for n in isa if "conv_gn_kernel" in n}
    assert set(names) == {1, 2}, list(isa)
    for ks, name in names.items():
        insns = isa[name]
        ops = Counter(x[1] for x in insns)
        assert not any(k.startswith("scratch_") for k in ops), (name, "scratch traffic")
        assert not any(k.startswith("buffer_") or k.startswith("flat_") for k in ops), name
        assert ops["v_mfma_f32_16x16x32_f16"] >= 81 and ops["v_mfma_f32_16x16x32_f16"] % 27 == 0, (name, ops["v_mfma_f32_16x16x32_f16"])
        nj, sites = (6, 3) if ks == 2 else (9, 2)
        assert ops["global_load_lds_dwordx4"] == nj * sites, (name, ops["global_load_lds_dwordx4"])
        ring = Counter()
        for k, x in enumerate(insns[:-1]):
            m = re.search(r"vmcnt\((\d+)\) lgkmcnt\(0\)", x[2]) if x[1] == "s_waitcnt" else None
            if m and insns[k + 1][1] == "s_barrier":
                ring[int(m.group(1))] += 1
        assert set(ring) == ({0, 5, 6} if ks == 2 else {0}), (name, dict(ring))

"""Write-through output stores (MTTS_STORE_WT, csrc/model.h Switches::store_wt; csrc/device_utils.h store16): a cache policy on the
stores of the P16 output images and, for the chain's q|k|v and the attention output, a lane exchange that widens 8-byte stores to
16 bytes.  Neither may change one bit, so every test compares MTTS_STORE_WT=0 with all bits set by ``torch.equal`` -- whatever the
default mask is.  The shapes have a last tile that is partly past the end at every store site (a wrong lane pairing, tail guard or
chunk address shows in the image or in the sentinel-filled guard rows behind it), and the model-level cases cross launch
boundaries, which is what write-through actually changes."""
import pytest
import torch

from conftest import sub

pytestmark = pytest.mark.gpu

ALL_BITS = "31"          # tiled P16 GEMM | conv_gn | chain x_out | chain q|k|v | attention (csrc/kernels.h StoreWt)
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("_hip")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def both(monkeypatch, call):
    """call() under MTTS_STORE_WT=0 and under all bits: the unit entries read the switch per call"""
    res = []
    for mask in ("0", ALL_BITS):
        monkeypatch.setenv("MTTS_STORE_WT", mask)
        res.append(call())
    return res


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ between MTTS_STORE_WT=0 and {ALL_BITS}"


# ------------------------------------------------------------------------------------------------ tiled P16 GEMM
@pytest.mark.parametrize("masked", [False, True])
def test_gemm_p16_image(hip, monkeypatch, masked):
    """80 rows = one 64-row tile + 16 rows, N = 160 = one 128-column tile + 32 columns; once with a row mask and a residual image"""
    B, T, K, N = 2, 40, 64, 160
    a, w, b = (rnd(B * T, K, seed=1) * 2 + 0.3).to(DEV), rnd(N, K, seed=2, scale=K ** -0.5).to(DEV), rnd(N, seed=3).to(DEV)
    kw = {}
    if masked:
        lens = torch.tensor([T, T - 9])
        mask = (torch.arange(T)[None] < lens[:, None]).float().reshape(-1).to(DEV)
        kw = dict(res16=rnd(B * T, N, seed=4).to(DEV), out_mask=mask, out16_mask=mask)
    lo, hi = both(monkeypatch, lambda: hip.gemm_p16_args(a, w, b, B=B, T_in=T, want_p16=True, force_bm=64, **kw))
    same(lo["out16"], hi["out16"], "image")
    same(lo["out"], hi["out"], "rows")
    assert lo["tag"] == hi["tag"] and "gemm_p16_kernel<64" in lo["tag"], (lo["tag"], hi["tag"])
    assert lo["out16"].abs().max().item() > 0.1


# ------------------------------------------------------------------------------------------------ conv + GroupNorm + Mish
@pytest.mark.parametrize("T,form", [(70, "conv_gn_kernel<2>"), (200, "conv_gn_kernel<1>")])
def test_conv_gn_image(hip, monkeypatch, T, form):
    """width 384, ragged through nrows: T = 70 the split-K form (last wave partly empty), T = 200 the eight-wave form"""
    B, C, N = 2, 384, 384
    lens = torch.tensor([T, T - 23])
    mask = (torch.arange(T)[None] < lens[:, None]).float().reshape(-1)
    x = ((rnd(B * T, C, seed=1) * 1.3 + 0.1) * mask[:, None]).to(DEV)
    w = (rnd(N, C, 3, seed=2) / (3 * C) ** 0.5).to(DEV)
    bias, gamma, beta, chb = (0.2 * rnd(N, seed=3)).to(DEV), (1 + 0.1 * rnd(N, seed=4)).to(DEV), (0.1 * rnd(N, seed=5)).to(DEV), (0.3 * rnd(N, seed=6)).to(DEV)
    nrows = lens.to(torch.int32).to(DEV)
    lo, hi = both(monkeypatch, lambda: hip.conv_gn(x, w, bias, gamma, beta, mask.to(DEV), B=B, T=T, chbias=chb, nrows=nrows))
    same(lo, hi, "rows")
    assert lo.abs().max().item() > 0.1
    # the raw image with the sentinel-filled guard rows behind it: nothing written past the end
    lo, hi = both(monkeypatch, lambda: hip.conv_gn_args(x, w, bias, gamma, beta, mask.to(DEV), B=B, T=T, chbias=chb, nrows=nrows))
    same(lo["image"], hi["image"], "image and guard rows")
    assert lo["tag"] == hi["tag"] == form


# ------------------------------------------------------------------------------------------------ transformer-block chain
def chain_case(M, C, inner, n_qkv, seed):
    att = rnd(M, inner, seed=seed + 1)
    x = rnd(M, C, seed=seed + 2) * 2 + 0.3
    w_out, b_out = rnd(C, inner, seed=seed + 3, scale=inner ** -0.5), rnd(C, seed=seed + 4)
    w1, b1 = rnd(4 * C, C, seed=seed + 5, scale=C ** -0.5), rnd(4 * C, seed=seed + 6)
    p0 = torch.exp(rnd(4 * C, seed=seed + 7, scale=0.2))
    p1 = 1.0 / (torch.exp(rnd(4 * C, seed=seed + 8, scale=0.2)) + 1e-9)
    w2, b2 = rnd(C, 4 * C, seed=seed + 9, scale=(4 * C) ** -0.5), rnd(C, seed=seed + 10)
    w_qkv = rnd(n_qkv, C, seed=seed + 11, scale=C ** -0.5) if n_qkv else None
    b_qkv = rnd(n_qkv, seed=seed + 12) if n_qkv else None
    return [att.to(DEV), x.to(DEV), w_out, b_out, w1, b1, p0, p1, w2, b2], dict(w_qkv=w_qkv, b_qkv=b_qkv)


@pytest.mark.parametrize("form", ["qkv", "x_out_masked", "pair"])
def test_chain_images(hip, monkeypatch, form):
    """C = 128, 32-row workgroups over 40 rows (one full tile + 8 rows): the lane-paired q|k|v stores, the last block's x_out with
    its row mask, and the pair form"""
    M, C = 40, 128
    n_qkv = 0 if form == "x_out_masked" else 384
    pos, kw = chain_case(M, C, 128, n_qkv, seed=300)
    if form == "x_out_masked":
        kw["out_mask"] = (torch.arange(M) % 5 != 3).float().to(DEV)
    kw.update(qb=32, ch=128, pair=form == "pair")
    lo, hi = both(monkeypatch, lambda: hip.tblock_chain(*pos, **kw))
    same(lo[0], hi[0], "x_out")
    assert lo[0].abs().max().item() > 0.1
    if n_qkv:
        same(lo[1], hi[1], "q|k|v")
        assert lo[1].abs().max().item() > 0.1
    # the raw images with their guard rows
    lo, hi = both(monkeypatch, lambda: hip.tblock_chain_args(*pos, **kw))
    same(lo["x_out_image"], hi["x_out_image"], "x_out image and guard rows")
    if n_qkv:
        same(lo["qkv_image"], hi["qkv_image"], "q|k|v image and guard rows")
    assert lo["tag"] == hi["tag"] and int(lo["flag"].abs().sum()) == 0 and int(hi["flag"].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("B,T,form", [(2, 70, "192>"), (1, 161, "192>"), (2, 200, "64>")])
def test_attention_image(hip, monkeypatch, B, T, form):
    """H = 2, D = 64.  T = 70 and T = 161: the whole-sequence form the launcher takes for 65..192 keys (one workgroup per utterance
    and head, its last wave partly or wholly past the end); T = 200: the tiled form, 64-query blocks, the last one 8 rows deep"""
    H = 2
    p16 = sub("_hip").to_p16_roundtrip
    qkv = rnd(B * T, 3 * H * 64, seed=200 + T)
    qkv[:, 2 * H * 64:] = qkv[:, 2 * H * 64:] * 1.5 + 0.4
    qkv = p16(qkv.to(DEV), lscale=1.0)["out"]
    lens = torch.tensor([T - 13 * i for i in range(B)])
    mask = (torch.arange(T)[None] < lens[:, None]).float().reshape(-1).to(DEV)
    for lscale in (2048.0, 1.0):
        lo, hi = both(monkeypatch, lambda: hip.attention_p16_run(qkv, mask, B, T, H, 64, 0.125, 0, out_lscale=lscale))
        same(lo["out"], hi["out"], f"rows (lscale {lscale})")
        assert lo["tag"] == hi["tag"] and lo["tag"].endswith(form), (lo["tag"], hi["tag"])
        assert lo["flag"] == hi["flag"] == 0 and lo["out"].abs().max().item() > 0.1


# ------------------------------------------------------------------------------------------------ producer -> consumer across launches
@pytest.mark.parametrize("env", [{}, {"MTTS_CHAIN_MIN_ROWS": "0"}, {"MTTS_CHAIN_MIN_ROWS": "0", "MTTS_RESNET_FUSE": "7"}],
                         ids=["default", "chain", "chain+conv_gn"])
def test_model_mel_is_bit_equal(hparams, synthetic, monkeypatch, env):
    """Three ragged utterances (48 / 40 / 29 tokens), euler/2: with the default switches, with the chain launch admitted at these
    row counts, and with the one-launch Block1D admitted as well -- the mel of mask 0 and of all bits is the same, bit for bit, and
    so are two runs of each (the context reads the switch when it is created)."""
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    inf = sub("inference")
    hp = hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7)
    x, x_len, spk = synthetic.make_inputs(hp, 3, 48, seed=99, lengths=[48, 40, 29])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mels = {}
    for mask in ("0", ALL_BITS):
        monkeypatch.setenv("MTTS_STORE_WT", mask)
        m = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV).eval()
        m.decoder.solver = "euler"
        runs = [m.synthesise(x.to(DEV), x_len.to(DEV), 2, speaker=spk.to(DEV))["mel"].clone() for _ in range(2)]
        assert torch.equal(runs[0], runs[1]), f"two runs differ under MTTS_STORE_WT={mask}"
        mels[mask] = runs[0]
    assert torch.isfinite(mels["0"]).all()
    same(mels["0"], mels[ALL_BITS], "mel")

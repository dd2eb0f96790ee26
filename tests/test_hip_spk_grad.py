"""Speaker-row gradients on the GPU: the two backward kernels against fp64 autograd of the oracle's pieces, the taped forward bit for
bit against the forward entries, the whole gradient against fp64 autograd (tests/spk_grad_restated.py), batch independence, a refused
utterance, the fine-tune loop and the command-line tool.

Bounds.
  * Unit kernels: fp64_bound(r, n) = 2 (r + log2(n / r) + 4) 2^-24 of tests/test_hip_score.py, r = the kernel's serial run (LayerNorm
    backward: ceil(C / 64) channels per lane then a butterfly; attention backward: one thread walks all len keys / queries), applied to
    the sum of the ABSOLUTE values of the terms it adds (the terms change sign here), times the count of fp32-rounded factors per term.
  * Whole gradient: err = max over rows of max|g - g64| / max|g64|.  The unit is err32, the same quantity for the oracle's float32 CPU
    autograd against fp64; the device must stay within 8 x err32 (4 for the 22-bit operands of the forward's split arithmetic against
    fp32's 24 bits, 2 for a different summation order).  Nothing here is taken from what the device returns.
Every figure is printed (and appended to $MTTS_SPK_GRAD_REPORT: the source of profiles/r11_spk_grad.md) before it is asserted.

Section 4b repeats the taped-forward, whole-gradient and batch-independence checks, bounds unchanged, beyond one tile (1044 rows,
Tx = 1024), under MTTS_P16=0 / MTTS_GEMM_TERMS=0 / 6, on the filter-80 encoder and through the range guard's rerun; the attention
backward runs at every head dim it dispatches.  The seed, gate and token-sum kernels have tests/test_hip_kernels_grad.py
(profiles/r32_grad_parity.md)."""
import dataclasses
import importlib.util
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import enroll_restated as E
import mas_restated as R
import score_restated as S
import spk_grad_restated as G

pytestmark = pytest.mark.gpu

DELTA_PRIOR, DELTA_DUR = 0.15, 0.3
REPORT = os.environ.get("MTTS_SPK_GRAD_REPORT")


def note(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


def make_model(hp, sd, dev):
    m = sub("inference").MatchaTTSInfer(**hp.as_reference_kwargs())
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def grad_hparams(hparams, size, n_spks=3):
    hp = hparams.tiny(n_spks=n_spks) if size == "tiny" else hparams.prod_v20(n_spks=n_spks)
    return dataclasses.replace(hp, prior_loss_threshold=DELTA_PRIOR, duration_loss_threshold=DELTA_DUR)


@pytest.fixture(scope="module", params=["tiny", "prod"])
def env(request, hparams, synthetic, dev):
    hp = grad_hparams(hparams, request.param)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)     # a duration projection that is not zero: logw depends on e_dur
    return request.param, hp, sd, make_model(hp, sd, dev)


def fp64_bound(r, n):
    return 2 * (r + math.log2(max(n / r, 1.0)) + 4) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1. unit kernels
@pytest.mark.parametrize("variant", ["plain", "silu", "film", "masked"])
@pytest.mark.parametrize("C", [288, 96, 32])
def test_layernorm_backward_against_fp64(oracle, dev, variant, C):
    hip = sub("_hip")
    B, T = 3, 37
    g = torch.Generator().manual_seed(C + len(variant))
    x0 = torch.randn(B, C, T, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B, C, T, generator=g)
    film = torch.cat([1 + 0.3 * torch.randn(B, C, generator=g), 0.3 * torch.randn(B, C, generator=g)], 1)
    mask = S.sequence_mask([37, 20, 1], T)[:, None, :].float()
    relu = variant == "film"                                # the duration predictor's order: conv -> ReLU -> LayerNorm -> FiLM
    # fp64 autograd of the oracle's channel_layer_norm and what follows it at each call site
    x64 = x0.double().requires_grad_(True)
    f64 = film.double().requires_grad_(True)
    xin = torch.relu(x64) if relu else x64
    y = oracle.channel_layer_norm(xin, gamma.double(), beta.double())
    if variant == "silu":
        y = torch.nn.functional.silu(y)
    if variant == "film":
        y = y * f64[:, :C, None] + f64[:, C:, None]
    if variant == "masked":
        y = y * mask.double()
    grads = torch.autograd.grad((y * dy.double()).sum(), [x64, f64], allow_unused=True)
    want = grads[0].transpose(1, 2).reshape(B * T, C)
    rows = lambda t: t.transpose(1, 2).reshape(B * T, -1).contiguous().to(dev)
    xk = torch.relu(x0) if relu else x0
    dx, dfilm = hip.channel_layernorm_bwd(rows(xk), rows(dy), gamma.to(dev), beta.to(dev), B, T, act=2 if variant == "silu" else 0,
                                          film=film.to(dev) if variant == "film" else None,
                                          mask=mask.reshape(-1).to(dev) if variant == "masked" else None, gate=1 if relu else 0)
    # per-row magnitude of what the kernel adds and subtracts: dx = rstd (g - mean(g) - xh mean(g xh)), g = d loss / d xh
    xin_d = xin.detach()
    mean = xin_d.mean(1, keepdim=True)
    rstd = torch.rsqrt(((xin_d - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (xin_d - mean) * rstd
    a = xh * gamma.double().view(1, -1, 1) + beta.double().view(1, -1, 1)
    gxh = dy.double() * gamma.double().view(1, -1, 1)
    if variant == "silu":
        sg = torch.sigmoid(a)
        gxh = gxh * sg * (1 + a * (1 - sg))
    if variant == "film":
        gxh = gxh * film.double()[:, :C, None]
    scale = (rstd * (gxh.abs().amax(1, keepdim=True) + gxh.abs().mean(1, keepdim=True) + xh.abs().amax(1, keepdim=True) * (gxh * xh).abs().mean(1, keepdim=True)))
    scale = scale.transpose(1, 2).reshape(B * T)
    r = math.ceil(C / 64)
    tol = 4 * fp64_bound(r, C)        # 4 fp32-rounded factors per term: xh, g with its affine / SiLU' / FiLM factor, the two means
    err = ((dx.cpu().double() - want).abs().amax(1) / scale).max().item()
    note(f"layernorm bwd {variant} C={C}: max err / row scale {err:.2e} (bound {tol:.2e})")
    assert tol <= 1e-5 and err <= tol
    if variant == "masked":
        assert (dx.cpu().view(B, T, C)[1, 20:] == 0).all() and (dx.cpu().view(B, T, C)[2, 1:] == 0).all()
    if variant == "film":
        want_f = grads[1]
        terms = torch.cat([(dy.double() * a).abs().sum(2), dy.double().abs().sum(2)], 1)       # sum of |terms| over the T rows
        rt = math.ceil(T / 4)
        errf = ((dfilm.cpu().double() - want_f).abs() / terms).max().item()
        tolf = 2 * fp64_bound(rt, T)
        note(f"layernorm bwd film C={C}: d film max err / sum|terms| {errf:.2e} (bound {tolf:.2e})")
        assert errf <= tolf


ATT_CASES = {"ragged_prod_heads": (6, 48, [70, 33, 1, 128, 5], 128), "tiny_heads": (2, 24, [19, 1, 8], 19), "tx1024": (2, 48, [1024, 513], 1024)}
# every head dim launch_attn_bwd dispatches, at the smallest T that crosses the 128-row workgroup: two workgroups per head, the second
# with one live row (utterance 0) or none
ATT_CASES.update({f"head_dim_{D}": (2, D, [129, 70, 33, 1], 129) for D in (8, 16, 24, 32, 40, 48, 56, 64)})


@pytest.mark.parametrize("case", list(ATT_CASES))
def test_rope_attention_backward_against_fp64(oracle, dev, case):
    hip = sub("_hip")
    H, D, lens, T = ATT_CASES[case]
    B = len(lens)
    g = torch.Generator().manual_seed(len(case))
    scale = 1.0 / math.sqrt(D)
    d_rope = D // 2
    q0, k0, v0 = (torch.randn(B, H, T, D, generator=g) for _ in range(3))
    do = torch.randn(B, H, T, D, generator=g)
    valid = S.sequence_mask(lens, T)
    do = do * valid[:, None, :, None]                       # padded queries receive zero upstream gradient
    # the saved rows: q, k after the rotation, rounded to fp32 -- the fp64 reference starts from exactly these values
    qr = oracle.apply_rope(q0.double(), d_rope).float().double().requires_grad_(True)
    kr = oracle.apply_rope(k0.double(), d_rope).float().double().requires_grad_(True)
    v = v0.double().requires_grad_(True)
    amask = (valid[:, None, :, None] & valid[:, None, None, :])
    o = oracle.sdpa_reference(qr, kr, v, amask, scale)
    dqr, dkr, dv = torch.autograd.grad((o * do.double()).sum(), [qr, kr, v])

    def unrope(gr):                                         # the transposed rotation, by autograd of the oracle's apply_rope
        z = torch.zeros_like(gr, requires_grad=True)
        return torch.autograd.grad(oracle.apply_rope(z, d_rope), z, grad_outputs=gr)[0]

    want = [unrope(dqr), unrope(dkr), dv]
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * T, H * D)
    qkv = torch.cat([rows(qr.detach()), rows(kr.detach()), rows(v.detach())], 1).float().contiguous().to(dev)
    cos, sin = sub("_hip").rope_tables(d_rope, T)
    got = hip.attention_rope_bwd(qkv, rows(o.detach()).float().contiguous().to(dev), rows(do).contiguous().to(dev), torch.tensor(lens), B, T, H, D,
                                 scale, cos.to(dev).contiguous(), sin.to(dev).contiguous()).cpu().double()
    got = [got[:, i * H * D:(i + 1) * H * D].reshape(B, T, H, D).permute(0, 2, 1, 3) for i in range(3)]
    # magnitudes of what each thread adds up, in absolute values
    with torch.no_grad():
        s = torch.matmul(qr, kr.transpose(-1, -2)) * scale
        p = torch.softmax(s.masked_fill(~amask, float("-inf")), -1).nan_to_num(0.0)
        dp = torch.matmul(do.double().abs(), v.abs().transpose(-1, -2))
        delta = (do.double() * o).abs().sum(-1, keepdim=True)
        ds_abs = p * (dp + delta) * scale
        mag = [torch.matmul(ds_abs, kr.abs()), torch.matmul(ds_abs.transpose(-1, -2), qr.abs()), torch.matmul(p.transpose(-1, -2), do.double().abs())]
    for b, n in enumerate(lens):
        tol = 2 * (fp64_bound(n, n) + 3 * fp64_bound(D, D))       # the serial run over n keys / queries + three D-long dot products, x 2 rounded factors
        for name, gt, wt, mg, rot in zip("qkv", got, want, mag, (1.5, 1.5, 1.0)):
            row_scale = rot * mg[b, :, :n].amax(-1)          # (|cos| + |sin| <= 1.5 of the transposed rotation)
            err = ((gt[b, :, :n] - wt[b, :, :n]).abs().amax(-1) / row_scale).max().item()
            note(f"attention bwd {case} b={b} len={n}: d{name} max err / row scale {err:.2e} (bound {tol:.2e})")
            assert err <= tol, (case, b, name)
            assert (gt[b, :, n:] == 0).all(), (case, b, name)        # nothing beyond the utterance
    assert fp64_bound(1024, 1024) < 2e-4


# ------------------------------------------------------------------------------------------------ recordings
def planted_case(synthetic, oracle, sd, hp, lengths, seed, sigma=DELTA_PRIOR, voice=None):
    """The recipe of tests/test_hip_score.py ``recording``: y_fine = expand(mu_x_oracle, dur) + sigma * noise.  sigma = delta_prior puts
    ~68 % of the prior terms in the quadratic branch; the durations of even tokens follow the predictor (|logw - log(2 + d)| small),
    those of odd tokens are drawn from 2..8, so the duration terms take both branches as well."""
    x, x_len, spk = synthetic.make_inputs(hp, len(lengths), max(lengths), seed=seed, lengths=lengths)
    if voice is not None:
        spk = torch.full_like(spk, voice)
    rng = np.random.default_rng(seed)
    B, Tx = x.shape
    with torch.inference_mode():
        e_enc, e_dur = sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk]
        mu_x, logw, _ = oracle.text_encoder_forward(sd, hp, x, x_len, e_enc, e_dur)
    dur = np.zeros((B, Tx), dtype=np.int64)
    for b in range(B):
        n = int(x_len[b])
        near = np.clip(np.round(np.exp(logw[b, 0, :n].numpy().astype(np.float64)) - 2), 1, 12).astype(np.int64)
        far = rng.integers(2, 9, size=n)
        dur[b, :n] = np.where(np.arange(n) % 2 == 0, near, far)
    fine_len = dur.sum(1)
    T = oracle.fix_len_compatibility(int(((fine_len + 1) // 2).max()))
    y_fine = torch.zeros(B, hp.n_feats, 2 * T)
    for b in range(B):
        n = int(x_len[b])
        y_fine[b, :, :fine_len[b]] = torch.from_numpy(R.expand(mu_x[b, :, :n].numpy(), dur[b, :n]) +
                                                      (sigma * rng.standard_normal((hp.n_feats, fine_len[b]))).astype(np.float32))
    return {"x": x, "x_len": x_len, "spk": spk, "e_enc": e_enc, "e_dur": e_dur, "dur": torch.from_numpy(dur), "y_fine": y_fine,
            "y_fine_len": torch.from_numpy(fine_len), "mu_x": mu_x, "logw": logw}


def device_grad(model, c, dev, durations="given", rows=None, **kw):
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    x, x_len = sel(c["x"]), sel(c["x_len"])
    n = int(x_len.max()) if rows is not None else x.shape[1]
    fine = int(sel(c["y_fine_len"]).max()) if rows is not None else c["y_fine"].shape[2]
    dur = sel(c["dur"])[:, :n].contiguous().to(dev) if durations == "given" else None
    return model.hip.speaker_grad(x[:, :n].contiguous().to(dev), x_len.to(dev), sel(c["e_enc"]).to(dev), sel(c["e_dur"]).to(dev),
                                  sel(c["y_fine"])[:, :, :max(fine, n)].contiguous().to(dev), sel(c["y_fine_len"]).to(dev), DELTA_PRIOR, DELTA_DUR,
                                  durations=dur, **kw)


LENGTHS = [14, 9, 12, 5, 1, 11]


# ------------------------------------------------------------------------------------------------ 2. taped forward
def test_taped_forward_is_the_forward_bit_for_bit(env, synthetic, oracle, dev):
    size, hp, sd, model = env
    check_taped_forward(model, planted_case(synthetic, oracle, sd, hp, LENGTHS, seed=321), dev)


def check_taped_forward(model, c, dev):
    hip = model.hip
    x, x_len = c["x"].to(dev), c["x_len"].to(dev)
    mu_x, logw, x_mask = hip.text_encoder(x, x_len, c["e_enc"].to(dev), c["e_dur"].to(dev))
    out = device_grad(model, c, dev, durations=None, return_tape=True)
    for name, want in (("mu_x", mu_x), ("logw", logw), ("x_mask", x_mask)):
        assert torch.equal(out[name], want), name
    y, yl = c["y_fine"].to(dev), c["y_fine_len"].to(dev)
    dur, _, _ = hip.mas(x_len, yl, mu_x=mu_x, y=y)
    assert torch.equal(out["durations"], dur)
    prior, dsum, _, _ = hip.score_prior_dur(mu_x, logw, dur, y, x_len, yl, DELTA_PRIOR, DELTA_DUR)
    assert torch.equal(out["prior_sum"], prior) and torch.equal(out["dur_sum"], dsum)
    given = device_grad(model, c, dev)
    prior, dsum, _, _ = hip.score_prior_dur(mu_x, logw, c["dur"].to(dev), y, x_len, yl, DELTA_PRIOR, DELTA_DUR)
    assert torch.equal(given["prior_sum"], prior) and torch.equal(given["dur_sum"], dsum)
    assert torch.equal(given["durations"].cpu().long(), c["dur"])


# ------------------------------------------------------------------------------------------------ 3. the whole gradient
def test_gradient_against_fp64_autograd(env, synthetic, oracle, dev):
    size, hp, sd, model = env
    c = planted_case(synthetic, oracle, sd, hp, LENGTHS, seed=321)
    check_gradient(size, model, oracle, sd, hp, c, device_grad(model, c, dev))


def yardsticks(oracle, sd, hp, c, dur, band=False):
    """(fp64 gradient, float32 CPU gradient) of a case with the durations held constant.  ``band``: a third entry, None or the fp64
    g_enc with ONE ReLU gate per utterance switched -- that of the FFN pre-activation nearest zero, where it lies within 8 x the
    float32 CPU twin's own forward error of zero (spk_grad_restated.relu_band).  The loss is not differentiable there: a forward
    pass that is accurate to fp32 may land on either side, and each side's gate is the exact derivative of what that pass computed.
    (prod, short case: one pre-activation of utterance 2 is -3.1e-7 in fp64 and the twin's error there 1.7e-6; with its gate on,
    g_enc of that row moves by 5.6e-4 of its largest entry, 21 x err32.  Found when the MTTS_GEMM_TERMS=6 context took the other
    side: profiles/r32_grad_parity.md.)"""
    args = (oracle, sd, hp, c["x"], c["x_len"], c["e_enc"], c["e_dur"], c["y_fine"], c["y_fine_len"], dur, DELTA_PRIOR, DELTA_DUR)
    if not band:
        return G.speaker_grad(*args), G.speaker_grad(*args, dtype=torch.float32)
    rec64, rec32 = [], []
    ref, cpu32 = G.speaker_grad(*args, record=rec64), G.speaker_grad(*args, dtype=torch.float32, record=rec32)
    units, count = G.relu_band(rec64, rec32, c["x_len"], hp.encoder.n_layers)
    note(f"gradient case: FFN pre-activations within 8 x the float32 twin's error of zero, per utterance {count}; switched {units}")
    other = G.speaker_grad(*args, switched=[(k, i) for k, i, _ in units])["g_enc"] if units else None
    return ref, cpu32, other


def check_gradient(size, model, oracle, sd, hp, c, got, dur=None, refs=None):
    """``got``: what the device returned for the case; ``dur``: the durations it held constant (None: the planted ones)."""
    dur = c["dur"] if dur is None else dur
    ref, cpu32, *other = refs if refs is not None else yardsticks(oracle, sd, hp, c, dur)
    other = other[0] if other else None
    c = dict(c, dur=dur)
    # the condition on the inputs: both Huber regimes occur, for the prior and for the durations
    m = S.sequence_mask(c["y_fine_len"], c["y_fine"].shape[2])[:, None, :]
    d_prior = (c["y_fine"].double() - torch.matmul(ref["mu_x"], S.path_from_durations(c["dur"], c["y_fine"].shape[2]).double()))[m.expand(-1, hp.n_feats, -1)]
    xm = S.sequence_mask(c["x_len"], c["x"].shape[1])
    d_dur = (ref["logw"][:, 0] - torch.log(2 + c["dur"].double()))[xm]
    fp, fd = float((d_prior.abs() < DELTA_PRIOR).double().mean()), float((d_dur.abs() < DELTA_DUR).double().mean())
    note(f"gradient case {size}: quadratic share prior {fp:.2f}, duration {fd:.2f}")
    assert 0.1 <= fp <= 0.9 and 0.1 <= fd <= 0.9
    def device_error(name):
        rows = G.row_error(got[name], ref[name])
        if name == "g_enc" and other is not None:                # (yardsticks: either side of a ReLU that fp32 cannot tell from zero)
            alt = G.row_error(got[name], other)
            if (alt < rows).any():
                note(f"gradient vs fp64 {size} {name}: rows {(alt < rows).nonzero().flatten().tolist()} match the switched gate: "
                     f"{[f'{a:.3e} against {r:.3e}' for a, r in zip(alt.tolist(), rows.tolist()) if a < r]}")
            rows = torch.minimum(rows, alt)
        return float(rows.max())

    for name in ("g_enc", "g_dur"):
        err32 = float(G.row_error(cpu32[name], ref[name]).max())
        err = device_error(name)
        note(f"gradient vs fp64 {size} {name}: err32 {err32:.3e}, device {err:.3e}, ratio {err / err32:.2f} (bound 8)")
    for name in ("g_enc", "g_dur"):
        err32 = float(G.row_error(cpu32[name], ref[name]).max())
        assert device_error(name) <= 8 * err32, (size, name, device_error(name), err32)


# ------------------------------------------------------------------------------------------------ 4. batch independence
def test_rows_do_not_depend_on_the_batch(env, synthetic, oracle, dev):
    size, hp, sd, model = env
    check_batch_independence(model, planted_case(synthetic, oracle, sd, hp, LENGTHS, seed=77), dev)


def check_batch_independence(model, c, dev):
    whole = device_grad(model, c, dev)
    whole = {k: v.clone() for k, v in whole.items()}
    again = device_grad(model, c, dev)
    for k in ("g_enc", "g_dur", "prior_sum", "dur_sum", "durations"):
        assert torch.equal(whole[k], again[k]), k
    assert whole["g_enc"].abs().max() > 0 and whole["g_dur"].abs().max() > 0
    for b in range(c["x"].shape[0]):
        solo = device_grad(model, c, dev, rows=[b])
        for k in ("g_enc", "g_dur", "prior_sum", "dur_sum"):
            assert torch.equal(solo[k][0], whole[k][b]), (k, b)


# ------------------------------------------------------------------------------------------------ 4b. beyond one tile, in every arithmetic
# The same three checks with the same bounds where the cases above do not reach:
#   long   [261, 130, 1, 64]: 1044 rows = nine 128-row GEMM tiles, conv halos across tile and utterance boundaries, a third
#          attention-backward workgroup that is partly live, tokens beyond 256 in the seed kernels; the solo rows have other padded shapes
#   cap    [1024]: Tx at the admitted maximum (tiny only)
#   arithmetics: MTTS_P16=0, MTTS_GEMM_TERMS=0 and 6 (gate mode 1 and the fp32-row FFN branch of the taped forward, which the default
#          arithmetic never takes on these models), each on a model created under its switches; the fp64 yardstick does not depend on them
#   odd    tests/encoder_cases.py's encoder with filter 80 and duration filter 36: the fp32-row branch under the default arithmetic,
#          widths 80 and 36 in ln_bwd_kernel and the token sums
# CPU figures of the long and cap cases (seed 321, sigma = delta_prior): fp64 yardstick 1.7 s (prod) / 0.3 s (tiny) / 0.1 s (cap);
# quadratic shares prior / duration 0.68 / 0.45 (prod), 0.69 / 0.54 (tiny), 0.68 / 0.50 (cap).
SHAPES = {"short": LENGTHS, "long": [261, 130, 1, 64], "cap": [1024]}
ARITHMETICS = {"default": {}, "p16-off": {"MTTS_P16": "0"}, "terms0": {"MTTS_GEMM_TERMS": "0"}, "terms6": {"MTTS_GEMM_TERMS": "6"}}
CELLS = ([("tiny", "default", "long"), ("prod", "default", "long"), ("tiny", "default", "cap"), ("odd", "default", "short"), ("odd", "default", "long")]
         + [(size, a, shape) for a in ("p16-off", "terms0", "terms6") for size, shape in (("tiny", "short"), ("prod", "short"), ("tiny", "long"))])


class Cells:
    """What the cells share: one model per (size, arithmetic), created under the switches (read at mtts_create only); one planted case
    and one pair of yardsticks per (size, shape, seed, durations held constant), computed once and left unchanged."""

    def __init__(self, hparams, synthetic, oracle, dev):
        self.hparams, self.synthetic, self.oracle, self.dev = hparams, synthetic, oracle, dev
        self._weights, self._models, self._cases, self._refs = {}, {}, {}, {}

    def weights(self, size):
        if size not in self._weights:
            if size == "odd":
                import encoder_cases as ec
                hp = dataclasses.replace(ec.weights("odd")[0], prior_loss_threshold=DELTA_PRIOR, duration_loss_threshold=DELTA_DUR)
            else:
                hp = grad_hparams(self.hparams, size)
            self._weights[size] = hp, self.synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
        return self._weights[size]

    def model(self, monkeypatch, size, arithmetic):
        if (size, arithmetic) not in self._models:
            hp, sd = self.weights(size)
            for k, v in ARITHMETICS[arithmetic].items():
                monkeypatch.setenv(k, v)
            m = make_model(hp, sd, self.dev)
            m.hip                                                # the context is created here, under the switches
            for k in ARITHMETICS[arithmetic]:
                monkeypatch.delenv(k)
            want = {"default": 2, "p16-off": 2, "terms0": 0, "terms6": 6}[arithmetic]
            assert m.hip.gemm_terms() == want
            self._models[size, arithmetic] = m
        return self._models[size, arithmetic]

    def case(self, size, shape, seed):
        if (size, shape, seed) not in self._cases:
            hp, sd = self.weights(size)
            self._cases[size, shape, seed] = planted_case(self.synthetic, self.oracle, sd, hp, SHAPES[shape], seed=seed)
        return self._cases[size, shape, seed]

    def refs(self, size, shape, seed, dur):
        key = size, shape, seed, dur.numpy().tobytes()           # (an arithmetic whose search settles a tie differently gets its own)
        if key not in self._refs:
            hp, sd = self.weights(size)
            self._refs[key] = yardsticks(self.oracle, sd, hp, self.case(size, shape, seed), dur, band=True)
        return self._refs[key]


@pytest.fixture(scope="module")
def cells(hparams, synthetic, oracle, dev):
    return Cells(hparams, synthetic, oracle, dev)


@pytest.mark.parametrize("size,arithmetic,shape", CELLS)
def test_taped_forward_bit_for_bit_beyond_one_tile(cells, monkeypatch, dev, size, arithmetic, shape):
    check_taped_forward(cells.model(monkeypatch, size, arithmetic), cells.case(size, shape, 321), dev)


@pytest.mark.parametrize("durations", ["given", "search"])
@pytest.mark.parametrize("size,arithmetic,shape", CELLS)
def test_gradient_against_fp64_autograd_beyond_one_tile(cells, monkeypatch, dev, size, arithmetic, shape, durations):
    """``search``: the device runs its alignment search; the durations it reports are checked to be an alignment (non-negative, zero
    beyond an utterance, summing to its frames) and are the constants of the yardstick, as they are of the reference's step."""
    model, c = cells.model(monkeypatch, size, arithmetic), cells.case(size, shape, 321)
    hp, sd = cells.weights(size)
    got = device_grad(model, c, dev, durations="given" if durations == "given" else None)
    dur = got["durations"].cpu().long()
    if durations == "given":
        assert torch.equal(dur, c["dur"])
    else:
        live = S.sequence_mask(c["x_len"], c["x"].shape[1])
        assert (dur >= 0).all() and (dur[~live] == 0).all() and torch.equal(dur.sum(1), c["y_fine_len"])
        assert (dur[live] >= 1).all()                            # a monotone path gives every token a frame
    tag = f"{size} {shape} {arithmetic} {durations}"
    check_gradient(tag, model, cells.oracle, sd, hp, c, got, dur=dur, refs=cells.refs(size, shape, 321, dur))


@pytest.mark.parametrize("size,arithmetic,shape", CELLS)
def test_rows_do_not_depend_on_the_batch_beyond_one_tile(cells, monkeypatch, dev, size, arithmetic, shape):
    check_batch_independence(cells.model(monkeypatch, size, arithmetic), cells.case(size, shape, 77), dev)


def test_range_guard_reruns_the_gradient_on_full_range_arithmetic(hparams, synthetic, oracle, dev):
    """``speaker_grad`` under the range policies, on weights that raise the flag in the text encoder: every FFN's first convolution
    times 2^17 and its second divided by 2^17 (exact scalings; ReLU is positively homogeneous, so the network's function -- and the
    fp64 and float32 yardsticks -- are those of the ordinary weights), which puts the hidden rows beyond +-65504.  `raise` raises;
    `rerun` switches the model to the three-term bf16 context, whose taped forward takes the fp32-row FFN branch and whose backward
    takes gate mode 1, and still meets 8 x err32."""
    hp = grad_hparams(hparams, "tiny")
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    for l in range(hp.encoder.n_layers):
        k = f"encoder.encoder.ffn_layers.{l}."
        sd[k + "conv_1.weight"], sd[k + "conv_1.bias"] = sd[k + "conv_1.weight"] * 2.0 ** 17, sd[k + "conv_1.bias"] * 2.0 ** 17
        sd[k + "conv_2.weight"] = sd[k + "conv_2.weight"] / 2.0 ** 17
    model = make_model(hp, sd, dev)
    c = planted_case(synthetic, oracle, sd, hp, LENGTHS, seed=321)
    run = lambda: model.speaker_grad(c["x"].to(dev), c["x_len"].to(dev), mel_fine=c["y_fine"].to(dev), mel_fine_lengths=c["y_fine_len"].to(dev),
                                     speaker_embeddings=(c["e_enc"].to(dev), c["e_dur"].to(dev)), durations=c["dur"].to(dev))
    model.range_policy = "raise"
    with pytest.raises(FloatingPointError):
        run()
    assert model.hip.gemm_terms() == 2
    model.range_policy = "rerun"
    got = run()
    assert model.hip.gemm_terms() == 6                          # the runtime switched to the three-term bf16 context
    check_gradient("tiny short range-guard rerun", model, oracle, sd, hp, c, got)
    again = run()
    assert torch.equal(got["g_enc"], again["g_enc"]) and torch.equal(got["g_dur"], again["g_dur"])


# ------------------------------------------------------------------------------------------------ 5. a bad utterance
def test_a_bad_utterance_gets_zero_rows_and_is_named(env, synthetic, oracle, dev):
    size, hp, sd, model = env
    c = planted_case(synthetic, oracle, sd, hp, LENGTHS, seed=77)
    good = {k: v.clone() for k, v in device_grad(model, c, dev).items()}
    for bad_len, pattern in ((3, "utterance 1 "), (0, "utterance 1 ")):          # fewer frames than tokens (9); no frames at all
        broken = dict(c)
        broken["y_fine_len"] = c["y_fine_len"].clone()
        broken["y_fine_len"][1] = bad_len
        out = device_grad(model, broken, dev, check_lengths=False)
        with pytest.raises(ValueError, match=pattern):
            model.hip.spk_grad_status()
        for k in ("g_enc", "g_dur", "prior_sum", "dur_sum"):
            assert (out[k][1] == 0).all(), k
            keep = [b for b in range(len(LENGTHS)) if b != 1]
            assert torch.equal(out[k][keep], good[k][keep]), k
        with pytest.raises(ValueError, match=pattern):
            device_grad(model, broken, dev, durations=None)                    # the search refuses it as well: zero durations, same verdict
    device_grad(model, c, dev)                                                  # a clean call afterwards reports nothing


# ------------------------------------------------------------------------------------------------ 6. fine-tuning
# Chosen on the CPU with the fp64 loop alone (tests/spk_grad_restated.py finetune, tiny model, these utterances, recordings of voice 0
# with sigma 0.05, start = voice 1): with lr 2e-2 the sum dur_loss + prior_loss decreases at every one of N = 12 steps; the test
# asserts that again before it looks at the device.
FT = dict(lengths=[16, 11, 13], seed=500, sigma=0.05, steps=12, track=4, lr=2e-2)


def test_finetuning_lowers_the_loss_and_tracks_the_fp64_loop(hparams, synthetic, oracle, dev):
    hp = grad_hparams(hparams, "tiny", n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    model = make_model(hp, sd, dev)
    c = planted_case(synthetic, oracle, sd, hp, FT["lengths"], seed=FT["seed"], sigma=FT["sigma"], voice=0)
    start = (sd["speaker_embeddings_enc.weight"][1:2], sd["speaker_embeddings_dur.weight"][1:2])
    trail, hist = G.finetune(oracle, sd, hp, c["x"], c["x_len"], c["y_fine"], c["y_fine_len"], start[0], start[1], steps=FT["steps"], lr=FT["lr"],
                             delta_prior=DELTA_PRIOR, delta_dur=DELTA_DUR)
    total = [d + p for d, p in hist]
    assert all(b < a for a, b in zip(total, total[1:])), total              # the yardstick's own condition
    x, x_len, y, yl = c["x"].to(dev), c["x_len"].to(dev), c["y_fine"].to(dev), c["y_fine_len"].to(dev)
    kw = dict(mel_fine=y, mel_fine_lengths=yl, lr=FT["lr"])
    # the first K steps' rows against the fp64 loop: the bound of the whole-gradient test (8 x err32, err32 of this case at the start rows)
    # times the step count, in units of the step.  Adam's update lr * m^ / (sqrt(v^) + eps) does not depend on the gradient's scale and
    # moves a coordinate by about lr (exactly lr * sign(g) at step 1), so a relative gradient error e moves a row by at most about lr * e
    # per step: tol = k * lr * 8 * err32.  The device keeps the rows in fp32 and the yardstick in fp64: each step's row is rounded once,
    # half an ulp of the row's largest entry, which is the second term.
    ref = G.speaker_grad(oracle, sd, hp, c["x"], c["x_len"], start[0], start[1], c["y_fine"], c["y_fine_len"], c["dur"], DELTA_PRIOR, DELTA_DUR)
    c32 = G.speaker_grad(oracle, sd, hp, c["x"], c["x_len"], start[0], start[1], c["y_fine"], c["y_fine_len"], c["dur"], DELTA_PRIOR, DELTA_DUR,
                         dtype=torch.float32)
    for k in range(1, FT["track"] + 1):
        e_enc, e_dur, h = model.finetune_speaker(x, x_len, speaker_embeddings=start, steps=k, **kw)
        for name, got, want, gname in (("e_enc", e_enc, trail[k][0], "g_enc"), ("e_dur", e_dur, trail[k][1], "g_dur")):
            tol = k * FT["lr"] * 8 * float(G.row_error(c32[gname], ref[gname]).max()) + k * 2.0 ** -24 * float(want.abs().max())
            err = float((got.cpu().double() - want).abs().max())
            note(f"finetune step {k} {name}: |row - fp64 loop| {err:.3e} (bound {tol:.3e})")
            assert err <= tol, (k, name)
        assert len(h["dur_loss"]) == k
    e_enc, e_dur, h = model.finetune_speaker(x, x_len, speaker_embeddings=start, steps=FT["steps"], **kw)
    assert e_enc.shape == (1, hp.spk_emb_dim) and e_dur.shape == (1, hp.spk_emb_dim) and len(h["prior_loss"]) == FT["steps"]
    # the loss by model.score on the resulting rows, not from the loop's history
    coarse = oracle.downsample(c["y_fine"])
    coarse_len = (c["y_fine_len"] + 1) // 2
    B = len(FT["lengths"])
    noise = torch.zeros(B, hp.n_feats, coarse.shape[2])

    def loss(rows):
        out = model.score(x, x_len, mel=coarse.to(dev), mel_lengths=coarse_len.to(dev), mel_fine=y, mel_fine_lengths=yl,
                          speaker_embeddings=(rows[0].to(dev), rows[1].to(dev)), t=torch.full((B,), 0.5), noise=noise.to(dev))
        return float(out["dur_loss"]) + float(out["prior_loss"])

    before, after = loss(start), loss((e_enc, e_dur))
    note(f"finetune {FT['steps']} steps: dur + prior loss by model.score {before:.5f} -> {after:.5f} (fp64 loop {total[0]:.5f} -> {total[-1]:.5f})")
    assert after < before
    # the start from a table row, batches, and the rows feed synthesise
    e2, d2, h2 = model.finetune_speaker(x, x_len, speaker=1, steps=3, batch_size=2, **kw)
    assert e2.shape == e_enc.shape and len(h2["dur_loss"]) == 3 and not torch.equal(e2.cpu(), start[0])
    out = model.synthesise(x[:1, :16], x_len[:1], 2, speaker_embeddings=(e_enc, e_dur))
    assert torch.isfinite(out["mel"]).all()
    full = model.speaker_grad(x, x_len, mel_fine=y, mel_fine_lengths=yl, speaker=1)
    assert full["g_enc"].shape == (B, hp.spk_emb_dim) and full["dur_loss"].dim() == 0 and full["durations"].dtype == torch.int32
    with pytest.raises(ValueError, match="either"):
        model.speaker_grad(x, x_len)


# ------------------------------------------------------------------------------------------------ 7. the tool
def test_finetune_speaker_tool(tmp_path, monkeypatch, capsys, dev):
    paths = []
    for i, n in enumerate([9000, 7300]):
        clip = E.synthetic_clip(n, 60 + i, "voiced")
        p = tmp_path / f"clip{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(24000)
            w.writeframes((clip.clamp(-1, 1) * 32767).to(torch.int16).numpy().astype("<i2").tobytes())
        paths.append(str(p))
    ids = tmp_path / "ids.txt"
    ids.write_text("5 17 120 33 8 91 4 250 7\n12 400 3 77 58 9\n")
    out = tmp_path / "voice"
    spec = importlib.util.spec_from_file_location("finetune_speaker_tool", ROOT / "tools" / "finetune_speaker.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["finetune_speaker.py", "--synthetic-model", "tiny", "--ids-file", str(ids), "--steps", "5", "--lr", "1e-2",
                                      "--speaker", "1", "--out", str(out), *paths])
    assert tool.main() == 0
    text = capsys.readouterr().out
    assert "dur_loss" in text and "prior_loss" in text
    hparams, synthetic = sub("hparams"), sub("synthetic")
    hp = hparams.tiny(n_spks=2)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    for name, key in (("enc", "speaker_embeddings_enc.weight"), ("dur", "speaker_embeddings_dur.weight")):
        row = np.load(str(out) + f"_{name}.npy")
        assert row.shape == (hp.spk_emb_dim,) and np.isfinite(row).all()
        assert np.abs(row - sd[key][1].numpy()).max() > 1e-4                   # the rows moved

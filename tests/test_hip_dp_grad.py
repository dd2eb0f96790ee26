"""Duration-predictor training on the GPU (csrc/dp_grad.hip): the three new reductions against fp64, bounded and exact; the forward
from the training component; the whole parameter gradient against fp64 autograd from ids, rows and durations; same bits and a refused
utterance; the trainer against the fp64 AdamW loop of the restatement; commit(); the command-line tool.

Bounds -- derived, never tuned; every budget is formed on the inputs before any device call.
  * Unit kernels, per element: fp64_bound(r, n) sum|terms| (tests/test_hip_spk_grad.py), n = B T rows and r = the longest serial chain
    the documented order implies: a phase's chunk_rows / 4 rows, three additions for the phases, chunks - 1 for the chunks
    (dp_grad_restated.serial_run).  A term is a product of fp32 numbers: one more U per rounded product on top.  For the LayerNorm
    reduction the normalised row is itself computed in fp32: with e_C = fp64_bound(ceil(C / 64) + 6, C) for the lane-strided sums and
    the butterfly, |d mean| <= e_C mean|x| and rstd carries e_C / 2 + 4 U relative (the variance is a sum of squares around a mean whose
    shift enters at second order), so |d xhat| <= rstd |d mean| + |xhat| (e_C / 2 + 5 U), weighted by |dy gf| and summed.
    At the largest shape (4097 rows, chunks of 512: r = 128 + 3 + 8 = 139) fp64_bound is 1.76e-5 of sum|terms| = 4097 E|term|, i.e.
    0.07 of ONE typical term: these cases do see a dropped, doubled or mis-masked row.
  * Exact cases: small-integer operands whose sums of absolute terms stay below 2^24 (checked on the inputs first): fp32 has nothing to
    round in any order, the device must equal fp64 with torch.equal.
  * Forward: logw of the predictor in the training component within 8 x the fp32 CPU twin's error against fp64 (the project's rule for
    non-exact operations: 4 for the 22-bit operands of the frozen part's split arithmetic, 2 for a different summation order).
  * Whole gradient, per tensor: max|g - g64| / max|g64| <= 8 max(err32, e_fwd) as tests/test_hip_style_grad.py defines it: err32 the
    same quantity for float32 CPU autograd, e_fwd the relative error of the device's frozen encoder rows against fp64.  A predictor
    ReLU whose pre-activation fp32 cannot tell from zero (spk_grad_restated.relu_band) may take either side: the better of the two
    yardsticks counts.
  * Trainer: see test_training_lowers_the_loss_and_tracks_the_fp64_loop.
Every figure is printed (and appended to $MTTS_DP_GRAD_REPORT) before it is asserted."""
import dataclasses
import importlib.util
import os
import sys
import wave

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import dp_grad_restated as R
import enroll_restated as E
import spk_grad_restated as G
import style_grad_restated as SR

pytestmark = pytest.mark.gpu

DELTA = 0.3
REPORT = os.environ.get("MTTS_DP_GRAD_REPORT")
SENT = 7.75e33           # sentinel: what no kernel of this file writes
GUARD = 64               # floats behind every output
U = 2.0 ** -24


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


@pytest.fixture(scope="module")
def hip(dev):
    h = sub("_hip")
    h.load()
    return h


def out_buf(n, dev):
    return torch.full((n + GUARD,), SENT, device=dev)


def whole(name, buf, n):
    assert (buf[n:] == SENT).all(), f"{name}: written past the end"
    assert not (buf[:n] == SENT).any() and torch.isfinite(buf[:n]).all(), f"{name}: an element was not written"
    return buf[:n].cpu()


# ------------------------------------------------------------------------------------------------ 1. unit kernels
#         (B, T)      lengths
UNIT = [((1, 1), [1]),                                   # a single row
        ((1, 255), [255]),                               # one row short of a chunk
        ((1, 256), [256]),                               # exactly one chunk
        ((2, 129), [129, 128]),                          # a chunk boundary inside an utterance
        ((4, 1024), [1024, 0, 1, 700]),
        ((17, 241), [241, 0, 1, 240, 100, 241, 7, 64, 241, 200, 3, 241, 128, 0, 55, 241, 241])]   # 4097 rows: chunks of 512 rows
UNIT_IDS = [f"{b}x{t}" for (b, t), _ in UNIT]


def run_ln_film(hip, dev, x, dy, film, lengths):
    lib = hip.load()
    B, T, C = x.shape
    need = lib.mtts_dp_unit_workspace_bytes(B, T, C)
    assert need == 4 * R.chunks_of(B * T) * 2 * C
    dg, db, ws = out_buf(C, dev), out_buf(C, dev), out_buf(need // 4, dev)
    d_x, d_dy, d_f = x.to(dev).contiguous(), dy.to(dev).contiguous(), film.to(dev).contiguous()
    d_len = torch.tensor(lengths, dtype=torch.long, device=dev)
    hip.check(lib.mtts_ln_film_wgrad(hip.ptr(d_x), hip.ptr(d_dy), hip.ptr(d_f), hip.ptr(d_len), B, T, C, R.EPS, hip.ptr(dg), hip.ptr(db),
                                     ws.data_ptr(), need, hip.stream_ptr()))
    torch.cuda.synchronize()
    return whole("d gamma", dg, C), whole("d beta", db, C), whole("partials", ws, need // 4)


def run_rows(hip, dev, seed, h, lengths):
    lib = hip.load()
    B, T, C = h.shape
    need = lib.mtts_dp_unit_workspace_bytes(B, T, C)
    dw, db, ws = out_buf(C, dev), out_buf(1, dev), out_buf(need // 4, dev)
    d_s, d_h = seed.to(dev).contiguous(), h.to(dev).contiguous()
    d_len = torch.tensor(lengths, dtype=torch.long, device=dev)
    hip.check(lib.mtts_rows_wgrad(hip.ptr(d_s), hip.ptr(d_h), hip.ptr(d_len), B, T, C, hip.ptr(dw), hip.ptr(db), ws.data_ptr(), need,
                                  hip.stream_ptr()))
    torch.cuda.synchronize()
    assert (ws[need // 4:] == SENT).all(), "partials: written past the end"
    return whole("dw", dw, C), whole("db", db, 1)


def poison(t, lengths):
    """NaN wherever nothing may be read as data: rows at or beyond an utterance's length."""
    for b, n in enumerate(lengths):
        t[b, n:] = float("nan")
    return t


@pytest.mark.parametrize("C", [32, 96, 100])
@pytest.mark.parametrize("shape,lengths", UNIT, ids=UNIT_IDS)
def test_ln_film_wgrad_against_fp64(hip, dev, shape, lengths, C):
    B, T = shape
    g = torch.Generator().manual_seed(1000 * C + B * T)
    x, dy = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    film = torch.cat([1 + 0.3 * torch.randn(B, C, generator=g), 0.3 * torch.randn(B, C, generator=g)], 1)
    # the budget, on the inputs
    want_g, want_b, mag_g, mag_b = R.ln_film_wgrad(x, dy, film, lengths)
    live = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None])[:, :, None]
    xd = torch.where(live, x.double(), torch.zeros((), dtype=torch.float64))
    mu = xd.mean(2, keepdim=True)
    rs = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(2, keepdim=True) + R.EPS)
    xh = (xd - mu) * rs
    gabs = torch.where(live, (dy.double() * film.double()[:, None, :C]).abs(), torch.zeros((), dtype=torch.float64))
    e_c = R.fp64_bound(-(-C // 64) + 6, C)
    d_xh = rs * e_c * xd.abs().mean(2, keepdim=True) + xh.abs() * (e_c / 2 + 5 * U)
    e_sum = R.fp64_bound(R.serial_run(B * T), B * T)
    bound_g = (e_sum + 2 * U) * mag_g + (gabs * d_xh).sum((0, 1))
    bound_b = (e_sum + U) * mag_b
    got_g, got_b, _ = run_ln_film(hip, dev, poison(x.clone(), lengths), poison(dy.clone(), lengths), film, lengths)
    err_g, err_b = (got_g.double() - want_g).abs(), (got_b.double() - want_b).abs()
    tiny = 1e-300
    note(f"ln_film_wgrad {B}x{T} C={C}: d gamma worst err / bound {(err_g / bound_g.clamp(min=tiny)).max().item():.3f}, d beta "
         f"{(err_b / bound_b.clamp(min=tiny)).max().item():.3f}; bound / typical term {(bound_g / (mag_g / max(sum(lengths), 1)).clamp(min=tiny)).max().item():.3f}")
    assert (err_g <= bound_g).all() and (err_b <= bound_b).all()
    again = run_ln_film(hip, dev, poison(x.clone(), lengths), poison(dy.clone(), lengths), film, lengths)
    assert torch.equal(again[0], got_g) and torch.equal(again[1], got_b)


@pytest.mark.parametrize("C", [32, 96, 100])
@pytest.mark.parametrize("shape,lengths", UNIT, ids=UNIT_IDS)
def test_rows_wgrad_against_fp64(hip, dev, shape, lengths, C):
    B, T = shape
    g = torch.Generator().manual_seed(2000 * C + B * T)
    seed, h = torch.randn(B, T, generator=g), torch.randn(B, T, C, generator=g)
    want_w, want_b, mag_w, mag_b = R.rows_wgrad(seed, h, lengths)
    e_sum = R.fp64_bound(R.serial_run(B * T), B * T)
    bound_w, bound_b = (e_sum + U) * mag_w, e_sum * mag_b
    got_w, got_b = run_rows(hip, dev, poison(seed.clone(), lengths), poison(h.clone(), lengths), lengths)
    err_w, err_b = (got_w.double() - want_w).abs(), (got_b.double() - want_b).abs()
    note(f"rows_wgrad {B}x{T} C={C}: dw worst err / bound {(err_w / bound_w.clamp(min=1e-300)).max().item():.3f}, db "
         f"{(err_b / bound_b.clamp(min=1e-300)).max().item():.3f}")
    assert (err_w <= bound_w).all() and (err_b <= bound_b).all()


@pytest.mark.parametrize("C", [32, 100])
@pytest.mark.parametrize("shape,lengths", UNIT, ids=UNIT_IDS)
def test_rows_wgrad_exact_on_integers(hip, dev, shape, lengths, C):
    B, T = shape
    g = torch.Generator().manual_seed(3000 * C + B * T)
    seed = torch.randint(-3, 4, (B, T), generator=g).float()
    h = torch.randint(-4, 5, (B, T, C), generator=g).float()
    want_w, want_b, mag_w, mag_b = R.rows_wgrad(seed, h, lengths)
    assert R.fp32_is_exact_on(mag_w, mag_b)                                    # the condition on the inputs, before any device call
    got_w, got_b = run_rows(hip, dev, poison(seed.clone(), lengths), poison(h.clone(), lengths), lengths)
    note(f"rows_wgrad integers {B}x{T} C={C}: largest sum of |terms| {mag_w.max().item():.0f}, max|dw - fp64| {(got_w.double() - want_w).abs().max().item():g}")
    assert torch.equal(got_w.double(), want_w) and torch.equal(got_b.double(), want_b)


@pytest.mark.parametrize("B,O,J", [(1, 64, 16), (3, 64, 16), (9, 192, 96), (32, 200, 33)])
def test_outer_batch_sum_exact_on_integers(hip, dev, B, O, J):
    lib = hip.load()
    g = torch.Generator().manual_seed(B * O + J)
    gm, e = torch.randint(-5, 6, (B, O), generator=g).float(), torch.randint(-5, 6, (B, J), generator=g).float()
    assert R.fp32_is_exact_on(torch.einsum("bo,bj->oj", gm.abs().double(), e.abs().double()), gm.abs().sum(0))
    want_w, want_b = R.outer_batch_sum(gm, e)
    dw, db = out_buf(O * J, dev), out_buf(O, dev)
    d_g, d_e = gm.to(dev), e.to(dev)
    hip.check(lib.mtts_outer_batch_sum(hip.ptr(d_g), hip.ptr(d_e), B, O, J, hip.ptr(dw), hip.ptr(db), hip.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(whole("dw", dw, O * J).double().reshape(O, J), want_w) and torch.equal(whole("db", db, O).double(), want_b)


@pytest.mark.parametrize("B,T,lengths", [(3, 40, [40, 17, 1]), (9, 116, [116, 115, 100, 64, 1, 2, 116, 77, 33])])
@pytest.mark.parametrize("Hd,Fd", [(48, 32), (288, 96)])
def test_conv_wgrad_through_the_moved_launcher_exact_at_the_first_layers_shape(hip, dev, B, T, lengths, Hd, Fd):
    """The predictor's first layer: cin = ldx = enc_channels + spk_emb_dim (48 tiny, 288 production), cout = the predictor's filter."""
    lib = hip.load()
    dz, x = SR.integer_wgrad_case(B, T, lengths, Hd, Fd, seed=B * T + Hd)
    x = x[:, :, :Hd].contiguous()                                              # ldx = cin
    sums = SR.wgrad_abs_sums(dz, x, lengths)
    assert SR.fp32_is_exact_on(sums, dz, x), sums
    want_w, _ = SR.conv_wgrad(dz, x, lengths)
    m = SR.prefix_mask(lengths, T)[:, :, None]
    want_b = (torch.nan_to_num(dz.double()) * m).sum((0, 1))
    need = lib.mtts_conv_wgrad_workspace_bytes(B, T, Hd, Fd)
    dw, db, ws = out_buf(Fd * Hd * 5, dev), out_buf(Fd, dev), out_buf(need // 4, dev)
    d_len = torch.tensor(lengths, dtype=torch.long, device=dev)
    d_dz, d_x = dz.to(dev).contiguous(), x.to(dev)
    hip.check(lib.mtts_conv_wgrad(hip.ptr(d_dz), hip.ptr(d_x), hip.ptr(d_len), B, T, Hd, Hd, Fd, hip.ptr(dw), hip.ptr(db),
                                  ws.data_ptr(), need, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(whole("dw", dw, Fd * Hd * 5).double().reshape(Fd, Hd, 5), want_w)
    assert torch.equal(whole("db", db, Fd).double(), want_b)


# ------------------------------------------------------------------------------------------------ models, cases, yardsticks
def make_model(hp, sd, dev):
    m = sub("inference").MatchaTTSInfer(**hp.as_reference_kwargs())
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def grad_hparams(hparams, size, n_spks=3):
    hp = hparams.tiny(n_spks=n_spks) if size == "tiny" else hparams.prod_v20(n_spks=n_spks)
    return dataclasses.replace(hp, duration_loss_threshold=DELTA)


SHAPES = {"short": [40, 17, 1], "cap": [1024, 1000, 513, 1, 300], "rows1044": [116, 115, 100, 64, 1, 2, 116, 77, 33]}
ARITHMETICS = {"default": {}, "p16-off": {"MTTS_P16": "0"}, "terms0": {"MTTS_GEMM_TERMS": "0"}, "terms6": {"MTTS_GEMM_TERMS": "6"}}


class Cells:
    """One model per (size, arithmetic), created under its switches (read at mtts_create only); one case and one set of yardsticks per
    (size, shape), computed once and left unchanged."""

    def __init__(self, hparams, synthetic, oracle, dev):
        self.hparams, self.synthetic, self.oracle, self.dev = hparams, synthetic, oracle, dev
        self._weights, self._models, self._cases = {}, {}, {}

    def weights(self, size):
        if size not in self._weights:
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
            assert m.hip.gemm_terms() == {"default": 2, "p16-off": 2, "terms0": 0, "terms6": 6}[arithmetic]
            self._models[size, arithmetic] = m
        return self._models[size, arithmetic]

    def case(self, size, shape):
        """ids, rows, durations (even tokens follow the predictor, odd ones are drawn from 2..8: both Huber branches) and the
        yardsticks: fp64 autograd, float32 autograd, the predictor's ReLU gates that fp32 cannot tell from zero, and fp64 autograd
        with those gates switched."""
        if (size, shape) in self._cases:
            return self._cases[size, shape]
        hp, sd = self.weights(size)
        lengths = SHAPES[shape]
        x, x_len, spk = self.synthetic.make_inputs(hp, len(lengths), max(lengths), seed=321, lengths=lengths)
        e_enc, e_dur = sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk]
        rng = np.random.default_rng(321)
        sd64, sd32 = G.cast_state_dict(sd, torch.float64), G.cast_state_dict(sd, torch.float32)
        with torch.no_grad():
            h64 = R.encoder_rows(self.oracle, sd64, hp, x, x_len, e_enc.double())
            h32 = R.encoder_rows(self.oracle, sd32, hp, x, x_len, e_enc.float())
            P64, P32 = R.params_of(sd, hp), R.params_of(sd, hp, torch.float32)
            logw = R.forward(P64, hp, h64, x_len, e_dur.double())
        dur = torch.zeros(x.shape, dtype=torch.long)
        for b, n in enumerate(lengths):
            near = np.clip(np.round(np.exp(logw[b, 0, :n].numpy()) - 2), 1, 12).astype(np.int64)
            dur[b, :n] = torch.from_numpy(np.where(np.arange(n) % 2 == 0, near, rng.integers(2, 9, size=n)))
        rec64, rec32 = [], []
        with G.relu_calls(rec64):
            g64, gd64, s64, l64 = R.autograd_grads(self.oracle, P64, hp, h64, x_len, e_dur.double(), dur, DELTA)
        with G.relu_calls(rec32):
            g32, gd32, s32, l32 = R.autograd_grads(self.oracle, P32, hp, h32, x_len, e_dur.float(), dur, DELTA)
        units, count = G.relu_band(rec64, rec32, x_len, hp.encoder.dp_n_layers)
        alt = None
        if units:
            with G.relu_calls(None, [(k, i) for k, i, _ in units]):
                alt = R.autograd_grads(self.oracle, P64, hp, h64, x_len, e_dur.double(), dur, DELTA)[0]
        d = (l64[:, 0] - torch.log(2 + dur.double()))[R.mask_of(x_len, x.shape[1], torch.float64)[:, 0] > 0]
        share = float((d.abs() < DELTA).double().mean())
        note(f"case {size} {shape}: quadratic share {share:.2f}; predictor pre-activations within 8 x the float32 twin's error of zero, per "
             f"utterance {count}; switched {units}")
        assert 0.1 <= share <= 0.9
        c = dict(x=x, x_len=x_len, e_enc=e_enc, e_dur=e_dur, dur=dur, h64=h64, h32=h32, g64=g64, g32=g32, gd64=gd64, gd32=gd32, s64=s64, s32=s32,
                 l64=l64, l32=l32, alt=alt)
        self._cases[size, shape] = c
        return c


@pytest.fixture(scope="module")
def cells(hparams, synthetic, oracle, dev):
    return Cells(hparams, synthetic, oracle, dev)


def device_grad(model, c, dev, params=None, rows=None, **kw):
    hip = model.hip
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    return hip.dp_grad(sel(c["x"]).to(dev), sel(c["x_len"]).to(dev), sel(c["e_enc"]).to(dev), sel(c["e_dur"]).to(dev), sel(c["dur"]).to(dev), DELTA,
                       hip.dp_train_buffer(params), **kw)


def guarded_grad(model, c, dev):
    """One mtts_dp_grad call straight on the library with every output buffer sentinel-filled and guard floats behind it: every
    element is written, nothing beyond."""
    hip_mod, hip = sub("_hip"), model.hip
    B, Tx = c["x"].shape
    Sd, n = hip.hp.spk_emb_dim, hip.dp_param_count()
    x, xl = c["x"].to(dev).contiguous(), c["x_len"].to(dev).contiguous()
    e_enc, e_dur, dur = c["e_enc"].to(dev).contiguous(), c["e_dur"].to(dev).contiguous(), c["dur"].to(dev, torch.int32).contiguous()
    buf = hip.dp_train_buffer(None)
    need = hip_mod.size(hip.lib.mtts_dp_grad_workspace_bytes(hip.ctx, B, Tx))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sizes = {"grad": n, "g_dur": B * Sd, "dur_sum": B, "logw": B * Tx}
    bufs = {k: out_buf(v, dev) for k, v in sizes.items()}
    hip_mod.check(hip.lib.mtts_dp_grad(hip.ctx, hip_mod.ptr(x), hip_mod.ptr(xl), hip_mod.ptr(e_enc), hip_mod.ptr(e_dur), hip_mod.ptr(dur), DELTA, B, Tx,
                                       buf.data_ptr(), hip_mod.ptr(bufs["grad"]), hip_mod.ptr(bufs["g_dur"]), hip_mod.ptr(bufs["dur_sum"]),
                                       hip_mod.ptr(bufs["logw"]), ws.data_ptr(), need, hip_mod.stream_ptr()))
    torch.cuda.synchronize()
    return {k: whole(k, bufs[k], v) for k, v in sizes.items()}


def rel(a, b):
    return (a.double().cpu() - b).abs().max().item() / b.abs().max().item()


# ------------------------------------------------------------------------------------------------ 2. the forward
@pytest.mark.parametrize("size", ["tiny", "prod"])
def test_forward_from_the_training_component(cells, monkeypatch, dev, size):
    model, c = cells.model(monkeypatch, size, "default"), cells.case(size, "short")
    out = device_grad(model, c, dev)
    err32, err = rel(c["l32"], c["l64"]), rel(out["logw"], c["l64"])
    note(f"forward {size}: logw err {err:.3e}, err32 {err32:.3e} (bound 8 x)")
    assert err <= 8 * err32
    s32, s = rel(c["s32"], c["s64"]), rel(out["dur_sum"], c["s64"])
    note(f"forward {size}: dur_sum err {s:.3e}, err32 {s32:.3e} (bound 8 x)")
    assert s <= 8 * s32
    lens = c["x_len"].tolist()
    assert all((out["logw"][b, 0, n:] == 0).all() for b, n in enumerate(lens))          # masked beyond an utterance


@pytest.mark.parametrize("size,arithmetic", [("tiny", "default"), ("prod", "default"), ("tiny", "p16-off"), ("tiny", "terms6")])
def test_frozen_rows_are_the_forward_bit_for_bit(cells, monkeypatch, dev, size, arithmetic):
    """In every arithmetic, the default one with its fp16 FFN images included: one mtts_spk_grad call whose taped forward gives mu_x and
    logw equal to mtts_text_encoder_forward's bits (so its encoder rows are that forward's) also exposes those rows
    (mtts_spk_grad_rows_offset), and mtts_dp_grad's frozen rows must equal them bit for bit -- in its own workspace layout, and again
    in the layout of a batch of two."""
    model, c = cells.model(monkeypatch, size, arithmetic), cells.case(size, "short")
    hp, _ = cells.weights(size)
    hip = model.hip
    x, x_len, rows = c["x"].to(dev), c["x_len"].to(dev), (c["e_enc"].to(dev), c["e_dur"].to(dev))
    B, Tx = x.shape
    mu_x, logw, _ = hip.text_encoder(x, x_len, *rows)
    two = (2 * R.mask_of(c["x_len"], Tx, torch.float32)[:, 0]).to(torch.int32).to(dev)       # a recording of two fine frames per token
    y = torch.randn(B, hp.n_feats, 2 * Tx, generator=torch.Generator().manual_seed(2)).to(dev)
    tape = hip.speaker_grad(x, x_len, *rows, y, 2 * x_len, 0.15, DELTA, durations=two, return_tape=True)
    assert torch.equal(tape["mu_x"], mu_x) and torch.equal(tape["logw"], logw)
    want = tape["enc_rows"].clone()
    out = device_grad(model, c, dev, return_tape=True)
    assert torch.equal(out["enc_rows"], want)
    part = device_grad(model, c, dev, rows=[0, 1], return_tape=True)                          # another B: another workspace layout
    assert torch.equal(part["enc_rows"], want[:2 * Tx])


def test_whole_forward_is_the_forward_under_native_fp32(cells, monkeypatch, dev):
    """Under MTTS_GEMM_TERMS=0 the context's own predictor runs the arithmetic of the training component, so with the model's own
    parameters the whole logw -- frozen rows and predictor launches -- equals mtts_text_encoder_forward's bits.  (Under the split
    arithmetics logw is NOT bit-equal, by design.)"""
    model, c = cells.model(monkeypatch, "tiny", "terms0"), cells.case("tiny", "short")
    _, logw, _ = model.hip.text_encoder(c["x"].to(dev), c["x_len"].to(dev), c["e_enc"].to(dev), c["e_dur"].to(dev))
    out = device_grad(model, c, dev, return_tape=True)
    assert torch.equal(out["logw"], logw)
    assert rel(out["enc_rows"].view(3, 40, -1).permute(0, 2, 1), c["h64"]) <= 8 * rel(c["h32"], c["h64"])


# ------------------------------------------------------------------------------------------------ 3. the whole gradient
WHOLE = [("tiny", "default", "short"), ("tiny", "default", "cap"), ("prod", "default", "short"), ("prod", "default", "rows1044"),
         ("tiny", "p16-off", "short"), ("tiny", "terms6", "short")]


@pytest.mark.parametrize("size,arithmetic,shape", WHOLE)
def test_whole_gradient_against_fp64_autograd(cells, monkeypatch, dev, size, arithmetic, shape):
    model, c = cells.model(monkeypatch, size, arithmetic), cells.case(size, shape)
    hp, _ = cells.weights(size)
    B, Tx = c["x"].shape
    out = device_grad(model, c, dev, return_tape=True)
    got = R.unflatten(out["grad"].cpu(), hp)
    e_fwd = rel(out["enc_rows"].view(B, Tx, -1).permute(0, 2, 1), c["h64"])
    tag = f"gradient {size} {arithmetic} {shape}"
    note(f"{tag}: e_fwd {e_fwd:.3e}")
    failed = []
    for k in list(c["g64"]) + ["g_dur"]:
        g, g64, g32 = (out["g_dur"], c["gd64"], c["gd32"]) if k == "g_dur" else (got[k], c["g64"][k], c["g32"][k])
        err, err32 = rel(g, g64), rel(g32, g64)
        if k != "g_dur" and c["alt"] is not None:
            err = min(err, rel(g, c["alt"][k]))
        bound = 8 * max(err32, e_fwd)
        note(f"{tag} {k}: err {err:.3e}, err32 {err32:.3e}, bound {bound:.3e}")
        if not err <= bound:
            failed.append(k)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 4. same bits, a refused utterance
@pytest.mark.parametrize("size", ["tiny", "prod"])
def test_same_bits_and_a_refused_utterance(cells, monkeypatch, dev, size):
    model, c = cells.model(monkeypatch, size, "default"), cells.case(size, "short")
    a = {k: v.clone() for k, v in device_grad(model, c, dev).items()}
    b = device_grad(model, c, dev)
    for k in ("grad", "g_dur", "dur_sum", "logw"):
        assert torch.equal(a[k], b[k]), k
    assert a["grad"].abs().max() > 0
    raw = guarded_grad(model, c, dev)                                           # sentinel-filled outputs with guards: all written, the same bits
    for k in ("grad", "g_dur", "dur_sum", "logw"):
        assert torch.equal(raw[k], a[k].cpu().reshape(-1)), k
    # the last utterance refused: the gradient of the batch without it, exactly (its rows come last, so every chunk keeps its rows)
    keep = [0, 1]
    good = {k: v.clone() for k, v in device_grad(model, c, dev, rows=keep).items()}
    for what, pattern in (("length", "utterance 2 has x_length = 0"), ("length+", "utterance 2 has x_length = 41"), ("duration", "utterance 2 has a negative duration at token 0")):
        broken = dict(c)
        if what == "duration":
            broken["dur"] = c["dur"].clone()
            broken["dur"][2, 0] = -1
        else:
            broken["x_len"] = c["x_len"].clone()
            broken["x_len"][2] = 0 if what == "length" else 41
        out = device_grad(model, broken, dev, check_lengths=False)
        with pytest.raises(ValueError, match=pattern):
            model.hip.dp_grad_status()
        assert torch.equal(out["grad"], good["grad"]), what
        assert (out["g_dur"][2] == 0).all() and out["dur_sum"][2] == 0
        assert torch.equal(out["g_dur"][keep], good["g_dur"]) and torch.equal(out["dur_sum"][keep], good["dur_sum"])
        with pytest.raises(ValueError, match=pattern):
            device_grad(model, broken, dev)
    device_grad(model, c, dev)                                                  # a clean call afterwards reports nothing


# ------------------------------------------------------------------------------------------------ 5. the trainer
TRAIN = dict(lengths=[24, 17, 9, 1], seed=900, steps=20, lr=2e-3, weight_decay=1e-4, betas=(0.9, 0.99), eps=1e-8, sigma=0.2)


def planted_training_case(hp, sd, synthetic, oracle):
    """Durations sampled from a predictor whose parameters were perturbed (every tensor by sigma times its own root mean square)."""
    x, x_len, spk = synthetic.make_inputs(hp, len(TRAIN["lengths"]), max(TRAIN["lengths"]), seed=TRAIN["seed"], lengths=TRAIN["lengths"])
    e_enc, e_dur = sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk]
    g = torch.Generator().manual_seed(TRAIN["seed"])
    with torch.no_grad():
        h64 = R.encoder_rows(oracle, G.cast_state_dict(sd, torch.float64), hp, x, x_len, e_enc.double())
        h32 = R.encoder_rows(oracle, G.cast_state_dict(sd, torch.float32), hp, x, x_len, e_enc.float())
        P = R.params_of(sd, hp)
        moved = {k: v + TRAIN["sigma"] * v.pow(2).mean().sqrt() * torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in P.items()}
        logw = R.forward(moved, hp, h64, x_len, e_dur.double())
        dur = ((torch.exp(logw[:, 0]) - 2).round().clamp(0, 60) * R.mask_of(x_len, x.shape[1], torch.float64)[:, 0]).long()
    return dict(x=x, x_len=x_len, spk=spk, e_enc=e_enc, e_dur=e_dur, dur=dur, h64=h64, h32=h32)


def test_training_lowers_the_loss_and_tracks_the_fp64_loop(hparams, synthetic, oracle, dev):
    """20 DurationTrainer steps on planted durations against the fp64 AdamW loop of the restatement (same groups, same update).  Both
    bounds are formed on the CPU before the device runs; nothing in them comes from the device's training run.

    The parameters, every tensor after every step.  tests/test_hip_spk_grad.py::test_finetuning_lowers_the_loss_and_tracks_the_fp64_loop
    allows a row k lr 8 err32 + k 2^-24 max|row|: a relative gradient error e moves an Adam coordinate by about lr e per step, e = 8 err32
    admitted.  That sentence is about a coordinate whose gradient is at the scale of the tensor's largest; Adam's normalised update
    m^ / sqrt(v^) sees each coordinate's OWN relative error, and a tensor of 7680 entries has many whose gradient is a hundredth of the
    largest (the float32 CPU loop itself leaves the plain formula at step 2, by 1.08 x, in conv_layers.1.weight).  So the admitted
    gradient error keeps the factor from there, e_t = 8 max(err32_t, e_fwd) of max|g_t| per tensor, exactly the whole-gradient test's
    bound, and is carried through the update coordinate by coordinate (dp_grad_restated.adam_drift_allowance, derived there):
    |u' - u| <= (Am + |u| Av) / (s - Av) per step, at most |u| + Adam's cap for a coordinate whose gradient lies below the error,
    plus one fp32 rounding of the parameter per step.  At the gradient's scale a step's share is 2 lr e_t (numerator and denominator).
    First order: the gradient's change caused by the drift itself (2e-8 after 20 steps) is not carried.

    dur_loss at step k (before that step's update), in addition: to first order |d loss| <= sum_i |g_i| |dp_i| <= 2 k lr sum_i |dg_i|
    <= 2 k lr N_t e_t max|g_t| per tensor of N_t entries, plus the loss evaluation itself, 8 max(err32 of the loss, e_fwd)."""
    hp = grad_hparams(hparams, "tiny")
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    c = planted_training_case(hp, sd, synthetic, oracle)
    kw = {k: TRAIN[k] for k in ("lr", "weight_decay", "betas", "eps")}
    P64, P32 = R.params_of(sd, hp), R.params_of(sd, hp, torch.float32)
    record = []
    trail, hist = R.adamw_loop(P64, hp, [(c["h64"], c["x_len"], c["e_dur"].double(), c["dur"])], TRAIN["steps"], delta=DELTA, record=record, **kw)
    _, hist32 = R.adamw_loop(P32, hp, [(c["h32"], c["x_len"], c["e_dur"].float(), c["dur"])], TRAIN["steps"], delta=DELTA, **kw)
    assert hist[-1] < 0.9 * hist[0], hist                                         # the yardstick's own condition: the loss falls
    tokens = float(c["x_len"].sum())
    g64 = R.param_grads(P64, hp, c["h64"], c["x_len"], c["e_dur"].double(), c["dur"], DELTA)[0]
    g32 = R.param_grads(P32, hp, c["h32"], c["x_len"], c["e_dur"].float(), c["dur"], DELTA)[0]
    model = make_model(hp, sd, dev)
    out = model.hip.dp_grad(c["x"].to(dev), c["x_len"].to(dev), c["e_enc"].to(dev), c["e_dur"].to(dev), c["dur"].to(dev), DELTA,
                            model.hip.dp_train_buffer(None), return_tape=True)
    B, Tx = c["x"].shape
    e_fwd = rel(out["enc_rows"].view(B, Tx, -1).permute(0, 2, 1), c["h64"])
    drift = sum(g64[k].numel() * 8 * max(rel(g32[k], g64[k]), e_fwd) * g64[k].abs().max().item() / tokens for k in g64)
    e_loss = 8 * max(abs(hist32[0] - hist[0]) / hist[0], e_fwd)
    admitted = {k: 8 * max(rel(g32[k], g64[k]), e_fwd) for k in g64}
    allowance = R.adam_drift_allowance(record, admitted, TRAIN["lr"], TRAIN["betas"], {k: float(P64[k].abs().max()) for k in P64})
    trainer = sub("duration").DurationTrainer(model, **kw)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    got, flats = [], []
    for _ in range(TRAIN["steps"]):
        got.append(trainer.step(c["x"].to(dev), c["x_len"].to(dev), c["dur"].to(dev), speaker=c["spk"].to(dev)))
        flats.append(trainer.flat.detach().clone())
    got = [float(v) for v in torch.stack(got).cpu()]
    late = []
    for k in range(1, TRAIN["steps"] + 1):
        p_dev = R.unflatten(flats[k - 1].cpu(), hp)
        worst = (0.0, None, 0.0, 0.0)
        for key in P64:
            diff = (p_dev[key].double() - trail[k][key]).abs()
            ratio = float((diff / allowance[k - 1][key]).max())
            plain = k * TRAIN["lr"] * admitted[key] + k * U * float(P64[key].abs().max())
            if ratio > worst[0]:
                worst = (ratio, key, float(diff.max()), plain)
            if not ratio <= 1.0:
                late.append((k, key, ratio))
        note(f"trainer step {k}: parameters, worst |p - fp64 loop| / allowance {worst[0]:.3f} in {worst[1]} (max|diff| {worst[2]:.3e}; the row formula "
             f"k lr 8 e + k 2^-24 max|p| there: {worst[3]:.3e})")
    assert not late, late
    for k in range(TRAIN["steps"]):
        tol = 2 * k * TRAIN["lr"] * drift + e_loss * hist[k]
        err = abs(got[k] - hist[k])
        note(f"trainer step {k}: dur_loss {got[k]:.8e}, fp64 loop {hist[k]:.8e}, float32 loop {hist32[k]:.8e}, |diff| {err:.3e} (bound {tol:.3e})")
    for k in range(TRAIN["steps"]):
        assert abs(got[k] - hist[k]) <= 2 * k * TRAIN["lr"] * drift + e_loss * hist[k], k
    assert got[-1] < 0.9 * got[0]
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())      # the model itself has not changed yet
    moved = R.unflatten(trainer.flat.detach().cpu(), hp)
    assert all((moved[k].double() - P64[k]).abs().max() > 0 for k in P64)             # every tensor is trained
    # a group that decays and one that does not
    assert trainer.optimizer.param_groups[0]["weight_decay"] == TRAIN["weight_decay"] and trainer.optimizer.param_groups[1]["weight_decay"] == 0.0
    hist2 = trainer.fit([(c["x"], c["x_len"], c["dur"], c["spk"])], epochs=2)["dur_loss"]
    assert len(hist2) == 2 and hist2[1] < got[0]


# ------------------------------------------------------------------------------------------------ 6. commit
def test_commit_pushes_the_predictor_into_the_model_once(hparams, synthetic, oracle, dev, tmp_path):
    D = sub("duration")
    hp = grad_hparams(hparams, "tiny")
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    c = planted_training_case(hp, sd, synthetic, oracle)
    model = make_model(hp, sd, dev)
    x, x_len = c["x"].to(dev), c["x_len"].to(dev)
    rows = (c["e_enc"].to(dev), c["e_dur"].to(dev))
    mu0, logw0, _ = (t.clone() for t in model.hip.text_encoder(x, x_len, *rows))
    # a recording for speaker_grad: two fine frames per token
    y = torch.randn(4, hp.n_feats, 2 * x.shape[1], generator=torch.Generator().manual_seed(1)).to(dev)
    yl = 2 * x_len
    two = (2 * R.mask_of(c["x_len"], x.shape[1], torch.float32)[:, 0]).to(torch.int32).to(dev)
    sg0 = {k: v.clone() for k, v in model.hip.speaker_grad(x, x_len, *rows, y, yl, 0.15, DELTA, durations=two).items()}
    trainer = D.DurationTrainer(model, lr=5e-3)
    for _ in range(3):
        trainer.step(x, x_len, c["dur"].to(dev), speaker=c["spk"].to(dev))
    gen = model.hip.generation
    trainer.commit()
    assert model.hip.generation == gen + 1 and model.hip.cache_hit is False
    trainer.save(tmp_path / "dp")
    saved = D.load_tensors(tmp_path / "dp")
    assert sorted(saved) == sorted(k for k in sd if k.startswith(R.PREFIX))
    assert (tmp_path / "dp" / D.DURATION_OPTIMIZER).exists()
    mu1, logw1, _ = model.hip.text_encoder(x, x_len, *rows)
    fresh = make_model(hp, {**sd, **saved}, dev)
    mu2, logw2, _ = fresh.hip.text_encoder(x, x_len, *rows)
    assert torch.equal(logw1, logw2) and not torch.equal(logw1, logw0)              # the new predictor, bit for bit that of a fresh load
    assert torch.equal(mu1, mu0) and torch.equal(mu2, mu0)                          # nothing else moved
    assert all(torch.equal(model.state_dict()[k].cpu(), v) for k, v in saved.items())
    sg1 = model.hip.speaker_grad(x, x_len, *rows, y, yl, 0.15, DELTA, durations=two)      # rebuilt backward panels
    sg2 = fresh.hip.speaker_grad(x, x_len, *rows, y, yl, 0.15, DELTA, durations=two)
    assert torch.equal(sg1["g_dur"], sg2["g_dur"]) and not torch.equal(sg1["g_dur"], sg0["g_dur"])
    assert torch.equal(sg1["g_enc"], sg0["g_enc"]) and torch.equal(sg1["prior_sum"], sg0["prior_sum"])
    out = model.synthesise(x[:1], x_len[:1], 2, speaker_embeddings=(rows[0][:1], rows[1][:1]))
    assert torch.isfinite(out["mel"]).all()
    # the model's own predictor is now the trained one: duration_grad without params= starts from it
    a = model.duration_grad(x, x_len, durations=c["dur"].to(dev), speaker_embeddings=rows)
    b = model.duration_grad(x, x_len, durations=c["dur"].to(dev), speaker_embeddings=rows, params=trainer.flat)
    assert torch.equal(a["grad"], b["grad"]) and a["dur_loss"].dim() == 0 and a["dur_loss_per_utterance"].shape == (4,)
    assert a["durations"].dtype == torch.int32 and a["logw"].shape == (4, 1, x.shape[1])


# ------------------------------------------------------------------------------------------------ 7. the tool
def test_finetune_durations_tool(tmp_path, monkeypatch, capsys, dev):
    paths = []
    for i, n in enumerate([9000, 7300, 8100]):
        clip = E.synthetic_clip(n, 70 + i, "voiced")
        p = tmp_path / f"clip{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(24000)
            w.writeframes((clip.clamp(-1, 1) * 32767).to(torch.int16).numpy().astype("<i2").tobytes())
        paths.append(str(p))
    ids = tmp_path / "ids.txt"
    ids.write_text("5 17 120 33 8 91 4 250 7\n12 400 3 77 58 9\n9 8 7 6 5 4 3\n")
    out = tmp_path / "dp_ft"
    spec = importlib.util.spec_from_file_location("finetune_durations_tool", ROOT / "tools" / "finetune_durations.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    argv = ["finetune_durations.py", "--synthetic-model", "tiny", "--ids-file", str(ids), "--epochs", "4", "--lr", "2e-3", "--batch-size", "2",
            "--speaker", "1", "--out", str(out), *paths]
    monkeypatch.setattr(sys, "argv", argv)
    assert tool.main() == 0
    text = capsys.readouterr().out
    assert "dur_loss" in text and "8 steps" in text
    D = sub("duration")
    saved = D.load_tensors(out)
    hp = sub("hparams").tiny(n_spks=2)
    sd = sub("synthetic").make_state_dict(hp, seed=7, duration_recipe=False)
    for k, v in saved.items():
        assert v.shape == sd[k].shape and torch.isfinite(v).all() and not torch.equal(v, sd[k]), k
    cache = np.load(out / "durations.npz")
    assert cache["durations"].shape == (3, 9) and (cache["durations"].sum(1) > 0).all()
    monkeypatch.setattr(sys, "argv", argv)
    assert tool.main() == 0 and "durations read from" in capsys.readouterr().out     # the second run reuses the cached alignment

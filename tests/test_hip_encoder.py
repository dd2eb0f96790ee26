"""GPU tests of mtts_text_encoder_forward (csrc/encoder.hip) as a whole: the prior mu_x and the log-durations logw of every case of
tests/encoder_cases.py against oracle.text_encoder_forward in fp64 (tests/test_encoder_oracle.py checks that reference on the CPU), in
four arithmetics -- the default (MTTS_GEMM_TERMS=2 with P16 images), MTTS_P16=0, MTTS_GEMM_TERMS=0 and MTTS_GEMM_TERMS=6 (what the range
guard reruns a call on) -- each on a context created under its switches.

Per cell: x_mask is sequence_mask exactly; mu_x and logw are finite and exactly 0 at padded tokens; max |mu_x - mu64| < 2e-5 and
max |logw - logw64| < 2e-5 (the project's bar of test_tiny_encoder_vs_golden and test_duration_predictor_live_vs_golden, about 5x the
fp32 oracle's own distance from fp64); mtts_durations of the GPU's logw gives the integer frames, cumulative sums and fine lengths of
oracle.durations_from_logw(logw64) on EVERY token for both factor pairs (no token sits where a logw inside the bar could flip a count:
test_encoder_oracle.test_no_token_sits_in_the_rounding_band); a second call is bit-equal and the range flag is clear; and the per-launch
event pass shows which FFN branch ran: under the default arithmetic on `tiny` and `production` each layer's second FFN conv is a
gemm_p16_kernel launch (the masked P16 hand-over), on `odd` (filter 80) and under the other arithmetics it is the fp32-row kernel with
a_mask and no launch of the call is a P16 one; the launch count is 8 + 2 prenet + 8 layers + 2 dp layers for all of them.

Properties (default arithmetic and MTTS_GEMM_TERMS=6, batch [65, 64, 63, 1], all three encoders): other valid token ids in the padded
slots leave all three outputs bit-equal; an utterance run alone, padded to the batch's Tx, gives the bits of its rows in the batch
(no kernel of the call picks another summation order between 65 and 260 rows); contexts under MTTS_GEMM_TERMS 1, 16 and 17 (fast16 and
the two 16-bit storage modes, which are the estimator's) give the default's mu_x and logw bit for bit.

No cell needed a library fix.  Three deliberate breakages of csrc/encoder.hip were tried once each: without out16_mask on the first
FFN conv the ragged default cells of tiny and production miss both bars (mu_x by 0.39 / 0.62) and 10 .. 20 frame counts; with
fast16 = true on the second FFN conv the same cells miss both bars (mu_x 1.0e-4 .. 1.3e-4, logw up to 1.1e-3) and one or two frame counts
flip; with col_off 0 in the speaker columns every test of this file fails (both bars, the second call's bits, the three properties).

Measured max-abs error against the fp64 oracle (MI355X), "(fp32)" = the fp32 oracle's own distance from the fp64 one on the same
case, share = the larger of the two errors over the 2e-5 bar, P16 launches = launches tagged gemm_p16_kernel of the call's launches.
More than half the bar: logw of production under MTTS_GEMM_TERMS 0 and 6 on the ragged batches (marked *), about 3x the fp32
oracle's distance; every other cell stays under 0.3.

    encoder     arithmetic batch        mu_x    (fp32)      logw    (fp32)  share  P16 launches
    tiny        default    one      2.13e-07  1.95e-07  2.57e-07  2.20e-07   0.01  2 of 41
    tiny        default    edge64   8.95e-07  8.71e-07  2.24e-06  2.63e-06   0.11  2 of 41
    tiny        default    three    8.86e-07  1.19e-06  2.07e-06  2.43e-06   0.10  2 of 41
    tiny        default    five     9.10e-07  1.07e-06  1.89e-06  2.22e-06   0.09  2 of 41
    tiny        p16-off    one      2.13e-07  1.95e-07  2.57e-07  2.20e-07   0.01  0 of 41
    tiny        p16-off    edge64   8.95e-07  8.71e-07  2.24e-06  2.63e-06   0.11  0 of 41
    tiny        p16-off    three    8.86e-07  1.19e-06  2.07e-06  2.43e-06   0.10  0 of 41
    tiny        p16-off    five     9.10e-07  1.07e-06  1.89e-06  2.22e-06   0.09  0 of 41
    tiny        terms0     one      3.64e-07  1.95e-07  1.38e-07  2.20e-07   0.02  0 of 41
    tiny        terms0     edge64   1.39e-06  8.71e-07  2.48e-06  2.63e-06   0.12  0 of 41
    tiny        terms0     three    1.12e-06  1.19e-06  3.27e-06  2.43e-06   0.16  0 of 41
    tiny        terms0     five     1.41e-06  1.07e-06  3.17e-06  2.22e-06   0.16  0 of 41
    tiny        terms6     one      2.50e-07  1.95e-07  5.77e-07  2.20e-07   0.03  0 of 41
    tiny        terms6     edge64   1.37e-06  8.71e-07  3.83e-06  2.63e-06   0.19  0 of 41
    tiny        terms6     three    1.05e-06  1.19e-06  2.92e-06  2.43e-06   0.15  0 of 41
    tiny        terms6     five     1.61e-06  1.07e-06  4.20e-06  2.22e-06   0.21  0 of 41
    production  default    one      7.75e-07  7.34e-07  5.63e-07  8.68e-07   0.04  4 of 61
    production  default    edge64   1.49e-06  1.66e-06  4.03e-06  4.02e-06   0.20  4 of 61
    production  default    three    1.45e-06  1.94e-06  5.74e-06  4.06e-06   0.29  4 of 61
    production  p16-off    one      7.75e-07  7.34e-07  8.61e-08  8.68e-07   0.04  0 of 61
    production  p16-off    edge64   1.59e-06  1.66e-06  5.34e-06  4.02e-06   0.27  0 of 61
    production  p16-off    three    1.78e-06  1.94e-06  4.79e-06  4.06e-06   0.24  0 of 61
    production  terms0     one      1.91e-06  7.34e-07  1.28e-06  8.68e-07   0.10  0 of 61
    production  terms0     edge64   3.18e-06  1.66e-06  1.12e-05  4.02e-06   0.56* 0 of 61
    production  terms0     three    3.04e-06  1.94e-06  1.17e-05  4.06e-06   0.58* 0 of 61
    production  terms6     one      1.39e-06  7.34e-07  1.52e-06  8.68e-07   0.08  0 of 61
    production  terms6     edge64   3.10e-06  1.66e-06  1.22e-05  4.02e-06   0.61* 0 of 61
    production  terms6     three    3.10e-06  1.94e-06  9.44e-06  4.06e-06   0.47  0 of 61
    odd         default    one      5.11e-07  1.42e-07  1.02e-07  5.79e-07   0.03  0 of 41
    odd         default    edge64   9.17e-07  1.11e-06  2.08e-06  2.66e-06   0.10  0 of 41
    odd         default    three    1.10e-06  1.07e-06  1.94e-06  2.66e-06   0.10  0 of 41
    odd         default    five     1.40e-06  1.17e-06  2.12e-06  2.80e-06   0.11  0 of 41
    odd         p16-off    one      5.11e-07  1.42e-07  1.02e-07  5.79e-07   0.03  0 of 41
    odd         p16-off    edge64   9.17e-07  1.11e-06  2.08e-06  2.66e-06   0.10  0 of 41
    odd         p16-off    three    1.10e-06  1.07e-06  1.94e-06  2.66e-06   0.10  0 of 41
    odd         p16-off    five     1.40e-06  1.17e-06  2.12e-06  2.80e-06   0.11  0 of 41
    odd         terms0     one      3.13e-07  1.42e-07  3.41e-07  5.79e-07   0.02  0 of 41
    odd         terms0     edge64   1.24e-06  1.11e-06  3.68e-06  2.66e-06   0.18  0 of 41
    odd         terms0     three    1.47e-06  1.07e-06  2.80e-06  2.66e-06   0.14  0 of 41
    odd         terms0     five     1.62e-06  1.17e-06  3.82e-06  2.80e-06   0.19  0 of 41
    odd         terms6     one      3.07e-07  1.42e-07  6.13e-07  5.79e-07   0.03  0 of 41
    odd         terms6     edge64   1.30e-06  1.11e-06  2.50e-06  2.66e-06   0.12  0 of 41
    odd         terms6     three    1.15e-06  1.07e-06  2.95e-06  2.66e-06   0.15  0 of 41
    odd         terms6     five     1.45e-06  1.17e-06  3.19e-06  2.80e-06   0.16  0 of 41
"""
import pytest
import torch

import encoder_cases as ec
from conftest import sub
from test_hip_path import make_model, maxabs

pytestmark = pytest.mark.gpu
P16_TAG = "gemm_p16_kernel"
ARITHMETICS = {"default": {}, "p16-off": {"MTTS_P16": "0"}, "terms0": {"MTTS_GEMM_TERMS": "0"}, "terms6": {"MTTS_GEMM_TERMS": "6"}}
STORAGE_MODES = {"fast16": "1", "fp16": "16", "bf16": "17"}           # MTTS_GEMM_TERMS of the estimator-only modes
PROPERTY_BATCH = "edge64"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


class Bench:
    """What the cells share: one model per (encoder, switches), created under the switches (read at mtts_create only), and the launch
    count of an encoder's first cell, which every later arithmetic must repeat."""

    def __init__(self, dev):
        self.dev = dev
        self._models, self.launches = {}, {}

    def model(self, monkeypatch, enc, env):
        key = enc, tuple(sorted(env.items()))
        if key not in self._models:
            hp, sd = ec.weights(enc)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            m = make_model(hp, sd, self.dev)
            m.hip
            for k in env:
                monkeypatch.delenv(k)
            self._models[key] = m
        return self._models[key]

    def inputs(self, enc, batch):
        return tuple(a.to(self.dev) for a in ec.inputs(enc, batch))

    def run(self, m, x, x_len, e_enc, e_dur):
        mu, logw, mask = m.hip.text_encoder(x, x_len, e_enc, e_dur)
        torch.cuda.synchronize()
        return mu, logw, mask

    def run_tagged(self, m, *args):
        """(outputs, kernel tag per launch) of one call with the per-launch event pass on."""
        m.hip.prof_enable(True)
        m.hip.prof_reset()
        try:
            out = self.run(m, *args)
            tags = m.hip.prof_tags()
            assert len(tags) == len(m.hip.prof_records())
        finally:
            m.hip.prof_enable(False)
        return out, tags


@pytest.fixture(scope="module")
def bench(dev):
    return Bench(dev)


def same_bits(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def ffn2_launches(hp):
    """(index of each layer's second FFN conv among the launches of mtts_text_encoder_forward, launches of the call): sequence mask,
    embedding, conv + LayerNorm per prenet layer, prenet projection, speaker columns, then per layer q|k|v, RoPE, attention,
    out-projection, LayerNorm, FFN conv 1, FFN conv 2, LayerNorm, then proj_m (two GEMMs and the transpose), FiLM, conv + LayerNorm per
    duration layer and the duration projection."""
    e = hp.encoder
    first = 2 + 2 * e.prenet_layers + 2
    return [first + 8 * l + 6 for l in range(e.n_layers)], first + 8 * e.n_layers + 3 + 1 + 2 * e.dp_n_layers + 1


@pytest.mark.parametrize("arith", list(ARITHMETICS))
@pytest.mark.parametrize("enc", ec.ENCODERS)
def test_encoder_vs_fp64_oracle(enc, arith, bench, oracle, monkeypatch):
    env = ARITHMETICS[arith]
    m = bench.model(monkeypatch, enc, env)
    hp, _ = ec.weights(enc)
    terms = int(env.get("MTTS_GEMM_TERMS", 2))
    assert m.hip.gemm_terms() == terms
    ffn2, n_launches = ffn2_launches(hp)
    p16_ffn = arith == "default" and hp.encoder.filter_channels % 32 == 0
    assert p16_ffn == (arith == "default" and enc != "odd")
    failed = []                                               # every named check of every batch is evaluated: (check, cell, detail)

    def check(ok, name, *detail):
        if not bool(ok):
            failed.append((name, *detail))

    for batch in ec.BATCHES_OF[enc]:
        cell = (enc, arith, batch)
        lengths = ec.BATCHES[batch]
        args = bench.inputs(enc, batch)
        x, x_len = args[0], args[1]
        args = (x, x_len, args[3], args[4])
        mu64, logw64, mask64 = ec.reference(enc, batch)
        mu32, logw32, _ = ec.reference(enc, batch, torch.float32)
        (mu, logw, mask), tags = bench.run_tagged(m, *args)
        assert mu.shape == mu64.shape and logw.shape == logw64.shape and mu.dtype == logw.dtype == torch.float32
        # ---- parity with the fp64 oracle
        e_mu, e_logw = maxabs(mu, mu64), maxabs(logw, logw64)
        o_mu, o_logw = maxabs(mu32, mu64), maxabs(logw32, logw64)
        share = max(e_mu / ec.MU_BAR, e_logw / ec.LOGW_BAR)
        print(f"encoder {enc} {arith} {batch}: max|mu_x - mu64| = {e_mu:.2e} (fp32 oracle {o_mu:.2e}), max|logw - logw64| = {e_logw:.2e} "
              f"(fp32 oracle {o_logw:.2e}), share of the 2e-5 bar {share:.2f}, P16 launches {sum(P16_TAG in t for t in tags)} of {len(tags)}"
              f"{' MORE THAN HALF THE BAR' if share > 0.5 else ''}")
        check(e_mu < ec.MU_BAR, "mu_x within 2e-5 of fp64", cell, e_mu)
        check(e_logw < ec.LOGW_BAR, "logw within 2e-5 of fp64", cell, e_logw)
        # ---- mask, padding
        want_mask = oracle.sequence_mask(x_len.cpu(), x.shape[1]).unsqueeze(1)
        check(torch.equal(mask.cpu(), want_mask.float()), "x_mask is sequence_mask", cell)
        check(torch.isfinite(mu).all() and torch.isfinite(logw).all(), "finite", cell)
        padded = ~want_mask
        assert bool(padded.any()) == (len(set(lengths)) > 1)
        check((logw.cpu()[padded] == 0).all() and (mu.cpu()[padded.expand_as(mu)] == 0).all(), "exactly 0 at padded tokens", cell)
        # ---- which kernels ran
        check(len(tags) == n_launches, "launch count", cell, len(tags), n_launches)
        check(bench.launches.setdefault((enc, batch), len(tags)) == len(tags), "launch count equal in every arithmetic", cell)
        p16_at = [i for i, t in enumerate(tags) if P16_TAG in t]
        check(p16_at == (ffn2 if p16_ffn else []), "P16 launches = second FFN convs", cell, p16_at)
        if not p16_ffn and len(tags) == n_launches:           # fp32 rows with a_mask: gemm_f32_kernel<BM, A_MASK, A_NORM, TERMS>
            check(all(tags[i].startswith("gemm_f32_kernel<") and tags[i].endswith(f", true, false, {terms}>") for i in ffn2),
                  "second FFN conv on fp32 rows with a_mask", cell, [tags[i] for i in ffn2])
        # ---- repeatability, range flag
        check(same_bits(bench.run(m, *args), (mu, logw, mask)), "second call bit-equal", cell)
        check(not m.hip.range_flags().any().item(), "range flag clear", cell)
        # ---- durations: equal integers on every token
        for sc, ls in ec.FACTORS:
            want = oracle.durations_from_logw(logw64, mask64, sc, ls)
            dur, cum, yfl = m.hip.durations(logw, mask, sc, ls)
            assert dur.shape == want.shape
            check(torch.equal(dur.cpu().double(), want), "frames per token equal the fp64 oracle's", cell, sc, ls,
                  f"{int((dur.cpu().double() != want).sum())} tokens differ")
            check(torch.equal(cum.cpu().long(), torch.cumsum(want.long(), 1)), "cumulative frames", cell, sc, ls)
            check(torch.equal(yfl.cpu(), want.sum(1).long().clamp_min(1)), "fine lengths", cell, sc, ls)
    assert not failed, "\n".join(str(f) for f in failed)


def property_cell(bench, monkeypatch, enc, arith):
    m = bench.model(monkeypatch, enc, ARITHMETICS[arith])
    x, x_len, _, e_enc, e_dur = bench.inputs(enc, PROPERTY_BATCH)
    return m, x, x_len, e_enc, e_dur, bench.run(m, x, x_len, e_enc, e_dur)


@pytest.mark.parametrize("arith", ["default", "terms6"])
@pytest.mark.parametrize("enc", ec.ENCODERS)
def test_padding_is_inert(enc, arith, bench, monkeypatch):
    """Whatever valid id sits beyond x_length (the k5 convs read across the sequence end, the attention runs over the padded keys,
    the LayerNorm kernel takes 4 rows per workgroup) reaches no output bit."""
    m, x, x_len, e_enc, e_dur, base = property_cell(bench, monkeypatch, enc, arith)
    beyond = torch.arange(x.shape[1], device=x.device)[None, :] >= x_len[:, None]
    assert bool(beyond.any())
    for other in (0, sub("hparams").N_VOCAB - 1):
        x2 = torch.where(beyond, torch.full_like(x, other), x)
        assert not torch.equal(x2, x)
        got = bench.run(m, x2, x_len, e_enc, e_dur)
        for name, a, b in zip(("mu_x", "logw", "x_mask"), got, base):
            assert torch.equal(a, b), (enc, arith, other, name, maxabs(a, b))


@pytest.mark.parametrize("arith", ["default", "terms6"])
@pytest.mark.parametrize("enc", ec.ENCODERS)
def test_rows_do_not_depend_on_the_batch(enc, arith, bench, monkeypatch):
    """Each utterance alone, padded to the batch's Tx (65 rows against 260), gives the bits of its rows in the batch."""
    m, x, x_len, e_enc, e_dur, base = property_cell(bench, monkeypatch, enc, arith)
    for b in range(x.shape[0]):
        got = bench.run(m, x[b:b + 1], x_len[b:b + 1], e_enc[b:b + 1], e_dur[b:b + 1])
        for name, a, full in zip(("mu_x", "logw", "x_mask"), got, base):
            assert torch.equal(a, full[b:b + 1]), (enc, arith, b, name, maxabs(a, full[b:b + 1]))


@pytest.mark.parametrize("enc", ec.ENCODERS)
def test_storage_modes_do_not_reach_the_text_side(enc, bench, monkeypatch):
    """fast16 and the 16-bit storage modes change the estimator only (host.h run_gemm: half_now is set while the estimator enqueues;
    encoder.hip hands its P16 image over with fast16 = false): the encoder's outputs are the default's bit for bit."""
    _, x, x_len, e_enc, e_dur, base = property_cell(bench, monkeypatch, enc, "default")
    for mode, terms in STORAGE_MODES.items():
        m = bench.model(monkeypatch, enc, {"MTTS_GEMM_TERMS": terms})
        assert m.hip.gemm_terms() == int(terms)
        got = bench.run(m, x, x_len, e_enc, e_dur)
        for name, a, b in zip(("mu_x", "logw", "x_mask"), got, base):
            assert torch.equal(a, b), (enc, mode, name, maxabs(a, b))
        assert not bool(m.hip.range_flags().any().item())

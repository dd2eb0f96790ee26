"""GPU tests of the estimator's launch forms: a transformer block's row-local part runs as the four tiled GEMM launches, as the chain
launch or as its pair form (csrc/decoder.hip tblock_plan), and every form must give the estimator's velocity on its own -- against
oracle.decoder_forward in fp64 (state dict, x, mask, mu and t cast to double, plain softmax attention), at every width, with each form
forced at small ragged shapes and with the default switches at the 3200-row batch where the pair form starts.

Per cell: max-abs error of v within the project's bar (1e-4 at width 384 as test_prod_chain_launch_vs_golden, 5e-5 on the narrow
estimators as test_tiny_decoder_vs_golden; both were set against fp32 references, the fp32 oracle is itself 4e-6 .. 1.1e-5 from the
fp64 one at these shapes), padded frames exactly 0, a second call bitwise equal, no range flag, no pair time-out, and the form that ran
(kernel tags and launch count of the per-launch event pass) is the form mtts_tblock_plan predicts for each block's (C, ch, M, switches).

Measured max-abs error of v against the fp64 oracle (MI355X), worst of t = 0.0 and t = 0.37; batch A = lengths [70, 45, 14], B = [100, 97,
61, 60, 33, 1], D = the default-switch batch of 10 x 320 frames (max |v| 4.6 .. 11.4 on A and B, 24.8 on D).  "chain-tall" = the chain
launch with MTTS_CHAIN_QB at the tall shape (48 rows with hidden chunk 256, else 64).  No cell uses more than half of its bar.

    estimator         switches       bar         A         B         D  share of bar
    production        tiled        1e-04  5.82e-06  8.01e-06         -  0.08
    production        chain        1e-04  5.33e-06  8.75e-06         -  0.09
    production        chain-tall   1e-04  5.33e-06  8.75e-06         -  0.09
    production        pair-asked   1e-04  4.78e-06  9.22e-06         -  0.09
    production-ch128  tiled        1e-04  5.82e-06  8.01e-06         -  0.08
    production-ch128  chain        1e-04  5.33e-06  8.75e-06         -  0.09
    production-ch128  chain-tall   1e-04  5.33e-06  8.75e-06         -  0.09
    production-ch128  pair-asked   1e-04  5.82e-06  8.01e-06         -  0.08
    narrow256         tiled        5e-05  4.31e-06  7.79e-06         -  0.16
    narrow256         chain        5e-05  4.11e-06  8.84e-06         -  0.18
    narrow256         chain-tall   5e-05  4.11e-06  8.84e-06         -  0.18
    narrow256         pair-asked   5e-05  4.31e-06  7.79e-06         -  0.16
    narrow128         tiled        5e-05  3.33e-06  7.79e-06         -  0.16
    narrow128         chain        5e-05  3.80e-06  1.04e-05         -  0.21
    narrow128         chain-tall   5e-05  3.80e-06  1.04e-05         -  0.21
    narrow128         pair-asked   5e-05  3.33e-06  7.79e-06         -  0.16
    mixed             tiled        5e-05  5.01e-06  6.34e-06         -  0.13
    mixed             chain        5e-05  4.29e-06  7.13e-06         -  0.14
    mixed             chain-tall   5e-05  4.29e-06  7.13e-06         -  0.14
    mixed             pair-asked   5e-05  5.01e-06  6.34e-06         -  0.13
    production        defaults     1e-04         -         -  1.54e-05  0.15
    production-ch128  defaults     1e-04         -         -  1.40e-05  0.14
    narrow256         defaults     5e-05         -         -  1.69e-05  0.34
"""
import dataclasses

import pytest
import torch

from test_hip_path import make_model, maxabs

pytestmark = pytest.mark.gpu
CHAIN_TAG = "tblock_chain_kernel"
T_VALUES = (0.37, 0.0)

# estimator -> (decoder channels, n_blocks, heads) or None for prod_v20's own, extra switches, bar on max |v - v_fp64|
ESTIMATORS = {
    "production": (None, {}, 1e-4),
    "production-ch128": (None, {"MTTS_CHAIN_CH": "128"}, 1e-4),
    "narrow256": (((256, 256), 2, 3), {}, 5e-5),
    "narrow128": (((128, 128), 2, 2), {}, 5e-5),
    "mixed": (((128, 256), 1, 2), {}, 5e-5),                  # one block per run: no chain launch carries a following q|k|v
}
FORMS = {
    "tiled": {"MTTS_CHAIN": "0"},
    "chain": {"MTTS_CHAIN_MIN_ROWS": "0", "MTTS_CHAIN_PAIR": "0"},
    "chain-tall": {"MTTS_CHAIN_MIN_ROWS": "0", "MTTS_CHAIN_PAIR": "0", "MTTS_CHAIN_QB": "tall"},      # 48 rows with hidden chunk 256, else 64
    "pair-asked": {"MTTS_CHAIN_PAIR_MIN_ROWS": "0"},          # only production with hidden chunk 256 takes the pair form
}
BATCHES = {
    "A": [70, 45, 14],                                        # 210 / 105 rows: a partly filled last tile at 32, 48 and 64 rows per workgroup
    "B": [100, 97, 61, 60, 33, 1],                            # 600 / 300 rows: 13 tiles of 48 = a second, partly idle group of 16 pair workgroups
    "D": [320, 319, 301, 288, 250, 222, 200, 180, 161, 1],    # 3200 / 1600 rows: default thresholds, pair form at the fine level only
}
SWITCH_OF = {"MTTS_CHAIN": "chain_on", "MTTS_CHAIN_CH": "chain_ch", "MTTS_CHAIN_QB": "chain_qb", "MTTS_CHAIN_MIN_ROWS": "chain_min_rows",
             "MTTS_CHAIN_PAIR": "pair_on", "MTTS_CHAIN_PAIR_MIN_ROWS": "pair_min_rows"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


class Bench:
    """What the cells share: hyper-parameters and weights per estimator, inputs per batch, the fp64 references (computed once each),
    the tiled models and their launch counts."""

    def __init__(self, hparams, synthetic, oracle, dev):
        self.hparams, self.synthetic, self.oracle, self.dev = hparams, synthetic, oracle, dev
        self._weights, self._inputs, self._refs, self._tiled, self._tiled_count = {}, {}, {}, {}, {}

    def weights(self, est):
        shape = ESTIMATORS[est][0]
        if shape not in self._weights:
            if shape is None:
                hp = self.hparams.prod_v20(n_spks=1)
                sd = self.synthetic.make_state_dict(hp, seed=7)
            else:
                channels, n_blocks, heads = shape
                hp = self.hparams.tiny(n_spks=2)
                hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64,
                                                                         n_blocks=n_blocks, num_mid_blocks=1, num_heads=heads))
                sd = self.synthetic.make_state_dict(hp, seed=21)
            self._weights[shape] = hp, sd
        return self._weights[shape]

    def inputs(self, est, batch):
        hp, _ = self.weights(est)
        key = hp.n_feats, batch
        if key not in self._inputs:
            lengths = torch.tensor(BATCHES[batch])
            B, T = len(lengths), int(lengths.max())
            g = torch.Generator().manual_seed(1000 + len(batch) + B)
            x = torch.randn(B, hp.n_feats, T, generator=g)
            mu = torch.randn(B, hp.n_feats, T, generator=g)
            mask = (torch.arange(T)[None, :] < lengths[:, None]).float()[:, None, :]
            self._inputs[key] = x, mask, mu
        return self._inputs[key]

    def reference(self, est, batch, tv):
        """oracle.decoder_forward in fp64 at the fp32 value of t the library is given."""
        key = ESTIMATORS[est][0], batch, tv
        if key not in self._refs:
            hp, sd = self.weights(est)
            sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
            x, mask, mu = (a.double() for a in self.inputs(est, batch))
            t = torch.tensor(tv, dtype=torch.float32).double()
            with torch.no_grad():
                self._refs[key] = self.oracle.decoder_forward(sd64, hp, x, mask, mu, t, use_torch_sdpa=False)
        return self._refs[key]

    def model(self, monkeypatch, est, env):
        """A model whose context was created under the estimator's switches and `env` (read at mtts_create only)."""
        hp, sd = self.weights(est)
        tiled = env == FORMS["tiled"]
        env = {**ESTIMATORS[est][1], **env}
        if tiled and est in self._tiled:                      # (kept: every cell of the estimator counts its launches against it)
            return self._tiled[est], env
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = make_model(hp, sd, self.dev)
        m.hip
        for k in env:
            monkeypatch.delenv(k)
        if tiled:
            self._tiled[est] = m
        return m, env

    def evaluate(self, m, est, batch, tv):
        """(v, per-launch tags) of one estimator evaluation with the per-launch event pass on."""
        x, mask, mu = (a.to(self.dev) for a in self.inputs(est, batch))
        m.hip.prof_enable(True)
        m.hip.prof_reset()
        try:
            v = m.hip.decoder_forward(x, mask, mu, tv)
            torch.cuda.synchronize()
            tags = m.hip.prof_tags()
            assert len(tags) == len(m.hip.prof_records())
        finally:
            m.hip.prof_enable(False)
        return v, tags

    def tiled_launches(self, monkeypatch, est, batch):
        """Launches of one evaluation on the estimator's tiled model (MTTS_CHAIN=0)."""
        if (est, batch) not in self._tiled_count:
            m, _ = self.model(monkeypatch, est, FORMS["tiled"])
            _, tags = self.evaluate(m, est, batch, T_VALUES[0])
            assert not any(CHAIN_TAG in t for t in tags)
            self._tiled_count[est, batch] = len(tags)
        return self._tiled_count[est, batch]


@pytest.fixture(scope="module")
def bench(hparams, synthetic, oracle, dev):
    return Bench(hparams, synthetic, oracle, dev)


def predicted(hip, hp, env, B, T):
    """The transformer blocks of one evaluation in launch order (csrc/decoder.hip unet_eval) with the plan mtts_tblock_plan gives each:
    [(C, ch, form, qb, carries the next q|k|v, the level's rows M)]."""
    d = hp.decoder
    kw = {SWITCH_OF[k]: int(v) for k, v in env.items()}
    nl, inner = len(d.channels), d.num_heads * d.attention_head_dim
    runs = [(d.channels[l], l) for l in range(nl)] + [(d.channels[-1], nl - 1)] * d.num_mid_blocks        # down path, mid blocks,
    runs += [(d.channels[nl - 2 - i] if i + 1 < nl else d.channels[0], nl - 1 - i) for i in range(nl)]    # up path
    out = []
    for width, level in runs:
        M = B * (T >> level)
        for j in range(d.n_blocks):
            n_qkv = 3 * inner if j + 1 < d.n_blocks else 0
            ch, form, qb, grid, pf = hip.tblock_plan(width, inner, n_qkv, M, 1, **kw)
            out.append((width, ch, int(form[0]), int(qb[0]), n_qkv > 0, M))
    return out


def check_cell(bench, monkeypatch, est, env, batches, expect_forms):
    from conftest import sub
    hip = sub("_hip")
    m, env = bench.model(monkeypatch, est, env)
    hp, _ = bench.weights(est)
    bar = ESTIMATORS[est][2]
    for batch in batches:
        lengths = BATCHES[batch]
        B, T = len(lengths), max(lengths)
        plan = predicted(hip, hp, env, B, T)
        per_rows = {}                                         # {level rows: forms}: the plan is what this cell is meant to run
        for p in plan:
            per_rows.setdefault(p[5], set()).add(p[2])
        assert per_rows == expect_forms(B, T), (est, batch, per_rows)
        want_tags = [f"{CHAIN_TAG}<{width}, {qb}, {ch}>" for width, ch, form, qb, _, _ in plan if form]
        # a chain or pair launch replaces out-projection, FF1 and FF2, and the following block's q|k|v where it carries it
        # (tests/test_hip_path.py test_chain_launch_ragged_batch_and_launch_count)
        saving = sum((3 if carries else 2) for _, _, form, _, carries, _ in plan if form)
        tiled = bench.tiled_launches(monkeypatch, est, batch)
        for tv in T_VALUES:
            ref = bench.reference(est, batch, tv)
            v, tags = bench.evaluate(m, est, batch, tv)
            assert v.shape == ref.shape and torch.isfinite(v).all()
            # the form that ran is the predicted one: the chain launches in order with their rows per workgroup, and the launch count
            assert [t for t in tags if CHAIN_TAG in t] == want_tags, (est, batch, tv)
            assert len(tags) == tiled - saving, (est, batch, len(tags), tiled, saving)
            x, mask, mu = (a.to(bench.dev) for a in bench.inputs(est, batch))
            again = m.hip.decoder_forward(x, mask, mu, tv)
            assert torch.equal(again, v), (est, batch, tv)
            assert not bool(m.hip.range_flags().any().item()) and not bool(m.hip.pair_timeouts().any().item())
            padded = (mask == 0).expand_as(v)
            assert padded.any() and bool((v[padded] == 0).all())
            err = maxabs(v, ref)
            print(f"dispatch {est} {'+'.join(f'{k}={env[k]}' for k in sorted(env)) or 'defaults'} batch {batch} t={tv}: "
                  f"max|v - v_fp64| = {err:.3e} (bar {bar:.0e}, max|v| {float(ref.abs().max()):.2f}), chain launches {len(want_tags)}"
                  f"{' MORE THAN HALF THE BAR' if err > 0.5 * bar else ''}")
            assert err < bar, (est, batch, tv, err)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("est", list(ESTIMATORS))
def test_forced_form_vs_fp64_oracle(est, form, bench, monkeypatch):
    """Each launch form forced at small ragged shapes, on every estimator.  "chain" takes 32-row workgroups at these sizes, "chain-tall"
    asks for the tall shape (MTTS_CHAIN_QB).  "pair-asked" lowers the pair threshold to 0 and leaves the chain
    threshold alone: production with hidden chunk 256 runs pair launches at both levels, every other estimator the tiled launches."""
    want = {"tiled": {0}, "chain": {1}, "chain-tall": {1}, "pair-asked": {2} if est == "production" else {0}}[form]
    env = {k: (("48" if est == "production" else "64") if v == "tall" else v) for k, v in FORMS[form].items()}
    check_cell(bench, monkeypatch, est, env, ["A", "B"], lambda B, T: {B * T: want, B * T // 2: want})


@pytest.mark.parametrize("est,fine", [("production", 2), ("production-ch128", 0), ("narrow256", 0)])
def test_default_switches_at_the_pair_threshold_vs_fp64_oracle(est, fine, bench, monkeypatch):
    """Nothing forced, 10 utterances x 320 frames (3200 rows at the fine level, 1600 at the coarse one): production runs pair launches at
    the fine level and tiled ones at the coarse level; a (256, 256) estimator and production with MTTS_CHAIN_CH=128 have no 48-row pair
    shape and run the tiled launches (they failed with the launcher's invalid-value error before the pair form was gated)."""
    check_cell(bench, monkeypatch, est, {}, ["D"], lambda B, T: {3200: {fine}, 1600: {0}})

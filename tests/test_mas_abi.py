"""Forced alignment without a GPU: the new C entries and their host-side refusals, the NumPy restatement of the search against a
brute-force enumeration of every monotone path (ties included), and the batcher's per-request durations field."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT, sub
import mas_restated as R


@pytest.fixture(scope="module")
def lib():
    return sub("_hip").load()


def test_symbols_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_mas_workspace_bytes.restype is C.c_int64
    for name in ("mtts_mas_logprior", "mtts_mas", "mtts_mas_status", "mtts_durations_given"):
        assert getattr(lib, name).restype is C.c_int
    assert lib.mtts_abi_version() == 2
    assert "mas.hip" in sub("_hip").SOURCES
    hip = sub("_hip").HipModel
    for method in ("mas", "mas_logprior", "mas_status", "durations_given"):
        assert callable(getattr(hip, method))


def test_workspace_bytes_positive_monotone_and_refusing(lib):
    ws = lib.mtts_mas_workspace_bytes
    by_b = [ws(B, 128, 1500) for B in (1, 2, 3, 8, 32, 64)]
    by_tx = [ws(4, Tx, 2300) for Tx in (1, 5, 64, 65, 128, 130, 600, 1024)]
    by_tm = [ws(4, 128, Tm) for Tm in (128, 129, 300, 1500, 2300, 5000)]
    for seq in (by_b, by_tx, by_tm):
        assert all(v > 0 for v in seq), seq
        assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[0] < seq[-1], seq
    assert all(a < b for a, b in zip(by_b, by_b[1:]))
    # the log-prior image [B][Tm][64 ceil(Tx / 64) rounded to a power of two] must fit
    assert ws(32, 128, 1500) >= 32 * 1500 * 128 * 4
    assert ws(1, 600, 2300) >= 2300 * 1024 * 4
    for bad in ((0, 10, 20), (-1, 10, 20), (1, 0, 20), (1, 1025, 2000), (1, 10, 9)):
        assert ws(*bad) < 0, bad
        assert lib.mtts_last_error()
    assert b"Tx" in lib.mtts_last_error()


def test_host_visible_refusals_need_no_device(lib):
    """Null pointers and bad shapes are turned away before anything is launched (a fake non-null pointer is never dereferenced)."""
    p = C.c_void_p(256)
    assert lib.mtts_mas(None, None, None, p, p, 1, 20, 4, 8, p, None, None, p, 1 << 30, None) == -1
    assert b"log-prior" in lib.mtts_last_error()
    assert lib.mtts_mas(p, None, None, None, p, 1, 20, 4, 8, p, None, None, p, 1 << 30, None) == -1
    assert lib.mtts_mas(p, None, None, p, p, 0, 20, 4, 8, p, None, None, p, 1 << 30, None) == -1
    assert lib.mtts_mas(p, None, None, p, p, 1, 20, 1025, 2000, p, None, None, p, 1 << 30, None) == -1
    assert lib.mtts_mas(p, None, None, p, p, 1, 20, 9, 8, p, None, None, p, 1 << 30, None) == -1
    assert b"Tm < Tx" in lib.mtts_last_error()
    assert lib.mtts_mas(p, None, None, p, p, 1, 20, 4, 8, p, None, None, p, 16, None) == -1
    assert b"workspace" in lib.mtts_last_error()
    assert lib.mtts_mas_logprior(None, p, p, p, 1, 20, 4, 8, p, None) == -1
    assert lib.mtts_mas_logprior(p, p, p, p, 1, 0, 4, 8, p, None) == -1
    assert lib.mtts_mas_status(None, None) == -1
    assert lib.mtts_durations_given(None, p, 1.0, None, None, 1, 4, p, p, p, None) == -1
    assert lib.mtts_durations_given(p, p, 1.0, None, None, 0, 4, p, p, p, None) == -1


@pytest.mark.parametrize("kind", ["normal", "integer", "constant"])
def test_restatement_equals_brute_force(kind):
    rng = np.random.default_rng(5)
    n = 0
    for Tx in range(1, 6):
        for Tm in range(Tx, 10):
            for _ in range(3):
                if kind == "normal":
                    lp = rng.standard_normal((Tx, Tm)).astype(np.float32)
                elif kind == "integer":
                    lp = rng.integers(-2, 2, size=(Tx, Tm)).astype(np.float32)        # ties everywhere
                else:
                    lp = np.zeros((Tx, Tm), dtype=np.float32)                        # every path ties
                dur, path, score = R.maximum_path(lp)
                best, best_d = R.brute_force(lp)
                assert score == best, (Tx, Tm)
                assert np.array_equal(dur, best_d), (Tx, Tm, lp)
                assert dur.sum() == Tm and (dur >= 1).all()
                assert np.array_equal(path.sum(1).astype(np.int32), dur) and (path.sum(0) == 1).all()
                starts = np.concatenate([[0], np.cumsum(dur)[:-1]])
                for x in range(Tx):
                    assert path[x, starts[x]:starts[x] + dur[x]].all()
                n += 1
    assert n > 100


def test_restatement_ragged_ignores_padding():
    rng = np.random.default_rng(6)
    lp = rng.standard_normal((7, 20)).astype(np.float32)
    dur, path, score = R.maximum_path(lp[:4, :11])
    poisoned = lp.copy()
    poisoned[4:, :] = np.nan
    poisoned[:, 11:] = np.nan
    dur2, path2, score2 = R.maximum_path(poisoned, 4, 11)
    assert np.array_equal(dur2[:4], dur) and (dur2[4:] == 0).all() and score2 == score
    assert np.array_equal(path2[:4, :11], path) and path2[4:].sum() == 0 and path2[:, 11:].sum() == 0


def test_restated_log_prior_and_planted_alignment():
    rng = np.random.default_rng(7)
    mu = rng.standard_normal((20, 9))
    d = rng.integers(1, 13, size=9)
    y = R.expand(mu, d)
    lp = R.log_prior(mu, y)
    direct = -0.5 * ((y[:, None, :] - mu[:, :, None]) ** 2).sum(0)
    assert np.abs(lp - direct).max() <= 1e-10
    dur, _, score = R.maximum_path(lp)
    assert np.array_equal(dur, d) and abs(score) <= 1e-9


def test_request_durations_round_trip_through_plan_batch():
    bt = sub("batcher")
    given = [3.0, 0.0, 7.0]
    reqs = [bt.Request(ids=[1, 2, 3], durations=given), bt.Request(ids=[4, 5, 6, 7]), bt.Request(ids=[1, 2], solver="euler"),
            bt.Request(ids=[9, 9, 9], durations=(1, 2, 3))]
    assert bt.Request(ids=[1]).durations is None
    take = bt.plan_batch(reqs, max_batch=8, max_tokens=64)
    assert take == [0, 1, 3]                                   # grouping is by (solver, n_timesteps): durations do not split a batch
    assert reqs[take[0]].durations is given and reqs[take[1]].durations is None and tuple(reqs[take[2]].durations) == (1, 2, 3)
    assert reqs[0].group == reqs[1].group
    rows = bt.duration_rows([reqs[i] for i in take])
    assert rows == [given, None, (1, 2, 3)]
    assert bt.duration_rows([reqs[1]]) is None                 # nobody brings durations: the predictor's path, as before
    with pytest.raises(ValueError, match="durations"):
        bt.duration_rows([bt.Request(ids=[1, 2, 3], durations=[1.0, 2.0])])

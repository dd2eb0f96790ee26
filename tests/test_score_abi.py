"""Scoring without a GPU: the new C entries and their host-side refusals, the restatement of the three training-forward losses
against closed forms worked out by hand, and the two Huber thresholds in the hyper-parameters."""
import ctypes as C
import math
from types import SimpleNamespace as NS

import pytest
import torch

from conftest import ROOT, sub
import score_restated as S

NEW = {"mtts_decoder_forward_rows": 11, "mtts_cfm_loss": 15, "mtts_score_workspace_bytes": 3, "mtts_score_serial_run": 4,
       "mtts_score_prior_dur": 19, "mtts_score_status": 2}


@pytest.fixture(scope="module")
def lib():
    return sub("_hip").load()


def test_symbols_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_score_workspace_bytes.restype is C.c_int64
    for name in NEW:
        if name != "mtts_score_workspace_bytes":
            assert getattr(lib, name).restype is C.c_int, name
    assert lib.mtts_abi_version() == 2
    assert "MTTS_ABI_VERSION 2" in header and "MTTS_IMAGE_REVISION 7" in header
    assert "score.hip" in sub("_hip").SOURCES
    hip = sub("_hip").HipModel
    for method in ("decoder_forward_rows", "cfm_loss", "score_prior_dur", "score_status"):
        assert callable(getattr(hip, method))
    assert callable(sub("modules").CFM.compute_loss) and callable(sub("inference").MatchaTTSInfer.score)
    # the header states what the reference's x_mask factor becomes here
    assert "huber(0 - 0) = 0" in header


def test_workspace_bytes_and_serial_runs(lib):
    ws = lib.mtts_score_workspace_bytes
    sizes = [ws(B, 128, Tm) for B, Tm in ((1, 128), (1, 2000), (5, 2000), (32, 2000), (32, 8000))]
    assert all(v > 0 for v in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert ws(32, 128, 2000) >= 32 * math.ceil(2000 / 64) * 4                        # one partial per 64 frames
    for bad in ((0, 10, 20), (-1, 10, 20), (1, 0, 20), (1, 1025, 2000), (1, 10, 9)):
        assert ws(*bad) < 0, bad
        assert lib.mtts_last_error()
    # serial chains of the documented summation order, and the fp64 bound the GPU test derives from them
    run = lib.mtts_score_serial_run
    assert run(0, 100, 300, 2000) == 7 + 16 + 1 and run(1, 100, 300, 2000) == 5 and run(2, 100, 0, 1000) == 4 + 4 + 2
    assert run(3, 1, 1, 1) == -1
    for which, n in ((0, 100 * 2000), (1, 300), (2, 100 * 1000)):
        r = run(which, 100, 300, 2000 if which < 2 else 1000)
        assert 2 * (r + math.log2(max(n / r, 1)) + 4) * 2.0 ** -24 <= 1e-5


def test_host_visible_refusals_need_no_device(lib):
    """Null pointers and bad shapes are turned away before anything is launched (a fake non-null pointer is never dereferenced)."""
    p = C.c_void_p(256)
    big = 1 << 30

    def score(mu=p, logw=p, dur=p, y=p, xl=p, yl=p, B=2, F=20, Tx=4, Tm=8, dp=0.15, dd=0.3, ps=p, ds=p, ws=p, n=big):
        return lib.mtts_score_prior_dur(mu, logw, dur, y, xl, yl, B, F, Tx, Tm, dp, dd, ps, ds, None, None, ws, n, None)

    for kw in (dict(mu=None), dict(logw=None), dict(dur=None), dict(y=None), dict(xl=None), dict(yl=None), dict(ps=None),
               dict(ds=None), dict(ws=None)):
        assert score(**kw) == -1 and b"null" in lib.mtts_last_error(), kw
    assert score(B=0) == -1 and b"B must be" in lib.mtts_last_error()
    assert score(F=0) == -1
    assert score(Tx=1025, Tm=2000) == -1 and b"1024" in lib.mtts_last_error()
    assert score(Tx=9, Tm=8) == -1 and b"Tm < Tx" in lib.mtts_last_error()
    assert score(dp=0.0) == -1 and b"threshold" in lib.mtts_last_error()
    need = lib.mtts_score_workspace_bytes(2, 4, 8)
    assert score(n=need - 1) == -1 and b"workspace" in lib.mtts_last_error()
    assert lib.mtts_score_status(None, None) == -1
    # the estimator entries: null pointers and B < 1 are refused before the context is looked at
    assert lib.mtts_decoder_forward_rows(None, p, p, p, None, 1, 8, p, p, big, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_decoder_forward_rows(None, p, p, p, p, 0, 8, p, p, big, None) == -1
    assert lib.mtts_decoder_forward_rows(None, p, p, p, p, 1, 8, p, p, big, None) == -1 and b"context" in lib.mtts_last_error()
    assert lib.mtts_cfm_loss(None, p, p, p, None, p, 1, 1e-4, 1, 8, p, None, p, big, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_cfm_loss(None, p, p, p, p, None, 1, 1e-4, 1, 8, p, None, p, big, None) == -1
    assert lib.mtts_cfm_loss(None, p, p, p, p, p, 1, 1e-4, 0, 8, p, None, p, big, None) == -1 and b"B >= 1" in lib.mtts_last_error()
    assert lib.mtts_cfm_loss(None, p, p, p, p, p, 1, 1.5, 1, 8, p, None, p, big, None) == -1 and b"sigma_min" in lib.mtts_last_error()
    assert lib.mtts_cfm_loss(None, p, p, p, p, p, 1, 1e-4, 1, 8, p, None, p, big, None) == -1 and b"context" in lib.mtts_last_error()


# ------------------------------------------------------------------------------------------------ closed forms
# 2 tokens x 5 fine frames x 3 features.  Token 0 is the zero vector with 2 frames, token 1 the ones vector with 3 frames.
E = torch.tensor([[0.1, 0.5, 0.0, -0.3, 0.1],
                  [0.0, 0.0, 0.1, 0.0, 0.0],
                  [-0.1, 0.0, 0.0, 0.5, 0.0]], dtype=torch.float64)
MU_X = torch.tensor([[0.0, 1.0]] * 3, dtype=torch.float64)[None]
DUR = torch.tensor([[2, 3]])
Y_FINE = (torch.repeat_interleave(MU_X[0], DUR[0], dim=1) + E)[None]


def test_prior_loss_by_hand():
    # delta 0.15: |0.1| -> 0.5 * 0.01 = 0.005 (four of them); |0.5| -> 0.15 * (0.5 - 0.075) = 0.06375 (two); |0.3| -> 0.15 * 0.225 = 0.03375
    want_sum = 4 * 0.005 + 2 * 0.06375 + 0.03375
    padded = torch.nn.functional.pad(Y_FINE, (0, 3), value=7.0)                      # padding beyond the length is masked out
    loss, sums, frame, mu_y_fine = S.prior_loss(MU_X, DUR, padded, [5], 0.15)
    assert torch.equal(mu_y_fine[0, :, :5], torch.repeat_interleave(MU_X[0], DUR[0], dim=1)) and (mu_y_fine[0, :, 5:] == 0).all()
    assert abs(float(sums[0]) - want_sum) < 1e-14 and abs(float(loss) - want_sum / 5) < 1e-14
    want_frame = [0.005 + 0.005, 0.06375, 0.005, 0.03375 + 0.06375, 0.005, 0, 0, 0]
    assert torch.allclose(frame[0], torch.tensor(want_frame, dtype=torch.float64), atol=1e-14, rtol=0)
    # and the search finds these durations from the recording
    dur, score = S.mas_durations(MU_X, Y_FINE, [2], [5])
    assert torch.equal(dur, DUR)
    assert abs(float(score[0]) + 0.5 * float((E ** 2).sum())) < 1e-12


def test_duration_loss_by_hand():
    # delta 0.3: error 0.2 -> 0.5 * 0.04 = 0.02; error -1.0 -> 0.3 * (1.0 - 0.15) = 0.255
    logw = torch.log(2 + DUR.double())[:, None, :] + torch.tensor([0.2, -1.0], dtype=torch.float64)
    loss, sums, err = S.duration_loss(logw, DUR, [2], 0.3)
    assert abs(float(sums[0]) - 0.275) < 1e-14 and abs(float(loss) - 0.1375) < 1e-14
    assert torch.allclose(err[0], torch.tensor([0.2, -1.0], dtype=torch.float64), atol=1e-14, rtol=0)
    # a padded token contributes huber(0 - 0) = 0: the encoder masks logw, the reference masks log(2 + d)
    padded = torch.nn.functional.pad(logw, (0, 2))
    loss2, sums2, err2 = S.duration_loss(padded, torch.nn.functional.pad(DUR, (0, 2)), [2], 0.3)
    assert float(loss2) == float(loss) and float(sums2[0]) == float(sums[0]) and (err2[0, 2:] == 0).all()


@pytest.mark.parametrize("use_mu_prior,y_t,d", [(False, 2.0, 0.5), (True, 2.75, 1.0)])
def test_flow_matching_loss_by_hand(use_mu_prior, y_t, d):
    # sigma_min 0.5, t 0.5, x1 = 1, noise = 2, mu = 1, a stub estimator that answers 0.5 on the 3 valid of 4 frames:
    #   no mu prior: x0 = 2, u = 1 - 0.5 * 2 = 0,    y_t = 0.75 * 2 + 0.5 = 2.0,  (0.5 - 0)^2 * 9 / 9 = 0.25
    #   mu prior:    x0 = 3, u = 1 - 0.5 * 3 = -0.5, y_t = 0.75 * 3 + 0.5 = 2.75, (0.5 + 0.5)^2 * 9 / 9 = 1
    x1 = torch.ones(1, 3, 4, dtype=torch.float64)
    mask = torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=torch.float64)[None, None]
    seen = {}

    def estimator(y, m, mu, t):
        seen["y"], seen["t"] = y, t
        return 0.5 * torch.ones_like(y)                                             # (unmasked: the loss masks both sides)

    loss, sums, pred = S.cfm_loss(estimator, x1, mask, x1.clone(), torch.tensor([0.5]), 2 * x1, use_mu_prior, 0.5)
    assert (seen["y"] == y_t).all() and seen["t"].shape == (1,)
    assert abs(float(sums[0]) - 9 * d * d) < 1e-14 and abs(float(loss) - d * d) < 1e-14


def test_hparams_read_the_two_thresholds(hparams):
    assert hparams.loss_thresholds({"prior_loss_threshold": 0.15, "duration_loss_threshold": 0.3}) == (0.15, 0.3)
    assert hparams.loss_thresholds({}) == (0.03, 1.0) and hparams.loss_thresholds(None) == (0.03, 1.0)
    assert hparams.loss_thresholds(NS(prior_loss_threshold=0.2)) == (0.2, 1.0)
    kw = hparams.tiny().as_reference_kwargs()
    assert kw["prior_loss_threshold"] == 0.03 and kw["duration_loss_threshold"] == 1.0
    kw.update(prior_loss_threshold=0.15, duration_loss_threshold=0.3)
    hp = hparams.from_reference_kwargs(**kw)
    assert (hp.prior_loss_threshold, hp.duration_loss_threshold) == (0.15, 0.3)
    kw.pop("prior_loss_threshold")
    kw.pop("duration_loss_threshold")
    hp = hparams.from_reference_kwargs(**kw, optimizer=None)
    assert (hp.prior_loss_threshold, hp.duration_loss_threshold) == (0.03, 1.0)
    v20 = hparams.prod_v20()
    assert (v20.prior_loss_threshold, v20.duration_loss_threshold) == (0.15, 0.3)
    model = sub("inference").MatchaTTSInfer(**{**hparams.tiny().as_reference_kwargs(), "prior_loss_threshold": 0.15})
    assert model.hp.prior_loss_threshold == 0.15 and model.hp.duration_loss_threshold == 1.0

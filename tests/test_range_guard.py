"""The host logic that every model-level call shares, driven without a device: the range guard (``Runtime.guarded``) on a stub in
place of ``HipModel``, the voice resolver and the clip-list helper of the recording entries."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import sub

POLICIES = ["rerun", "raise", "ignore"]


class StubHip:
    def __init__(self, terms=2, saturate=False):
        self.terms, self.saturate = terms, saturate

    def gemm_terms(self):
        return self.terms

    def weights_saturate(self):
        return self.saturate

    def speaker_embedding(self, table, ids):
        return (ids.to(torch.float32) + 100 * table)[:, None].expand(-1, 4)


def runtime(terms=2, weights=False):
    """A Runtime whose ``ready()`` hands the narrow stub back, and the wide one once ``use_wide`` is set."""
    rt = sub("modules").Runtime(SimpleNamespace(mel_mean=0.0, mel_std=1.0), owner=None)
    rt.hip, rt.wide, rt.dirty = StubHip(terms, weights), StubHip(6), False
    return rt


class Call:
    """One guarded call: ``run`` notes the arithmetic it ran on and returns its own number, ``verdict`` counts its reads."""

    def __init__(self, rt, flag=False, timeout=False):
        self.rt, self.flag, self.timeout = rt, flag, timeout
        self.runs, self.reads = [], 0

    def run(self):
        hip = self.rt.ready()
        assert hip is (self.rt.wide if self.rt.use_wide else self.rt.hip)
        self.runs.append(hip.gemm_terms())
        return len(self.runs)

    def verdict(self, out):
        assert out == len(self.runs)
        self.reads += 1
        return self.flag, self.timeout

    def __call__(self, policy, **kw):
        return self.rt.guarded(policy, self.run, self.verdict, **kw)


@pytest.mark.parametrize("policy", POLICIES)
def test_flag_clear(policy):
    c = Call(runtime())
    assert c(policy) == 1
    assert c.runs == [2] and c.reads == (0 if policy == "ignore" else 1) and not c.rt.use_wide


@pytest.mark.parametrize("policy", POLICIES)
def test_flag_set(policy):
    c = Call(runtime(), flag=True)
    if policy == "raise":
        with pytest.raises(FloatingPointError):
            c(policy)
        assert c.runs == [2] and c.reads == 1 and not c.rt.use_wide
    elif policy == "rerun":
        assert c(policy) == 2                  # the second run's result
        assert c.runs == [2, 6] and c.reads == 1 and c.rt.use_wide
    else:
        assert c(policy) == 1
        assert c.runs == [2] and c.reads == 0 and not c.rt.use_wide


@pytest.mark.parametrize("policy", POLICIES)
def test_saturating_weights_skip_the_narrow_run(policy):
    c = Call(runtime(weights=True))
    if policy == "raise":
        with pytest.raises(FloatingPointError):
            c(policy)
        assert c.runs == [] and c.reads == 0
    elif policy == "rerun":
        assert c(policy) == 1
        assert c.runs == [6] and c.reads == 0 and c.rt.use_wide
    else:
        assert c(policy) == 1
        assert c.runs == [2] and c.reads == 0 and not c.rt.use_wide


def test_a_call_that_cannot_rerun_raises():
    c = Call(runtime(), flag=True)
    with pytest.raises(FloatingPointError):
        c("rerun", can_rerun=False)
    assert c.runs == [2] and not c.rt.use_wide


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("terms", [0, 3, 6, "wide"])
def test_nothing_is_read_where_nothing_saturates(policy, terms):
    rt = runtime() if terms == "wide" else runtime(terms)
    rt.use_wide = terms == "wide"
    c = Call(rt, flag=True, timeout=True)
    assert c(policy) == 1
    assert len(c.runs) == 1 and c.reads == 0 and rt.use_wide == (terms == "wide")


@pytest.mark.parametrize("terms", [1, 2, 16, 17])
def test_every_fp16_based_arithmetic_is_guarded(terms):
    c = Call(runtime(terms), flag=True)
    assert c("rerun") == 2 and c.runs == [terms, 6]


@pytest.mark.parametrize("policy", ["rerun", "raise"])
def test_pair_timeout_raises_and_keeps_the_arithmetic(policy):
    c = Call(runtime(), flag=True, timeout=True)
    with pytest.raises(RuntimeError, match="timed out waiting for its partner"):
        c(policy)
    assert c.runs == [2] and not c.rt.use_wide


def test_the_switch_is_announced_once_per_model(capsys):
    rt = runtime()
    Call(rt, flag=True)("rerun")
    assert "three-term bf16 products" in capsys.readouterr().out
    rt.use_wide = False                        # (what new weights do: the model may saturate a second time)
    c = Call(rt, flag=True)
    assert c("rerun") == 2 and rt.use_wide
    assert capsys.readouterr().out == ""


# ------------------------------------------------------------------------------------------------ voice resolver
class VoiceModel:
    """What ``_voice_rows`` touches of a model: the runtime, ``mix_speakers`` and a parameter's device."""

    def __init__(self):
        inference = sub("inference")
        self._rt = runtime()
        self._voice_rows = inference.MatchaTTSInfer._voice_rows.__get__(self)
        self.mix_speakers = inference.MatchaTTSInfer.mix_speakers.__get__(self)

    def parameters(self):
        return iter([torch.zeros(1)])


def test_voice_rows_precedence():
    m, dev = VoiceModel(), torch.device("cpu")
    given = (torch.full((2, 4), 7.0), torch.full((2, 4), 8.0))
    mix = [(1, 0.5), (3, 0.5)]
    e, d = m._voice_rows(2, dev, 5, mix, given)
    assert e is given[0] and d is given[1]
    e, d = m._voice_rows(2, dev, 5, mix, None)
    assert torch.equal(e, torch.full((1, 4), 2.0)) and torch.equal(d, torch.full((1, 4), 102.0))
    e, d = m._voice_rows(2, dev, torch.tensor([5, 9]))
    assert torch.equal(e, torch.tensor([5.0, 9.0])[:, None].expand(-1, 4)) and torch.equal(d, e + 100)
    e, d = m._voice_rows(2, dev, 5)
    assert e.shape == (1, 4) and float(e[0, 0]) == 5.0 and float(d[0, 0]) == 105.0


def test_voice_rows_need_one_id_per_utterance():
    m = VoiceModel()
    with pytest.raises(ValueError, match="speaker must be an int or a LongTensor with one id per utterance"):
        m._voice_rows(2, torch.device("cpu"), torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="one id per utterance"):
        m._voice_rows(2, torch.device("cpu"), 0, None, (torch.zeros(3, 4), torch.zeros(3, 4)))


# ------------------------------------------------------------------------------------------------ clip list
def test_clip_list():
    clips = sub("inference").MatchaTTSInfer._clips
    rows = torch.arange(12.0).reshape(3, 4)
    out = clips(rows, 3, "align")
    assert len(out) == 3 and all(torch.equal(out[b], rows[b]) for b in range(3))
    one = torch.zeros(5)
    assert clips(one, 1, "align")[0] is one
    arr = np.zeros(5, dtype=np.float32)
    out = clips(arr, 1, "score")
    assert len(out) == 1 and out[0] is arr
    given = [one, arr]
    out = clips(given, 2, "score")
    assert len(out) == 2 and out[0] is one and out[1] is arr
    for who in ("align", "score", "speaker_grad"):
        with pytest.raises(ValueError, match=rf"{who} needs one clip per utterance \(2\), got 3"):
            clips(rows, 2, who)
    with pytest.raises(ValueError, match=r"align needs one clip per utterance \(2\), got 1"):
        clips(one, 2, "align")

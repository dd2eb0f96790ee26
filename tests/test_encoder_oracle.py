"""CPU checks of what tests/test_hip_encoder.py measures the text encoder against (tests/encoder_cases.py): the fp64 reference is
oracle.text_encoder_forward on doubles for every case, it agrees with the recording of the reference's own code
(tests/golden/tiny_encoder.npz) and with the fp32 oracle, and the precondition of the integer check on the durations holds with no
token left out.

Measured on the CPU: the fp32 oracle is within 1.9e-6 (mu_x) and 4.1e-6 (logw) of the fp64 one over all cases; 0 of 1 .. 457 valid tokens
per case sit inside the rounding band for both factor pairs (two cases take token ids of seed 2 for that, encoder_cases.SEED_X), with
frame counts up to 139."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
import encoder_cases as ec


def _t(a):
    return torch.from_numpy(np.asarray(a))


def maxabs(a, b):
    return (a.double() - b.double()).abs().max().item()


@pytest.mark.parametrize("enc,batch", ec.CASES)
def test_fp64_reference_is_double_masked_and_near_the_fp32_oracle(enc, batch, oracle):
    """The reference comes back as float64 (a silently fp32 intermediate would make it no reference), its mask is sequence_mask, it is
    exactly 0 at padded tokens, and the fp32 oracle sits within half of the GPU bar of it: the 2e-5 bar then measures the kernels, not
    the fp32 formulation."""
    hp, _ = ec.weights(enc)
    x, x_len, spk, e_enc, _ = ec.inputs(enc, batch)
    mu64, logw64, mask64 = ec.reference(enc, batch)
    mu32, logw32, mask32 = ec.reference(enc, batch, torch.float32)
    B, Tx = x.shape
    assert mu64.dtype == logw64.dtype == mask64.dtype == torch.float64 and mu32.dtype == logw32.dtype == torch.float32
    assert mu64.shape == (B, hp.n_feats, Tx) and logw64.shape == (B, 1, Tx)
    assert torch.isfinite(mu64).all() and torch.isfinite(logw64).all()
    want = oracle.sequence_mask(x_len, Tx).unsqueeze(1)
    assert torch.equal(mask64.bool(), want) and torch.equal(mask32.bool(), want)
    assert len(set(spk.tolist())) == min(B, hp.n_spks)                  # a different speaker per row where n_spks allows
    padded = ~want
    assert bool(padded.any()) == (len(set(ec.BATCHES[batch])) > 1)
    assert bool((logw64[padded] == 0).all()) and bool((mu64[padded.expand_as(mu64)] == 0).all())
    e_mu, e_logw = maxabs(mu32, mu64), maxabs(logw32, logw64)
    print(f"encoder oracle {enc} {batch}: fp32 vs fp64 max|mu_x| {e_mu:.3e} max|logw| {e_logw:.3e} "
          f"(max |mu_x| {float(mu64.abs().max()):.2f}, |logw| {float(logw64.abs().max()):.2f})")
    assert e_mu < 0.5 * ec.MU_BAR and e_logw < 0.5 * ec.LOGW_BAR, (e_mu, e_logw)


def test_fp64_reference_vs_recording_of_the_reference(oracle, synthetic):
    """The same fp64 call on the inputs of tests/golden/tiny_encoder.npz against what the reference's own code recorded (fp32, with the
    constant-duration weights of synthetic.make_state_dict(hp, seed=7)), at test_oracle_golden's tolerance."""
    hp, _ = ec.weights("tiny")
    sd = synthetic.make_state_dict(hp, seed=7)
    g = np.load(GOLDEN / "tiny_encoder.npz")
    spk = _t(g["speakers"])
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        mu, logw, mask = oracle.text_encoder_forward(sd64, hp, _t(g["x"]), _t(g["x_lengths"]), sd64["speaker_embeddings_enc.weight"][spk],
                                                     sd64["speaker_embeddings_dur.weight"][spk], use_torch_sdpa=False)
    assert mu.dtype == logw.dtype == torch.float64
    assert torch.equal(mask.float(), _t(g["x_mask"]).float())
    assert maxabs(mu, _t(g["mu_x"])) < 1e-5 and maxabs(logw, _t(g["logw"])) < 1e-5


@pytest.mark.parametrize("sc,ls", ec.FACTORS)
@pytest.mark.parametrize("enc,batch", ec.CASES)
def test_no_token_sits_in_the_rounding_band(enc, batch, sc, ls, oracle):
    """encoder_cases.rounding_band: no valid token's fp64 duration is close enough to a half-integer for a logw inside the 2e-5 bar to
    flip its frame count, so the GPU test may ask for equal integers on every token.  The cap on excluded tokens is zero."""
    _, logw64, mask = ec.reference(enc, batch)
    bad, valid, frames = ec.rounding_band(logw64, mask, sc, ls)
    d = oracle.durations_from_logw(logw64, mask, sc, ls)
    assert d.dtype == torch.float64 and bool((d == d.round()).all()) and bool((d[mask.squeeze(1) > 0] >= 1).all())
    assert valid == sum(ec.BATCHES[batch]) and int(d.max()) == frames
    print(f"encoder oracle {enc} {batch} sc={sc} ls={ls}: {bad} of {valid} tokens in the rounding band, frame counts up to {frames}")
    assert bad == 0


def test_durations_vary_per_token():
    """Not the constant-duration recipe: the duration check sees many different frame counts."""
    _, logw64, mask = ec.reference("production", "three")
    assert float(logw64[0, 0, :129].std()) > 0.3

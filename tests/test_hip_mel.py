"""GPU parity of the log-mel front end (mtts_melfe_forward through mel.py) against the fp64 CPU restatement
(torch.stft(center=True, reflect, hann) -> abs -> HTK filterbank -> log(clamp))."""
import math

import pytest
import torch

from conftest import sub
import enroll_restated as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mel():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("mel")


def run(mel, clips, hop, mean=0.0, std=1.0, **kw):
    lengths = [int(c.numel()) for c in clips]
    audio = torch.zeros(len(clips), (max(lengths) + 3) // 4 * 4)
    for b, c in enumerate(clips):
        audio[b, :lengths[b]] = c
    out, n = mel.extract(audio.cuda(), lengths, hop, mean, std, **kw)
    torch.cuda.synchronize()
    return out.cpu(), n.cpu().tolist()


def lin_excess(out_log, lin):
    """Largest excess of |exp(out) - mel| over its bound 2e-4 * mel + 2e-4: relative where a band carries energy, absolute near
    the floor (a DFT output's error is set by the frame's energy, not by the bin's own magnitude -- in any fp32 transform)."""
    lin = lin.clamp(min=1e-7)
    return ((out_log.double().exp() - lin).abs() - (2e-4 * lin + 2e-4)).max().item()


@pytest.mark.parametrize("hop", [128, 256])
def test_white_noise_matches_fp64(mel, hop):
    y = R.synthetic_clip(24000, 1, "noise")
    out, n = run(mel, [y], hop)
    ref = R.log_mel(y, hop)
    assert n == [24000 // hop + 1] and out.shape == (1, 100, n[0])
    err = (out[0].double() - ref).abs().max().item()
    # the rule of tests/test_hip_kernels_frontend.py in place of the fixed 2e-4: 8 x the error of the same pipeline as fp32 matrix
    # products on the CPU (frames x the library's basis table, its filterbank table, log) plus one fp32 ulp of the largest value; the
    # new bound must itself stay under the old one
    fe = mel.front_end()
    c32 = R.mel_from_mag(R.stft_mag(y, hop, 1024, torch.from_numpy(fe.basis())), torch.from_numpy(fe.filterbank())).T
    top = ref.abs().max().item()
    bound = 8 * (c32.double() - ref).abs().max().item() + 2.0 ** (math.floor(math.log2(top)) - 23)
    print(f"white noise hop {hop}: err {err:.3e}, bound {bound:.3e} (was 2e-4)")
    assert bound < 2e-4 and err <= bound, (err, bound)


@pytest.mark.parametrize("hop", [128, 256])
def test_sine_sweep_matches_fp64(mel, hop):
    """A sweep leaves most bands near the noise floor at any moment: the strong bands are held to the log-domain bound, every band
    to a bound on the magnitude itself (a DFT output carries an absolute error set by the frame's energy, in fp32 as here)."""
    y = R.synthetic_clip(36000, 2, "sweep")
    out, _ = run(mel, [y], hop)
    lin = R.mel_linear(y, hop)
    ref = torch.log(lin.clamp(min=1e-7))
    strong = lin >= 1.0
    assert strong.sum() > 1000
    err_log = (out[0].double() - ref)[strong].abs().max().item()
    assert err_log <= 2e-4, err_log
    assert lin_excess(out[0], lin) <= 0.0, lin_excess(out[0], lin)


def test_silent_tail_clamps(mel):
    """Frames wholly inside digital silence are exactly log(1e-7); the others follow the restatement."""
    y = R.synthetic_clip(24000, 3, "voiced")
    y[12000:] = 0.0
    out, n = run(mel, [y], 256)
    lin = R.mel_linear(y, 256)
    assert lin_excess(out[0], lin) <= 0.0, lin_excess(out[0], lin)
    silent = out[0][:, (12000 + 512) // 256 + 1:]
    assert silent.shape[1] > 30
    assert (silent.double().exp() - 1e-7).abs().max().item() <= 1e-6
    assert (silent - math.log(1e-7)).abs().max().item() <= 1e-5
    voiced = lin[:, :40] >= 1.0
    assert ((out[0][:, :40].double() - torch.log(lin[:, :40]))[voiced]).abs().max().item() <= 2e-4


def test_normalisation_and_n_mels(mel):
    y = R.synthetic_clip(9000, 4, "voiced")
    out, n = run(mel, [y], 128, -4.0, 2.0, n_mels=20)
    ref = R.log_mel(y, 128, -4.0, 2.0, n_mels=20)
    assert out.shape == (1, 20, 9000 // 128 + 1)
    strong = R.mel_linear(y, 128, n_mels=20) >= 1.0
    assert (out[0].double() - ref)[strong].abs().max().item() <= 2e-4


@pytest.mark.parametrize("hop", [128, 256])
def test_ragged_batch_rows_equal_batch_of_one_bitwise(mel, hop):
    clips = [R.synthetic_clip(n, 10 + i, k) for i, (n, k) in enumerate([(30000, "voiced"), (7777, "noise"), (18001, "sweep"), (1024, "noise")])]
    out, n = run(mel, clips, hop)
    assert n == [c.numel() // hop + 1 for c in clips]
    for b, c in enumerate(clips):
        solo, ns = run(mel, [c], hop)
        assert ns == [n[b]]
        assert torch.equal(out[b, :, :n[b]], solo[0]), b
        assert (out[b, :, n[b]:] == 0).all()
    again, _ = run(mel, clips, hop)
    assert torch.equal(out, again)


def test_length_is_trimmed_to_a_multiple_of_hop(mel):
    y = R.synthetic_clip(10000, 5, "voiced")            # 10000 = 39 * 256 + 16
    out, n = run(mel, [y], 256)
    cut, nc = run(mel, [y[:39 * 256]], 256)
    assert n == nc == [40]
    assert torch.equal(out, cut)


def test_reference_signature(mel):
    fn = mel.get_mel_extractor(hop_length=256)
    y = R.synthetic_clip(8192, 6, "noise")
    out = fn(y.cuda()[None])
    assert out.shape == (1, 100, 33)
    assert (out[0].cpu().double() - R.log_mel(y, 256)).abs().max().item() <= 2e-4


def test_short_clip_raises(mel):
    with pytest.raises(ValueError, match="reflect padding"):
        mel.extract(torch.zeros(1, 512).cuda(), [512], 256)
    with pytest.raises(ValueError, match="reflect padding"):
        mel.extract(torch.zeros(2, 4096).cuda(), [4096, 600], 128)      # 600 -> 512 after trimming

"""GPU parity of the style encoder's forward pass (mtts_style_forward through style.py) against the fp64 CPU restatement
(F.conv1d + ReLU, masked mean, two Linear layers)."""
import math

import pytest
import torch

from conftest import sub
import enroll_restated as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def style():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("style")


def make(style, cfg, seed):
    torch.manual_seed(seed)
    m = style.StyleEncoder(*cfg)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.cuda().eval(), sd


def inputs(n_feats, T, lengths, seed):
    mel = torch.randn(len(lengths), n_feats, T, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lengths):
        mel[b, :, n:] = float("nan")          # the padded part is never read as data
    return mel


@pytest.mark.parametrize("cfg", [(100, 256, 4, 96), (100, 128, 3, 96), (20, 32, 2, 16)])
def test_rows_match_fp64(style, cfg):
    model, sd = make(style, cfg, 5)
    lengths = [200, 157, 64, 1]
    mel = inputs(cfg[0], 200, lengths, 6)
    e_enc, e_dur = model(mel.cuda(), lengths=lengths)
    assert e_enc.shape == e_dur.shape == (4, cfg[3])
    # the rule of tests/test_hip_kernels_frontend.py in place of the fixed 1e-4: 8 x the error of the same operations in fp32 on the
    # CPU plus one fp32 ulp of the row's largest entry, which must itself stay under the old bound
    for b, n in enumerate(lengths):
        ref = R.style_rows(sd, torch.nan_to_num(mel[b]), n)
        c32 = R.style_rows(sd, torch.nan_to_num(mel[b]), n, dtype=torch.float32)
        for got, r, c in zip((e_enc[b], e_dur[b]), ref, c32):
            top = r.abs().max().item()
            bound = 8 * (c.double() - r).abs().max().item() + 2.0 ** (math.floor(math.log2(top)) - 23)
            err = (got.cpu().double() - r).abs().max().item()
            print(f"style rows {cfg} b={b}: err {err:.3e}, bound {bound:.3e} (was 1e-4)")
            assert bound < 1e-4 and err <= bound


def test_mask_argument_as_the_reference_passes_it(style):
    model, sd = make(style, (100, 256, 4, 96), 5)
    mel = inputs(100, 90, [90, 40], 7)
    mask = (torch.arange(90)[None, None, :] < torch.tensor([90, 40])[:, None, None]).float()
    a = model(torch.nan_to_num(mel).cuda(), mask.cuda())
    b = model(mel.cuda(), lengths=[90, 40])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_ragged_batch_equals_batch_of_one_and_runs_repeat(style):
    model, _ = make(style, (100, 256, 4, 96), 8)
    lengths = [300, 211, 97]
    mel = inputs(100, 300, lengths, 9)
    e_enc, e_dur = model(mel.cuda(), lengths=lengths)
    e_enc2, e_dur2 = model(mel.cuda(), lengths=lengths)
    assert torch.equal(e_enc, e_enc2) and torch.equal(e_dur, e_dur2)
    for b, n in enumerate(lengths):
        s_enc, s_dur = model(mel[b:b + 1, :, :n].contiguous().cuda())
        assert torch.equal(s_enc[0], e_enc[b]) and torch.equal(s_dur[0], e_dur[b]), b


def test_grouped_average_is_the_mean_of_the_rows(style):
    model, _ = make(style, (100, 256, 4, 96), 10)
    lengths = [120, 80, 101, 64, 33]
    group = [1, 0, 1, 2, 1]
    mel = inputs(100, 120, lengths, 11)
    rows_enc, rows_dur = model(mel.cuda(), lengths=lengths)
    g_enc, g_dur = model(mel.cuda(), lengths=lengths, group=group, n_groups=4)
    assert g_enc.shape == (4, 96)
    for g in range(3):
        idx = [b for b, x in enumerate(group) if x == g]
        assert (g_enc[g] - rows_enc[idx].mean(0)).abs().max().item() <= 1e-6
        assert (g_dur[g] - rows_dur[idx].mean(0)).abs().max().item() <= 1e-6
    assert (g_enc[3] == 0).all() and (g_dur[3] == 0).all()      # a voice without clips
    again = model(mel.cuda(), lengths=lengths, group=group, n_groups=4)
    assert torch.equal(again[0], g_enc) and torch.equal(again[1], g_dur)

"""The batched waveform tail on the GPU: ragged Vocos decode (mtts_vocos_decode_ragged), per-row peak normalisation and
trailing-silence trim lengths (mtts_waveform_finish), `inference.to_waveforms` and its use by the batcher.  Everything is
checked against what the per-request code gives on each utterance's exact-length mel (reference inference.py:246,260-287)."""
import importlib.util

import numpy as np
import pytest
import torch

from conftest import GOLDEN, sub

pytestmark = pytest.mark.gpu
HOP, WIN = 256, 240


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    import vocos_oracle
    syn = sub("synthetic")
    sd = syn.make_vocos_state_dict(seed=11)
    wrapper = sub("vocoder").load_model("cuda", state_dict=sd)
    return vocos_oracle, sd, wrapper, sub("inference")


def ragged_mel(lengths, T, seed, pad_fill=True):
    """mel [B, 100, T] in the range of a log-mel, its padding filled with large values that a kernel must not read as data."""
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn(len(lengths), 100, T, generator=g) * 2.0 - 4.0
    if pad_fill:
        for b, n in enumerate(lengths):
            mel[b, :, n:] = torch.randn(100, T - n, generator=g) * 50.0
    return mel


LENGTHS, T_MAX = [96, 61, 33, 2], 96


def test_ragged_decode_equals_separate_decodes(env):
    V, sd, wrapper, _ = env
    mel = ragged_mel(LENGTHS, T_MAX, 3)
    out = wrapper(mel.cuda(), torch.tensor(LENGTHS)).cpu()
    assert out.shape == (4, HOP * (T_MAX - 1))
    for b, n in enumerate(LENGTHS):
        solo = wrapper(mel[b:b + 1, :, :n].cuda()).cpu()[0]
        with torch.inference_mode():
            ref = V.decode(sd, mel[b:b + 1, :, :n])[0]
        L = HOP * (n - 1)
        tol = 2e-4 * max(1.0, ref.abs().max().item())
        assert (out[b, :L] - solo).abs().max().item() < tol, b
        assert (out[b, :L] - ref).abs().max().item() < tol, b
        assert torch.count_nonzero(out[b, L:]) == 0, b
    # non-finite padding stays out as well (the padded rows are selected away, not multiplied by zero)
    mel_nan = mel.clone()
    for b, n in enumerate(LENGTHS):
        mel_nan[b, :, n:] = float("nan")
    again = wrapper(mel_nan.cuda(), torch.tensor(LENGTHS).cuda()).cpu()
    assert torch.equal(again, out)


def test_decode_without_lengths_changes_the_end_of_a_short_row(env):
    """Negative control, and the reason the lengths argument exists: decoded over all T frames a short row's last frames see
    its neighbours' padding through nine seven-tap convolutions."""
    V, sd, wrapper, _ = env
    mel = ragged_mel(LENGTHS, T_MAX, 3)
    plain = wrapper(mel.cuda()).cpu()
    b, n = 1, LENGTHS[1]
    solo = wrapper(mel[b:b + 1, :, :n].cuda()).cpu()[0]
    L = HOP * (n - 1)
    tol = 2e-4 * max(1.0, solo.abs().max().item())
    assert (plain[b, L - 8 * HOP:L] - solo[L - 8 * HOP:]).abs().max().item() > 10 * tol
    # ... and also with a silent (zero) padding, which is what a padded batch usually carries
    mel0 = ragged_mel(LENGTHS, T_MAX, 3, pad_fill=False)
    mel0[b, :, n:] = 0.0
    plain0 = wrapper(mel0.cuda()).cpu()
    assert (plain0[b, L - 8 * HOP:L] - solo[L - 8 * HOP:]).abs().max().item() > tol


def test_full_length_rows_are_bit_identical_to_the_plain_decode(env):
    _, _, wrapper, _ = env
    mel = ragged_mel([77, 77, 77], 77, 5).cuda()
    assert torch.equal(wrapper(mel, [77, 77, 77]), wrapper(mel))


def test_length_one_is_empty_and_bad_lengths_raise(env):
    _, _, wrapper, inf = env
    mel = ragged_mel([40, 1], 40, 6).cuda()
    out = wrapper(mel, [40, 1])
    assert torch.count_nonzero(out[1]) == 0
    wavs = inf.to_waveforms(mel, [40, 1], wrapper)
    assert wavs[1].numel() == 0 and 0 < wavs[0].numel() <= HOP * 39
    with pytest.raises(ValueError, match=r"lengths\[1\] = 41"):
        wrapper(mel, [40, 41])
    with pytest.raises(ValueError, match=r"lengths\[0\] = 0"):
        wrapper(mel, torch.tensor([0, 41]).cuda())
    with pytest.raises(ValueError, match=r"mel_lengths\[1\] = 41"):
        inf.to_waveforms(mel, [40, 41], wrapper)
    assert torch.equal(wrapper(mel, [40, 1]), out)              # the context works on after a refused call


def stack_rows(rows, pad_value=0.0):
    """1-D tensors -> ([B, ld] with ld a multiple of 4, lengths)."""
    ld = (max(len(r) for r in rows) + 3) // 4 * 4
    a = torch.full((len(rows), max(ld, 4)), pad_value)
    for b, r in enumerate(rows):
        a[b, :len(r)] = r
    return a, torch.tensor([len(r) for r in rows])


def test_finish_matches_the_recorded_reference_trim_lengths(env, synthetic):
    _, _, _, inf = env
    spec = importlib.util.spec_from_file_location("make_golden", GOLDEN / "make_golden.py")
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    cases = mg.trim_cases(synthetic)
    g = np.load(GOLDEN / "trim.npz")
    assert {"all_silent", "threshold_equality", "loud_remainder_ignored", "nan_window_stops_the_run"} <= set(cases)
    for db in sorted({db for _, db in cases.values()}):
        names = [k for k, (_, d) in cases.items() if d == db]
        audio, lengths = stack_rows([cases[k][0] for k in names], pad_value=0.7)      # loud padding: must not be examined
        dev_audio = audio.cuda()
        out_len, scale = inf.finish_waveforms(dev_audio, lengths, silence_threshold_db=db)
        for k, n, s in zip(names, out_len.tolist(), scale.tolist()):
            assert n == int(g[f"len_{k}"]), (k, n)
            assert s == 1.0, k
        assert torch.equal(dev_audio.cpu().nan_to_num(), audio.nan_to_num())           # no peak above 1: nothing is touched


def torch_finish(row, db=-60.0):
    """The per-request code on one row: (normalised samples, kept length)."""
    inf = sub("inference")
    peak = row.abs().max()
    a = row / peak * 0.95 if peak > 1.0 else row
    return a, len(inf.trim_trailing_silence(a, db))


def test_peak_normalisation_is_bit_equal_to_torch(env):
    _, _, _, inf = env
    g = torch.Generator().manual_seed(9)
    rows = [torch.randn(5000, generator=g) * 0.8, torch.randn(3001, generator=g) * 0.1, torch.randn(4097, generator=g) * 0.05,
            torch.randn(2 * WIN + 3, generator=g) * 3.0]
    rows[1][1234] = -1.0                                        # peak exactly 1.0: untouched
    rows[1].clamp_(-1.0, 1.0)
    rows[0][-WIN * 3:] *= 1e-5                                  # a silent tail on the row that is scaled
    assert rows[0].abs().max() > 1 and rows[1].abs().max() == 1 and rows[2].abs().max() < 1 and rows[3].abs().max() > 1
    audio, lengths = stack_rows(rows, pad_value=9.0)            # a peak in the padding must not count
    dev_audio = audio.cuda()
    out_len, scale = inf.finish_waveforms(dev_audio, lengths)
    got = dev_audio.cpu()
    for b, r in enumerate(rows):
        want, keep = torch_finish(r)
        assert torch.equal(got[b, :len(r)], want), b
        assert torch.equal(got[b, len(r):], audio[b, len(r):]), b
        assert int(out_len[b]) == keep, b
        assert (float(scale[b]) == 1.0) == (float(r.abs().max()) <= 1.0), b
    assert int(out_len[0]) < 5000 and int(out_len[3]) == 2 * WIN + 3


@pytest.mark.parametrize("shape", ["one_long_row", "many_short_rows"])
def test_finish_on_the_chunked_grid(env, shape):
    _, _, _, inf = env
    g = torch.Generator().manual_seed(21)
    if shape == "one_long_row":
        r = torch.randn(1_500_003, generator=g) * 0.3
        r[700_001] = 2.5                                       # the peak sits in a chunk far from both ends
        r[-(40 * WIN + 3):] *= 1e-6
        rows = [r]
    else:
        rows = []
        for b in range(64):
            n = 300 + 97 * b
            r = torch.randn(n, generator=g) * (0.2 if b % 3 else 1.5)
            r[n - (b % 5) * WIN - n % WIN:] *= 1e-6
            rows.append(r)
    audio, lengths = stack_rows(rows)
    dev_audio = audio.cuda()
    out_len, _ = inf.finish_waveforms(dev_audio, lengths.cuda())
    got = dev_audio.cpu()
    for b, r in enumerate(rows):
        want, keep = torch_finish(r)
        assert torch.equal(got[b, :len(r)], want), b
        assert int(out_len[b]) == keep, b
    assert any(int(n) < len(r) for n, r in zip(out_len, rows))


def test_to_waveforms_is_reproducible_and_equals_the_per_request_tail(env):
    _, _, wrapper, inf = env
    lengths = [120, 75, 33, 8]
    mel = ragged_mel(lengths, 120, 12)
    mel[0, :, 100:120] = -11.5                                   # a quiet stretch at the end of the longest row
    dev_mel = mel.cuda()
    first = inf.to_waveforms(dev_mel, torch.tensor(lengths).cuda(), wrapper)
    second = inf.to_waveforms(dev_mel, lengths, wrapper)
    untrimmed = inf.to_waveforms(dev_mel, lengths, wrapper, trim=False)
    assert len(first) == 4 and all(a.dim() == 1 and a.device.type == "cpu" for a in first)
    for b, n in enumerate(lengths):
        assert torch.equal(first[b], second[b]), b
        one = dev_mel[b:b + 1, :, :n]
        want = inf.trim_trailing_silence(inf.to_waveform(one, wrapper))
        assert first[b].shape == want.shape, (b, first[b].shape, want.shape)
        assert (first[b] - want).abs().max().item() < 2e-4, b
        full = inf.to_waveform(one, wrapper)
        assert untrimmed[b].shape == full.shape and (untrimmed[b] - full).abs().max().item() < 2e-4, b


def test_batcher_uses_the_batched_tail(env, hparams, synthetic, monkeypatch):
    _, _, wrapper, inf = env
    bt = sub("batcher")
    hp = hparams.prod_v20(n_spks=10)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.cuda().eval()
    ids = [synthetic.make_inputs(hp, 1, n, seed=70 + i)[0][0].tolist() for i, n in enumerate([30, 22, 41])]

    def run(flag):
        if flag is None:
            monkeypatch.delenv("MTTS_WAVE_BATCH", raising=False)
        else:
            monkeypatch.setenv("MTTS_WAVE_BATCH", flag)
        with bt.FrameBudgetBatcher(model, max_batch=8, max_tokens=4096, max_wait_ms=200.0, vocoder=wrapper) as q:
            assert q.wave_batch == (flag != "0")
            futs = [q.submit(tok, speaker=3 * i, solver="midpoint", n_timesteps=2) for i, tok in enumerate(ids)]
            res = [f.result(timeout=120) for f in futs]
            assert q.batches_run == 1
        return res

    batched, looped = run(None), run("0")
    assert len({r["mel_length"] for r in batched}) > 1           # the batch is ragged
    for a, b in zip(batched, looped):
        assert set(a) == set(b) == {"mel", "mel_length", "audio"}
        assert a["mel_length"] == b["mel_length"] and torch.equal(a["mel"], b["mel"])
        assert a["audio"].device.type == "cpu" and a["audio"].dim() == 1 and a["audio"].dtype == torch.float32
        assert a["audio"].shape == b["audio"].shape
        if a["audio"].numel():
            assert (a["audio"] - b["audio"]).abs().max().item() < 2e-4

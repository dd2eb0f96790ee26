"""Loudness on the device (csrc/loudness.hip) against the NumPy fp64 restatement (tests/loudness_restated.py): every length at which
the kernels take another path, one row alone and seven in one ld, three rates, the gates, the ceiling, refusals, and the stage inside
``to_waveforms``.

Bounds.  ``lufs``: 1e-7 dB.  The worst-case fp64 accumulation over 2^21 samples is 2.3e-10 relative = 1e-9 dB; two orders are left
for the rounding of the carried state (2e-13 absolute on rms 0.09).  ``gain``: one fp32 unit in the last place of the restated gain
(the device's pow and the restatement's may round the fp64 value to different neighbours).  Samples: ``fl32(x * gain_device)`` bit
for bit.  No test rests on a gate flip: the restatement shows every block of every input at least 0.01 dB from both gates, and the
reference fixture asserts it."""
import math

import numpy as np
import pytest
import torch

from conftest import sub
import loudness_restated as lr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(7.25)
TILE = 61440                    # MTTS_LOUDNESS_TILE, asserted against the library below
CHUNK = 240
LENGTHS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2399, 2400, 9599, 9600, 11999, 12000, TILE - 1, TILE, TILE + 1, 4 * TILE + 3, 72000]


def am_noise(n, seed, rms=0.09, fs=24000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (rng.standard_normal(n) * rms * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t))).astype(np.float32)


def batch_rows():
    """Seven rows of one ld: (samples, length, target).  Length -1: a row refused upstream."""
    fs = 24000
    loud_quiet = am_noise(4 * fs, 11)
    loud_quiet[2 * fs:] *= np.float32(10 ** (-30 / 20))          # the relative gate drops the quiet half's blocks
    spiky = am_noise(fs, 15, rms=0.01)
    spiky[5000] = np.float32(0.9)                                 # -16 LUFS would push this peak over the ceiling
    return [(am_noise(3 * fs, 10), 3 * fs, -23.0),
            (loud_quiet, 4 * fs, -23.0),
            (np.zeros(30000, dtype=np.float32), 30000, -23.0),   # -inf, gain 1, bits untouched
            (am_noise(30000, 13, rms=1e-5), 30000, -23.0),       # under the absolute gate
            (spiky, fs, -16.0),
            (am_noise(5000, 16), -1, -23.0),
            (am_noise(1000, 17), 1000, math.nan)]                 # measure only


def restated(x, n, target, fs=24000):
    if n < 0:
        return dict(lufs=math.nan, gain=np.float32(1.0), peak=0.0, margin=math.inf)
    m = lr.measure(x[:n], fs)
    m["gain"] = lr.gain(m["lufs"], target, m["peak"], 0.95, n)
    return m


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    mod = sub("loudness")
    assert mod.TILE == TILE and mod.chunk(24000) == CHUNK
    return mod


@pytest.fixture(scope="module")
def ref():
    """The restatement of every input, computed once; asserts the condition on the inputs (no block near a gate)."""
    out = {"single": {}, "batch": [], "rates": {}}
    for i, n in enumerate(LENGTHS):
        out["single"][n] = restated(am_noise(n, 100 + i), n, -20.0)
    out["batch"] = [restated(x, n, t) for x, n, t in batch_rows()]
    for fs in (8000, 24000, 48000):
        x = am_noise(int(1.5 * fs) + 7, 30, fs=fs)
        out["rates"][fs] = [restated(x, len(x), None, fs), restated(x, fs // 2 + 3, None, fs)]
    margins = [m["margin"] for m in list(out["single"].values()) + out["batch"] + sum(out["rates"].values(), [])]
    print(f"smallest distance of a block from a gate: {min(margins):.4f} dB")
    assert min(margins) >= 0.01
    return out


def device_rows(rows, ld=None):
    """Rows [(x, n, target)] as a sentinel-filled [B, ld] device tensor, its host copy, and the lengths."""
    ld = ld or max(4, (max(len(x) for x, _, _ in rows) + 3) // 4 * 4 + 8)
    host = np.full((len(rows), ld), SENTINEL, dtype=np.float32)
    for b, (x, n, _) in enumerate(rows):
        host[b, :len(x)] = x
    return torch.from_numpy(host.copy()).cuda(), host, [n for _, n, _ in rows]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_row(tag, want, lufs, gain, before, after, n, worst):
    if math.isnan(want["lufs"]) or math.isinf(want["lufs"]):
        assert (math.isnan(lufs) and math.isnan(want["lufs"])) or lufs == want["lufs"], (tag, lufs, want["lufs"])
    else:
        worst.append(abs(lufs - want["lufs"]))
        assert abs(lufs - want["lufs"]) <= 1e-7, (tag, lufs, want["lufs"])
    g = np.float32(gain)
    assert abs(float(g) - float(want["gain"])) <= float(np.spacing(want["gain"])), (tag, gain, want["gain"])
    n = max(n, 0)
    if g == np.float32(1.0):
        assert np.array_equal(bits(after[:n]), bits(before[:n])), tag
    else:
        assert np.array_equal(bits(after[:n]), bits(before[:n] * g)), tag          # one fp32 multiply per sample
    assert np.array_equal(bits(after[n:]), bits(before[n:])), tag                   # nothing beyond the length is written
    return g


# ------------------------------------------------------------------------------------------------ one row
@pytest.mark.parametrize("n", LENGTHS)
def test_one_row_at_every_length(L, ref, n):
    i = LENGTHS.index(n)
    audio, host, lengths = device_rows([(am_noise(n, 100 + i), n, -20.0)])
    lufs, gain, peak = L.normalize(audio, lengths, -20.0)
    worst = []
    want = ref["single"][n]
    check_row(n, want, float(lufs[0]), float(gain[0]), host[0], audio[0].cpu().numpy(), n, worst)
    assert float(peak[0]) == np.float32(want["peak"])
    if worst:
        print(f"length {n}: lufs {float(lufs[0]):.9f}, |device - restated| = {worst[0]:.3e} dB")
    if n >= 2400:
        assert gain[0] != 1.0                                     # (the row was levelled: nothing above is vacuous)


# ------------------------------------------------------------------------------------------------ seven rows in one ld
def test_batch_of_seven_matches_rows_alone_and_the_restatement(L, ref):
    rows = batch_rows()
    targets = [t for _, _, t in rows]
    audio, host, lengths = device_rows(rows)
    with pytest.raises(ValueError, match=r"row 5 \(length -1\)"):
        L.normalize(audio.clone(), lengths, targets)              # the verdict names the refused row ...
    lufs, gain, peak = L.normalize(audio, lengths, targets, check=False)          # ... and without the wait the others are right
    lufs, gain, peak, after = lufs.cpu().tolist(), gain.cpu().numpy(), peak.cpu().numpy(), audio.cpu().numpy()
    worst = []
    for b, (x, n, t) in enumerate(rows):
        check_row(b, ref["batch"][b], lufs[b], gain[b], host[b], after[b], n, worst)
    print(f"batch of 7: largest |device - restated| = {max(worst):.3e} dB; lufs {lufs}")
    assert lufs[2] == -math.inf and lufs[3] == -math.inf and math.isnan(lufs[5])
    assert gain[2] == gain[3] == gain[5] == gain[6] == 1.0 and math.isfinite(lufs[6])
    assert np.array_equal(bits(after[5]), bits(host[5]))          # the refused row is not touched
    # the relative gate dropped blocks of row 1; the ceiling bound on row 4
    assert min(ref["batch"][1]["blocks"]) < ref["batch"][1]["gate"]
    assert gain[4] == np.float32(0.95) / peak[4] or gain[4] == np.nextafter(np.float32(0.95) / peak[4], np.float32(0))
    assert np.abs(after[4, :lengths[4]]).max() <= np.float32(0.95) and peak[4] == np.float32(0.9)
    assert float(gain[4]) < 10 ** ((-16.0 - lufs[4]) / 20.0)
    # each row alone: the same lufs, gain and bits
    for b, (x, n, t) in enumerate(rows):
        if n < 0:
            continue
        one, _, _ = device_rows([(x, n, t)])
        l1, g1, p1 = L.normalize(one, [n], [t])
        l1 = float(l1[0])
        assert (l1 == lufs[b] or (math.isnan(l1) and math.isnan(lufs[b]))) and float(g1[0]) == gain[b] and float(p1[0]) == peak[b], b
        assert np.array_equal(bits(one[0, :n].cpu().numpy()), bits(after[b, :n])), b
    # two calls give the same bits
    again, _, _ = device_rows(rows)
    l2, g2, _ = L.normalize(again, lengths, targets, check=False)
    assert np.array_equal(np.array(l2.cpu().tolist()).view(np.uint64), np.array(lufs).view(np.uint64))
    assert np.array_equal(bits(g2.cpu().numpy()), bits(gain)) and np.array_equal(bits(again.cpu().numpy()), bits(after))


def test_measure_leaves_the_audio_alone_and_needs_no_aligned_rows(L, ref):
    x, n, _ = batch_rows()[0]
    audio = torch.from_numpy(x[:n - 1].copy()).cuda()             # 1-D, an odd count: measured from a padded copy
    got = L.measure(audio)
    assert got.dtype == torch.float64 and got.shape == (1,)
    assert abs(float(got[0]) - lr.measure(x[:n - 1], 24000)["lufs"]) <= 1e-7
    assert np.array_equal(bits(audio.cpu().numpy()), bits(x[:n - 1]))
    with pytest.raises(ValueError, match="in place"):
        L.normalize(audio, None, -23.0)


@pytest.mark.parametrize("fs", [8000, 24000, 48000])
def test_measure_at_three_rates(L, ref, fs):
    x = am_noise(int(1.5 * fs) + 7, 30, fs=fs)
    lengths = [len(x), fs // 2 + 3]
    audio, host, _ = device_rows([(x, lengths[0], None), (x, lengths[1], None)])
    got = L.measure(audio, lengths, fs).cpu().tolist()
    for b in range(2):
        want = ref["rates"][fs][b]["lufs"]
        print(f"fs {fs}, {lengths[b]} samples: {got[b]:.9f} LUFS, |device - restated| = {abs(got[b] - want):.3e} dB")
        assert abs(got[b] - want) <= 1e-7
    assert np.array_equal(bits(audio.cpu().numpy()), bits(host))


# ------------------------------------------------------------------------------------------------ through the interface
SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)             # tests/test_hip_vocos.py's second configuration


@pytest.fixture(scope="module")
def env(L, synthetic):
    inf, voc = sub("inference"), sub("vocoder")
    vocos = voc.Vocos(**SMALL)
    vocos.load_state_dict(synthetic.make_vocos_state_dict(seed=23, **{k: v for k, v in SMALL.items() if k != "hop"}), strict=True)
    mel = (torch.randn(4, SMALL["n_mels"], 40, generator=torch.Generator().manual_seed(3)) * 2.0 - 4.0).cuda()
    return inf, voc.VocosWrapper(vocos.to("cuda").eval()), mel, [40, 33, 25, 12]


def padded(rows):
    ld = (max(r.numel() for r in rows) + 3) // 4 * 4
    out = torch.zeros(len(rows), ld, dtype=torch.float32)
    for b, r in enumerate(rows):
        out[b, :r.numel()] = r
    return out.cuda(), [r.numel() for r in rows]


def test_to_waveforms_loudness_is_normalize_on_its_rows(L, env):
    inf, vocos, mel, lengths = env
    plain = inf.to_waveforms(mel, lengths, vocos)
    assert all(p.numel() > 0 for p in plain)
    levelled, report = inf.to_waveforms(mel, lengths, vocos, loudness=-23, return_loudness=True)
    rows, n = padded(plain)
    lufs, gain, _ = L.normalize(rows, n, -23.0)
    for b in range(4):
        assert torch.equal(levelled[b].view(torch.int32), rows[b, :n[b]].cpu().view(torch.int32)), b
        assert report[b] == (float(lufs[b]), float(gain[b])) and report[b][1] != 1.0
    # a target per row: a row without one keeps its bits
    mixed = inf.to_waveforms(mel, lengths, vocos, loudness=[-23, None, -30.0, None])
    assert torch.equal(mixed[0], levelled[0]) and torch.equal(mixed[1], plain[1]) and torch.equal(mixed[3], plain[3])
    assert not torch.equal(mixed[2], plain[2])
    # sample_rate=8000, encoding="ulaw": the stage ran ahead of the conversion and the encoder
    R, AC = sub("resample"), sub("audio_codec")
    coded = inf.to_waveforms(mel, lengths, vocos, loudness=-23, sample_rate=8000, encoding="ulaw")
    conv, n8 = R.resample(rows, torch.tensor(n, device="cuda"), 24000, 8000, check=False)
    data, nbytes = AC.encode(conv, n8, "ulaw")
    for b in range(4):
        assert coded[b].dtype == torch.uint8 and torch.equal(coded[b], data[b, :int(nbytes[b])].cpu()), b
    for bad in ("loud", 3.0, [-23.0, -23.0]):
        with pytest.raises((TypeError, ValueError)):
            inf.to_waveforms(mel, lengths, vocos, loudness=bad)


def test_documents_take_one_gain_each_and_land_on_the_target(L, env):
    inf, vocos, mel, lengths = env
    docs = dict(documents=[2, 2], gaps=[120, 0, 96, 0])
    plain, measured = inf.to_waveforms(mel, lengths, vocos, return_loudness=True, **docs)
    assert len(plain) == 2 and all(g == 1.0 and math.isfinite(l) for l, g in measured)
    targets = [measured[0][0] - 6.0, measured[1][0] - 9.0]       # attenuations: the ceiling cannot bind
    out, seg, report = inf.to_waveforms(mel, lengths, vocos, loudness=targets, return_loudness=True, return_segments=True, **docs)
    assert len(seg) == 2 and [r[0] for r in report] == [m[0] for m in measured]
    for g in range(2):
        gain = np.float32(report[g][1])
        assert np.array_equal(bits(out[g].numpy()), bits(plain[g].numpy() * gain)), g          # ONE gain per document
        got = float(L.measure(out[g].cuda())[0])
        print(f"document {g}: target {targets[g]:.6f}, measured after the gain {got:.6f}, residue {abs(got - targets[g]):.3e} dB")
        assert abs(got - targets[g]) <= 1e-3                      # the residue: fp32 rounding of the gain and the samples
    only, rep = inf.to_waveforms(mel, lengths, vocos, loudness=[None, targets[1]], return_loudness=True, **docs)
    assert torch.equal(only[0], plain[0]) and torch.equal(only[1], out[1]) and rep[0][1] == 1.0


def test_without_a_target_nothing_of_the_stage_runs(L, env):
    inf, vocos, mel, lengths = env
    lib = sub("_hip").load()
    L.measure(torch.zeros(1, 8).cuda())
    assert lib.mtts_last_kernel_tag().startswith(b"loud_")       # (the tag is this stage's while nothing else has launched)
    held = sub("loudness")._ws.bytes_held()
    plain = inf.to_waveforms(mel, lengths, vocos)
    same = inf.to_waveforms(mel, lengths, vocos, loudness=None)
    none = inf.to_waveforms(mel, lengths, vocos, loudness=[None] * 4)
    assert not lib.mtts_last_kernel_tag().startswith(b"loud_")
    assert sub("loudness")._ws.bytes_held() == held               # nothing new allocated
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(plain, same, none))

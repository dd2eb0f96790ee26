"""``mtts_loudness_r128`` on the device (csrc/loudness.hip) against the NumPy restatement (tests/r128_restated.py): the true peak bit
for bit at every length at which the true-peak pass takes another path, the halo at a tile edge, a NaN sample, the three
oversampling factors; ``lufs`` / ``peak`` / ``gain`` bit for bit against ``mtts_loudness``; the loudness range, the maximum momentary and
short-term loudness; batch independence; the gain with the true-peak ceiling; and the stage inside ``to_waveforms`` and the batcher.

Bounds.  True peak: bit-equal (fp32 products added in a fixed order, evaluated with the library's own table; a maximum has no order).
``lra``, ``momentary_max``, ``short_term_max``: 1e-7 dB, the bound ``lufs`` has in test_hip_loudness.py and for its reason: they are
log10 of the same fp64 sums (worst-case fp64 accumulation over 2^21 samples: 1e-9 dB).  ``gain``: one fp32 unit in the last place of
the restated gain.  Samples: ``fl32(x * gain_device)`` bit for bit.  True peak after the gain: at most ``c_tp (1 + 2^-19)`` -- the scaled
row's interpolated values are thirteen fp32 roundings (the sample's own, twelve products and sums less the first exact one) away
from ``g`` times the measured ones, 13 * 2^-24 < 2^-20 relative to the sum of the magnitudes, which for this filter is under 2 times
the value at a peak.  No test rests on a gate flip: every short-term block of every input is at least 0.01 dB from both gates of
the loudness range, and every 400 ms block from those of the integrated loudness; the reference fixture asserts it."""
import math

import numpy as np
import pytest
import torch

from conftest import sub
import loudness_restated as lr
import r128_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(7.25)
TILE = 4096                     # MTTS_TRUE_PEAK_TILE, asserted against the library below
LENGTHS = [0, 1, 5, 6, 7, 11, 12, 13, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
FS = 24000


def am_noise(n, seed, rms=0.09, fs=24000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (rng.standard_normal(n) * rms * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t))).astype(np.float32)


def figure_rows():
    """Eight rows of one ld: (samples, length).  Length -1: a row refused upstream."""
    two_levels = am_noise(8 * FS, 21)
    two_levels[4 * FS:] *= np.float32(10 ** (-12 / 20))                # LRA 12.03 LU, 51 blocks
    dip = am_noise(10 * FS, 22)
    dip[3 * FS:6 * FS] *= np.float32(10 ** (-35 / 20))                 # LRA 8.94 LU, 70 of 71 blocks above the gates
    return [(two_levels, 8 * FS), (dip, 10 * FS), (am_noise(4 * FS, 23), 4 * FS), (am_noise(int(2.9 * FS), 24), int(2.9 * FS)),
            (am_noise(int(0.3 * FS), 25), int(0.3 * FS)), (np.zeros(FS, dtype=np.float32), FS), (am_noise(100, 26), 0),
            (am_noise(5000, 27), -1)]


def halo_rows():
    """Rows whose true peak is interpolated (1.25 times the sample value and more) and needs the halo of a tile."""
    v = np.float32(0.4)
    astride = np.zeros(2 * TILE, dtype=np.float32)
    astride[TILE - 1:TILE + 1] = v                                     # the peak at TILE - 1/2: tile 0 reads x[TILE] from its halo
    last_two = np.zeros(TILE + 1, dtype=np.float32)
    last_two[TILE - 1:] = v                                            # the same at the row's end: tile 1 holds one sample
    left = np.zeros(TILE + 8, dtype=np.float32)
    left[TILE:TILE + 2] = v                                            # the peak at TILE + 1/2: tile 1 reads x[TILE - 1] from its halo
    left[TILE - 1] = left[TILE + 2] = np.float32(-0.3)
    return [astride, last_two, left]


def refused():
    return dict(lufs=math.nan, peak=0.0, true_peak=np.float32(0.0), lra=math.nan, momentary_max=math.nan, short_term_max=math.nan,
                margin=math.inf, base_margin=math.inf, n=0)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    mod = sub("loudness")
    assert mod.TRUE_PEAK_TILE == TILE
    return mod


@pytest.fixture(scope="module")
def tables(L):
    """The library's own interpolator tables, float32 [F, 12]."""
    out = {}
    for fs in (8000, 24000, 48000, 96000):
        F, h = L.true_peak_filter(fs)
        assert F == rr.factor(fs)
        out[fs] = h.numpy()
    return out


def restated(x, n, fs, table):
    if n < 0:
        return refused()
    m = rr.meter(x[:n], fs, table)
    m["base_margin"] = lr.measure(x[:n], fs)["margin"]
    return m


@pytest.fixture(scope="module")
def ref(tables):
    """The restatement of the loudness figures of every input, computed once; asserts the condition on the inputs."""
    out = {"figures": [restated(x, n, FS, tables[FS]) for x, n in figure_rows()], "rates": {}}
    for fs in (8000, 24000, 48000, 96000):
        x = am_noise(int(3.2 * fs) + 7, 30, fs=fs)
        out["rates"][fs] = restated(x, len(x), fs, tables[fs])
    every = out["figures"] + list(out["rates"].values())
    print(f"smallest distance of a short-term block from a gate: {min(m['margin'] for m in every):.4f} dB; "
          f"of a 400 ms block: {min(m['base_margin'] for m in every):.4f} dB")
    assert min(m["margin"] for m in every) >= 0.01 and min(m["base_margin"] for m in every) >= 0.01
    assert abs(out["figures"][0]["lra"] - 12.03) < 0.005 and out["figures"][0]["n"] == 51
    assert abs(out["figures"][1]["lra"] - 8.94) < 0.005 and out["figures"][1]["n"] == 70
    return out


def device_rows(rows, ld=None):
    """Rows [(x, n)] as a sentinel-filled [B, ld] device tensor, its host copy, and the lengths."""
    ld = ld or max(4, (max(len(x) for x, _ in rows) + 3) // 4 * 4 + 8)
    host = np.full((len(rows), ld), SENTINEL, dtype=np.float32)
    for b, (x, _) in enumerate(rows):
        host[b, :len(x)] = x
    return torch.from_numpy(host.copy()).cuda(), host, [n for _, n in rows]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(m):
    return {k: v.cpu().numpy() for k, v in m.items()}


def close(got, want, tag, worst):
    got = float(got)
    if math.isnan(want) or math.isinf(want):
        assert (math.isnan(got) and math.isnan(want)) or got == want, (tag, got, want)
    else:
        worst.append(abs(got - want))
        assert abs(got - want) <= 1e-7, (tag, got, want)


# ------------------------------------------------------------------------------------------------ true peak
@pytest.mark.parametrize("n", LENGTHS)
def test_true_peak_of_one_row_at_every_length(L, tables, n):
    x = am_noise(n, 200 + LENGTHS.index(n))
    audio, before, lengths = device_rows([(x, n)])
    m = host(L.meter(audio, lengths))
    want = rr.true_peak(x, FS, tables[FS])
    print(f"length {n}: true peak {float(m['true_peak'][0]):.9f}, sample peak {float(m['peak'][0]):.9f}")
    assert bits(m["true_peak"])[0] == bits(want)
    assert m["peak"][0] == (np.abs(x).max() if n else 0.0) and m["true_peak"][0] >= m["peak"][0]
    assert np.array_equal(bits(audio.cpu().numpy()), bits(before))            # a meter writes nothing


def test_true_peak_in_the_halo_of_a_tile(L, tables):
    rows = halo_rows()
    audio, _, lengths = device_rows([(x, len(x)) for x in rows])
    got = host(L.meter(audio, lengths))["true_peak"]
    for b, x in enumerate(rows):
        want = rr.true_peak(x, FS, tables[FS])
        print(f"halo row {b}: true peak {got[b]:.7f} = {got[b] / 0.4:.4f} x the sample value")
        assert bits(got[b]) == bits(want) and got[b] > 1.2 * 0.4
    # without its halo a tile would read 0.625 of the sample value at the midpoint, and the sample itself as the peak
    # (an ideal sinc reads 4 / pi = 1.27 there; the Hann window and the normalisation make it 1.2504)
    assert abs(got[0] / np.float32(0.4) - 1.2504) < 0.001 and got[0] == got[1]


def test_true_peak_passes_over_a_nan_sample(L, tables):
    x = am_noise(3000, 210)
    x[1234] = np.float32(math.nan)
    audio, _, lengths = device_rows([(x, len(x))])
    m = host(L.meter(audio, lengths))
    want = rr.true_peak(x, FS, tables[FS])
    assert math.isfinite(want) and want > 0 and bits(m["true_peak"])[0] == bits(want)
    assert m["peak"][0] == np.nanmax(np.abs(x))


@pytest.mark.parametrize("fs", [8000, 24000, 48000, 96000])
def test_every_oversampling_factor(L, tables, ref, fs):
    x = am_noise(int(3.2 * fs) + 7, 30, fs=fs)
    audio, _, lengths = device_rows([(x, len(x))])
    m = host(L.meter(audio, lengths, fs))
    want = ref["rates"][fs]
    assert bits(m["true_peak"])[0] == bits(want["true_peak"]) and tables[fs].shape == ({8000: 8, 24000: 8, 48000: 4, 96000: 2}[fs], 12)
    worst = []
    for key in ("lufs", "lra", "momentary_max", "short_term_max"):
        close(m[key][0], want[key], (fs, key), worst)
    print(f"fs {fs}: true peak {m['true_peak'][0]:.7f} ({L.dbtp(float(m['true_peak'][0])):.3f} dBTP), lra {m['lra'][0]:.6f}, "
          f"largest |device - restated| = {max(worst):.3e} dB")
    assert math.isfinite(m["short_term_max"][0]) and m["momentary_max"][0] >= m["short_term_max"][0]


# ------------------------------------------------------------------------------------------------ the loudness figures
def test_figures_match_the_restatement_and_mtts_loudness_bit_for_bit(L, ref):
    rows = figure_rows()
    targets = [-23.0, -20.0, None, -23.0, -23.0, -23.0, -23.0, -23.0]
    audio, before, lengths = device_rows(rows)
    plain, _, _ = device_rows(rows)
    with pytest.raises(ValueError, match=r"row 7 \(length -1\)"):
        L.normalize(audio.clone(), lengths, targets, return_meter=True)         # the same verdict, read by the same status entry
    l0, g0, p0 = L.normalize(plain, lengths, targets, check=False)               # mtts_loudness
    l1, g1, p1, m = L.normalize(audio, lengths, targets, check=False, return_meter=True)     # mtts_loudness_r128, no ceiling
    assert np.array_equal(bits64(l1.cpu().numpy()), bits64(l0.cpu().numpy()))
    assert np.array_equal(bits(p1.cpu().numpy()), bits(p0.cpu().numpy())) and np.array_equal(bits(g1.cpu().numpy()), bits(g0.cpu().numpy()))
    assert np.array_equal(bits(audio.cpu().numpy()), bits(plain.cpu().numpy()))
    m = host(m)
    worst = []
    for b, want in enumerate(ref["figures"]):
        for key in ("lufs", "lra", "momentary_max", "short_term_max"):
            close(m[key][b], want[key], (b, key), worst)
        assert bits(m["true_peak"][b]) == bits(want["true_peak"]) and m["peak"][b] == np.float32(want["peak"]), b
    print(f"largest |device - restated| = {max(worst):.3e} dB; lra {m['lra'].tolist()}; short-term max {m['short_term_max'].tolist()}; "
          f"momentary max {m['momentary_max'].tolist()}")
    assert abs(m["lra"][0] - 12.03) < 0.005 and abs(m["lra"][1] - 8.94) < 0.005 and 0.0 < m["lra"][2] < 3.0
    assert m["lra"][3] == 0.0 and m["short_term_max"][3] == -math.inf and math.isfinite(m["momentary_max"][3])
    assert m["lra"][4] == 0.0 and m["short_term_max"][4] == -math.inf and math.isfinite(m["momentary_max"][4])
    assert m["lra"][5] == 0.0 and m["momentary_max"][5] == -math.inf and m["short_term_max"][5] == -math.inf and m["true_peak"][5] == 0.0
    assert m["lra"][6] == 0.0 and m["momentary_max"][6] == -math.inf and m["lufs"][6] == -math.inf and m["gain"][6] == 1.0
    assert all(math.isnan(m[k][7]) for k in ("lufs", "lra", "momentary_max", "short_term_max"))
    assert m["peak"][7] == 0.0 and m["true_peak"][7] == 0.0 and m["gain"][7] == 1.0
    assert np.array_equal(bits(audio[7].cpu().numpy()), bits(before[7]))        # the refused row is not touched


def test_rows_in_a_batch_equal_the_rows_alone_in_either_order(L, ref):
    rows = figure_rows()
    keys = ("lufs", "lra", "momentary_max", "short_term_max", "peak", "true_peak")

    def run(rs):
        audio, _, lengths = device_rows(rs)
        return host(L.meter(audio, lengths))

    def same(a, i, b, j):
        for k in keys:
            x, y = a[k][i:i + 1], b[k][j:j + 1]
            eq = np.array_equal(bits64(x), bits64(y)) if x.dtype == np.float64 else np.array_equal(bits(x), bits(y))
            assert eq or (np.isnan(x[0]) and np.isnan(y[0])), (k, i, j, x, y)

    batch, again, back = run(rows), run(rows), run(rows[::-1])
    for b, (x, n) in enumerate(rows):
        same(batch, b, again, b)                                               # two calls give the same bits
        same(batch, b, back, len(rows) - 1 - b)
        if n >= 0:
            same(batch, b, run([(x, n)]), 0)                                    # another ld, B = 1


# ------------------------------------------------------------------------------------------------ the gain with two ceilings
def test_gain_with_the_true_peak_ceiling(L, tables):
    loud = am_noise(FS, 11)                                                      # true peak 0.61 dB over the sample peak
    rows = [(loud, FS), (am_noise(3 * FS, 10), 3 * FS), (am_noise(2000, 12), 2000), (loud, FS)]
    targets = [-8.0, -30.0, None, None]                                          # both ceilings bind; neither does; no target twice
    want = [rr.meter(x[:n], FS, tables[FS]) for x, n in rows]
    assert 20 * math.log10(want[0]["true_peak"] / want[0]["peak"]) > 0.5
    audio, before, lengths = device_rows(rows)
    plain, _, _ = device_rows(rows)
    _, g_plain, _ = L.normalize(plain, lengths, targets)
    lufs, gain, peak, m = L.normalize(audio, lengths, targets, true_peak=-1.0, return_meter=True)
    gain, g_plain, after = gain.cpu().numpy(), g_plain.cpu().numpy(), audio.cpu().numpy()
    c_tp = rr.ceiling_linear(-1.0)
    for b, (x, n) in enumerate(rows):
        g = rr.gain(want[b]["lufs"], targets[b], want[b]["peak"], want[b]["true_peak"], -1.0, 0.95, n)
        print(f"row {b}: gain {gain[b]:.9f} (restated {g:.9f}), without the true-peak ceiling {g_plain[b]:.9f}")
        assert abs(float(gain[b]) - float(g)) <= float(np.spacing(g)), (b, gain[b], g)
        if gain[b] == np.float32(1.0):
            assert np.array_equal(bits(after[b, :n]), bits(before[b, :n])), b
        else:
            assert np.array_equal(bits(after[b, :n]), bits(before[b, :n] * gain[b])), b
        assert np.array_equal(bits(after[b, n:]), bits(before[b, n:])), b      # nothing at or beyond the length is written
    assert gain[0] < g_plain[0] and g_plain[0] < 10 ** ((-8.0 - float(lufs[0])) / 20.0)     # the sample ceiling bound, then the second
    assert gain[1] == g_plain[1] != 1.0 and gain[2] == gain[3] == 1.0
    tp_after = host(L.meter(audio, lengths))["true_peak"]
    print(f"true peak after the gain: {tp_after[0]:.9f}, ceiling {c_tp:.9f}")
    assert tp_after[0] <= float(c_tp) * (1.0 + 2.0 ** -19) and tp_after[0] > 0.98 * float(c_tp)
    assert np.abs(after[0, :FS]).max() <= c_tp
    with pytest.raises(ValueError):
        L.normalize(audio, lengths, targets, true_peak=0.5)


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


def same_report(entry, m, b):
    inf = sub("inference")
    assert set(entry) == set(inf.METER_FIGURES)
    for k in inf.METER_FIGURES:
        want = float(m[k][b])
        assert entry[k] == want or (math.isnan(entry[k]) and math.isnan(want)), (b, k, entry[k], want)


def test_to_waveforms_true_peak_is_normalize_on_its_rows(L, env):
    inf, vocos, mel, lengths = env
    plain = inf.to_waveforms(mel, lengths, vocos)
    today, today_report = inf.to_waveforms(mel, lengths, vocos, loudness=-16, return_loudness=True)
    levelled, report = inf.to_waveforms(mel, lengths, vocos, loudness=-16, true_peak=-1.0, return_meter=True)
    rows, n = padded(plain)
    _, _, _, m = L.normalize(rows, n, -16.0, true_peak=-1.0, return_meter=True)
    c_tp = float(rr.ceiling_linear(-1.0))
    for b in range(4):
        assert torch.equal(levelled[b].view(torch.int32), rows[b, :n[b]].cpu().view(torch.int32)), b
        same_report(report[b], m, b)
        assert report[b]["lufs"] == today_report[b][0] and report[b]["gain"] <= today_report[b][1]
        assert np.float32(report[b]["true_peak"]) * np.float32(report[b]["gain"]) <= np.float32(c_tp)
        assert report[b]["true_peak"] >= report[b]["peak"] > 0.0 and report[b]["lra"] == 0.0       # (rows of a few hundred samples)
    # towards 0 LUFS the ceiling binds on every row, and is the lower of the two
    hot, hot_report = inf.to_waveforms(mel, lengths, vocos, loudness=0.0, true_peak=-1.0, return_meter=True)
    _, sample_only = inf.to_waveforms(mel, lengths, vocos, loudness=0.0, return_loudness=True)
    after = host(L.meter(*padded(hot)))["true_peak"]
    for b in range(4):
        print(f"row {b}: true peak {L.dbtp(hot_report[b]['true_peak']):.2f} dBTP, sample peak {L.dbtp(hot_report[b]['peak']):.2f} dB, "
              f"gain {hot_report[b]['gain']:.6f} (sample ceiling alone {sample_only[b][1]:.6f}), true peak after {L.dbtp(float(after[b])):.4f} dBTP")
        assert hot_report[b]["gain"] < sample_only[b][1] and after[b] <= c_tp * (1.0 + 2.0 ** -19)
    # without true_peak the results are today's bit for bit, whatever else is asked
    again, again_report = inf.to_waveforms(mel, lengths, vocos, loudness=-16, true_peak=None, return_loudness=True)
    assert all(torch.equal(a.view(torch.int32), t.view(torch.int32)) for a, t in zip(again, today)) and again_report == today_report
    metered, meter_report = inf.to_waveforms(mel, lengths, vocos, loudness=-16, return_meter=True)
    assert all(torch.equal(a.view(torch.int32), t.view(torch.int32)) for a, t in zip(metered, today))
    assert [(r["lufs"], r["gain"]) for r in meter_report] == today_report
    # a ceiling per row: a row without one takes today's gain; a ceiling on a row without a target is refused before the vocoder runs
    mixed, mixed_report = inf.to_waveforms(mel, lengths, vocos, loudness=[0.0, 0.0, None, -16], true_peak=[-1.0, -3.0, None, None],
                                           return_meter=True)
    assert torch.equal(mixed[0], hot[0]) and torch.equal(mixed[2], plain[2]) and torch.equal(mixed[3], today[3])
    assert mixed_report[1]["gain"] < hot_report[1]["gain"] and mixed_report[2]["gain"] == 1.0
    for kw in (dict(true_peak=-1.0), dict(loudness=[-16, None, -16, -16], true_peak=[-1.0] * 4), dict(loudness=-16, true_peak=0.5)):
        with pytest.raises(ValueError):
            inf.to_waveforms(mel, lengths, vocos, **kw)


def test_documents_take_one_gain_each_under_their_own_ceiling(L, env):
    inf, vocos, mel, lengths = env
    docs = dict(documents=[2, 2], gaps=[120, 0, 96, 0])
    plain = inf.to_waveforms(mel, lengths, vocos, **docs)
    out, seg, report = inf.to_waveforms(mel, lengths, vocos, loudness=0.0, true_peak=[-1.0, -2.0], return_meter=True, return_segments=True,
                                        **docs)
    assert len(out) == 2 and len(seg) == 2 and len(report) == 2
    for g, db in enumerate((-1.0, -2.0)):
        rows, n = padded([plain[g]])
        _, _, _, m = L.normalize(rows, n, 0.0, true_peak=db, return_meter=True)
        same_report(report[g], m, 0)
        gain = np.float32(report[g]["gain"])
        assert np.array_equal(bits(out[g].numpy()), bits(plain[g].numpy() * gain)), g            # ONE gain per document
        assert np.float32(report[g]["true_peak"]) * gain <= rr.ceiling_linear(db) and gain != 1.0


def test_encoded_rows_keep_the_single_synchronisation(L, env, monkeypatch):
    inf, vocos, mel, lengths = env
    calls = []
    for name in ("cpu", "tolist", "item"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                calls.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    kw = dict(loudness=-16, encoding="pcm16", return_loudness=True)
    inf.to_waveforms(mel, lengths, vocos, **kw)
    today = list(calls)
    calls.clear()
    coded, report = inf.to_waveforms(mel, lengths, vocos, true_peak=-1.0, return_meter=True, **kw)
    print(f"device reads: {calls}")
    assert calls == today == ["cpu", "cpu"]                       # the meta words (the one wait), then the copy of the bytes
    monkeypatch.undo()
    AC = sub("audio_codec")
    levelled = inf.to_waveforms(mel, lengths, vocos, loudness=-16, true_peak=-1.0)
    rows, n = padded(levelled)
    data, nbytes = AC.encode(rows, torch.tensor(n, device="cuda"), "pcm16")
    for b in range(4):
        assert coded[b].dtype == torch.uint8 and torch.equal(coded[b], data[b, :int(nbytes[b])].cpu()) and set(report[b]) == set(inf.METER_FIGURES)


def test_a_request_with_a_ceiling_carries_true_peak_and_lra(L, env):
    inf, vocos, mel, lengths = env
    bt = sub("batcher")
    batch = [bt.Request(ids=[1], loudness=0.0, true_peak=-1.0), bt.Request(ids=[1]), bt.Request(ids=[1], loudness=-16.0),
             bt.Request(ids=[1], loudness=0.0, true_peak=-3)]
    res = [{"mel": mel[b, :, :lengths[b]], "mel_length": lengths[b]} for b in range(4)]
    bt.waveforms_into(res, mel, torch.tensor(lengths), vocos, True, batch)
    one = [{"mel": mel[b, :, :lengths[b]], "mel_length": lengths[b]} for b in range(4)]
    bt.waveforms_into(one, mel, torch.tensor(lengths), vocos, False, batch)            # the per-request tail says the same
    _, report = inf.to_waveforms(mel, lengths, vocos, loudness=0.0, true_peak=-1.0, return_meter=True)
    assert set(res[0]) == {"mel", "mel_length", "audio", "loudness", "gain", "true_peak", "lra"} == set(res[3])
    assert set(res[1]) == {"mel", "mel_length", "audio"} and set(res[2]) == {"mel", "mel_length", "audio", "loudness", "gain"}
    assert res[0]["true_peak"] == L.dbtp(report[0]["true_peak"]) and res[0]["gain"] == report[0]["gain"] and res[0]["lra"] == 0.0
    assert res[3]["gain"] < report[3]["gain"]
    for b in range(4):
        assert set(one[b]) == set(res[b]) and torch.equal(one[b]["audio"].view(torch.int32), res[b]["audio"].view(torch.int32)), b
        assert all(one[b][k] == res[b][k] for k in ("loudness", "gain", "true_peak", "lra") if k in res[b]), b

"""Pitch on the GPU (include/mtts.h "pitch"; csrc/pitch.hip) against the NumPy restatement of tests/pitch_restated.py: frame counts
at every boundary of the window and of the block tile, refused rows beside good ones, padding that must never be read, outputs that
must not be overrun; aperiodicity inside the derived budget of fp64 and the decisions (voicing, lag, f0) equal on every decidable
frame; independence of the batch, bit for bit; non-finite samples; ``mtts_pitch_stats`` bit-equal to selection by sorting; the
Python entries, ``speaker_delta`` and ``tools/prepare_corpus.py pitch``.

A device lag is not an output: on a voiced frame it is the integer within 0.5 of fs / f0 (|delta| <= 0.5), on an unvoiced one the
lag shows through the aperiodicity, which is d' at that lag.  Every figure is printed before it is asserted."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import pitch_restated as pr

pytestmark = pytest.mark.gpu
SENTINEL = -777.0
GUARD = 64


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def raw(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def pitch():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("pitch")


def padded(rows, extra=0):
    """Rows -> [B, ld] with NaN beyond every row's own length: a kernel that reads there shows it."""
    ld = max(4, (max(len(r) for r in rows) + extra + 3) // 4 * 4)
    x = np.full((len(rows), ld), np.nan, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).cuda()


def raw_track(pitch, audio, lengths, fs, hop, fmin=60.0, fmax=500.0, thr=0.15, extra_cols=0):
    """``mtts_pitch_track`` on sentinel-filled outputs with guard elements behind them; returns (f0, aper, frames) on the host after
    checking that the guards kept their sentinel and that every column of every row was written."""
    hip = sub("_hip")
    lib = hip.load()
    hop, window, _, max_lag = pitch.plan(fs, hop, fmin, fmax)
    B, ld = audio.shape
    T = max(1, pitch.n_frames(ld, hop, window, max_lag)) + extra_cols
    f0 = torch.full((B * T + GUARD,), SENTINEL, device="cuda")
    aper = torch.full((B * T + GUARD,), SENTINEL, device="cuda")
    frames = torch.full((B + GUARD,), -555, dtype=torch.long, device="cuda")
    d_len = torch.tensor(lengths, dtype=torch.long, device="cuda")
    ws = torch.empty(lib.mtts_pitch_workspace_bytes(ld, B, fs, hop, fmin, fmax), dtype=torch.uint8, device="cuda")
    hip.check(lib.mtts_pitch_track(audio.data_ptr(), ld, d_len.data_ptr(), B, fs, hop, fmin, fmax, thr, f0.data_ptr(), aper.data_ptr(), T,
                                   frames.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr()))
    status = lib.mtts_pitch_status(ws.data_ptr(), hip.stream_ptr())
    message = lib.mtts_last_error().decode() if status else ""
    f0, aper, frames = f0.cpu(), aper.cpu(), frames.cpu()
    assert (f0[B * T:] == SENTINEL).all() and (aper[B * T:] == SENTINEL).all() and (frames[B:] == -555).all()
    f0, aper = f0[:B * T].reshape(B, T), aper[:B * T].reshape(B, T)
    assert not (f0 == SENTINEL).any() and not (aper == SENTINEL).any()
    return f0.numpy(), aper.numpy(), frames[:B].numpy(), message


def compare(name, ref, f0, aper, n, fs, hop, report):
    """One row against its fp64 analysis: returns the number of undecidable frames."""
    assert n == ref["n"], (name, n, ref["n"])
    assert np.all(f0[n:] == 0) and np.all(aper[n:] == 1), name       # columns at or beyond n
    if n == 0:
        return 0
    budget = pr.rel_budget(hop)
    dp = ref["dprime"]
    decidable = ref["margin"] > 0
    worst = 0.0
    for k in range(n):
        if ref["nonfinite"][k]:
            assert f0[k] == 0 and np.isnan(aper[k]), (name, k)
            continue
        if decidable[k]:
            e = budget * ref["aperiodicity"][k]
            err = abs(float(aper[k]) - ref["aperiodicity"][k])
            worst = max(worst, err / max(ref["aperiodicity"][k], 1e-300))
            assert err <= e, (name, k, err, e)
            assert (f0[k] > 0) == bool(ref["voiced"][k]), (name, k)
            if ref["voiced"][k]:
                assert abs(float(f0[k]) - ref["f0"][k]) <= ref["f0_budget"][k], (name, k, f0[k], ref["f0"][k], ref["f0_budget"][k])
                assert abs(fs / float(f0[k]) - ref["lag"][k]) <= 0.5 + 1e-3, (name, k)
        else:                                                       # within the budget of fp64's d' at SOME lag of the frame
            assert np.min(np.abs(float(aper[k]) - dp[k]) - budget * dp[k]) <= 0, (name, k)
    report.append(f"{name}: {n} frames, {int(ref['voiced'].sum())} voiced, {int((~decidable).sum())} undecidable, worst relative "
                  f"|aperiodicity - fp64| {worst:.3e} (budget {budget:.3e})")
    return int((~decidable).sum())


def voiced_clip(L, fs, seed, f=150.0):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / fs
    x = 0.4 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 2 * f * t + 1.0) + 0.1 * np.sin(2 * np.pi * 3 * f * t + 2.0)
    return (x + 0.004 * rng.standard_normal(L)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ lengths
def test_lengths_at_every_boundary(pitch):
    """fs 8000, hop 16, fmin 100: W = 128, max_lag = 80, a tile of 8 blocks; a clip of n frames has n + 7 blocks."""
    fs, hop, fmin = 8000, 16, 100.0
    assert pitch.plan(fs, hop, fmin)[1:] == (128, 16, 80) and sub("_hip").load().mtts_pitch_tile() == 8
    need = 128 + 80
    lengths = [0, need - 1, need, need + hop - 1, need + hop,                     # 0, 0, 1, 1, 2 frames
               need + 7 * hop, need + 8 * hop, need + 9 * hop, need + 9 * hop + 5,    # 15, 16, 17 blocks: two tiles -1, two tiles, +1
               need + 17 * hop + 3, 3]                                            # three tiles and a block; a clip shorter than a block
    rows = [voiced_clip(L, fs, 10 + i, 140.0 + 7 * i) for i, L in enumerate(lengths)]
    audio = padded(rows, extra=40)                                                # ld > L everywhere, NaN beyond L
    ld = audio.shape[1]
    given = lengths + [-1, ld + 1]                                                # refused rows beside the good ones
    audio = torch.cat([audio, torch.zeros(2, ld, device="cuda")])
    f0, aper, frames, message = raw_track(pitch, audio, given, fs, hop, fmin, extra_cols=3)
    print(message)
    assert "row 11 has length -1" in message and f"ld = {ld}" in message
    assert frames.tolist() == [0, 0, 1, 1, 2, 8, 9, 10, 10, 18, 0, -1, -1]
    report = []
    for b, row in enumerate(rows):
        ref = pr.analyse(row, fs, hop, fmin)
        compare(f"L={lengths[b]}", ref, f0[b], aper[b], int(frames[b]), fs, hop, report)
    print("\n".join(report))
    for b in (11, 12):
        assert np.all(f0[b] == 0) and np.all(aper[b] == 1)
    assert (f0[5:10, 0] > 0).all() and not np.isnan(aper[:11]).any()              # voiced clips, and the padding was never read
    with pytest.raises(ValueError, match="row 11 has length -1"):
        pitch.track(audio, given, fs, hop, fmin)
    got = pitch.track(audio[:11], lengths, fs, hop, fmin)                         # the Python entry gives the same bits
    assert got["frames"].tolist() == frames[:11].tolist() and (got["hop"], got["window"], got["max_lag"]) == (16, 128, 80)
    T = got["f0"].shape[1]
    assert np.array_equal(got["f0"].cpu().numpy().view(np.int32), f0[:11, :T].view(np.int32))
    assert np.array_equal(got["aperiodicity"].cpu().numpy().view(np.int32), aper[:11, :T].view(np.int32))


def test_defaults_on_short_clips_and_an_odd_hop(pitch):
    """The 24 kHz defaults (hop 128, 400 lags: two lag chunks per wave) on clips under 1 s, and 22.05 kHz with its default hop of 118
    (no multiple of 4 or 7)."""
    report = []
    for fs, lens in ((24000, [1423, 1424, 1424 + 127, 1424 + 128, 1424 + 8 * 128 + 1, 9000]), (22050, [5000, 1311, 1312])):
        hop, W, _, tmax = pitch.plan(fs)
        rows = [voiced_clip(L, fs, 30 + i, 95.0 + 40 * i) for i, L in enumerate(lens)]
        f0, aper, frames, message = raw_track(pitch, padded(rows, extra=8), lens, fs, hop)
        assert message == "" and frames.tolist() == [pr.n_frames(L, hop, tmax) for L in lens]
        for b, row in enumerate(rows):
            compare(f"{fs} Hz L={lens[b]}", pr.analyse(row, fs, hop), f0[b], aper[b], int(frames[b]), fs, hop, report)
    print("\n".join(report))


# ------------------------------------------------------------------------------------------------ values
_device = {}


def device_signals(pitch):
    """The decision signals of tests/pitch_restated.py, one ragged batch per sample rate: computed once."""
    if not _device:
        for fs, hop in ((24000, 128), (8000, 40)):
            sig = [s for s in pr.decision_signals() if s[2] == fs]
            f0, aper, frames, message = raw_track(pitch, padded([s[1] for s in sig]), [len(s[1]) for s in sig], fs, hop)
            assert message == ""
            for b, s in enumerate(sig):
                _device[s[0]] = (f0[b], aper[b], int(frames[b]), fs, hop)
    return _device


def test_values_and_decisions_on_the_glides(pitch):
    """Five-harmonic glides 90 -> 250 Hz and 220 -> 140 Hz with noise at -40 dB, an unvoiced gap and leading digital zeros, at 24 kHz /
    hop 128 and 8 kHz / hop 40: aperiodicity inside the derived budget, decisions and f0 equal on decidable frames, and at most 2 % of
    any signal's frames undecidable."""
    report, total = [], 0
    for name, (f0, aper, n, fs, hop) in device_signals(pitch).items():
        ref = pr.analysed(name)
        undecidable = compare(name, ref, f0, aper, n, fs, hop, report)
        total += n
        assert undecidable <= 0.02 * n, (name, undecidable, n)
        # the order of every sum is the header's: the fp32 twin written from it reproduces the device's bits, undecidable frames included
        twin = pr.analysed(name, True)
        assert np.array_equal(aper[:n].view(np.int32), twin["aperiodicity"].astype(np.float32).view(np.int32)), name
        assert np.array_equal(f0[:n].view(np.int32), twin["f0"].astype(np.float32).view(np.int32)), name
    print("\n".join(report))
    assert total > 500


def test_batch_invariance(pitch):
    """A row alone, first of 3, last of 3 and in reversed order: identical bits."""
    sig = [s for s in pr.decision_signals() if s[2] == 8000]
    a, b = sig[0][1], sig[1][1][:5003]
    c = voiced_clip(3000, 8000, 77)
    def run(rows):
        f0, aper, frames, _ = raw_track(pitch, padded(rows), [len(r) for r in rows], 8000, 40)
        return [(f0[i, :frames[i]].view(np.int32), aper[i, :frames[i]].view(np.int32)) for i in range(len(rows))]
    alone = run([a])[0]
    assert alone[0].size == pr.n_frames(len(a), 40, 134) > 100
    for rows, at in (([a, b, c], 0), ([c, b, a], 2), ([b, a], 1)):
        got = run(rows)[at]
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1]), at
    fwd, rev = run([a, b, c]), run([c, b, a])
    for i in range(3):
        assert np.array_equal(fwd[i][0], rev[2 - i][0]) and np.array_equal(fwd[i][1], rev[2 - i][1])


def test_nonfinite_samples(pitch):
    """One NaN (or Inf) sample marks exactly the frames that read it; the others keep the clean run's bits."""
    fs, hop, fmin = 8000, 16, 100.0
    span = 128 + 80
    clean = voiced_clip(span + 40 * hop, fs, 5)
    n = pr.n_frames(len(clean), hop, 80)
    k0 = 12
    cases = [(k0 * hop + span - 1, np.nan), (k0 * hop, np.inf), (len(clean) - 1, -np.inf), (0, np.nan)]
    rows = [clean]
    for p, v in cases:
        x = clean.copy()
        x[p] = v
        rows.append(x)
    f0, aper, frames, message = raw_track(pitch, padded(rows), [len(r) for r in rows], fs, hop, fmin)
    assert message == "" and (frames == n).all() and n == 41
    for i, (p, v) in enumerate(cases, start=1):
        reads = np.array([k * hop <= p < k * hop + span for k in range(n)])
        assert reads.sum() == min(p // hop, n - 1) - max(0, -(-(p - span + 1) // hop)) + 1
        assert np.all(f0[i, :n][reads] == 0) and np.isnan(aper[i, :n][reads]).all(), (p, v)
        assert np.array_equal(f0[i, :n][~reads].view(np.int32), f0[0, :n][~reads].view(np.int32)), (p, v)
        assert np.array_equal(aper[i, :n][~reads].view(np.int32), aper[0, :n][~reads].view(np.int32)), (p, v)
        ref = pr.analyse(rows[i], fs, hop, fmin)
        assert np.array_equal(ref["nonfinite"], reads)
    assert not np.isnan(aper[0]).any()
    assert [int(np.isnan(aper[i, :n]).sum()) for i in range(1, 5)] == [13, 13, 1, 1]   # frames 0..12 (last sample of 0; first of 12), the last, the first


# ------------------------------------------------------------------------------------------------ statistics
def test_stats_equal_selection_by_sorting(pitch):
    dev = device_signals(pitch)
    rng = np.random.default_rng(9)
    T = 160
    rows, counts = [], []

    def row(values, n):
        r = np.zeros(T, dtype=np.float32)
        r[:len(values)] = values
        rows.append(r)
        counts.append(n)

    f0, _, n, _, _ = dev["up_24000"]
    row(f0[:n], n)                                                               # the device's own contour
    row(np.zeros(50), 50)                                                        # m = 0
    row([0, 0, 123.5, 0], 4)                                                     # m = 1
    row([0, 201.0, 0, 0, 0, 0, 0, 99.0], 8)                                      # m = 2, one in the tail
    row([100, 0, 0, 0, 0, 0, 0, 0, 150, 0, 140], 11)                             # a tail with 2 voiced frames (tail_frames = 3)
    row([100, 0, 0, 0, 0, 0, 0, 160, 150, 0, 140], 11)                           # ... with 3
    row(rng.uniform(60, 500, T), T)                                              # all voiced
    row(rng.uniform(60, 500, T), 37)                                             # ... but only 37 columns count
    mixed = rng.uniform(60, 500, T) * (rng.uniform(size=T) < 0.6)
    mixed[::7] = mixed[3]                                                        # equal values among the voiced ones
    row(mixed, T - 5)
    row(rng.uniform(60, 500, T), -1)                                             # refused rows
    row(rng.uniform(60, 500, T), T + 1)
    row(np.concatenate([np.zeros(100), [77.0]]), 101)                            # the only voiced frame is the last
    batch = torch.from_numpy(np.stack(rows)).cuda()
    got = pitch.stats(batch, counts, 128, 24000, tail=3 * 128 / 24000)
    hz = torch.stack([got[k] for k in ("p05_hz", "median_hz", "p95_hz", "tail_median_hz")], 1).cpu().numpy()
    cnt = torch.stack([got[k] for k in ("frames", "voiced", "tail_voiced")], 1).cpu().numpy()
    for b, (r, n) in enumerate(zip(rows, counts)):
        want, c = pr.select(r, n, 3)
        assert cnt[b].tolist() == list(c), (b, cnt[b], c)
        assert np.array_equal(hz[b].view(np.int32), want.view(np.int32)), (b, hz[b], want)
    assert cnt[1].tolist() == [50, 0, 0] and np.isnan(hz[1]).all()
    assert cnt[4, 2] == 2 and np.isnan(hz[4, 3]) and cnt[5, 2] == 3 and hz[5, 3] == 150.0
    assert cnt[6].tolist() == [T, T, 4] and cnt[9].tolist() == [-1, 0, 0] and cnt[10].tolist() == [-1, 0, 0]
    vf = got["voiced_fraction"].cpu().numpy()
    assert vf.dtype == np.float64 and vf[6] == 1.0 and vf[1] == 0.0 and vf[2] == 0.25 and vf[9] == 0.0
    for key, num, den in (("range_st", 2, 0), ("final_rise_st", 3, 1)):
        want = 12.0 * np.log2(hz[:, num].astype(np.float64) / hz[:, den].astype(np.float64))
        assert got[key].dtype == torch.float64
        np.testing.assert_allclose(got[key].cpu().numpy(), want, rtol=1e-14, equal_nan=True)
    # the verdict of the statistics call names the first row whose frame count is out of range
    hip = sub("_hip")
    lib = hip.load()
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    out, c3 = torch.empty(len(rows), 4, device="cuda"), torch.empty(len(rows), 3, dtype=torch.long, device="cuda")
    d_n = torch.tensor(counts, device="cuda")
    hip.check(lib.mtts_pitch_stats(batch.data_ptr(), T, d_n.data_ptr(), len(rows), 3, out.data_ptr(), c3.data_ptr(), ws.data_ptr(), 256, hip.stream_ptr()))
    assert lib.mtts_pitch_status(ws.data_ptr(), hip.stream_ptr()) == -1 and b"row 9 has -1 frames" in lib.mtts_last_error()
    assert np.array_equal(out.cpu().numpy().view(np.int32), hz.view(np.int32))


# ------------------------------------------------------------------------------------------------ Python, end to end
def test_measure_pitch_end_to_end(pitch):
    corpus, ac = sub("corpus"), sub("audio_codec")
    up, down = (s[1] for s in pr.decision_signals() if s[2] == 24000)
    clips = [torch.from_numpy(up), torch.from_numpy(down[:20001]).cuda()]         # a list of clips, host and device, ragged
    got = corpus.measure_pitch(clips)
    tr = pitch.track(clips)
    st = pitch.stats(tr["f0"], tr["frames"], tr["hop"], 24000)
    for k in ("f0", "aperiodicity"):
        assert torch.equal(bits(got[k]), bits(tr[k])), k
    for k, v in st.items():
        assert raw(got[k]) == raw(v), k
    assert (got["hop"], got["window"], got["max_lag"]) == (128, 1024, 400)
    rise = got["final_rise_st"].tolist()
    print(f"final rise: glide up {rise[0]:+.2f} st, glide down {rise[1]:+.2f} st; median {got['median_hz'].tolist()} Hz; "
          f"range {got['range_st'].tolist()} st")
    assert rise[0] > 0 > rise[1]
    assert 90 < float(got["p05_hz"][0]) < float(got["median_hz"][0]) < float(got["p95_hz"][0]) < 250 and float(got["range_st"][0]) > 6
    assert 0.5 < float(got["voiced_fraction"][0]) < 1.0
    # other parameters pass through: a shorter tail, another hop
    short = corpus.measure_pitch(clips, tail=0.05, hop=96, fmin=80.0)
    assert short["hop"] == 96 and short["max_lag"] == 300 and short["final_rise_st"][0] > 0
    # a PCM16 recording gives the answer of the floats it decodes to
    pcm = np.clip(np.round(up.astype(np.float64) * 32767.0), -32768, 32767).astype("<i2")
    enc = ac.Encoded(pcm.tobytes(), "pcm16", 24000)
    wave, n = ac.decode_clips([enc], torch.device("cuda"))
    floats = wave[0, :n[0]].clone()
    a, b = corpus.measure_pitch([enc]), corpus.measure_pitch([floats])
    for k in ("f0", "aperiodicity", "median_hz", "final_rise_st", "frames"):
        assert raw(a[k]) == raw(b[k]), k
    assert abs(float(a["median_hz"][0]) - float(got["median_hz"][0])) < 0.5       # quantisation moves it by little
    t = pitch.frame_times(int(tr["frames"][0]), tr["hop"], tr["window"], tr["max_lag"], 24000)
    assert t[0] == 712 / 24000 and t.numel() == int(tr["frames"][0])


def test_speaker_delta(hparams, synthetic):
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    inference = sub("inference")
    hp = hparams.tiny(n_spks=4)
    model = inference.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to("cuda:0").eval()
    plus, minus = [0, [(1, 0.25), (3, 0.75)]], [2, 3, 1]
    d_enc, d_dur = model.speaker_delta(plus, minus)
    (pe, pd), (me, md) = model.speaker_rows(plus), model.speaker_rows(minus)
    assert d_enc.shape == d_dur.shape == (1, hp.spk_emb_dim) and d_enc.is_cuda
    assert torch.equal(d_enc, pe.mean(0, keepdim=True) - me.mean(0, keepdim=True))
    assert torch.equal(d_dur, pd.mean(0, keepdim=True) - md.mean(0, keepdim=True))
    assert d_enc.abs().max() > 0
    e_enc, e_dur = model.speaker_rows([2])
    moved = model.speaker_rows([(e_enc + 0.5 * d_enc, e_dur + 0.5 * d_dur)])       # what synthesise(speaker_embeddings=...) takes
    assert torch.equal(moved[0], e_enc + 0.5 * d_enc)
    with pytest.raises(ValueError, match="at least one voice"):
        model.speaker_delta([], [0])


# ------------------------------------------------------------------------------------------------ the tool
def test_prepare_corpus_pitch(pitch, tmp_path):
    tool = str(ROOT / "tools" / "prepare_corpus.py")
    res = subprocess.run([sys.executable, tool, "pitch", "--synthetic", "4", "--root", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = res.stdout
    print(out)
    assert "pitch of 4 files, 0 of them questions" in out                       # both filelists: 3 + 1
    table = out.split("Pitch per speaker")[1].splitlines()
    assert table[1] == "=" * 98 and table[3] == "-" * 98 and table[6] == "=" * 98
    assert table[2].split() == ["Speaker", "Count", "Median", "Hz", "Range", "st", "Rise", "?", "st", "Rise", "rest", "st", "Difference", "st"]
    rows = [line.split() for line in table[4:6]]
    assert [r[:2] for r in rows] == [["0", "2"], ["1", "2"]]                     # one row per speaker
    # the synthetic clips are sines of 120 + 20 i Hz: speaker 0 has clips 0 and 2, speaker 1 has 1 and 3
    assert abs(float(rows[0][2]) - 140.0) < 1.0 and abs(float(rows[1][2]) - 160.0) < 1.0
    assert rows[0][4] == "nan" and abs(float(rows[0][5])) < 0.1 and rows[0][6] == "nan"      # no questions; a steady tone does not rise

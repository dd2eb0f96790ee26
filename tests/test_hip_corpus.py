"""Corpus preparation on the GPU: the silence kernels against the reference's recorded numbers (tests/golden/silence.npz) and the
NumPy restatement (bit for bit), the mel sums against the restatement in the documented order and against math.fsum,
MelStatistics / precompute_mels against the front end, the ``silence=`` wiring of the recording entries, and
tools/prepare_corpus.py end to end."""
import json
import subprocess
import sys
import wave as wave_mod

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, sub
import corpus_restated as cr

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def corpus():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("corpus")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "silence.npz")


def padded(rows, poison=np.nan, extra=0):
    """Rows -> [B, ld] with everything beyond a row's own length poisoned: a kernel that reads there shows it."""
    ld = (max(len(r) for r in rows) + extra + 3) // 4 * 4
    x = np.full((len(rows), max(ld, 4)), poison, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).cuda(), [len(r) for r in rows]


_shared = {}


def fixture_run(corpus, synthetic):
    """The fixture's cases per sample rate (the 24 kHz ones in ONE ragged batch), both passes: computed once."""
    if _shared:
        return _shared
    cases = cr.clips(synthetic)
    for sr in sorted({sr for _, sr in cases.values()}):
        names = [k for k, (_, r) in cases.items() if r == sr]
        rows = [cases[k][0] for k in names]
        audio, lengths = padded(rows)
        m = corpus.measure_silence(audio, lengths, sample_rate=sr)
        out, out_len, info = corpus.normalize_silence(audio, lengths, cr.LEAD_S, cr.TRAIL_S, sample_rate=sr)
        out2, out_len2, info2 = corpus.normalize_silence(out, out_len, cr.LEAD_S, cr.TRAIL_S, sample_rate=sr)
        _shared[sr] = dict(names=names, rows=rows, lengths=lengths, six=m["samples"].cpu(), seconds=m["seconds"].cpu(), out=out.cpu(),
                           out_len=out_len.cpu(), info={k: v.cpu() for k, v in info.items()}, out2=out2.cpu(), out_len2=out_len2.cpu(),
                           info2={k: v.cpu() for k, v in info2.items()})
    return _shared


# ------------------------------------------------------------------------------------------------ silence
def test_silence_equals_the_reference_fixture(corpus, golden, synthetic):
    runs = fixture_run(corpus, synthetic)
    assert sorted(runs) == [24000, 44100] and len(runs[24000]["names"]) == 8
    for sr, r in runs.items():
        lead, trail = cr.samples(cr.LEAD_S, sr), cr.samples(cr.TRAIL_S, sr)
        assert r["out"].shape[1] % 4 == 0
        for b, name in enumerate(r["names"]):
            x, L = r["rows"][b], r["lengths"][b]
            six = r["six"][b].tolist()
            assert six[:2] == golden[f"bounds_{name}"].tolist(), name                # effective threshold: the content bounds
            assert six[2:] == golden[f"measured_{name}"].tolist(), name              # both thresholds: the four run lengths
            assert six == cr.measure(x, sr), name
            assert r["seconds"][b].tolist() == [v / sr for v in six]
            changed, n = int(r["info"]["changed"][b]), int(r["out_len"][b])
            assert [changed, n] == golden[f"pass1_{name}"].tolist(), name
            want, want_changed, (cs, ce) = cr.normalize(x, sr)
            row = r["out"][b]
            assert torch.equal(bits(row[:n]), bits(torch.from_numpy(want))), name    # the restatement, bit for bit
            assert not row[n:].view(torch.int32).any(), name                         # zeros (+0.0) run to ld_out
            if changed:                                                              # the body's bits are the input's
                assert torch.equal(bits(row[lead:lead + ce - cs]), bits(torch.from_numpy(x[cs:ce]))), name
                assert n == lead + (ce - cs) + trail
            assert r["info"]["bounds"][b, :2].tolist() == [cs, ce]
            assert float(r["info"]["current_leading"][b]) == cs / sr and float(r["info"]["current_trailing"][b]) == (L - ce) / sr
            assert float(r["info"]["leading_delta"][b]) == ((lead - cs) / sr if changed else 0.0)
            assert float(r["info"]["trailing_delta"][b]) == ((trail - (L - ce)) / sr if changed else 0.0)


def test_second_pass_equals_the_fixtures_second_pass(corpus, golden, synthetic):
    for sr, r in fixture_run(corpus, synthetic).items():
        for b, name in enumerate(r["names"]):
            n1, n2 = int(r["out_len"][b]), int(r["out_len2"][b])
            assert r["info2"]["bounds"][b, :2].tolist() == golden[f"bounds2_{name}"].tolist(), name
            assert [int(r["info2"]["changed"][b]), n2] == golden[f"pass2_{name}"].tolist(), name
            want, _, _ = cr.normalize(r["out"][b, :n1].numpy(), sr)
            assert torch.equal(bits(r["out2"][b, :n2]), bits(torch.from_numpy(want))), name
            assert not r["out2"][b, n2:].view(torch.int32).any()
            if not int(r["info2"]["changed"][b]):                                    # a no-op pass copies the row
                assert torch.equal(bits(r["out2"][b, :n2]), bits(r["out"][b, :n1])), name


def test_each_end_alone_keeps_the_other_ends_samples(corpus, synthetic):
    r = fixture_run(corpus, synthetic)[24000]
    audio, lengths = padded(r["rows"])
    for leading, trailing in ((None, 0.8), (0.2, None), (None, None)):
        out, out_len, info = corpus.normalize_silence(audio, lengths, leading, trailing)
        out, out_len = out.cpu(), out_len.cpu()
        for b, name in enumerate(r["names"]):
            x = r["rows"][b]
            want, changed, (cs, ce) = cr.normalize(x, 24000, leading, trailing)
            n = int(out_len[b])
            assert n == want.size and int(info["changed"][b]) == changed, (name, leading, trailing)
            assert torch.equal(bits(out[b, :n]), bits(torch.from_numpy(want))), (name, leading, trailing)
            assert not out[b, n:].view(torch.int32).any()
            if leading is None:
                assert torch.equal(bits(out[b, :ce]), bits(torch.from_numpy(x[:ce]))), name           # the leading samples stay
                assert float(info["leading_delta"][b]) == 0.0
            if trailing is None and changed:
                tail = x[ce:]
                assert torch.equal(bits(out[b, n - tail.size:n]), bits(torch.from_numpy(tail))), name  # the trailing samples stay


def window_rows(W, seed):
    """Rows that walk the kernel's paths at window length W: multiples of W, k W + 1, one sample into a 16-byte vector, a partial
    window of low noise, sub-window clips; amplitudes are 0, 3e-4 (between the thresholds) or 0.1 (content)."""
    rng = np.random.default_rng(seed)

    def seg(n, amp):
        return (rng.standard_normal(n) * amp).astype(np.float32)
    rows = [np.concatenate([seg(3 * W, 0), seg(5 * W, 0.1), seg(2 * W + 1, 0)]),                  # k W + 1
            np.concatenate([seg(W, 3e-4), seg(4 * W + 7, 0.1), seg(6 * W, 3e-4), seg(2 * W, 0)]),
            np.concatenate([seg(2 * W + 3, 0), seg(700 * W + 5, 0.1)]),                           # several workgroups of windows
            seg(1, 0.1), seg(W - 1, 0.1), seg(W, 0.1), seg(W + 1, 0.1)]
    n = 9 * W
    n += (1 - n) % 4                                                                              # ends one sample into a quad
    rows.append(np.concatenate([seg(W, 0), seg(n - W, 0.1)]))
    assert rows[0].size % W == 1 and rows[-1].size % 4 == 1
    return rows


@pytest.mark.parametrize("sr", [8000, 16000, 24000, 44100])
def test_window_lengths_match_the_restatement(corpus, sr):
    W = cr.window(sr)
    assert W == {8000: 80, 16000: 160, 24000: 240, 44100: 441}[sr]
    rows = window_rows(W, sr)
    audio, lengths = padded(rows)
    lead, trail = 10 * W / sr, 3 * W / sr
    six = corpus.measure_silence(audio, lengths, sample_rate=sr, effective_db=-60.0, absolute_db=-90.0)["samples"].cpu()
    out, out_len, info = corpus.normalize_silence(audio, lengths, lead, trail, sample_rate=sr)
    out, out_len = out.cpu(), out_len.cpu()
    for b, x in enumerate(rows):
        rms = cr.window_rms(x, W)
        for t in cr.thresholds(-60.0, -90.0):                       # the inputs keep their distance from both thresholds
            assert np.min(np.abs(rms.astype(np.float64) - float(t)) / float(t)) > 1e-3
        assert six[b].tolist() == cr.measure(x, sr, rms=rms), (sr, b)
        want, changed, _ = cr.normalize(x, sr, lead, trail)
        n = int(out_len[b])
        assert n == want.size and int(info["changed"][b]) == changed, (sr, b)
        assert torch.equal(bits(out[b, :n]), bits(torch.from_numpy(want))), (sr, b)
        assert not out[b, n:].view(torch.int32).any()


def test_a_nan_window_is_neither_content_nor_silence(corpus):
    W = 240
    x = np.zeros(20 * W, dtype=np.float32)
    x[6 * W:9 * W] = 0.1
    x[2 * W + 5] = np.nan                                           # window 2: ends the leading run, starts no content
    x[15 * W + 1] = np.nan                                          # window 15: ends the trailing run, is not content
    audio, lengths = padded([x], poison=7.0)
    six = corpus.measure_silence(audio, lengths)["samples"].cpu()[0].tolist()
    assert six == [6 * W, 9 * W, 2 * W, 2 * W, 4 * W, 4 * W]
    assert six == cr.measure(x, 24000)
    y = np.full(3 * W, np.nan, dtype=np.float32)                    # nothing but NaN windows: no content, no silent run
    assert corpus.measure_silence(*padded([y]))["samples"].cpu()[0].tolist() == [0, 0, 0, 0, 0, 0]


def test_batch_independence_and_repeatability(corpus, synthetic):
    r = fixture_run(corpus, synthetic)[24000]
    b = r["names"].index("low_both_ends")
    x = r["rows"][b]
    alone, n_alone = padded([x])
    one = corpus.normalize_silence(alone, n_alone, cr.LEAD_S, cr.TRAIL_S)
    two = corpus.normalize_silence(alone, n_alone, cr.LEAD_S, cr.TRAIL_S)
    n = int(one[1][0])
    assert n == int(r["out_len"][b]) == int(two[1][0])
    assert torch.equal(bits(one[0][0, :n]), bits(r["out"][b, :n])) and torch.equal(bits(one[0]), bits(two[0]))
    assert one[2]["bounds"].cpu()[0].tolist() == r["info"]["bounds"][b].tolist()
    assert corpus.measure_silence(alone, n_alone)["samples"].cpu()[0].tolist() == r["six"][b].tolist()
    audio, lengths = padded(r["rows"])
    again = corpus.measure_silence(audio, lengths)["samples"].cpu()
    assert torch.equal(again, r["six"])


def raw_normalize(corpus, audio, lengths, bounds, lead, trail, ld_out, sr=24000):
    """mtts_silence_normalize with a caller-chosen ld_out."""
    hip = sub("_hip")
    lib = hip.load()
    B, ld = audio.shape
    out = torch.full((B, ld_out), 3.0, dtype=torch.float32, device="cuda")
    out_len = torch.full((B,), 99, dtype=torch.long, device="cuda")
    changed = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    ws = torch.zeros(512, dtype=torch.uint8, device="cuda")
    d_len = torch.tensor(lengths, dtype=torch.long, device="cuda")
    hip.check(lib.mtts_silence_normalize(hip.ptr(audio), ld, hip.ptr(d_len), hip.ptr(bounds), B, sr, lead, trail, hip.ptr(out), ld_out,
                                         hip.ptr(out_len), hip.ptr(changed), ws.data_ptr(), ws.numel(), hip.stream_ptr()))
    rc = lib.mtts_silence_status(ws.data_ptr(), hip.stream_ptr())
    return out.cpu(), out_len.cpu(), changed.cpu(), rc, lib.mtts_last_error().decode()


def test_guarded_lengths_refuse_their_row_only(corpus, synthetic):
    r = fixture_run(corpus, synthetic)[24000]
    audio, lengths = padded(r["rows"], poison=0.25)
    ld = audio.shape[1]
    for bad_row, bad_len in ((2, -1), (5, ld + 1)):
        bent = list(lengths)
        bent[bad_row] = bad_len
        m = corpus.measure_silence(audio, bent, check=False)["samples"].cpu()
        out, out_len, info = corpus.normalize_silence(audio, bent, cr.LEAD_S, cr.TRAIL_S, check=False)
        out, out_len = out.cpu(), out_len.cpu()
        for b in range(len(lengths)):
            if b == bad_row:
                assert m[b].tolist() == [-1] * 6 and int(out_len[b]) == -1 and not out[b].view(torch.int32).any()
            else:                                                   # the other rows are unaffected
                n = int(r["out_len"][b])
                assert m[b].tolist() == r["six"][b].tolist() and int(out_len[b]) == n
                assert torch.equal(bits(out[b, :n]), bits(r["out"][b, :n]))
        with pytest.raises(ValueError, match=f"mtts_silence_measure: row {bad_row} has length {bad_len}"):
            corpus.measure_silence(audio, bent)
        with pytest.raises(ValueError, match=f"mtts_silence_normalize: row {bad_row} has length {bad_len}"):
            corpus.normalize_silence(audio, bent, cr.LEAD_S, cr.TRAIL_S)
    # an ld_out that holds every rebuilt row but the longest
    bounds = r["info"]["bounds"].cuda()
    lead, trail = cr.samples(cr.LEAD_S, 24000), cr.samples(cr.TRAIL_S, 24000)
    longest = int(r["out_len"].argmax())
    ld_out = (int(r["out_len"][longest]) - 1) // 4 * 4
    assert sorted(r["out_len"].tolist())[-2] <= ld_out < int(r["out_len"][longest])
    out, out_len, changed, rc, msg = raw_normalize(corpus, audio, lengths, bounds, lead, trail, ld_out)
    assert rc == -1 and f"row {longest} has length {lengths[longest]}" in msg and f"ld_out = {ld_out}" in msg
    for b in range(len(lengths)):
        if b == longest:
            assert int(out_len[b]) == -1 and not out[b].view(torch.int32).any()
        else:
            n = int(r["out_len"][b])
            assert int(out_len[b]) == n and int(changed[b]) == int(r["info"]["changed"][b])
            assert torch.equal(bits(out[b, :n]), bits(r["out"][b, :n])) and not out[b, n:].view(torch.int32).any()
    # with room for all of them the verdict is clean
    ok = raw_normalize(corpus, audio, lengths, bounds, lead, trail, (int(r["out_len"].max()) + 3) // 4 * 4)
    assert ok[3] == 0 and ok[1].tolist() == r["out_len"].tolist()


# ------------------------------------------------------------------------------------------------ mel sums
@pytest.mark.parametrize("F,T,lengths", [(100, 37, [0, 1, 36, 37, 20]), (7, 600, [600, 257, 256, 1, 0, 513])], ids=["F100", "F7"])
def test_mel_sums_in_the_documented_order(corpus, F, T, lengths):
    rng = np.random.default_rng(F)
    B = len(lengths)
    mel = rng.normal(-3.0, 2.0, (B, F, T)).astype(np.float32)
    for b, n in enumerate(lengths):
        mel[b, :, n:] = np.nan                                      # padding frames: never read, never flagged
    got = corpus.mel_sums(torch.from_numpy(mel).cuda(), lengths)
    s, q = got["sum"].cpu().numpy(), got["sum_sq"].cpu().numpy()
    assert got["frames"].tolist() == lengths and not got["nonfinite"].any()
    for b, n in enumerate(lengths):
        ws, wq, flag = cr.mel_sums(mel[b], n)
        assert (s[b].tobytes(), q[b].tobytes()) == (np.float64(ws).tobytes(), np.float64(wq).tobytes()), (b, n)   # bit-equal
        fs, fq, mag_s, mag_q, count = cr.fsum_sums(mel[b], n)
        assert abs(s[b] - fs) <= count * 2.0 ** -53 * mag_s and abs(q[b] - fq) <= count * 2.0 ** -53 * mag_q
    # another T padding and another batch: the same bits
    wide = np.full((2, F, T + 11), np.nan, dtype=np.float32)
    pick = [int(np.argmax(lengths)), 2]
    for i, b in enumerate(pick):
        wide[i, :, :lengths[b]] = mel[b, :, :lengths[b]]
    other = corpus.mel_sums(torch.from_numpy(wide).cuda(), [lengths[b] for b in pick])
    for i, b in enumerate(pick):
        assert other["sum"][i].cpu().numpy().tobytes() == s[b].tobytes() and other["sum_sq"][i].cpu().numpy().tobytes() == q[b].tobytes()
    # a NaN or an Inf in a valid frame sets that clip's flag only
    b = int(np.argmax(lengths))
    mel[b, F // 2, lengths[b] - 1] = np.inf
    mel[2, 0, 0] = np.nan
    flagged = corpus.mel_sums(torch.from_numpy(mel).cuda(), lengths)["nonfinite"].tolist()
    assert flagged == [i in (b, 2) for i in range(B)]
    with pytest.raises(ValueError, match=r"mtts_mel_stats: row 1 has length"):
        corpus.mel_sums(torch.from_numpy(mel).cuda(), [1, T + 1] + lengths[2:])
    res = corpus.mel_sums(torch.from_numpy(mel).cuda(), [1, T + 1] + lengths[2:], check=False)
    assert res["frames"].tolist() == [1, -1] + lengths[2:] and float(res["sum"][1]) == 0.0


def speechlike(seconds, i, rate=24000):
    t = torch.arange(int(seconds * rate), dtype=torch.float32) / rate
    g = torch.Generator().manual_seed(70 + i)
    return (0.4 * torch.sin(2 * np.pi * (110.0 + 25.0 * i) * t) + 0.05 * torch.randn(t.numel(), generator=g)).clamp(-1, 1)


def test_mel_statistics_equal_the_formula_on_the_devices_own_mel(corpus):
    M = sub("mel")
    clips = [speechlike(0.3 + 0.07 * i, i) for i in range(6)]
    stats = corpus.MelStatistics(n_mels=100, hop=256)
    stats.update(clips[:4])
    stats.update(clips[4:])
    tot_s = tot_q = 0.0
    frames = 0
    for c in clips:                                                  # the front end's un-normalised mel, summed in NumPy fp64
        mel, n = M.extract(c.cuda()[None], [c.numel()], 256, 0.0, 1.0)
        v = mel[0, :, :int(n[0])].cpu().numpy().astype(np.float64)
        tot_s, tot_q, frames = tot_s + v.sum(), tot_q + (v * v).sum(), frames + int(n[0])
    mean, std = cr.statistics(tot_s, tot_q, frames, 100)
    got_mean, got_std = stats.raw()
    print(f"mel statistics: device {got_mean!r} {got_std!r}  numpy {mean!r} {std!r}")
    assert stats.total_frames == frames and stats.ok == 6 and stats.failures == []
    assert abs(got_mean - mean) <= 1e-9 and abs(got_std - std) <= 1e-9
    res = stats.result()
    assert abs(res["mel_mean"] - mean) <= 1e-6 and abs(res["mel_std"] - std) <= 1e-6
    assert res == {"mel_mean": round(got_mean, 6), "mel_std": round(got_std, 6)}
    bad = torch.zeros(2, 100, 9, device="cuda")
    bad[1, 3, 4] = float("nan")
    stats.update_mel(bad, [9, 9])
    assert stats.failures == [(7, "the mel holds a NaN or an Inf")] and stats.ok == 7 and stats.total_frames == frames + 9


def test_precompute_mels_equals_two_front_end_calls(corpus):
    M = sub("mel")
    clips = [speechlike(0.3 + 0.11 * i, i) for i in range(3)]
    out = corpus.precompute_mels(clips, None, mel_mean=-5.5, mel_std=2.1, hop=256)
    wave, lengths = padded([c.numpy() for c in clips], poison=0.0)
    mel, n = M.extract(wave, lengths, 256, -5.5, 2.1)
    fine, nf = M.extract(wave, lengths, 128, -5.5, 2.1)
    assert torch.equal(bits(out["mel"]), bits(mel)) and torch.equal(bits(out["mel_fine"]), bits(fine))
    assert out["mel_lengths"].tolist() == n.tolist() and out["mel_fine_lengths"].tolist() == nf.tolist()
    assert out["ok"].tolist() == [True] * 3 and out["mel"].shape[1] == 100


# ------------------------------------------------------------------------------------------------ wiring
@pytest.fixture(scope="module")
def model_env(corpus, hparams, synthetic):
    inf = sub("inference")
    hp = hparams.prod_v20(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    return hp, model.to("cuda").eval()


def test_silence_keyword_equals_normalising_by_hand(corpus, model_env, synthetic):
    hp, model = model_env
    x, x_len, _ = synthetic.make_inputs(hp, 2, 12, seed=321, lengths=[12, 9])
    x, x_len = x.cuda(), x_len.cuda()
    clips = [torch.cat([torch.zeros(1000), speechlike(0.8, 1), torch.zeros(5000)]), torch.cat([torch.zeros(7300), speechlike(0.7, 2)])]
    out, out_len, info = corpus.normalize_silence(clips, None, 0.2, 0.8)
    assert info["changed"].tolist() == [True, True]
    by_hand = [out[b, :int(out_len[b])].clone() for b in range(2)]
    a = model.align(x, x_len, audio=clips, silence=(0.2, 0.8))
    b = model.align(x, x_len, audio=by_hand)
    plain = model.align(x, x_len, audio=clips)
    none = model.align(x, x_len, audio=clips, silence=None)
    assert a["mel_fine_lengths"].tolist() == b["mel_fine_lengths"].tolist() == [int(n) // 128 + 1 for n in out_len.tolist()]
    assert a["mel_fine_lengths"].tolist() != plain["mel_fine_lengths"].tolist()
    for k in ("durations", "predicted_durations", "scale_correction", "score"):
        assert torch.equal(bits(a[k].float()), bits(b[k].float())), k
        assert torch.equal(bits(none[k].float()), bits(plain[k].float())), k
    t, noise_seed = torch.tensor([0.3, 0.6]), torch.Generator(device="cuda").manual_seed(3)
    T = sub("inference").fix_len_compatibility(max(int(n) // 256 + 1 for n in out_len.tolist()))
    noise = torch.randn(2, hp.n_feats, T, device="cuda", generator=noise_seed)
    s1 = model.score(x, x_len, audio=clips, t=t, noise=noise, silence=(0.2, 0.8))
    s2 = model.score(x, x_len, audio=by_hand, t=t, noise=noise)
    for k in ("dur_loss", "prior_loss", "diff_loss"):
        assert torch.equal(bits(s1[k].float()), bits(s2[k].float())), k
    with pytest.raises(ValueError, match="multiple of 10 ms"):
        model.align(x, x_len, audio=clips, silence=(0.2, 0.805))


# ------------------------------------------------------------------------------------------------ the tool
def read_pcm16(path):
    with wave_mod.open(str(path), "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2"), w.getframerate()


def test_prepare_corpus_tool_end_to_end(corpus, tmp_path):
    tool = str(ROOT / "tools" / "prepare_corpus.py")

    def run(*args):
        res = subprocess.run([sys.executable, tool, *args, "--synthetic", "4", "--root", str(tmp_path)], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout

    out = run("measure")
    assert "Leading silence per speaker" in out and "Trailing silence per speaker" in out and "measured 3 files" in out       # the train filelist, as the reference
    table = out.split("Trailing silence per speaker")[1].splitlines()
    assert table[1] == "=" * 98 and table[2].split() == ["Speaker", "Count", "Effective", "Mean", "Effective", "Std", "Absolute", "Mean", "Absolute", "Std"]
    assert [row.split()[:2] for row in table[4:6]] == [["0", "2"], ["1", "1"]]
    wavs = sorted((tmp_path / "wav").rglob("*.wav"))
    assert len(wavs) == 4
    before = {p: read_pcm16(p) for p in wavs}
    norm = ("normalize", "--target_leading_silence", "0.2", "--target_trailing_silence", "0.8", "--report", str(tmp_path / "normalize_report.json"))
    out = run(*norm)
    assert "normalized 4 files, 4 rewritten" in out
    report = json.loads((tmp_path / "normalize_report.json").read_text())
    for p in wavs:
        (old, sr), (new, sr2) = before[p], read_pcm16(p)
        assert sr == sr2 == 24000
        e = report[str(p.relative_to(tmp_path / "wav").with_suffix(""))]
        cs, ce = e["content_start"], e["content_end"]
        assert e["changed"] and new.size == 4800 + (ce - cs) + 19200
        assert not new[:4800].any() and not new[4800 + ce - cs:].any()
        assert np.array_equal(new[4800:4800 + ce - cs], old[cs:ce])                  # 16-bit content samples survive unchanged
    assert "normalized 4 files, 0 rewritten" in run(*norm)
    assert all(not e["changed"] for e in json.loads((tmp_path / "normalize_report.json").read_text()).values())      # idempotent
    out = run("stats")
    assert "data_statistics:" in out and "mel_mean:" in out and "mel_std:" in out
    run("mels")
    meta = json.loads((tmp_path / "mel" / "metadata.json").read_text())
    assert meta["num_files"] == 4 and meta["num_ok"] == 4 and meta["num_fail"] == 0 and meta["hop_length"] == 256 and meta["n_mels"] == 100
    for p in wavs:
        rel = p.relative_to(tmp_path / "wav").with_suffix("")
        n = read_pcm16(p)[0].size
        mel, fine = np.load(tmp_path / "mel" / (str(rel) + ".npy")), np.load(tmp_path / "mel" / (str(rel) + ".fine.npy"))
        assert mel.dtype == np.float32 and mel.shape == (100, n // 256 + 1) and fine.shape == (100, n // 128 + 1)
        assert np.isfinite(mel).all() and np.isfinite(fine).all()
    assert not (tmp_path / "mel" / "failures.txt").exists()

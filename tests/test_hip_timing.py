"""GPU tests of token timing (include/mtts.h "token timing", "shaped durations"; csrc/timing.hip, csrc/norm_glue.hip) against the NumPy
restatement of tests/timing_restated.py: shaped durations (bit-equal to the plain entries under identity shaping, integer-equal to
the fp32 and fp64 restatements, the clamps and the NaN rule), the marks and the break plan (integer-exact), the gather (bit-equal,
every word of out_ld), the verdicts (each refuses its row alone), and the path from ``synthesise`` to the batcher on the tiny model."""
import numpy as np
import pytest
import torch

from conftest import sub
import timing_restated as tr

pytestmark = pytest.mark.gpu

SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)             # tests/test_hip_vocos.py's second configuration
HOP = SMALL["hop"]
FINE = HOP // 2


@pytest.fixture(scope="module")
def hipenv():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("_hip"), sub("_hip").load(), sub("inference")


@pytest.fixture(scope="module")
def tm(hipenv):
    return sub("timing")


@pytest.fixture(scope="module")
def hipmodel(hipenv):
    return hipenv[0].HipModel(sub("hparams").tiny())            # durations need no weights


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ shaped durations
B3, TX, XLEN = 3, 300, [1, 5, 300]
SC, LS = [1.0, 0.93, 1.1], [1.0, 0.8, 1.25]


def shaping_case(seed):
    g = torch.Generator().manual_seed(seed)
    logw = torch.randn(B3, 1, TX, generator=g) * 0.6 + 1.4
    mask = (torch.arange(TX)[None] < torch.tensor(XLEN)[:, None]).float()[:, None]
    s = torch.rand(B3, TX, generator=g) * 2.0
    s[torch.rand(B3, TX, generator=g) < 0.15] = 0.0
    s[0, 0], s[1, 1] = 0.0, 0.0
    a = torch.rand(B3, TX, generator=g) * 6.0 - 3.0
    given = torch.randint(0, 7, (B3, TX), generator=g).float()
    return logw, mask, s, a, given


def test_identity_shaping_is_the_plain_entries_bit_for_bit(hipmodel):
    logw, mask, _, _, given = shaping_case(1)
    dl, dm = logw.cuda(), mask.cuda()
    want = hipmodel.durations(dl, dm, SC, LS)
    for kw in ({}, dict(token_scale=torch.ones(B3, TX).cuda()), dict(token_extend=torch.zeros(B3, TX).cuda()),
               dict(token_scale=torch.ones(B3, TX).cuda(), token_extend=torch.zeros(B3, TX).cuda())):
        got = hipmodel.durations_shaped(dl, dm, SC, LS, **kw)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), list(kw)
    assert want[2].tolist()[0] == max(int(want[0][0, 0]), 1) and int(want[1][2, -1]) > TX      # ragged rows, a long scan
    # given rows mixed with predicted ones: the two launches of before against the one
    pred = hipmodel.durations(dl, dm, SC, LS)[0]
    want = hipmodel.durations_given(given.cuda(), dm, LS, given_rows=[0, 1, 1], out=pred)
    got = hipmodel.durations_shaped(dl, dm, SC, LS, given=given.cuda(), given_rows=[0, 1, 1], token_scale=torch.ones(B3, TX).cuda())
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    allg = hipmodel.durations_shaped(None, dm, SC, LS, given=given.cuda())
    want = hipmodel.durations_given(given.cuda(), dm, LS)
    assert torch.equal(bits(allg[0]), bits(want[0])) and torch.equal(allg[1], want[1]) and torch.equal(allg[2], want[2])


def test_shaped_durations_are_the_fp32_restatement_on_the_devices_exp(hipmodel):
    logw, mask, s, a, given = shaping_case(2)
    e_dev = torch.exp(logw.cuda()).cpu().numpy()[:, 0]          # the device's own fp32 expf
    for kw, rkw in ((dict(), dict()), (dict(given=given.cuda(), given_rows=[1, 0, 1]), dict(given=given.numpy(), given_rows=[1, 0, 1]))):
        dur, cum, yfl = hipmodel.durations_shaped(logw.cuda(), mask.cuda(), SC, LS, token_scale=s.cuda(), token_extend=a.cuda(), **kw)
        d, c, y, _ = tr.shaped_durations(e_dev, mask.numpy()[:, 0], SC, LS, s.numpy(), a.numpy(), **rkw)
        assert np.array_equal(dur.cpu().numpy(), d) and np.array_equal(cum.cpu().numpy(), c) and np.array_equal(yfl.cpu().numpy(), y)
        assert (d[2][s[2].numpy() == 0] <= 3).all() and (d >= 0).all() and (d[0, 1:] == 0).all()
    assert (d[1, :5][(s[1, :5] == 0).numpy() & (a[1, :5] < 0.5).numpy()] == 0).all()           # a scale of 0 drops the token


def test_shaped_durations_are_the_fp64_restatement_away_from_ties(hipmodel):
    """Inputs are redrawn on the CPU until every value in front of the rounding has |v| <= 128 and lies at least 2^-10 from a
    half-integer; the fp32 chain (expf at ~2 ulp, five roundings) errs below 1e-4 at that magnitude, so fp32 and fp64 round alike and
    no token is left out."""
    logw, mask, s, a, _ = shaping_case(3)
    m = mask.numpy()[:, 0].astype(np.float64)
    lw, sn, an = logw.numpy()[:, 0].astype(np.float32), s.numpy(), a.numpy()
    rng = np.random.default_rng(5)
    for _ in range(200):
        _, _, _, v = tr.shaped_durations(np.exp(lw.astype(np.float64)), m, SC, LS, sn, an, dtype=np.float64)
        bad = ((np.abs(v) > 128) | (np.abs(v - np.floor(v) - 0.5) < 2.0 ** -10)) & (m > 0)
        if not bad.any():
            break
        lw[bad] = (rng.standard_normal(int(bad.sum())) * 0.6 + 1.4).astype(np.float32)
        an[bad] = (rng.random(int(bad.sum())) * 6.0 - 3.0).astype(np.float32)      # (a dropped token's value is its extension alone)
    assert not bad.any()
    a = torch.from_numpy(an)
    d64, c64, y64, _ = tr.shaped_durations(np.exp(lw.astype(np.float64)), m, SC, LS, sn, an, dtype=np.float64)
    dur, cum, yfl = hipmodel.durations_shaped(torch.from_numpy(lw)[:, None].cuda(), mask.cuda(), SC, LS, token_scale=s.cuda(), token_extend=a.cuda())
    assert np.array_equal(dur.cpu().numpy().astype(np.int64), d64.astype(np.int64))
    assert np.array_equal(cum.cpu().numpy(), c64) and np.array_equal(yfl.cpu().numpy(), y64)


def test_the_clamps_and_the_nan_rule_hold_on_the_device(hipmodel):
    logw, mask, _, _, given = shaping_case(4)
    s = torch.ones(B3, TX)
    a = torch.zeros(B3, TX)
    s[2, :6] = torch.tensor([-5.0, 1000.0, float("nan"), float("inf"), -float("inf"), 16.0])
    a[2, 6:12] = torch.tensor([-1e9, 1e9, float("nan"), float("inf"), -float("inf"), 4096.0])
    a[1, 0], s[1, 1] = float("nan"), float("nan")
    e_dev = torch.exp(logw.cuda()).cpu().numpy()[:, 0]
    for kw, rkw in ((dict(), dict()), (dict(given=given.cuda()), dict(given=given.numpy()))):
        dur, cum, yfl = hipmodel.durations_shaped(logw.cuda(), mask.cuda(), SC, LS, token_scale=s.cuda(), token_extend=a.cuda(), **kw)
        d, c, y, _ = tr.shaped_durations(e_dev, mask.numpy()[:, 0], SC, LS, s.numpy(), a.numpy(), **rkw)
        assert np.array_equal(dur.cpu().numpy(), d) and np.array_equal(cum.cpu().numpy(), c) and np.array_equal(yfl.cpu().numpy(), y)
        ident = tr.shaped_durations(e_dev, mask.numpy()[:, 0], SC, LS, **rkw)[0]
        assert (d >= 0).all() and d[2, 0] == 0 and d[2, 4] == 0                       # s < 0 and s = -inf are 0: the token is dropped
        assert d[2, 6] <= 1 and d[2, 10] <= 1                                         # a = -1e9 and -inf are -4096
        assert all(4096 <= d[2, k] <= 4096 + 64 for k in (7, 9, 11))                  # a = 1e9, inf and 4096 are 4096
        assert all(ident[2, k] <= d[2, k] <= 16 * 64 for k in (1, 3, 5))              # s = 1000, inf and 16 are 16
        assert all(d[r, k] == ident[r, k] for r, k in ((2, 2), (2, 8), (1, 0), (1, 1)))     # NaN: s = 1, a = 0
    with pytest.raises(ValueError, match="token_scale"):        # a host value outside the range is refused before any launch
        hipmodel.durations_shaped(logw.cuda(), mask.cuda(), SC, LS, token_scale=s)
    with pytest.raises(ValueError, match="token_extend"):
        hipmodel.durations_shaped(logw.cuda(), mask.cuda(), SC, LS, token_extend=a.numpy())


# ------------------------------------------------------------------------------------------------ marks, plan and gather
def csr(breaks):
    first, tok, pause = [0], [], []
    for row in breaks:
        for t, p in row or ():
            tok.append(t)
            pause.append(p)
        first.append(len(tok))
    return (torch.tensor(first, dtype=torch.int32), torch.tensor(tok, dtype=torch.int32), torch.tensor(pause, dtype=torch.long))


def device_plan(tm, cum, x_len, keep, breaks=None, keep_max=1 << 30, out_ld=None, pause_max=1 << 20, fine_hop=128):
    """token_marks on the device through the CSR route (only the device judges): marks, lengths, plan and the status message."""
    kw = {}
    if breaks is not None:
        extra = max([sum(max(p, 0) for _, p in r or ()) for r in breaks] + [0])
        kw = dict(out_ld=(keep_max + extra + 3) // 4 * 4 if out_ld is None else out_ld, pause_max=pause_max)
    marks, lengths, plan = tm.token_marks(torch.as_tensor(cum, dtype=torch.int32).cuda(), x_len, keep, None if breaks is None else csr(breaks),
                                          fine_hop=fine_hop, keep_max=keep_max, check=False, **kw)
    message = None
    try:
        plan.raise_refused()
    except ValueError as e:
        message = str(e)
    return marks.cpu().numpy(), lengths.cpu().numpy(), plan, message


def durations_case(seed, B, Tx, lengths, zeros=True):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(0 if zeros else 1, 7, (B, Tx), generator=g)
    for b, n in enumerate(lengths):
        d[b, n:] = 0
    return torch.cumsum(d, 1).numpy()


def test_marks_are_the_restatement(tm):
    Tx = 300
    x_len = [300, 1, 7, 40, 300, 12]
    cum = durations_case(11, 6, Tx, x_len)
    cum[2, :7] = np.cumsum([0, 0, 3, 0, 2, 0, 0])               # tokens of no duration at both ends and in the middle
    nominal = [128 * int(cum[b, -1]) for b in range(6)]
    keep = [nominal[0] + 500, nominal[1], nominal[2] - 100, 0, -1, nominal[5] // 2]      # above, at, inside, 0, refused, below
    marks, lengths, _, message = device_plan(tm, cum, x_len, keep)
    reasons, want, want_len, _ = tr.plan(cum, x_len, keep, None)
    assert reasons.tolist() == [0, 0, 0, 0, 1, 0]
    assert np.array_equal(marks, want) and np.array_equal(lengths, want_len)
    assert (marks[4] == -1).all() and lengths[4] == -1 and "row 4" in message and "kept length -1" in message
    assert (marks[3, :40] == 0).all() and (marks[3, 40:] == -1).all()
    assert marks[1, 0].tolist() == [0, min(max(128 * int(cum[1, 0]) - 64, 0), keep[1])]
    assert marks[0, 299, 1] == nominal[0] - 64 and (np.diff(marks[5, :12].reshape(-1)) >= 0).all() and marks[5, 11, 1] == keep[5]
    # a batch of 1 gives the row the marks it has in a batch of 6
    for b in (0, 2, 5):
        one, one_len, _, _ = device_plan(tm, cum[b:b + 1], x_len[b:b + 1], keep[b:b + 1])
        assert np.array_equal(one[0], marks[b]) and one_len[0] == lengths[b]
    # x_len outside [1, Tx] refuses its row alone
    marks2, lengths2, _, message = device_plan(tm, cum, [300, 0, 7, 301, 300, 12], [nominal[0]] * 6)
    assert lengths2.tolist()[1] == -1 and lengths2.tolist()[3] == -1 and (lengths2[[0, 2, 4, 5]] >= 0).all()
    assert "row 1" in message and "token count 0" in message


ROWS = [0, 1, 7, 2047, 2049, 4100]


def gather_case(seed, ld):
    g = torch.Generator().manual_seed(seed)
    audio = torch.randn(len(ROWS), ld, generator=g) * 0.5
    return audio


def breaks_for(cum, x_len, keep, which):
    """A row's breaks for the named case, from its own boundaries."""
    e = tr.edges(cum, x_len, keep, 128)
    inner = [t for t in range(x_len) if 0 < e[t + 1] < keep]
    if which == "none" or x_len < 2:
        return []
    if which == "ends":                                          # after the first token, somewhere inside, after the last (dropped)
        toks = sorted({0, inner[len(inner) // 2] if inner else 0, x_len - 1})
        return [(t, 37 + 100 * k) for k, t in enumerate(toks)]
    if which == "pause0":
        return [(t, 0) for t in inner[:3]]
    if which == "dense":                                         # every token: segments shorter than 2 * fade, and two breaks at one cut
        return [(t, 5 + (t % 3)) for t in range(x_len)]
    raise KeyError(which)


@pytest.mark.parametrize("fade", [0, 120])
@pytest.mark.parametrize("which", ["ends", "dense", "pause0", "none"])
def test_the_gather_is_the_restatement_on_every_word(tm, fade, which):
    ld = 4104                                                   # not a row's length; 16-byte rows
    Tx = 40
    audio = gather_case(21, ld)
    x_len = [1, 1, 2, 17, 40, 33]
    cum = np.zeros((len(ROWS), Tx), dtype=np.int64)
    for b, (n, L) in enumerate(zip(x_len, ROWS)):
        d = np.random.default_rng(30 + b).integers(0, 3, n)
        d[n // 2] = 0                                            # a token of no duration: its break cuts where its neighbour's does
        if n > 2:
            d[n // 2 - 1] = 0
        scale = -(-(L + 64) // (128 * max(int(d.sum()), 1)))         # the nominal length is beyond keep: the last boundaries are held to it
        cum[b, :n] = np.cumsum(d * max(scale, 1))
        cum[b, n:] = cum[b, n - 1]
    breaks = [breaks_for(cum[b], x_len[b], ROWS[b], which if b != 2 or which == "none" else "ends") for b in range(len(ROWS))]
    marks, lengths, plan, message = device_plan(tm, cum, x_len, ROWS, breaks, keep_max=ld)
    assert message is None
    reasons, want_marks, want_len, cuts = tr.plan(cum, x_len, ROWS, breaks)
    assert not reasons.any() and np.array_equal(marks, want_marks) and np.array_equal(lengths, want_len)
    if which != "none":
        assert sum(len(c) for c in cuts) >= 2                                                             # breaks applied ...
    if which in ("ends", "dense"):
        assert all(len(r) > len(c) for r, c in zip(breaks[3:], cuts[3:]))                                 # ... and dropped (after the last token)
    if which == "dense":
        assert any(c[k][0] == c[k + 1][0] for c in cuts for k in range(len(c) - 1))                      # two breaks at one position
        assert any(0 < c[k + 1][0] - c[k][0] < 2 * 120 for c in cuts for k in range(len(c) - 1))         # a segment shorter than 2 * fade
    got = tm.apply_breaks(audio.cuda(), plan, fade).cpu().numpy()      # (the output buffer is torch.empty: every word is written)
    assert got.shape[1] == plan.out_ld and plan.out_ld % 4 == 0
    for b in range(len(ROWS)):
        want = tr.spliced_row(audio[b].numpy(), ROWS[b], int(want_len[b]), cuts[b], fade, plan.out_ld)
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (b, which, fade)
        if not cuts[b]:                                          # a row without (applied) breaks is its input, bit for bit
            assert np.array_equal(got[b, :ROWS[b]].view(np.uint32), audio[b, :ROWS[b]].numpy().view(np.uint32))
    # a row in a batch of 1 is the row it is in this batch
    for b in (3, 5):
        m1, l1, p1, _ = device_plan(tm, cum[b:b + 1], x_len[b:b + 1], ROWS[b:b + 1], breaks[b:b + 1], keep_max=ld)
        g1 = tm.apply_breaks(audio[b:b + 1].cuda(), p1, fade).cpu().numpy()
        n = int(l1[0])
        assert np.array_equal(m1[0], marks[b]) and n == lengths[b] and np.array_equal(g1[0, :n].view(np.uint32), got[b, :n].view(np.uint32))
        assert not g1[0, n:].any()


def test_each_reason_refuses_its_row_alone(tm):
    Tx, ld = 12, 2052
    x_len = [12, 10, 12, 12, 12, 12]
    cum = np.stack([np.minimum(np.arange(1, Tx + 1), n) for n in x_len])       # one fine frame per token: e_k = 128 k - 64
    keep = [1500, 1200, 1500, 1500, 1500, 2053]
    good = [(2, 100), (5, 50)]
    audio = torch.randn(6, ld, generator=torch.Generator().manual_seed(2)) * 0.3
    clean = device_plan(tm, cum, x_len, [1500, 1200, 1500, 1500, 1500, 1500], [good] * 6, keep_max=ld, pause_max=1000)
    assert clean[3] is None
    clean_audio = tm.apply_breaks(audio.cuda(), clean[2], 8).cpu()
    cases = {1: ([(2, 100), (10, 5)], "break 1 names a token outside"), 2: ([(5, 100), (5, 50)], "break 1 does not follow a later token"),
             3: ([(2, 100), (5, 1001)], "the pause of break 1 is outside [0, 1000]"), 4: ([(2, -1)], "the pause of break 0"),
             5: (good, "kept length 2053 is outside [0, 2052]")}
    for row, (bad, word) in cases.items():
        breaks = [good] * 6
        breaks[row] = bad
        k = [1500, 1200, 1500, 1500, 1500, keep[5] if row == 5 else 1500]
        marks, lengths, plan, message = device_plan(tm, cum, x_len, k, breaks, keep_max=ld, pause_max=1000, out_ld=clean[2].out_ld)
        reasons, want, want_len, _ = tr.plan(cum, x_len, k, breaks, keep_max=ld, pause_max=1000)
        assert [r != 0 for r in reasons] == [b == row for b in range(6)]
        assert np.array_equal(marks, want) and np.array_equal(lengths, want_len)
        assert f"row {row}" in message and word in message, message
        got = tm.apply_breaks(audio.cuda(), plan, 8).cpu()
        for b in range(6):                                       # the refused row is zeros; the others are what they are without it
            assert (torch.count_nonzero(got[b]) == 0) if b == row else torch.equal(got[b], clean_audio[b]), (row, b)
    # the lengthened row does not fit: refused alone, named
    marks, lengths, plan, message = device_plan(tm, cum, x_len, [1500] * 6, [good] * 2 + [[(2, 900), (5, 900)]] + [good] * 3, keep_max=ld,
                                                pause_max=1000, out_ld=ld + 152)
    assert lengths.tolist() == [1650, 1650, -1, 1650, 1650, 1650] and "row 2" in message and "does not fit" in message
    # the Python entry with host lists raises before a launch; with check=True it raises the device's verdict and names the row
    d_cum = torch.as_tensor(cum, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match=r"breaks\[1\].*strictly increase"):
        tm.token_marks(d_cum, x_len, [1500] * 6, [good, [(3, 1), (3, 1)]] + [None] * 4, keep_max=ld)
    with pytest.raises(ValueError, match=r"row 1 is refused: break 1 names a token outside"):
        tm.token_marks(d_cum, x_len, [1500] * 6, [good, [(2, 100), (11, 5)]] + [None] * 4, keep_max=ld)
    with pytest.raises(ValueError, match="keep_max="):
        tm.token_marks(d_cum, x_len, [1500] * 6, [good] + [None] * 5)


# ------------------------------------------------------------------------------------------------ end to end, tiny model
@pytest.fixture(scope="module")
def env(hipenv, hparams, synthetic):
    inf, voc = hipenv[2], sub("vocoder")
    hp = hparams.tiny(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to("cuda").eval()
    model.decoder.solver = "midpoint"
    vocos = voc.Vocos(**SMALL)
    vocos.load_state_dict(synthetic.make_vocos_state_dict(seed=23, **{k: v for k, v in SMALL.items() if k != "hop"}), strict=True)
    x, x_len, spk = synthetic.make_inputs(hp, 2, 12, seed=1234, lengths=[12, 9])
    out = model.synthesise(x.cuda(), x_len.cuda(), 2, speaker=spk.cuda(), debug=True, return_timing=True)     # once, shared, left unchanged
    return inf, hp, model, voc.VocosWrapper(vocos.to("cuda").eval()), (x, x_len, spk), out


def test_marks_from_synthesise_to_waveforms(env, tm):
    inf, hp, model, vocos, (x, x_len, spk), out = env
    durs = out["phoneme_durations"].cpu().numpy().astype(np.int64)
    assert np.array_equal(out["token_ends"].cpu().numpy(), np.cumsum(durs, 1)) and torch.equal(out["durations"], out["phoneme_durations"])
    plain = inf.to_waveforms(out["mel"], out["mel_lengths"], vocos)
    audio, marks = inf.to_waveforms(out["mel"], out["mel_lengths"], vocos, token_ends=out["token_ends"], x_lengths=x_len, return_marks=True)
    assert all(torch.equal(a, b) for a, b in zip(audio, plain))
    print("kept", [a.numel() for a in audio], "durations", durs.tolist())
    for b in range(2):
        n = int(x_len[b])
        _, want, _, _ = tr.plan_row(np.cumsum(durs[b]), n, audio[b].numel(), None, 12, fine_hop=FINE)
        assert marks[b] == [(int(s) / 24000, int(e) / 24000) for s, e in want[:n]] and len(marks[b]) == n
        assert marks[b][-1][1] <= audio[b].numel() / 24000 and marks[b][0][0] == 0.0
    # shaping through synthesise: one launch, the restatement's integers
    s = [[1.0] * 12, None]
    s[0][3], s[0][4] = 0.0, 2.0
    a = torch.zeros(2, 12)
    a[1, 2] = 3.0
    shaped = model.synthesise(x.cuda(), x_len.cuda(), 2, speaker=spk.cuda(), token_scale=s, token_extend=a, return_timing=True)
    d = shaped["durations"].cpu().numpy().astype(np.int64)
    s_full = np.ones((2, 12), dtype=np.float32)
    s_full[0, 3], s_full[0, 4] = 0.0, 2.0
    mask = (np.arange(12)[None] < x_len.numpy()[:, None]).astype(np.float32)
    want, want_cum, _, _ = tr.shaped_durations(torch.exp(out["logw"]).cpu().numpy()[:, 0], mask, [1.0, 1.0], [1.0, 1.0], s_full, a.numpy())
    assert np.array_equal(d, want.astype(np.int64)) and np.array_equal(shaped["token_ends"].cpu().numpy(), want_cum)
    assert d[0, 3] == 0 and d[0, 4] >= durs[0, 4] and d[1, 2] >= durs[1, 2] + 2
    assert np.array_equal(np.delete(d[0], [3, 4]), np.delete(durs[0], [3, 4])) and np.array_equal(np.delete(d[1], 2), np.delete(durs[1], 2))


def test_breaks_through_a_document_at_16k_pcm16(env, tm):
    inf, hp, model, vocos, (x, x_len, spk), out = env
    R = sub("resample")
    ends = dict(token_ends=out["token_ends"], x_lengths=x_len)
    doc = dict(documents=[2], gaps=[48, 0], fade_ms=0.5)
    breaks = [[(3, 10.0), (7, 2.5)], [(2, 5.0), (8, 1.0)]]
    base, seg0 = inf.to_waveforms(out["mel"], out["mel_lengths"], vocos, return_segments=True, **doc)
    floats, seg, marks = inf.to_waveforms(out["mel"], out["mel_lengths"], vocos, return_segments=True, breaks=breaks, return_marks=True,
                                          **doc, **ends)
    coded, seg16, marks16 = inf.to_waveforms(out["mel"], out["mel_lengths"], vocos, return_segments=True, breaks=breaks, return_marks=True,
                                             sample_rate=16000, encoding="pcm16", **doc, **ends)
    assert marks == marks16 and seg == seg16 and len(marks) == 1 and [len(m) for m in marks[0]] == [12, 9]
    # the restatement on the rows as the plan saw them: the plain rows' kept lengths, the durations of the shared call
    rows = inf.to_waveforms(out["mel"], out["mel_lengths"], vocos)
    durs = out["phoneme_durations"].cpu().numpy().astype(np.int64)
    at, applied = 0, 0
    for b in range(2):
        n = int(x_len[b])
        pauses = [(t, int(round(p * 24))) for t, p in breaks[b]]
        _, want, new_len, cuts = tr.plan_row(np.cumsum(durs[b]), n, rows[b].numel(), pauses, 12, fine_hop=FINE)
        assert marks[0][b] == [((int(s) + at) / 24000, (int(e) + at) / 24000) for s, e in want[:n]]
        assert seg[0][b] == (at / 24000, (at + new_len) / 24000)
        applied += sum(p for _, p in cuts)
        at += new_len + 48
    print("applied", applied, "joined", floats[0].numel())
    assert applied > 0 and floats[0].numel() == base[0].numel() + applied and floats[0].numel() == at - 48
    conv, n16 = R.resample(floats[0].cuda().reshape(1, -1), None, 24000, 16000)
    assert coded[0].dtype == torch.uint8 and coded[0].numel() == 2 * int(n16[0])
    # a break the device refuses names its row, through to_waveforms
    with pytest.raises(ValueError, match="row 1 is refused: break 0 names a token outside"):
        inf.to_waveforms(out["mel"], out["mel_lengths"], vocos, breaks=[None, [(9, 5.0)]], **ends)


def test_a_plain_request_a_marked_request_and_a_document_share_a_batch(env, tm, synthetic):
    inf, hp, model, vocos, _, _ = env
    bt = sub("batcher")
    ids = [synthetic.make_inputs(hp, 1, n, seed=60 + i)[0][0].tolist() for i, n in enumerate([14, 11, 9, 13])]
    kw = dict(speaker=1, solver="midpoint", n_timesteps=2)
    groups = [0, 0, 0, -1, 1, 1, 1, 1, -1, 2, 2]
    with bt.FrameBudgetBatcher(model, max_batch=8, max_tokens=4096, max_wait_ms=50.0, vocoder=vocos) as q:
        f_plain = q.submit(ids[0], **kw)
        f_marks = q.submit(ids[1], marks=True, word_groups=groups, **kw)
        f_doc = q.submit_document(ids[2:], [2.0, 0.0], breaks=[[(4, 3.0)], None], marks=True, level="sentence", **kw)
        plain, marked, doc = f_plain.result(timeout=120), f_marks.result(timeout=120), f_doc.result(timeout=120)
    assert q.batches_run == 1
    # today's path: the same batch without the new fields
    old = bt.synthesise_batch(model, [bt.Request(ids=ids[0], **kw), bt.Request(ids=ids[1], **kw),
                                      bt.Document(rows=[bt.Request(ids=t, **kw) for t in ids[2:]], pauses_ms=[2.0, 0.0], level="sentence")], vocos)
    assert set(plain) == set(old[0]) == {"mel", "mel_length", "audio"} and torch.equal(bits(plain["audio"]), bits(old[0]["audio"]))
    assert set(marked) == set(old[1]) | {"marks"} and torch.equal(bits(marked["audio"]), bits(old[1]["audio"]))
    tokens = marked["marks"]["tokens"]
    assert len(tokens) == 11 and tokens[0][0] == 0.0 and all(e0 == s1 for (_, e0), (s1, _) in zip(tokens, tokens[1:]))
    assert tokens[-1][1] <= marked["audio"].numel() / 24000
    assert marked["marks"]["words"] == [(tokens[0][0], tokens[2][1]), (tokens[4][0], tokens[7][1]), (tokens[9][0], tokens[10][1])]
    assert set(doc) == set(old[2]) | {"marks"} and [len(t) for t in doc["marks"]["tokens"]] == [9, 13] and "words" not in doc["marks"]
    pause = doc["audio"].numel() - old[2]["audio"].numel()
    assert pause in (0, 72)                                      # the break is applied (3 ms at 24 kHz) unless the trim left nothing behind its cut
    first, second = doc["marks"]["tokens"]
    assert first[5][0] - first[4][1] == pytest.approx(pause / 24000) and second[0][0] == pytest.approx(doc["segments"][1][0])
    assert second[-1][1] <= doc["audio"].numel() / 24000

"""CPU checks of token timing (nothing runs on a GPU): the new entries are declared in include/mtts.h, exported and bound with the
declared arity; every refusal the host can see returns -1 with a message and launches nothing; the host layers validate their fields
(``Request`` / ``Document`` / ``StepBatcher``); ``word_groups`` / ``word_marks`` on hand-written symbol lists; the caption writers parse
back; the identities of the restatement (tests/timing_restated.py); and ``synthesise`` / ``to_waveforms`` without the new arguments
make exactly the calls they made before."""
import inspect
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import timing_restated as tr


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


@pytest.fixture(scope="module")
def tm():
    return sub("timing")


@pytest.fixture(scope="module")
def bt():
    return sub("batcher")


def test_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_abi_version() == 2                          # entries were only added
    assert "timing.hip" in sub("_hip").SOURCES
    for word in ("e_k = min(max(fine_hop * cum[k - 1] - fine_hop / 2, 0), keep)", "start_i = e_i + P(<i)", "NOMINAL", "center=True",
                 "v = v * s;  v = v + a;", "(float)(2 i + 1) / (float)(2 F')"):
        assert word in header, word


#       cum      x_len    keep     B  Tx fine keep_max first    token    pause    NB pause_max out_max marks    out_len  ws       bytes    stream
PLAN = [0x10000, 0x20000, 0x30000, 3, 40, 128, 8192, 0x40000, 0x50000, 0x60000, 5, 24000, 40000, 0x70000, 0x80000, 0x90000, 1 << 20, None]
PLAN_NAMES = ["cum", "x_len", "keep", "B", "Tx", "fine_hop", "keep_max", "first", "token", "pause", "NB", "pause_max", "out_max", "marks",
              "out_len", "ws", "bytes"]
#         audio      ld    first    B  NB fade out        out_ld ws       bytes    stream
GATHER = [0x1000000, 1024, 0x40000, 3, 5, 120, 0x2000000, 2048, 0x90000, 1 << 20, None]
GATHER_NAMES = ["audio", "ld", "first", "B", "NB", "fade", "out", "out_ld", "ws", "bytes"]


def refused(fn, base, names, lib, **change):
    args = list(base)                                            # never launched: every call below is refused before
    for k, v in change.items():
        args[names.index(k)] = v
    assert fn(*args) == -1
    return lib.mtts_last_error()


def test_the_plan_refuses_what_the_host_can_see(lib):
    no = lambda **kw: refused(lib.mtts_token_timing, PLAN, PLAN_NAMES, lib, **kw)
    for k in ("cum", "x_len", "keep", "marks", "out_len", "ws", "token", "pause"):
        assert b"null" in no(**{k: None}), k
    for B in (0, -1, 70000):
        assert b"1 <= B <= 65535" in no(B=B), B
    assert b"Tx >= 1" in no(Tx=0)
    for v in (0, 1, 127, -128, 1 << 20):
        assert b"fine_hop" in no(fine_hop=v), v
    for kw in (dict(NB=-1), dict(NB=(1 << 27) + 1), dict(first=None, token=None, pause=None, NB=5)):
        assert b"NB" in no(**kw), kw
    for kw in (dict(keep_max=-1), dict(out_max=8191), dict(pause_max=-1), dict(out_max=(1 << 40) + 1)):
        assert b"keep_max <= out_max" in no(**kw), kw
    assert b"16-byte aligned" in no(ws=0x90008)
    need = lib.mtts_token_timing_workspace_bytes(3, 5)
    assert need >= 256 + 3 * 16 + 3 * 16 + 2 * 5 * 8
    assert b"workspace too small" in no(bytes=need - 257)
    assert b"workspace too small" in no(bytes=16)
    assert b"workspace too small" in no(bytes=-5)
    for B, NB in ((0, 0), (70000, 1), (3, -1), (3, (1 << 27) + 1)):
        assert lib.mtts_token_timing_workspace_bytes(B, NB) == -1 and b"1 <= B <= 65535" in lib.mtts_last_error()
    assert lib.mtts_token_timing_workspace_bytes(65535, 1 << 27) > 2 * 8 * (1 << 27)
    assert lib.mtts_token_timing_status(None, 3, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_token_timing_status(0x90000, 0, None) == -1 and b"1 <= B" in lib.mtts_last_error()


def test_the_gather_refuses_what_the_host_can_see(lib):
    no = lambda **kw: refused(lib.mtts_wave_breaks, GATHER, GATHER_NAMES, lib, **kw)
    for k in ("audio", "out", "ws"):
        assert b"null" in no(**{k: None}), k
    for B in (0, -3, 65536):
        assert b"1 <= B <= 65535" in no(B=B), B
    for kw in (dict(NB=-1), dict(first=None)):
        assert b"NB" in no(**kw), kw
    for k in ("ld", "out_ld"):
        for v in (1022, 0, -4, 2):
            assert b"multiples of 4" in no(**{k: v}), (k, v)
    for k, v in (("audio", GATHER[0] + 4), ("out", GATHER[6] + 8), ("ws", 0x90004)):
        assert b"16-byte aligned" in no(**{k: v}), k
    assert b"negative" in no(fade=-1)
    for out in (GATHER[0], GATHER[0] + 4096, GATHER[0] + 3 * 4096 - 16, GATHER[0] - 3 * 2048 * 4 + 16):
        assert b"overlaps" in no(out=out), hex(out)
    assert b"workspace too small" in no(bytes=lib.mtts_token_timing_workspace_bytes(3, 5) - 257)
    assert b"workspace too small" in no(bytes=0)


def test_shaped_durations_refuse_what_the_host_can_see(lib):
    #      logw     mask     sc       ls       given    rows     s        a        B  Tx dur      cum      yfl      stream
    ok = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 3, 9, 0x90000, 0xa0000, 0xb0000, None]
    names = ["logw", "mask", "sc", "ls", "given", "rows", "s", "a", "B", "Tx", "dur", "cum", "yfl"]
    no = lambda **kw: refused(lib.mtts_durations_shaped, ok, names, lib, **kw)
    for k in ("mask", "sc", "ls", "dur", "cum", "yfl"):
        assert b"null" in no(**{k: None}), k
    assert b"d_logw" in no(logw=None)                            # given rows are marked: the others are predicted
    assert b"d_logw" in no(logw=None, given=None, rows=None)
    assert b"d_given_rows without d_given" in no(given=None)
    assert b"bad shape" in no(B=0) and b"bad shape" in no(Tx=0)


def test_python_signatures_and_host_refusals(tm):
    inf = sub("inference")
    p = inspect.signature(inf.to_waveforms).parameters
    for name, default in (("token_ends", None), ("x_lengths", None), ("breaks", None), ("return_marks", False)):
        assert p[name].default is default and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-1] == "sample_rate"
    for fn in (inf.MatchaTTSInfer.synthesise, inf.MatchaTTSInfer._synthesise):
        p = inspect.signature(fn).parameters
        for name, default in (("token_scale", None), ("token_extend", None), ("return_timing", False)):
            assert p[name].default is default and p[name].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(sub("batcher").waveforms_into).parameters
    assert "units" in p and not {"loudness", "true_peak", "sample_rates", "encodings", "dithers", "dither_keys", "breaks"} & set(p)    # no per-field list to misplace
    mel = torch.zeros(2, 100, 8)
    for kw in (dict(return_marks=True), dict(breaks=[None, None]), dict(token_ends=torch.zeros(2, 3)), dict(return_marks=True, x_lengths=[3, 3])):
        with pytest.raises(ValueError, match="token_ends= and x_lengths="):
            inf.to_waveforms(mel, [8, 8], None, **kw)
    ends = dict(token_ends=torch.zeros(2, 3), x_lengths=[3, 3])
    for bad, word in (([[(0, 10.0)]], "one entry per row"), ([[(1, 5.0), (1, 5.0)], None], "strictly increase"), ([[(-1, 5.0)], None], "outside"),
                      ([[(0, -1.0)], None], "pause"), ([[(0, float("nan"))], None], "pause"), ([[(0, 1e9)], None], "pause"), ([[3], None], "entry")):
        with pytest.raises(ValueError, match=word):
            inf.to_waveforms(mel, [8, 8], None, breaks=bad, **ends)
    for name, bad in (("token_scale", [1.0, -0.5]), ("token_scale", [16.5]), ("token_scale", torch.tensor([float("nan")])),
                      ("token_extend", [4097.0]), ("token_extend", [[0.0], [-5000.0]]), ("token_extend", np.array([np.nan]))):
        with pytest.raises(ValueError, match=name):
            tm.check_shaping(bad, name)
    tm.check_shaping([[0.0, 16.0], None], "token_scale")
    tm.check_shaping(torch.tensor([-4096.0, 4096.0]), "token_extend")
    with pytest.raises(RuntimeError, match="HIP device"):
        tm.token_marks(torch.zeros(2, 3, dtype=torch.int32), [3, 3], [100, 100])


def test_request_and_document_fields_are_checked(bt):
    R = lambda **kw: bt.Request(ids=[1, 2, 3, 4], **kw)
    r = R(token_scale=[1, 0, 2, 16], token_extend=[0, -3, 4096, 0], breaks=[(0, 100), (3, 0.0)], marks=True, word_groups=[0, 0, -1, 1])
    assert r.breaks == [(0, 100.0), (3, 0.0)] and r.marks is True
    for kw, word in ((dict(token_scale=[1, 1, 1]), "one value per token"), (dict(token_extend=[0] * 5), "one value per token"),
                     (dict(word_groups=[0]), "one value per token"), (dict(token_scale=[1, 1, 1, 17]), "token_scale"),
                     (dict(token_scale=[1, 1, 1, -1]), "token_scale"), (dict(token_extend=[0, 0, 0, 5000]), "token_extend"),
                     (dict(breaks=[(4, 10)]), "outside"), (dict(breaks=[(2, 10), (1, 10)]), "strictly increase"),
                     (dict(breaks=[(1, 10), (1, 10)]), "strictly increase"), (dict(breaks=[(1, -10)]), "pause"),
                     (dict(breaks=[(1, 1e7)]), "pause"), (dict(breaks=[(1.5, 10)]), "outside")):
        with pytest.raises(ValueError, match=word):
            R(**kw)
    ends = ("token_ends", "x_lengths")                          # (what a synthesise call that was asked for its timing hands the tail)
    tail_breaks = lambda units: bt.tail_options(units, ends)["breaks"]
    assert bt.shaping_kwargs([R(), R()]) == {} and not {"token_ends", "breaks", "return_marks"} & set(bt.tail_options([R(), R()]))
    f = [R(), R(breaks=[(1, 20)]), R(token_scale=[1, 2, 1, 1])]
    assert tail_breaks(f) == [None, [(1, 20.0)], None] and not any(r.marks for r in f)
    assert bt.shaping_kwargs(f) == dict(token_scale=[None, None, [1, 2, 1, 1]], return_timing=True)
    assert bt.shaping_kwargs([R(token_extend=[0, 1, 0, 0])]) == dict(token_extend=[[0, 1, 0, 0]])
    assert bt.shaping_kwargs([R(marks=True)]) == dict(return_timing=True) and tail_breaks([R(marks=True)]) is None
    d = bt.Document(rows=[R(), R(breaks=[(0, 5)])], pauses_ms=[10.0, 0.0], marks=True)
    assert bt.shaping_kwargs(d.rows, [d]) == dict(return_timing=True) and tail_breaks([d]) == [None, [(0, 5.0)]]
    assert bt.shaping_kwargs([R(), R()], [bt.Document(rows=[R(), R()], pauses_ms=[0, 0], marks=True)]) == dict(return_timing=True)

    log = []

    def run(batch):
        log.append(batch)
        return [{"audio": torch.zeros(1)} for _ in batch]
    with bt.FrameBudgetBatcher(None, max_batch=4, max_tokens=100, max_wait_ms=20.0, run_batch=run) as q:
        with pytest.raises(ValueError, match="one entry per segment"):
            q.submit_document([[1, 2], [3]], [0.0, 0.0], breaks=[[(0, 10)]])
        with pytest.raises(ValueError, match="outside"):
            q.submit_document([[1, 2], [3]], [0.0, 0.0], breaks=[[(0, 10)], [(1, 10)]])
        fut = q.submit_document([[1, 2], [3]], [0.0, 0.0], breaks=[[(0, 10)], None], token_scale=[None, [0.5]], marks=True, speaker=2)
        fut.result(timeout=30)
    d = log[0][0]
    assert d.marks is True and [r.breaks for r in d.rows] == [[(0, 10.0)], None] and [r.token_scale for r in d.rows] == [None, [0.5]]
    assert all(r.speaker == 2 and r.marks is False for r in d.rows)


def test_step_batcher_refuses_the_timing_fields(bt):
    q = bt.StepBatcher.__new__(bt.StepBatcher)                  # submit refuses before it touches the queue: no model, no thread
    q.max_tokens = 100
    for kw in (dict(marks=True), dict(breaks=[(0, 10)]), dict(token_scale=[1.0, 2.0]), dict(token_extend=[0.0, 1.0])):
        with pytest.raises(ValueError, match="FrameBudgetBatcher"):
            q.submit([1, 2], **kw)


def test_word_groups_and_word_marks(tm):
    sym = [" ", "h", "ə", "l", "oʊ", " ", ",", " ", " ", "w", " ", "!", " "]
    g = tm.word_groups(sym)
    assert g == [-1, 0, 0, 0, 0, -1, 1, -1, -1, 2, -1, 3, -1]
    marks = [(float(i), float(i) + 1.0) for i in range(len(sym))]
    assert tm.word_marks(marks, g) == [(1.0, 5.0), (6.0, 7.0), (9.0, 10.0), (11.0, 12.0)]
    assert tm.word_groups([]) == [] and tm.word_groups([" ", " "]) == [-1, -1] and tm.word_marks([], []) == []
    assert tm.word_groups(["a"]) == [0] and tm.word_marks([(0.25, 0.5)], [0]) == [(0.25, 0.5)]
    assert tm.word_groups(["a", "_", "b"], space="_") == [0, -1, 1]
    assert tm.word_marks(marks[:3], g) == [(1.0, 3.0)]          # marks that end early: the word ends with them
    rows = tm.marks_rows(torch.tensor([[[0, 24000], [24000, 36000], [-1, -1]], [[-1, -1]] * 3]), offsets=[12000, 0])
    assert rows == [[(0.5, 1.5), (1.5, 2.0)], []]


def test_caption_writers_parse_back(tm):
    cues = [(0.0, 1.2345, "Dr. Smith arrived."), (1.5345, 3725.001, "Was he\nlate?  "), (3725.5, 3726.0, "a --> b")]
    vtt = tm.webvtt(cues)
    assert vtt.startswith("WEBVTT\n\n")
    got = re.findall(r"^(\d\d):(\d\d):(\d\d)\.(\d\d\d) --> (\d\d):(\d\d):(\d\d)\.(\d\d\d)\n(.*)\n$", vtt, flags=re.M)
    secs = lambda h, m, s, ms: int(h) * 3600 + int(m) * 60 + int(s) + int(ms) / 1000
    assert len(got) == 3
    for (start, end, text), g in zip(cues, got):
        assert abs(secs(*g[:4]) - start) <= 0.0005 and abs(secs(*g[4:8]) - end) <= 0.0005
        assert g[8] == " ".join(text.replace("-->", "->").split())
    body = tm.srt(cues)
    blocks = body.strip().split("\n\n")
    assert [b.split("\n")[0] for b in blocks] == ["1", "2", "3"]
    for (start, end, text), b in zip(cues, blocks):
        m = re.fullmatch(r"(\d\d):(\d\d):(\d\d),(\d\d\d) --> (\d\d):(\d\d):(\d\d),(\d\d\d)", b.split("\n")[1])
        assert m and abs(secs(*m.groups()[:4]) - start) <= 0.0005 and abs(secs(*m.groups()[4:]) - end) <= 0.0005
        assert "-->" not in b.split("\n")[2]
    assert "01:02:05.001" in vtt and "01:02:05,001" in body
    assert tm.webvtt([]) == "WEBVTT\n" and tm.srt([]) == ""


def test_restatement_identities():
    rng = np.random.default_rng(7)
    for trial in range(60):
        Tx = int(rng.integers(1, 30))
        x_len = int(rng.integers(1, Tx + 1))
        d = rng.integers(0, 6, Tx)
        d[x_len:] = 0
        cum = np.cumsum(d)
        total = 128 * int(cum[-1])
        # no breaks and keep at or above the nominal length: an interior token lasts fine_hop * d_i samples
        reason, marks, new_len, cuts = tr.plan_row(cum, x_len, total + int(rng.integers(0, 300)), None, Tx)
        assert reason == 0 and cuts == [] and new_len >= total
        first = next((i for i in range(x_len) if d[i] > 0), x_len)
        for i in range(first + 1, x_len):
            assert marks[i, 1] - marks[i, 0] == 128 * d[i], (trial, i)
        assert (marks[x_len:] == -1).all()
        # any keep, any breaks: marks do not decrease, and the new length is keep + the applied pauses
        keep = int(rng.integers(0, total + 200))
        toks = sorted(rng.choice(x_len, size=int(rng.integers(0, x_len + 1)), replace=False).tolist())
        breaks = [(t, int(rng.integers(0, 500))) for t in toks]
        reason, marks, new_len, cuts = tr.plan_row(cum, x_len, keep, breaks, Tx)
        assert reason == 0
        flat = marks[:x_len].reshape(-1)
        assert (np.diff(flat) >= 0).all() and flat[0] == 0
        assert new_len == keep + sum(p for _, p in cuts) and all(0 < c < keep for c, _ in cuts)
        assert marks[x_len - 1, 1] <= new_len
        audio = rng.standard_normal(keep + 8).astype(np.float32)
        row = tr.spliced_row(audio, keep, new_len, cuts, 0, new_len + 5)
        kept = np.concatenate([row[a:b] for a, b in zip([0] + [c + sum(p for _, p in cuts[:k + 1]) for k, (c, _) in enumerate(cuts)],
                                                         [c + sum(p for _, p in cuts[:k]) for k, (c, _) in enumerate(cuts)] + [new_len])])
        assert np.array_equal(kept, audio[:keep]) and not row[new_len:].any()     # fade 0: every sample is moved, nothing is lost
    # verdicts, one per reason
    cum = np.array([2, 4, 6, 6])
    assert tr.plan_row(cum, 0, 100, None, 4)[0] == 5 and tr.plan_row(cum, 5, 100, None, 4)[0] == 5
    assert tr.plan_row(cum, 3, -1, None, 4)[0] == 1 and tr.plan_row(cum, 3, 101, None, 4, keep_max=100)[0] == 1
    assert tr.plan_row(cum, 3, 100, [(3, 5)], 4)[0] == 2 and tr.plan_row(cum, 3, 100, [(1, 5), (1, 5)], 4)[0] == 3
    assert tr.plan_row(cum, 3, 100, [(1, 50)], 4, pause_max=49)[0] == 4 and tr.plan_row(cum, 3, 700, [(1, 50)], 4, out_max=749)[0] == 7
    # by hand: fine_hop 128, durations 2 2 2: e = 0, 192, 448, 704; a break of 100 after token 0
    reason, marks, new_len, cuts = tr.plan_row(cum, 3, 1000, [(0, 100)], 4)
    assert marks.tolist() == [[0, 192], [292, 548], [548, 804], [-1, -1]] and new_len == 1100 and cuts == [(192, 100)]
    row = tr.spliced_row(np.ones(1000, dtype=np.float32), 1000, 1100, cuts, 2, 1104)
    assert row[188:196].tolist() == [1, 1, .75, .25, 0, 0, 0, 0] and row[290:296].tolist() == [0, 0, .25, .75, 1, 1]
    assert row[0] == 1 and row[1099] == 1 and not row[1100:].any()
    # shaped durations by hand: identity shaping is the plain formula; a scale of 0 drops a token; the clamps and the NaN rule
    e = np.array([[4.0, 2.6, 9.0, 3.0]], dtype=np.float32)
    mask = np.ones((1, 4), dtype=np.float32)
    d, cumd, yfl, _ = tr.shaped_durations(e, mask, [1.0], [1.0])
    assert d.tolist() == [[2, 1, 7, 1]] and cumd.tolist() == [[2, 3, 10, 11]] and yfl.tolist() == [11]
    d, _, yfl, _ = tr.shaped_durations(e, mask, [1.0], [1.0], s=[[0, 2, -3, np.nan]], a=[[0, 0.4, 5, np.nan]])
    assert d.tolist() == [[0, 2, 5, 1]] and yfl.tolist() == [8]
    d, _, _, _ = tr.shaped_durations(e, mask, [1.0], [2.0], s=[[100, 1, 1, 1]], a=[[0, -1e9, 1e9, 0]], given=[[1, 3, 0, 2]])
    assert d.tolist() == [[32, 0, 4096, 4]]


class Recorder:
    """Stands for the ``hip`` object: records which methods are called and answers with small host tensors."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            if name.startswith("durations"):
                B, _, Tx = a[1].shape
                return torch.ones(B, Tx), torch.arange(1, Tx + 1, dtype=torch.int32).repeat(B, 1), torch.full((B,), Tx, dtype=torch.long)
            if name == "align_pool":
                B = a[0].shape[0]
                return torch.zeros(B, 4, a[3]), torch.ones(B, 1, a[3]), torch.full((B,), 2, dtype=torch.long)
            raise AssertionError(name)
        return call


def test_synthesise_without_the_new_arguments_makes_the_calls_of_before():
    inf = sub("inference")
    hip = Recorder()
    me = types.SimpleNamespace(
        _rt=types.SimpleNamespace(ready=lambda: hip, mel_std=1.0, mel_mean=0.0),
        _voice_rows=lambda B, dev, *a: (torch.zeros(B, 2), torch.zeros(B, 2)),
        encoder=lambda x, xl, e, d: (torch.zeros(x.shape[0], 4, x.shape[1]), torch.zeros(x.shape[0], 1, x.shape[1]), torch.ones(x.shape[0], 1, x.shape[1])),
        decoder=lambda mu_y, y_mask, n, **kw: torch.zeros(mu_y.shape[0], 4, kw["t_out"]),
        _given_durations=inf.MatchaTTSInfer._given_durations, _shaped_durations=inf.MatchaTTSInfer._shaped_durations)
    x = torch.zeros(2, 3, dtype=torch.long)
    run = lambda **kw: inf.MatchaTTSInfer._synthesise(me, x, torch.tensor([3, 2]), 2, **kw)
    out = run()
    assert hip.calls == ["durations", "align_pool"] and set(out) == {"mel", "mel_lengths"}
    hip.calls.clear()
    run(durations=torch.ones(2, 3))
    assert hip.calls == ["durations_given", "align_pool"]
    hip.calls.clear()
    out = run(return_timing=True)
    assert hip.calls == ["durations", "align_pool"] and set(out) == {"mel", "mel_lengths", "token_ends", "durations"}
    assert out["token_ends"].dtype == torch.int32
    for kw in (dict(token_scale=torch.ones(2, 3)), dict(token_extend=[None, [1.0, 0.0]]), dict(token_scale=[[0.5], None], durations=[None, [2, 2]])):
        hip.calls.clear()
        run(**kw)
        assert hip.calls == ["durations_shaped", "align_pool"], kw
    hip.calls.clear()
    with pytest.raises(ValueError, match="token_scale"):
        run(token_scale=[[17.0], None])
    with pytest.raises(ValueError, match="token_extend"):
        run(token_extend=torch.full((2, 3), -5000.0))
    assert hip.calls == []                                      # refused before anything is launched


def test_to_waveforms_without_the_new_arguments_makes_the_calls_of_before(monkeypatch, tm):
    inf, tail = sub("inference"), sub("waveform")
    calls = []

    class Head:
        cfg = {"hop": 256}

        def decode(self, mel, lengths, check=True):
            calls.append("decode")
            return torch.arange(2 * 256 * 7, dtype=torch.float32).reshape(2, -1) / 4096.0

    def finish(audio, lengths, hop=0, silence_threshold_db=-60.0):
        calls.append("finish")
        return torch.tensor([1000, 700]), torch.ones(2)

    def marks(cum, x_lengths, keep, breaks=None, **kw):
        calls.append("token_marks")
        assert kw == dict(fine_hop=128, keep_max=256 * 7, check=False) and keep.tolist() == [1000, 700]
        new = keep + torch.tensor([0 if not b else sum(p for _, p in b) for b in (breaks or [None, None])])
        plan = types.SimpleNamespace(NB=sum(len(b or ()) for b in (breaks or [])), raise_refused=lambda: None, lengths=new)
        m = torch.tensor([[[0, 500], [500, 1000]], [[0, 700], [-1, -1]]])
        return m, new, plan

    def gather(audio, plan, fade):
        calls.append(("apply_breaks", fade))
        return torch.cat([audio, torch.zeros(2, 2400)], 1)

    monkeypatch.setattr(tail, "finish_waveforms", finish)
    monkeypatch.setattr(tail._hip, "aligned_rows", lambda t, q, what, layout="": (t, t.shape[1]))
    monkeypatch.setattr(tm, "token_marks", marks)
    monkeypatch.setattr(tm, "apply_breaks", gather)
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, _e=torch.empty, **kw: _e(*a, **kw))
    mel = torch.zeros(2, 100, 8)
    plain = inf.to_waveforms(mel, [8, 5], Head())
    assert calls == ["decode", "finish"] and [len(a) for a in plain] == [1000, 700]
    calls.clear()
    ends = dict(token_ends=torch.zeros(2, 2, dtype=torch.int32), x_lengths=[2, 1])
    audio, got = inf.to_waveforms(mel, [8, 5], Head(), return_marks=True, **ends)
    assert calls == ["decode", "finish", "token_marks"]          # no break in the batch: the gather is not launched
    assert all(torch.equal(a, b) for a, b in zip(audio, plain))
    assert got == [[(0.0, 500 / 24000), (500 / 24000, 1000 / 24000)], [(0.0, 700 / 24000)]]
    calls.clear()
    audio = inf.to_waveforms(mel, [8, 5], Head(), breaks=[None, [(0, 100.0)]], fade_ms=5.0, **ends)
    assert calls == ["decode", "finish", "token_marks", ("apply_breaks", 120)] and [len(a) for a in audio] == [1000, 3100]


def test_the_service_carries_marks_to_the_batcher(bt, tm):
    sv = sub("serving")
    seen = []

    class Queue:
        def submit(self, ids, **kw):
            seen.append(("submit", list(ids), kw))
            return "future"

        def submit_document(self, segments, pauses, **kw):
            seen.append(("document", [list(s) for s in segments], kw))
            return "future"

    symbols = lambda text: [c for c in text]
    phonemize = lambda text, language: [ord(c) % 50 + 1 for c in text]
    groups = lambda text, language, ids: tm.word_groups(symbols(text))
    plain = sv.SpeechService(Queue(), phonemize)
    assert plain.submit("a bc") == "future" and "marks" not in seen[-1][2] and "word_groups" not in seen[-1][2]
    assert plain.timed().submit("a bc") == "future" and seen[-1][2]["marks"] is True and "word_groups" not in seen[-1][2]
    timed = sv.SpeechService(Queue(), phonemize, marks=True, word_groups=groups)
    timed.submit(" a bc ")
    assert seen[-1][2]["marks"] is True and seen[-1][2]["word_groups"] == [0, -1, 1, 1]        # the text is stripped, as it is phonemized
    assert timed.levelled(-16.0).marks is True and timed.timed(False).marks is False and timed.timed(False).word_groups is groups
    timed.timed(False).submit("a bc")
    assert "marks" not in seen[-1][2]
    timed.submit_long("One go. Two.")
    kind, segments, kw = seen[-1]
    assert kind == "document" and kw["marks"] is True and kw["word_groups"] == [tm.word_groups(symbols("One go.")), tm.word_groups(symbols("Two."))]
    timed.submit_long("One go. Two.", marks=False)
    assert "marks" not in seen[-1][2] and "word_groups" not in seen[-1][2]
    plain.submit_long("One go. Two.", marks=True)
    assert seen[-1][2]["marks"] is True and "word_groups" not in seen[-1][2]
    assert list(inspect.signature(sv.SpeechService.submit).parameters)[-1] == "response_format"                # submit and speak stay as they are
    assert list(inspect.signature(sv.SpeechService.speak).parameters)[-1] == "response_format"

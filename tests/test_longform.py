"""CPU checks of the host layers of long texts: the splitter of longform.py (the round-trip invariant and fixed cases), the unit
planner of the batcher (``plan_units`` equals ``plan_batch`` where there are no documents; documents are taken whole),
``submit_document`` (refusals at submit, a failing batch releases the future) and ``SpeechService.speak_long`` over a fake
``run_batch``.  Nothing touches a device."""
import asyncio
import random

import pytest
import torch

from conftest import sub


@pytest.fixture(scope="module")
def lf():
    return sub("longform")


@pytest.fixture(scope="module")
def bt():
    return sub("batcher")


# ------------------------------------------------------------------------------------------------ the splitter
def test_round_trip_on_punctuation_soup(lf):
    rng = random.Random(1234)
    words = ["a", "Bee", "sea", "Dr", "e.g", "3.14", "x,y", "Mr", "und", "NASA", "été", "naïve", "o'clock", "(so)", "“quoted”", "7"]
    marks = [".", "!", "?", "…", "?!", "...", ",", ";", ":", " —", ".\"", "?)", "", "", "", ""]
    spaces = [" ", " ", " ", "  ", "\n", "\n\n", " \n \n ", "\t"]
    for trial in range(300):
        text = "".join(rng.choice(words) + rng.choice(marks) + rng.choice(spaces) for _ in range(rng.randrange(1, 60)))
        for max_chars in (300, 40, 7, 1):
            pieces = lf.split_text(text, max_chars=max_chars)
            assert " ".join(seg for seg, _ in pieces) == lf.normalise_space(text), (trial, max_chars, text)
            assert all(seg and seg == seg.strip() for seg, _ in pieces)
            assert all(pause >= 0 for _, pause in pieces)
            assert all(len(seg) <= max_chars or " " not in seg for seg, _ in pieces), (trial, max_chars)
    assert lf.split_text("") == [] and lf.split_text(" \n\n \n") == []


def test_fixed_cases(lf):
    segs = lambda text, **kw: [s for s, _ in lf.split_text(text, **kw)]
    assert segs("Dr. Smith arrived. He sat down.") == ["Dr. Smith arrived.", "He sat down."]
    assert segs("Dr. Smith arrived. He sat.", abbreviations=()) == ["Dr.", "Smith arrived.", "He sat."]
    assert segs("Pi is 3.14 exactly. Or 3. 14 even.") == ["Pi is 3.14 exactly.", "Or 3. 14 even."]
    assert segs('"Really?" she said. "Yes."') == ['"Really?" she said.', '"Yes."']
    assert segs("What?! No way... Fine.") == ["What?!", "No way...", "Fine."]
    assert segs("Wait… Then go. (He went.) Done") == ["Wait…", "Then go.", "(He went.)", "Done"]
    assert segs("See e.g. the map, i.e. this one. Next.") == ["See e.g. the map, i.e. this one.", "Next."]
    assert segs("Das ist z.B. gut. Ende.", language="de-DE") == ["Das ist z.B. gut.", "Ende."]
    # the terminator stays with its sentence: the phonemizer reads "?" for intonation
    assert all(s[-1] in "?.!" for s in segs("Is it? It is! Good."))


def test_pauses(lf):
    text = "One. Two!\n\nThree? Four.\n \nFive"
    assert lf.split_text(text) == [("One.", 300.0), ("Two!", 600.0), ("Three?", 300.0), ("Four.", 600.0), ("Five", 600.0)]
    assert lf.split_text(text, sentence_ms=10, paragraph_ms=20)[:2] == [("One.", 10.0), ("Two!", 20.0)]
    assert lf.split_text("One.\nTwo.") == [("One.", 300.0), ("Two.", 600.0)]           # a single newline is a space


def test_long_sentences(lf):
    s = "alpha beta, gamma delta; epsilon zeta: eta theta — iota kappa lambda mu."
    pieces = lf.split_text(s, max_chars=30, clause_ms=120)
    assert pieces == [("alpha beta, gamma delta;", 120.0), ("epsilon zeta: eta theta —", 120.0), ("iota kappa lambda mu.", 600.0)]
    rng = random.Random(5)
    long = " ".join("".join(rng.choice("abcdefgh") for _ in range(rng.randrange(1, 9))) for _ in range(230))[:999] + "."
    assert len(long) == 1000 and "," not in long
    pieces = lf.split_text(long, max_chars=300)
    assert " ".join(seg for seg, _ in pieces) == long
    assert all(len(seg) <= 300 for seg, _ in pieces) and len(pieces) == 4
    assert [p for _, p in pieces] == [0.0, 0.0, 0.0, 600.0]       # cut at spaces: no pause is invented
    assert lf.split_text("x" * 50 + " y", max_chars=10) == [("x" * 50, 0.0), ("y", 600.0)]    # a word is never cut
    with pytest.raises(ValueError):
        lf.split_text("a", max_chars=0)


# ------------------------------------------------------------------------------------------------ the planner
def test_plan_units_is_plan_batch_without_documents(bt):
    rng = random.Random(99)
    for trial in range(200):
        n = rng.randrange(0, 40)
        waiting = [bt.Request(ids=[1] * rng.randrange(1, 200), solver=rng.choice(["midpoint", "euler"]), n_timesteps=rng.choice([2, 4]))
                   for _ in range(n)]
        max_batch, max_tokens = rng.choice([1, 2, 4, 8, 32]), rng.choice([64, 256, 1024, 8192])
        assert bt.plan_units(waiting, max_batch, max_tokens) == bt.plan_batch(waiting, max_batch, max_tokens), trial


def doc(bt, sizes, **kw):
    return bt.Document(rows=[bt.Request(ids=[1] * n, **kw) for n in sizes], pauses_ms=[100.0] * len(sizes))


def test_documents_are_taken_whole(bt):
    r = lambda n, **kw: bt.Request(ids=[1] * n, **kw)
    # the head document goes whole, then the nearest units that still fit: 3 + 3 + 1 rows = 7 <= 8; the 2-row document would make 9,
    # and the 300-token request 8 rows x 300 tokens
    waiting = [doc(bt, [50, 40, 45]), r(48), doc(bt, [52, 30]), doc(bt, [50, 50, 50]), r(300)]
    assert bt.plan_units(waiting, 8, 2000) == [0, 1, 3]
    assert bt.plan_units(waiting, 8, 8192) == [0, 1, 3, 4]
    assert bt.plan_units(waiting, 3, 8192) == [0]
    assert bt.plan_units(waiting, 2, 8192) == [0]               # the head is always taken, whole (submit keeps such a one out)
    # the token budget counts rows x longest over the whole batch: with the 300-token request the 4 rows would cost 1200
    assert bt.plan_units([doc(bt, [50, 40, 45]), r(300)], 8, 1000) == [0]
    assert bt.plan_units([doc(bt, [50, 40, 45]), r(300)], 8, 1200) == [0, 1]
    # other groups stay behind, documents included
    waiting = [r(40), doc(bt, [40, 40], solver="euler"), doc(bt, [41, 39])]
    assert bt.plan_units(waiting, 8, 8192) == [0, 2]
    # a plain request at the head takes a document as one unit
    assert bt.plan_units([r(40), doc(bt, [40] * 7), r(41)], 8, 8192) == [0, 1]
    assert bt.plan_units([r(40), doc(bt, [40] * 8), r(41)], 8, 8192) == [0, 2]


def test_document_fields_are_checked(bt):
    with pytest.raises(ValueError, match="at least one segment"):
        bt.Document(rows=[], pauses_ms=[])
    with pytest.raises(ValueError, match="empty segment"):
        doc(bt, [3, 0])
    with pytest.raises(ValueError, match="one value per segment"):
        bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[1.0, 2.0])
    with pytest.raises(ValueError, match="level"):
        bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0.0], level="word")
    with pytest.raises(ValueError):
        bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0.0], encoding="mp3")
    assert doc(bt, [3, 4]).gaps() == [2400, 2400] and bt.Document(rows=[bt.Request(ids=[1])], pauses_ms=[0.5]).gaps() == [12]


def fake_run(log):
    def run(batch):
        log.append(batch)
        bt = sub("batcher")
        res = []
        for u in batch:
            if isinstance(u, bt.Document):
                at, seg = 0.0, []
                for r, g in zip(u.rows, u.gaps()):
                    seg.append((at, at + len(r.ids) / 100.0))
                    at += len(r.ids) / 100.0 + g / 24000
                r = {"audio": torch.arange(sum(len(r.ids) for r in u.rows), dtype=torch.float32) / 1000.0, "segments": seg,
                     "mel_lengths": [len(r.ids) for r in u.rows]}
                if u.encoding is not None:
                    r["audio"] = torch.arange(8, dtype=torch.uint8)
                    r["encoding"] = u.encoding
                if u.sample_rate != 24000:
                    r["sample_rate"] = u.sample_rate
                res.append(r)
            else:
                res.append({"mel": None, "mel_length": len(u.ids)})
        return res
    return run


def test_submit_document(bt):
    log = []
    with bt.FrameBudgetBatcher(None, max_batch=4, max_tokens=100, max_wait_ms=50.0, run_batch=fake_run(log)) as q:
        with pytest.raises(ValueError, match="exceeds the batch of 4"):
            q.submit_document([[1]] * 5, [0.0] * 5)
        with pytest.raises(ValueError, match="exceeds the batch budget of 100"):
            q.submit_document([[1] * 30, [1] * 10, [1] * 10, [1] * 10], [0.0] * 4)
        with pytest.raises(ValueError, match="empty segment"):
            q.submit_document([[1, 2], []], [0.0, 0.0])
        with pytest.raises(ValueError, match="at least one segment"):
            q.submit_document([], [])
        with pytest.raises(ValueError, match="one value per segment"):
            q.submit_document([[1, 2]], [])
        f_doc = q.submit_document([[1] * 10, [2] * 12, [3] * 9], [300.0, 600.0, 0.0], speaker=4, n_timesteps=2, sample_rate=8000, encoding="ulaw")
        f_one = q.submit([5] * 11, n_timesteps=2)
        res, one = f_doc.result(timeout=30), f_one.result(timeout=30)
    assert not hasattr(bt.StepBatcher, "submit_document")
    assert q.batches_run == 1 and len(log) == 1 and len(log[0]) == 2      # one batch: a document and a request
    d = log[0][0]
    assert isinstance(d, bt.Document) and [r.speaker for r in d.rows] == [4, 4, 4] and d.gaps() == [7200, 14400, 0]
    assert all(r.sample_rate == 24000 and r.encoding is None for r in d.rows) and (d.sample_rate, d.encoding) == (8000, "ulaw")
    assert set(res) == {"audio", "segments", "mel_lengths", "sample_rate", "encoding"} and res["mel_lengths"] == [10, 12, 9]
    assert one == {"mel": None, "mel_length": 11}


def test_a_failing_batch_releases_the_document(bt):
    def boom(batch):
        raise RuntimeError("device lost")
    with bt.FrameBudgetBatcher(None, max_batch=4, max_tokens=100, max_wait_ms=20.0, run_batch=boom) as q:
        f_doc = q.submit_document([[1] * 10, [2] * 12], [300.0, 0.0])
        f_one = q.submit([5] * 11)
        with pytest.raises(RuntimeError, match="device lost"):
            f_doc.result(timeout=30)
        with pytest.raises(RuntimeError, match="device lost"):
            f_one.result(timeout=30)


def test_synthesise_batch_needs_a_vocoder_for_a_document(bt):
    with pytest.raises(ValueError, match="needs a vocoder"):
        bt.synthesise_batch(None, [doc(bt, [3, 4])], None)


# ------------------------------------------------------------------------------------------------ the service
def test_speak_long_over_a_fake_batch(bt):
    sv = sub("serving")
    log, spoken = [], []

    def phonemize(text, language):
        spoken.append((text, language))
        return [ord(c) % 50 + 1 for c in text]

    text = "Dr. Smith arrived. Was he late?\n\nNo."
    with bt.FrameBudgetBatcher(None, max_batch=512, max_tokens=4096, max_wait_ms=20.0, run_batch=fake_run(log)) as q:
        service = sv.SpeechService(q, phonemize)
        audio = asyncio.run(service.speak_long(text, voice=0, speed=2.0))
        body = asyncio.run(service.speak_long(text, voice=0, response_format="ulaw", sample_rate=8000, sentence_ms=50))
        with pytest.raises(ValueError, match="unknown response_format"):
            service.submit_long(text, response_format="mp3")
        with pytest.raises(ValueError, match="exceeds 10 characters"):
            service.submit_long(text, max_document_length=10)
        with pytest.raises(ValueError, match="empty text"):
            service.submit_long("  \n ")
        with pytest.raises(ValueError, match="Text exceeds 1000 characters"):      # the one-utterance route keeps its cap
            service.submit("x" * 1001)
        long = asyncio.run(service.speak_long("Go on. " * 400))                    # 2800 characters: above submit's cap
    assert [t for t, _ in spoken[:3]] == ["Dr. Smith arrived.", "Was he late?", "No."]
    assert len({lang for _, lang in spoken}) == 1
    d = log[0][0]
    assert isinstance(d, bt.Document) and list(d.pauses_ms) == [300.0, 600.0, 600.0]
    assert all(r.length_scale == 0.5 and r.solver == d.rows[0].solver for r in d.rows)
    assert torch.is_tensor(audio) and audio.numel() == sum(len(t) for t, _ in spoken[:3])
    assert isinstance(body, bytes) and body == bytes(range(8))
    assert list(log[1][0].pauses_ms) == [50.0, 600.0, 600.0] and (log[1][0].sample_rate, log[1][0].encoding) == (8000, "ulaw")
    assert long.numel() == 400 * 6

    class NoDocuments:
        def submit(self, ids, **kw):
            raise AssertionError("not reached")
    with pytest.raises(TypeError, match="submit_document"):
        sv.SpeechService(NoDocuments(), phonemize).submit_long(text)

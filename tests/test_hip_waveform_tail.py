"""The batched waveform tail on an MI355X, everything at once: one ``to_waveforms`` call with documents, gaps, a break, a loudness
target under a true-peak ceiling, two output rates, an encoded and a float document, segments, meter and marks equals, bit for bit and
entry for entry, the same stages called by hand in the documented order through the public functions; and the per-request tail --
``waveforms_into(wave_batch=False)`` and ``finish_request``, which ``pipeline`` ends in -- gives the bytes of the batched one.  And the
layer above: a document and four requests that each ask something else, through ``synthesise_batch`` in one call, get the results of one
``waveform.tail`` call written out by hand on the same mel.
The small vocoder of tests/test_hip_r128.py: ragged rows, a two-row document and a row shorter than one trim window."""
import math

import pytest
import torch

from conftest import sub

pytestmark = pytest.mark.gpu

SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)
LENGTHS, T = [40, 33, 25, 12], 40


@pytest.fixture(scope="module")
def env(synthetic):
    voc = sub("vocoder")
    vocos = voc.Vocos(**SMALL)
    vocos.load_state_dict(synthetic.make_vocos_state_dict(seed=23, **{k: v for k, v in SMALL.items() if k != "hop"}), strict=True)
    mel = (torch.randn(4, SMALL["n_mels"], T, generator=torch.Generator().manual_seed(3)) * 2.0 - 4.0).cuda()
    return voc.VocosWrapper(vocos.to("cuda").eval()), mel


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_everything_at_once_is_the_stages_by_hand(env):
    vocos, mel = env
    inf, tm, L, R, AC = sub("inference"), sub("timing"), sub("loudness"), sub("resample"), sub("audio_codec")
    hop, fade_ms = SMALL["hop"], 2.0
    gaps, breaks = [120, 0, 96, 0], [None, [(0, 10.0)], None, None]
    ends = torch.tensor([[2 * n // 3, 4 * n // 3, 2 * n] for n in LENGTHS], dtype=torch.int32).cuda()     # fine frames: hop / 2 samples each
    x_len = [3, 3, 3, 3]
    out, segments, report, marks = inf.to_waveforms(
        mel, LENGTHS, vocos, documents=[2, 2], gaps=gaps, fade_ms=fade_ms, breaks=breaks, token_ends=ends, x_lengths=x_len,
        loudness=[-16.0, None], true_peak=[-1.0, None], sample_rate=[16000, 24000], encoding=["pcm16", None], dither=[True, False],
        dither_keys=[5, 0], return_segments=True, return_meter=True, return_marks=True)
    # by hand, in the documented order: decode, finish, timing plan + breaks gather, join, loudness, rate conversion, encode
    lengths = torch.tensor(LENGTHS).cuda()
    fade = int(round(fade_ms * 24000 / 1000.0))
    audio = vocos.model.decode(mel, lengths)
    keep, scale = inf.finish_waveforms(audio, lengths, hop=hop)
    cuts = [[(t, int(round(p * 24.0))) for t, p in row or ()] for row in breaks]
    d_marks, n, plan = tm.token_marks(ends, x_len, keep, cuts, fine_hop=hop // 2, keep_max=audio.shape[1])
    rows = tm.apply_breaks(audio, plan, fade)
    wave, doc_len, starts = inf.join_waveforms(rows, n, [2, 2], gaps, fade=fade, scale=scale)
    meter = L.normalize(wave, doc_len, [-16.0, None], true_peak=-1.0, return_meter=True)[3]
    conv, conv_len = R.resample(wave[:1], doc_len[:1], 24000, 16000)
    data, nbytes = AC.encode(conv, conv_len, "pcm16", dither=True, keys=[5])
    assert len(out) == 2 and same(out[0], data[0, :int(nbytes[0])].cpu()) and same(out[1], wave[1, :int(doc_len[1])].cpu())
    assert out[0].dtype == torch.uint8 and out[0].numel() == 2 * int(conv_len[0]) and out[1].dtype == torch.float32
    begin, n = starts.tolist(), n.tolist()
    assert n[1] > int(keep[1]) and begin[1] >= n[0] + 120 and begin[3] >= n[2] + 96                   # the break lengthened row 1
    assert segments == [[(begin[b] / 24000, (begin[b] + n[b]) / 24000) for b in doc] for doc in ((0, 1), (2, 3))]
    per_row = tm.marks_rows(d_marks.cpu(), 4, begin)
    assert marks == [per_row[0:2], per_row[2:4]] and all(len(r) == 3 for r in per_row)
    assert [set(r) for r in report] == [set(inf.METER_FIGURES)] * 2
    for g, r in enumerate(report):
        for k in inf.METER_FIGURES:
            want = float(meter[k][g])
            assert r[k] == want or (math.isnan(r[k]) and math.isnan(want)), (g, k, r[k], want)
    assert report[0]["gain"] != 1.0 and report[1]["gain"] == 1.0


def test_the_per_request_tails_give_the_bytes_of_the_batched_one(env):
    vocos, mel = env
    bt, wf = sub("batcher"), sub("waveform")
    rates, encs, dith, keys = [24000, 16000, 24000, 8000], [None, "pcm16", "ulaw", None], [False, True, False, False], [0, 7, 0, 0]
    loud, ceil = [-16.0, None, -20.0, None], [-1.0, None, None, None]

    def requests(wave_batch):
        res = [{"mel": mel[b, :, :n], "mel_length": n} for b, n in enumerate(LENGTHS)]
        units = [bt.Request(ids=[1], sample_rate=rates[b], encoding=encs[b], dither=dith[b], dither_key=keys[b], loudness=loud[b], true_peak=ceil[b])
                 for b in range(4)]
        bt.waveforms_into(res, mel, torch.tensor(LENGTHS).cuda(), vocos, wave_batch, units)
        return res
    batched, looped = requests(True), requests(False)
    for b, (a, r) in enumerate(zip(batched, looped)):
        one = wf.trim_trailing_silence(wf._waveform_on_device(mel[b:b + 1, :, :LENGTHS[b]], vocos).squeeze())
        alone, rep = wf.finish_request(one, loudness=loud[b], true_peak=ceil[b], report=True, sample_rate=rates[b], encoding=encs[b],
                                       dither=dith[b], dither_key=keys[b])
        assert same(a["audio"], r["audio"]) and same(a["audio"], alone), b
        assert set(a) == set(r) and all(a[k] == r[k] for k in set(a) - {"audio", "mel"}), (b, a, r)
        assert (rep is None) == (loud[b] is None) and a["audio"].dtype == (torch.float32 if encs[b] is None else torch.uint8)


def test_a_document_and_requests_through_the_batcher_are_one_tail_call_by_hand(env, hparams, synthetic, monkeypatch):
    vocos, _ = env
    bt, wf, inf, tm, L = sub("batcher"), sub("waveform"), sub("inference"), sub("timing"), sub("loudness")
    hp = hparams.tiny(n_spks=2)                                   # (n_feats = 20: the mel the small vocoder takes)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.cuda().eval()
    counts = [9, 12, 5, 8, 11, 7]
    ids = [synthetic.make_inputs(hp, 1, n, seed=60 + i)[0][0].tolist() for i, n in enumerate(counts)]
    kw = dict(speaker=1, solver="midpoint", n_timesteps=2)
    groups = [[i // 3 for i in range(9)], [i // 4 for i in range(12)]]
    sentences = lambda: [bt.Request(ids=ids[0], word_groups=groups[0], **kw), bt.Request(ids=ids[1], word_groups=groups[1], breaks=[(3, 15.0)], **kw)]
    requests = lambda: [bt.Request(ids=ids[2], **kw), bt.Request(ids=ids[3], sample_rate=8000, encoding="ulaw", **kw),
                        bt.Request(ids=ids[4], encoding="flac", dither_key=7, **kw), bt.Request(ids=ids[5], loudness=-20, **kw)]
    doc = bt.Document(rows=sentences(), pauses_ms=[200.0, 0.0], level="document", sample_rate=16000, encoding="pcm16", dither=True, loudness=-16,
                      true_peak=-1, marks=True)
    kept, synthesise = [], model.synthesise
    monkeypatch.setattr(model, "synthesise", lambda *a, **k: kept.append(synthesise(*a, **k)) or kept[-1])
    got = bt.synthesise_batch(model, [doc] + requests(), vocos, True, 4.0)
    out = kept[0]
    hand = wf.tail(out["mel"], out["mel_lengths"], vocos, documents=[2, 1, 1, 1, 1], gaps=[4800, 0, 0, 0, 0, 0], fade_ms=4.0,
                   level=["document", "sentence", "sentence", "sentence", "sentence"], return_segments=True,
                   sample_rate=[16000, 24000, 8000, 24000, 24000], encoding=["pcm16", None, "ulaw", "flac", None],
                   dither=[True, False, False, False, False], dither_keys=[0, 0, 0, 7, 0], loudness=[-16.0, None, None, None, -20.0],
                   return_loudness=True, true_peak=[-1.0, None, None, None, None], return_meter=True, token_ends=out["token_ends"],
                   x_lengths=counts, breaks=[None, [(3, 15.0)], None, None, None, None], return_marks=True)
    value = lambda a, b: a == b or (a != a and b != b)          # (a figure that is no number is the same one on both sides)
    lens = [int(n) for n in out["mel_lengths"].tolist()]
    assert len(kept) == 1 and len(got) == 5 == len(hand.rows) and all(same(r["audio"], a) for r, a in zip(got, hand.rows))
    d, rep = got[0], hand.report[0]
    assert set(d) == {"audio", "segments", "mel_lengths", "sample_rate", "encoding", "loudness", "gain", "true_peak", "lra", "marks"}
    assert d["audio"].dtype == torch.uint8 and d["mel_lengths"] == lens[:2] and d["segments"] == hand.segments[0] and len(d["segments"]) == 2
    assert (d["sample_rate"], d["encoding"]) == (16000, "pcm16")
    assert d["marks"] == {"tokens": hand.marks[0], "words": [tm.word_marks(t, g) for t, g in zip(hand.marks[0], groups)]}
    assert [len(t) for t in d["marks"]["tokens"]] == counts[:2] and [len(w) for w in d["marks"]["words"]] == [3, 3]
    assert value(d["loudness"], rep["lufs"]) and value(d["gain"], rep["gain"]) and value(d["true_peak"], L.dbtp(rep["true_peak"])) and value(d["lra"], rep["lra"])
    for g, (r, extra) in enumerate(zip(got[1:], (set(), {"sample_rate", "encoding"}, {"encoding"}, {"loudness", "gain"})), 1):
        assert set(r) == {"mel", "mel_length", "audio"} | extra, g
        assert r["mel_length"] == lens[g + 1] and torch.equal(r["mel"], out["mel"][g + 1, :, :lens[g + 1]]), g
    assert (got[2]["sample_rate"], got[2]["encoding"], got[3]["encoding"]) == (8000, "ulaw", "flac")
    assert got[1]["audio"].dtype == torch.float32 and got[2]["audio"].dtype == got[3]["audio"].dtype == torch.uint8
    assert value(got[4]["loudness"], hand.report[4]["lufs"]) and value(got[4]["gain"], hand.report[4]["gain"])
    # the same six rows as plain requests, no document: every plain request keeps exactly its keys and its bits
    alone = bt.synthesise_batch(model, sentences() + requests(), vocos, True, 4.0)
    assert len(alone) == 6
    for g, (a, b) in enumerate(zip(got[1:], alone[2:])):
        assert set(a) == set(b), g
        assert a["mel_length"] == b["mel_length"] and torch.equal(a["mel"], b["mel"]) and same(a["audio"], b["audio"]), g
        assert all(value(a[k], b[k]) for k in set(a) - {"mel", "audio"}), (g, a, b)

"""The document join on the GPU (mtts_wave_join): every comparison is bit-equal to the torch restatement of tests/join_restated.py,
and the output buffer is pre-filled with NaN, so a word the kernels did not write shows.  Then the join inside
`inference.to_waveforms(documents=...)` and inside the batcher, on the synthetic model and vocoder of tests/test_hip_wave_batch.py."""
import numpy as np
import pytest
import torch

from conftest import sub
import join_restated as jr

pytestmark = pytest.mark.gpu
SENTINEL = 3.0e30          # what sits in a row beyond its length: a kernel that reads there shows it


@pytest.fixture(scope="module")
def hipenv():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("_hip"), sub("_hip").load(), sub("inference")


def rows(lengths, ld, seed, amp=0.5):
    g = torch.Generator().manual_seed(seed)
    audio = torch.randn(len(lengths), ld, generator=g) * amp
    for b, n in enumerate(lengths):
        if 0 <= n < ld:
            audio[b, n:] = SENTINEL
    return audio


def device_join(hipenv, audio, lengths, first_row, gaps, fade=0, scale=None, out_ld=None, gap_max=None):
    """mtts_wave_join on a NaN-filled output: (out, out_lengths, starts) on the host and the status call's message (None: accepted)."""
    hip, lib, _ = hipenv
    B, ld = audio.shape
    G = len(first_row) - 1
    out_ld = jr.default_out_ld(ld, first_row, gaps) if out_ld is None else out_ld
    gap_max = max([0] + list(gaps)) if gap_max is None else gap_max
    d_audio = audio.cuda()
    d_len = torch.tensor(lengths, dtype=torch.long).cuda()
    d_first = torch.tensor(first_row, dtype=torch.int32).cuda()
    d_gap = torch.tensor(gaps, dtype=torch.long).cuda()
    d_scale = None if scale is None else torch.as_tensor(scale, dtype=torch.float32).cuda()
    out = torch.full((G, out_ld), float("nan"), dtype=torch.float32).cuda()
    out_len = torch.full((G,), -7, dtype=torch.long).cuda()
    starts = torch.full((B,), -7, dtype=torch.long).cuda()
    ws = torch.zeros(lib.mtts_wave_join_workspace_bytes(B, G), dtype=torch.uint8).cuda()
    hip.check(lib.mtts_wave_join(hip.ptr(d_audio), ld, hip.ptr(d_len), hip.ptr(d_scale), hip.ptr(d_first), hip.ptr(d_gap), B, G, fade, gap_max,
                                 hip.ptr(out), out_ld, hip.ptr(out_len), hip.ptr(starts), ws.data_ptr(), ws.numel(), hip.stream_ptr()))
    message = None
    if lib.mtts_wave_join_status(ws.data_ptr(), hip.stream_ptr()) != 0:
        message = lib.mtts_last_error().decode()
    assert torch.equal(d_audio.cpu(), audio)                     # the input is read only
    return out.cpu(), out_len.cpu(), starts.cpu(), message


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


def check_against_restatement(hipenv, audio, lengths, first_row, gaps, **kw):
    got = device_join(hipenv, audio, lengths, first_row, gaps, **kw)
    want = jr.join(audio, lengths, first_row, gaps, **kw)
    assert got[1].tolist() == want[1].tolist(), (got[1].tolist(), want[1].tolist())
    assert got[2].tolist() == want[2].tolist(), (got[2].tolist(), want[2].tolist())
    assert not torch.isnan(got[0]).any(), "a word of the output was not written"
    assert same_bits(got[0], want[0])
    if want[3] is None:
        assert got[3] is None, got[3]
    else:
        row, length, reason = want[3]
        assert got[3] is not None and f"row {row} (length {length})" in got[3], (got[3], want[3])
        assert {1: "its length is outside", 2: "the layout or a gap", 3: "does not fit out_ld"}[reason] in got[3], (got[3], want[3])
    return got, want


FIRST = [0, 3, 4, 6, 7]                                          # documents of 3 / 1 / 2 / 1 rows
LAYOUTS = {
    # a full row, a row of no samples inside a document, a document of one empty row; rows of 0 / 5 / 1 / 2 samples at joints
    "a": ([1024, 0, 5, 0, 1, 2, 777], [1, 5, 0, 0, 241, 0, 0]),
    "b": ([2, 1, 1024, 0, 5, 1000, 3], [0, 0, 7, 3, 241, 0, 0]),
}


@pytest.mark.parametrize("fade", [0, 1, 3, 120])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_alignments_and_edges(hipenv, layout, fade):
    lengths, gaps = LAYOUTS[layout]
    audio = rows(lengths, 1024, 5)
    got, _ = check_against_restatement(hipenv, audio, lengths, FIRST, gaps, fade=fade)
    if fade == 0:                                                # no weights at all: every kept sample is moved
        for g in range(4):
            for b in range(FIRST[g], FIRST[g + 1]):
                s = int(got[2][b])
                assert same_bits(got[0][g, s:s + lengths[b]], audio[b, :lengths[b]])


def test_the_two_layouts_cover_every_alignment_of_a_start():
    seen = set()
    for lengths, gaps in LAYOUTS.values():
        seen |= {int(s) % 4 for s in jr.join(torch.zeros(7, 1024), lengths, FIRST, gaps)[2]}
    assert seen == {0, 1, 2, 3}


def test_tile_seam(hipenv):
    # 2 tiles of 2048 and 3 samples: the gap after row 0 lies across the first seam (2044 .. 2052), the joint of rows 1 and 2 on the
    # second one (row 1 fades out up to sample 4095, row 2 fades in from sample 4096)
    lengths, gaps = [2044, 2044, 3], [8, 0, 0]
    audio = rows(lengths, 2048, 6)
    got, _ = check_against_restatement(hipenv, audio, lengths, [0, 3], gaps, fade=3)
    assert got[1].tolist() == [2 * 2048 + 3] and got[2].tolist() == [0, 2052, 4096]


def test_one_gain_per_document(hipenv):
    lengths, gaps, first = [300, 200, 257, 100, 50], [3, 0, 0, 9, 0], [0, 3, 5]
    audio = rows(lengths, 300, 7)
    scale = torch.tensor([1.0, 0.95 / 1.3, 0.95 / 2.9, 1.0, 1.0])
    got, _ = check_against_restatement(hipenv, audio, lengths, first, gaps, fade=0, scale=scale)
    out, starts = got[0], got[2].tolist()
    for b in (2, 3, 4):                                          # the loudest row of document 0 and all of document 1: moved bit for bit
        g = 0 if b < 3 else 1
        assert same_bits(out[g, starts[b]:starts[b] + lengths[b]], audio[b, :lengths[b]]), b
    r = scale[2] / scale[0]
    assert same_bits(out[0, :300], audio[0] * r) and float(r) < 1.0
    got, _ = check_against_restatement(hipenv, audio, lengths, first, gaps, fade=3, scale=scale)
    w = torch.tensor([1.0, 3.0, 5.0]) / torch.tensor(6.0)
    r1 = scale[2] / scale[1]
    s1 = got[2].tolist()[1]
    assert same_bits(got[0][0, s1:s1 + 3], (audio[1, :3] * r1) * w)           # (x * r) * w, in that order


def test_more_rows_than_the_plan_has_threads(hipenv):
    g = torch.Generator().manual_seed(8)
    lengths = [int(v) for v in torch.randint(1, 9, (257,), generator=g)]
    gaps = [0] * 257
    audio = rows(lengths, 8, 9)
    got, _ = check_against_restatement(hipenv, audio, lengths, [0, 257], gaps, fade=2)
    assert int(got[1][0]) == sum(lengths) < 2048                 # one tile holds all 257 rows: more than one stage of the move
    lengths[-1] = 9
    got, _ = check_against_restatement(hipenv, audio, lengths, [0, 257], gaps, fade=2)
    assert got[1].tolist() == [-1] and set(got[2].tolist()) == {-1} and torch.count_nonzero(got[0]) == 0
    assert "row 256 (length 9)" in got[3] and "its length is outside [0, ld = 8]" in got[3]


REFUSALS = {
    "refused_upstream": dict(lengths=[1024, 0, 5, 0, -1, 2, 777]),
    "length_above_ld": dict(lengths=[1024, 0, 5, 0, 1, 1025, 777]),
    "bad_csr": dict(first_row=[0, 3, 4, 6, 9]),
    "empty_document": dict(first_row=[0, 3, 3, 6, 7]),
    "negative_gap": dict(gaps=[1, -5, 0, 0, 241, 0, 0]),
    "out_ld_too_small": dict(out_ld=1028),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(hipenv, case):
    lengths, gaps = LAYOUTS["a"]
    audio = rows(lengths, 1024, 5)
    out_ld = jr.default_out_ld(1024, FIRST, gaps)
    clean = device_join(hipenv, audio, lengths, FIRST, gaps, fade=3, out_ld=out_ld)
    assert clean[3] is None
    kw = dict(lengths=lengths, first_row=FIRST, gaps=gaps, out_ld=out_ld)
    kw.update(REFUSALS[case])
    got, want = check_against_restatement(hipenv, audio, kw["lengths"], kw["first_row"], kw["gaps"], fade=3, out_ld=kw["out_ld"], gap_max=241)
    out, out_len, starts, message = got
    assert message is not None and want[3] is not None
    refused = [g for g in range(4) if out_len[g] < 0]
    assert refused and len(refused) < 4
    for g in range(4):
        if g in refused:
            assert torch.count_nonzero(out[g]) == 0
            if case not in ("bad_csr", "empty_document"):
                assert all(int(starts[b]) == -1 for b in range(FIRST[g], FIRST[g + 1]))
        else:                                                    # every other document: the clean run, bit for bit
            assert int(out_len[g]) == int(clean[1][g])
            assert same_bits(out[g], clean[0][g, :out.shape[1]])
            assert starts[FIRST[g]:FIRST[g + 1]].tolist() == clean[2][FIRST[g]:FIRST[g + 1]].tolist()


def test_python_entry_raises_and_names_the_row(hipenv):
    _, _, inf = hipenv
    lengths, gaps = LAYOUTS["a"]
    audio = rows(lengths, 1024, 5).cuda()
    out, out_len, starts = inf.join_waveforms(audio, lengths, [3, 1, 2, 1], gaps, fade=3)
    want = jr.join(audio.cpu(), lengths, FIRST, gaps, fade=3)
    assert same_bits(out.cpu(), want[0]) and out_len.tolist() == want[1].tolist() and starts.tolist() == want[2].tolist()
    bad = list(lengths)
    bad[4] = -1
    with pytest.raises(ValueError, match=r"row 4 \(length -1\).*its length is outside"):
        inf.join_waveforms(audio, torch.tensor(bad).cuda(), FIRST, gaps, fade=3)
    with pytest.raises(ValueError, match=r"row 6 .*layout"):
        inf.join_waveforms(audio, lengths, [0, 3, 4, 6, 9], gaps)
    with pytest.raises(ValueError, match=r"row 0 .*does not fit out_ld = 1028"):
        inf.join_waveforms(audio, lengths, FIRST, gaps, out_ld=1028)
    out2, out_len2, _ = inf.join_waveforms(audio, torch.tensor(bad).cuda(), FIRST, gaps, fade=3, check=False)
    assert out_len2.tolist() == [want[1][0], want[1][1], -1, want[1][3]]
    assert torch.equal(inf.join_waveforms(audio, lengths, FIRST, gaps, fade=3)[0], out)      # the entry works on after a refusal


def test_a_document_does_not_depend_on_its_batch(hipenv):
    lengths, gaps, first = [300, 0, 257, 100, 50, 211, 64, 5], [3, 17, 0, 0, 9, 0, 1, 0], [0, 1, 4, 6, 8]
    audio = rows(lengths, 300, 10)
    scale = torch.tensor([1.0, 0.4, 0.7, 1.0, 1.0, 0.9, 0.5, 1.0])
    full = device_join(hipenv, audio, lengths, first, gaps, fade=40, scale=scale)
    assert full[3] is None
    for g in range(4):
        r0, r1 = first[g], first[g + 1]
        alone = device_join(hipenv, audio[r0:r1].contiguous(), lengths[r0:r1], [0, r1 - r0], gaps[r0:r1], fade=40, scale=scale[r0:r1])
        n = int(alone[1][0])
        assert n == int(full[1][g]) and alone[2].tolist() == full[2][r0:r1].tolist()
        assert same_bits(alone[0][0, :n], full[0][g, :n])
        assert torch.count_nonzero(full[0][g, n:]) == 0 and torch.count_nonzero(alone[0][0, n:]) == 0


# ------------------------------------------------------------------------------------------------ through the tail
HOP = 256


@pytest.fixture(scope="module")
def tail(hipenv):
    syn = sub("synthetic")
    sd = syn.make_vocos_state_dict(seed=11)
    sd["head.out.bias"][:513] += 2.5                            # log-magnitudes up: the rows' peaks then lie on both sides of 1 (0.96 .. 1.07)
    wrapper = sub("vocoder").load_model("cuda", state_dict=sd)
    lengths = [96, 61, 33, 40, 25, 50]
    g = torch.Generator().manual_seed(3)
    mel = torch.randn(len(lengths), 100, 96, generator=g) * 2.0 - 4.0
    for b, n in enumerate(lengths):
        mel[b, :, n:] = torch.randn(100, 96 - n, generator=g) * 50.0
    inf = hipenv[2]
    dev_mel = mel.cuda()
    plain = inf.to_waveforms(dev_mel, lengths, wrapper)          # today's per-row results: computed once, shared, left unchanged
    return wrapper, dev_mel, lengths, plain


def finished(inf, tail):
    """The rows as the join sees them inside to_waveforms: the decoded, normalised batch, the trim lengths and the scales."""
    wrapper, dev_mel, lengths, _ = tail
    lens = torch.tensor(lengths).cuda()
    audio = wrapper.model.decode(dev_mel, lens, check=False)
    keep, scale = inf.finish_waveforms(audio, lens, hop=HOP)
    return audio.cpu(), keep.cpu(), scale.cpu()


def test_sentence_level_join_is_the_host_concatenation(hipenv, tail):
    _, _, inf = hipenv
    wrapper, dev_mel, lengths, plain = tail
    docs = inf.to_waveforms(dev_mel, lengths, wrapper, documents=[3, 2], fade_ms=0, level="sentence")
    assert len(docs) == 3 and all(d.dim() == 1 and d.device.type == "cpu" and d.dtype == torch.float32 for d in docs)
    assert same_bits(docs[0], torch.cat(plain[0:3])) and same_bits(docs[1], torch.cat(plain[3:5]))
    assert same_bits(docs[2], plain[5])                          # a row behind the last document is a document of one row
    again = inf.to_waveforms(dev_mel, lengths, wrapper)          # documents=None: what it returned before
    assert len(again) == 6 and all(same_bits(a, b) for a, b in zip(again, plain))
    singles = inf.to_waveforms(dev_mel, lengths, wrapper, documents=[1] * 6)
    assert all(same_bits(a, b) for a, b in zip(singles, plain))  # one row has no joint and is its own loudest sentence


def test_document_level_join_is_the_restatement_on_the_finished_rows(hipenv, tail):
    _, _, inf = hipenv
    wrapper, dev_mel, lengths, _ = tail
    audio, keep, scale = finished(inf, tail)
    print("scales", scale.tolist(), "kept", keep.tolist())
    assert float(scale[0]) < 1.0 and float(scale[1]) == 1.0      # the document gain has something to do: row 0 was normalised, row 1 not
    gaps = [7200, 2880, 0, 14400, 0, 0]
    docs, segments = inf.to_waveforms(dev_mel, lengths, wrapper, documents=[3, 2, 1], gaps=gaps, fade_ms=5.0, return_segments=True)
    want, want_len, starts, verdict = jr.join(audio, keep, [0, 3, 5, 6], gaps, fade=120, scale=scale)
    assert verdict is None
    for g in range(3):
        assert same_bits(docs[g], want[g, :int(want_len[g])]), g
    flat = [s for doc in segments for s in doc]
    assert [len(d) for d in segments] == [3, 2, 1]
    for b, (t0, t1) in enumerate(flat):
        assert t0 == int(starts[b]) / 24000 and t1 == (int(starts[b]) + int(keep[b])) / 24000
    with pytest.raises(ValueError, match=r"mel_lengths\[4\] = 97"):
        inf.to_waveforms(dev_mel, [96, 61, 33, 40, 97, 50], wrapper, documents=[3, 2, 1])


def test_joined_documents_are_converted_and_encoded_once(hipenv, tail):
    _, _, inf = hipenv
    wrapper, dev_mel, lengths, _ = tail
    R, AC = sub("resample"), sub("audio_codec")
    gaps = [7200, 2880, 0, 14400, 0, 0]
    floats = inf.to_waveforms(dev_mel, lengths, wrapper, documents=[3, 2, 1], gaps=gaps)
    coded = inf.to_waveforms(dev_mel, lengths, wrapper, documents=[3, 2, 1], gaps=gaps, sample_rate=8000, encoding="ulaw")
    assert len(coded) == 3
    for g, row in enumerate(floats):
        conv, n = R.resample(row.cuda().reshape(1, -1), None, 24000, 8000)
        data, nbytes = AC.encode(conv[:, :int(n[0])], None, "ulaw")
        assert coded[g].dtype == torch.uint8 and coded[g].numel() == int(nbytes[0]) == -(-row.numel() // 3)
        assert torch.equal(coded[g], data[0, :int(nbytes[0])].cpu()), g


# ------------------------------------------------------------------------------------------------ through the batcher
def test_a_document_and_plain_requests_share_one_batch(hipenv, tail, hparams, synthetic):
    _, _, inf = hipenv
    wrapper = tail[0]
    bt = sub("batcher")
    hp = hparams.prod_v20(n_spks=10)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.cuda().eval()
    ids = [synthetic.make_inputs(hp, 1, n, seed=90 + i)[0][0].tolist() for i, n in enumerate([30, 22, 41, 17, 25, 36])]
    kw = dict(speaker=3, solver="midpoint", n_timesteps=2)
    pauses = [300.0, 120.0, 600.0, 0.0]
    doc = bt.Document(rows=[bt.Request(ids=t, **kw) for t in ids[:4]], pauses_ms=pauses, level="sentence")
    mixed = bt.synthesise_batch(model, [doc, bt.Request(ids=ids[4], **kw), bt.Request(ids=ids[5], speaker=6, solver="midpoint", n_timesteps=2)],
                                wrapper)
    plain = bt.synthesise_batch(model, [bt.Request(ids=t, **kw) for t in ids[:5]] + [bt.Request(ids=ids[5], speaker=6, solver="midpoint", n_timesteps=2)],
                                wrapper)
    assert len(mixed) == 3 and len(plain) == 6
    for a, b in zip(mixed[1:], plain[4:]):                       # plain requests keep exactly their keys and values
        assert set(a) == set(b) == {"mel", "mel_length", "audio"}
        assert a["mel_length"] == b["mel_length"] and torch.equal(a["mel"], b["mel"]) and same_bits(a["audio"], b["audio"])
    d = mixed[0]
    assert set(d) == {"audio", "segments", "mel_lengths"}
    assert d["mel_lengths"] == [r["mel_length"] for r in plain[:4]]
    sent = [r["audio"] for r in plain[:4]]
    ld = (max(a.numel() for a in sent) + 3) // 4 * 4
    stack = torch.zeros(4, ld)
    for b, a in enumerate(sent):
        stack[b, :a.numel()] = a
    gaps = [7200, 2880, 14400, 0]
    want, want_len, starts, _ = jr.join(stack, [a.numel() for a in sent], [0, 4], gaps, fade=120)
    assert same_bits(d["audio"], want[0, :int(want_len[0])])
    assert d["segments"] == [(int(s) / 24000, (int(s) + a.numel()) / 24000) for s, a in zip(starts, sent)]

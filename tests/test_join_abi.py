"""CPU checks of the document-join boundary (nothing runs on a GPU): the three entries are declared in include/mtts.h, exported by
the built library and bound in _hip.py with the declared number of arguments; every refusal the host can see returns -1 with a
message and launches nothing; the workspace size stays in int64 for large B and G; the torch restatement of
tests/join_restated.py agrees bit for bit with an independent sample-by-sample formulation at tiny sizes, and its verdicts are the
documented ones."""
import inspect

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
import join_restated as jr


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def test_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_abi_version() == 2                           # entries were only added
    assert "wave_join.hip" in sub("_hip").SOURCES
    for word in ("g_doc / scale[b]", "(float)(2 i + 1) / (float)(2 F')", "min(fade, len_b / 2)"):
        assert word in header, word


def test_python_signatures():
    inf = sub("inference")
    p = inspect.signature(inf.join_waveforms).parameters
    assert list(p)[:7] == ["audio", "lengths", "documents", "gaps", "fade", "scale", "check"]
    assert (p["fade"].default, p["scale"].default, p["check"].default) == (0, None, True)
    p = inspect.signature(inf.to_waveforms).parameters
    assert (p["documents"].default, p["gaps"].default, p["fade_ms"].default, p["level"].default) == (None, None, 5.0, "document")
    assert inf.document_csr([3, 1, 2, 1], 7) == [0, 3, 4, 6, 7] == inf.document_csr([0, 3, 4, 6, 7], 7)
    assert inf.document_csr([2], 4, pad=True) == [0, 2, 3, 4]
    for bad in ([3, 0, 4], [3, 5], [2, 2], []):
        with pytest.raises(ValueError):
            inf.document_csr(bad, 7)


#      audio    ld    lengths  scale    first    gap      B  G  fade gap_max out      out_ld out_len  starts   ws       bytes    stream
OK = [0x1000000, 1024, 0x20000, 0x30000, 0x40000, 0x50000, 7, 4, 120, 241, 0x2000000, 8192, 0x60000, 0x70000, 0x80000, 1 << 20, None]


def refused(lib, **change):
    names = ["audio", "ld", "lengths", "scale", "first", "gap", "B", "G", "fade", "gap_max", "out", "out_ld", "out_len", "starts", "ws", "bytes"]
    args = list(OK)                                              # never launched: every call below is refused before
    for k, v in change.items():
        args[names.index(k)] = v
    assert lib.mtts_wave_join(*args) == -1
    return lib.mtts_last_error()


def test_join_refuses_what_the_host_can_see(lib):
    for k in ("audio", "lengths", "first", "gap", "out", "out_len", "starts", "ws"):
        assert b"null" in refused(lib, **{k: None}), k
    for B, G in ((0, 1), (-2, 1), (7, 0), (7, -1), (7, 8), (70000, 4)):
        assert b"1 <= G <= B" in refused(lib, B=B, G=G), (B, G)
    for k in ("ld", "out_ld"):
        for v in (1022, 0, -4, 2):
            assert b"multiples of 4" in refused(lib, **{k: v}), (k, v)
    for k in ("audio", "out", "ws"):
        assert b"16-byte aligned" in refused(lib, **{k: OK[0] + 4 if k == "audio" else 0x2000008}), k
    # d_out inside, over the end of, over the start of, and exactly on d_audio (7 rows of 1024 floats; d_out is 4 rows of 8192)
    for out in (OK[0], OK[0] + 4096, OK[0] + 7 * 4096 - 16, OK[0] - 4 * 8192 * 4 + 16):
        assert b"overlaps" in refused(lib, out=out), hex(out)
    assert b"negative" in refused(lib, fade=-1)
    assert b"negative" in refused(lib, gap_max=-1)
    assert b"workspace too small" in refused(lib, bytes=lib.mtts_wave_join_workspace_bytes(7, 4) - 257)
    assert b"workspace too small" in refused(lib, bytes=16)
    assert lib.mtts_wave_join_status(None, None) == -1 and b"null" in lib.mtts_last_error()
    # a buffer that ends where d_audio begins, or begins where it ends, does not overlap: not refused for that (null scale is allowed
    # too); the call is then refused for its next fault, the workspace
    for out in (OK[0] - 4 * 8192 * 4, OK[0] + 7 * 4096):
        assert b"workspace too small" in refused(lib, out=out, scale=None, bytes=16), hex(out)


def test_workspace_bytes_stay_in_int64(lib):
    small = lib.mtts_wave_join_workspace_bytes(7, 4)
    assert small >= 256 + 7 * 8 and small % 4 == 0
    big = lib.mtts_wave_join_workspace_bytes(1 << 33, 1 << 32)
    assert big >= 8 * (1 << 33) and big < 9 * (1 << 33)
    assert lib.mtts_wave_join_workspace_bytes(1 << 33, 1) == big                  # G only has to be a possible count
    for B, G in ((0, 1), (4, 0), (4, 5), (-1, -1)):
        assert lib.mtts_wave_join_workspace_bytes(B, G) == -1 and b"1 <= G <= B" in lib.mtts_last_error()


def tiny_case(seed, with_scale):
    g = torch.Generator().manual_seed(seed)
    ld = 12
    first_row = [0, 3, 4, 6, 9]
    B = 9
    lengths = [int(v) for v in torch.randint(0, ld + 1, (B,), generator=g)]
    lengths[1], lengths[3], lengths[7] = 0, 0, ld
    gaps = [int(v) for v in torch.randint(0, 6, (B,), generator=g)]
    audio = torch.randn(B, ld, generator=g)
    scale = None
    if with_scale:
        scale = torch.ones(B)
        scale[0], scale[2], scale[6] = 0.95 / 1.7, 0.95 / 3.1, 0.95 / 1.01
    return audio, lengths, first_row, gaps, scale


@pytest.mark.parametrize("fade", [0, 1, 3, 100])
@pytest.mark.parametrize("with_scale", [False, True])
def test_restatement_equals_the_sample_by_sample_formulation(fade, with_scale):
    for seed in range(6):
        audio, lengths, first_row, gaps, scale = tiny_case(seed, with_scale)
        out, out_len, starts, verdict = jr.join(audio, lengths, first_row, gaps, fade=fade, scale=scale)
        want, want_len, want_starts = jr.join_by_samples(audio, lengths, first_row, gaps, fade=fade, scale=scale)
        assert verdict is None
        assert out_len.tolist() == want_len and starts.tolist() == want_starts
        assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32)), (seed, fade)
        if fade == 0 and scale is None:                          # samples are moved: every kept sample is somewhere in its document
            for g in range(4):
                for b in range(first_row[g], first_row[g + 1]):
                    assert torch.equal(out[g, starts[b]:starts[b] + lengths[b]], audio[b, :lengths[b]])


def test_restatement_weights_and_gain_by_hand():
    audio = torch.ones(2, 8)
    out, out_len, starts, _ = jr.join(audio, [8, 8], [0, 2], [2, 0], fade=2)
    assert out_len.tolist() == [18] and starts.tolist() == [0, 10]
    want = [1, 1, 1, 1, 1, 1, .75, .25, 0, 0, .25, .75, 1, 1, 1, 1, 1, 1, 0, 0]
    assert out[0].tolist() == want
    # F' = min(fade, len / 2): a row of 5 samples between two others fades 2 in and 2 out, its middle sample stays
    out, _, starts, _ = jr.join(torch.ones(3, 8), [8, 5, 8], [0, 3], [0, 0, 0], fade=4)
    assert out[0, 8:13].tolist() == [.25, .75, 1, .75, .25]
    # one gain per document: the row that was scaled most (the loudest) sets it, and keeps its samples
    scale = torch.tensor([1.0, 0.5, 1.0])
    out, _, _, _ = jr.join(torch.ones(3, 4), [4, 4, 4], [0, 2, 3], [0, 0, 0], scale=scale)
    assert out[0].tolist() == [.5, .5, .5, .5, 1, 1, 1, 1] and out[1, :4].tolist() == [1, 1, 1, 1]


def test_restatement_verdicts():
    audio = torch.ones(7, 8)
    first, gaps, lens = [0, 3, 4, 6, 7], [1, 0, 0, 0, 2, 0, 0], [8, 0, 3, 5, 8, 1, 2]
    clean = jr.join(audio, lens, first, gaps, out_ld=32)
    assert clean[3] is None and clean[1].tolist() == [12, 5, 11, 2]

    def case(lens=lens, first=first, gaps=gaps, out_ld=32):
        out, out_len, starts, verdict = jr.join(audio, lens, first, gaps, out_ld=out_ld, gap_max=2)
        for g in range(len(first) - 1):
            if out_len[g] >= 0:
                assert torch.equal(out[g], clean[0][g, :out.shape[1]]) and out_len[g] == clean[1][g]
            else:
                assert torch.count_nonzero(out[g]) == 0
        return out_len.tolist(), starts.tolist(), verdict

    assert case(lens=[8, 0, 3, 5, -1, 1, 2]) == ([12, 5, -1, 2], [0, 9, 9, 0, -1, -1, 0], (4, -1, 1))
    assert case(lens=[8, 9, 3, 5, 8, 1, 2])[2] == (1, 9, 1)
    assert case(gaps=[1, 0, 0, 0, -1, 0, 0]) == ([12, 5, -1, 2], [0, 9, 9, 0, -1, -1, 0], (4, 8, 2))
    assert case(gaps=[1, 0, 7, 0, 2, 0, -5])[2] is None            # the gap after a document's last row is not looked at
    assert case(first=[0, 3, 4, 6, 9]) == ([12, 5, 11, -1], [0, 9, 9, 0, 0, 10, -1], (6, 2, 2))
    assert case(first=[0, 3, 3, 6, 7]) == ([12, -1, -1, -1], [0, 9, 9, -1, -1, -1, -1], (3, 5, 2))
    assert case(out_ld=8) == ([-1, 5, -1, 2], [-1, -1, -1, 0, -1, -1, 0], (0, 8, 3))

"""CPU checks of the sample-rate conversion's boundary (nothing runs on a GPU): the entries are declared in include/mtts.h, exported
by the built library and bound in _hip.py with the declared number of arguments; the host table equals the restated formulae
rounded to fp32, bit for bit; the factors and output lengths are the formulae's; create and forward refuse what the host can
see; the kernel is in the gfx950 code object without scratch; the Python entries carry ``sample_rate=24000``."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sub
import resample_restated as rr

LLVM = "/opt/rocm/lib/llvm/bin"
PKG = ROOT / "matcha-tts-24k_amd"
PAIRS = [(48000, 24000), (44100, 24000), (16000, 24000), (24000, 8000), (24000, 44100)]
FACTORS = {(48000, 24000): (2, 1, 13, 28), (44100, 24000): (147, 80, 12, 171), (16000, 24000): (2, 3, 7, 16),
           (24000, 8000): (3, 1, 19, 41), (24000, 44100): (80, 147, 7, 94)}
BANDS = {(48000, 24000): 25, (44100, 24000): 23, (24000, 8000): 37, (24000, 44100): 13}      # the issue's table


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def make(lib, a, b, lpw=6, rolloff=0.99):
    return lib.mtts_resampler_create(a, b, lpw, rolloff)


def query(lib, r):
    v = [C.c_int(0) for _ in range(5)]
    assert lib.mtts_resample_factors(r, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def test_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert "sample-rate conversion" in header and "utmos_validate.py:78" in header
    assert re.search(r"#define MTTS_ABI_VERSION 2\b", header)    # additive entries
    tile = int(re.search(r"#define MTTS_RESAMPLE_TILE (\d+)", header).group(1))
    assert lib.mtts_resample_tile() == tile == sub("resample").TILE


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_bank_factors_and_lengths_are_the_restated_formulae(lib, pair):
    r = make(lib, *pair)
    assert r, lib.mtts_last_error()
    try:
        o, n, width, taps, band = query(lib, r)
        assert (o, n, width, taps) == FACTORS[pair] == rr.factors(*pair)
        K = np.empty((n, taps), dtype=np.float32)
        assert lib.mtts_resample_bank(r, K.ctypes.data, K.size) == 0
        want = rr.bank32(*pair)
        assert K.view(np.uint32).tolist() == want.view(np.uint32).tolist()          # bit for bit
        assert band == rr.band_of(want)
        if pair in BANDS:
            assert band == BANDS[pair]
        assert lib.mtts_resample_bank(r, K.ctypes.data, K.size - 1) == -1
        for L in (0, 1, o - 1, o, 3 * o, 2531):
            assert lib.mtts_resample_out_length(r, L) == -(-n * L // o) == rr.out_length(L, o, n)
        assert lib.mtts_resample_workspace_bytes(r, 4, 1024) > 0
        assert lib.mtts_resample_workspace_bytes(r, 0, 1024) == -1
    finally:
        lib.mtts_resampler_destroy(r)


def test_every_common_rate_pairs_with_24000(lib):
    for rate in (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000):
        for pair in ((rate, 24000), (24000, rate)):
            r = make(lib, *pair)
            assert r, (pair, lib.mtts_last_error())
            o, n, width, taps, band = query(lib, r)
            lib.mtts_resampler_destroy(r)
            assert n * band < 4200, (pair, n * band)             # "the banded bank of every common pair is under 4.2 k floats"


def test_create_refusals(lib):
    for args, word in (((24000, 24000, 6, 0.99), b"equal"), ((0, 24000, 6, 0.99), b"[4000, 384000]"), ((24000, 500000, 6, 0.99), b"[4000, 384000]"),
                       ((48000, 24000, 6, 0.0), b"rolloff"), ((48000, 24000, 6, 1.5), b"rolloff"), ((48000, 24000, 0, 0.99), b"lowpass_filter_width"),
                       ((44101, 24000, 6, 0.99), b"too large")):        # coprime rates: a bank far beyond the LDS cap
        assert not make(lib, *args), args
        assert word in lib.mtts_last_error(), (args, lib.mtts_last_error())
    r = make(lib, 48000, 24000, 6, 1.0)                          # rolloff 1 is inside (0, 1]
    assert r
    lib.mtts_resampler_destroy(r)
    res = sub("resample")
    with pytest.raises(ValueError, match="equal"):
        res.Resampler(24000, 24000)


def test_forward_refuses_what_the_host_can_see(lib):
    r = make(lib, 48000, 24000)
    try:
        ok = (r, 0x10000, 1024, 0x20000, 2, 0x30000, 512, 0x40000, 0x50000, 256, None)       # never launched: refused before
        for i in (0, 1, 3, 5, 7, 8):                             # every pointer
            bad = list(ok)
            bad[i] = None
            assert lib.mtts_resample_forward(*bad) == -1
            assert b"null" in lib.mtts_last_error()
        bad = list(ok); bad[4] = 0
        assert lib.mtts_resample_forward(*bad) == -1 and b"B must" in lib.mtts_last_error()
        bad = list(ok); bad[2] = 1022
        assert lib.mtts_resample_forward(*bad) == -1 and b"16-byte aligned" in lib.mtts_last_error()
        bad = list(ok); bad[6] = 510
        assert lib.mtts_resample_forward(*bad) == -1 and b"16-byte aligned" in lib.mtts_last_error()
        bad = list(ok); bad[9] = 8
        assert lib.mtts_resample_forward(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()
        assert lib.mtts_resample_status(None, None) == -1
    finally:
        lib.mtts_resampler_destroy(r)


def test_kernel_is_in_the_gfx950_code_object_without_scratch(tmp_path):
    sub("_hip").build()
    obj = PKG / "build" / "resample.o"
    assert obj.exists(), obj
    fat, co = tmp_path / "resample.fat", tmp_path / "resample.co"
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, flags=re.M)
        scratch = re.search(r"^    \.private_segment_fixed_size:\s+(\d+)", block, flags=re.M)
        if name and scratch:
            meta[name.group(1)] = int(scratch.group(1))
    hits = [k for k in meta if "resample_kernel" in k]
    assert len(hits) == 1, sorted(meta)
    assert meta[hits[0]] == 0, meta


def test_restated_chain_equals_fp64_within_the_serial_sum_bound():
    """The restatement itself, on the CPU: the fp32 chain against the dense fp64 sum, inside (band + 1) * 2^-24 * sum |K x|."""
    rng = np.random.default_rng(5)
    for pair in PAIRS:
        o, n, width, taps = rr.factors(*pair)
        K = rr.bank32(*pair)
        x = rng.uniform(-1, 1, 2531).astype(np.float32)
        got = rr.resample32(x, K, o, n, width)
        ref, mag = rr.resample64(x, K, o, n, width)
        assert got.shape[0] == rr.out_length(2531, o, n)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= (rr.band_of(K) + 1) * 2.0 ** -24 * mag)


def test_sample_rate_keyword_defaults_to_24000():
    inf = sub("inference")
    for fn in (inf.MatchaTTSInfer.enroll_voice, inf.MatchaTTSInfer.align, inf.MatchaTTSInfer.score, inf.MatchaTTSInfer.speaker_grad,
               inf.MatchaTTSInfer.finetune_speaker, inf.to_waveforms, inf.pipeline):
        params = inspect.signature(fn).parameters
        assert params["sample_rate"].default == 24000, fn
        assert list(params)[-1] == "sample_rate", fn             # the last keyword: no positional caller moves
    bt, sv = sub("batcher"), sub("serving")
    assert bt.Request(ids=[1]).sample_rate == 24000
    assert inspect.signature(sv.SpeechService.submit).parameters["sample_rate"].default == 24000
    assert inspect.signature(sv.SpeechService.speak).parameters["sample_rate"].default == 24000
    assert sub("resample").cached() == 0                         # importing and inspecting converts nothing

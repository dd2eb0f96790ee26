"""Loudness (include/mtts.h "loudness") without a GPU: the NumPy restatement against the standard's own numbers and against
``scipy.signal.lfilter``, the chunk / scan scheme against the plain recurrence, and the C ABI's host-visible side."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from conftest import ROOT, sub
import loudness_restated as lr

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): shelf b0 b1 b2 a1 a2, high-pass a1 a2
TABLE = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621]


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def _noise(n, seed, rms=0.09):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * rms).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_coefficients_are_the_bs1770_table_at_48k():
    k = lr.coefficients(48000)
    got = k[:5] + k[8:]
    worst = max(abs(g - t) for g, t in zip(got, TABLE))
    print(f"largest difference from the BS.1770 table: {worst:.3e}")
    assert worst <= 1e-12
    assert k[5:8] == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("fs", [8000, 24000, 48000])
def test_restated_cascade_is_scipy_lfilter(fs):
    from scipy import signal                                      # (the independent anchor of the restatement: a missing scipy fails)
    x = _noise(6000, 1)
    k = lr.coefficients(fs)
    y, _ = lr.cascade(x, k)
    ref = signal.lfilter(k[5:8], [1.0] + k[8:], signal.lfilter(k[:3], [1.0] + k[3:5], x.astype(np.float64)))
    worst = float(np.max(np.abs(y - ref)))
    print(f"fs {fs}: cascade vs lfilter {worst:.3e}")
    assert worst <= 1e-12


def test_full_scale_997_hz_sine_reads_minus_3_01_lufs_at_48k():
    """The standard's own calibration point.  At other rates the bilinear coefficients read differently (-2.984 at 24 kHz, -2.996
    at 8 kHz), so those are held to the restatement only."""
    fs = 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(3 * fs) / fs).astype(np.float32)
    got = lr.measure(x, fs)["lufs"]
    print(f"997 Hz full scale at 48 kHz: {got:.4f} LUFS")
    assert abs(got - (-3.01)) <= 0.01


@pytest.mark.parametrize("fs", [8000, 24000, 48000])
def test_chunked_scheme_is_the_plain_recurrence(fs):
    chunk = lr.chunk_of(fs)
    assert (fs // 100) % chunk == 0
    x = _noise(70 * chunk + 17, 2)                                # three runs of the scan's second level, the last one partial
    k = lr.coefficients(fs)
    plain, _ = lr.cascade(x, k)
    cut = lr.chunked_cascade(x, k, chunk, run=32)
    worst = float(np.max(np.abs(plain - cut)))
    print(f"fs {fs}, chunk {chunk}: chunked vs plain {worst:.3e}")
    assert worst <= 1e-12                                         # measured 2e-13 on rms 0.09; the states are fp64


def test_restated_gates_and_short_rows():
    fs = 24000
    loud, quiet = _noise(fs, 3), _noise(fs, 4) * np.float32(10 ** (-30 / 20))
    both = lr.measure(np.concatenate([loud, quiet]), fs)
    alone = lr.measure(loud, fs)
    assert min(both["blocks"]) < both["gate"] < max(both["blocks"])              # the relative gate drops the quiet blocks
    assert alone["lufs"] - 1.0 < both["lufs"] < alone["lufs"]                   # (ungated, the quiet half would cost 3 dB)
    assert lr.measure(np.zeros(fs, dtype=np.float32), fs)["lufs"] == -math.inf
    assert lr.measure(_noise(fs, 5) * np.float32(1e-5 / 0.09), fs)["lufs"] == -math.inf   # under the absolute gate
    short = lr.measure(loud[:1000], fs)                                           # one block of its own length
    assert len(short["blocks"]) == 1 and math.isfinite(short["lufs"])
    assert lr.measure(np.zeros(0, dtype=np.float32), fs)["lufs"] == -math.inf
    # the gain: plain, limited by the ceiling, and exactly 1 where there is nothing to do
    g = lr.gain(-20.0, -23.0, 0.5)
    assert g.dtype == np.float32 and abs(float(g) - 10 ** (-3 / 20)) < 1e-7
    g = lr.gain(-30.0, -10.0, 0.5)
    assert np.float32(0.5) * g <= np.float32(0.95) and abs(float(g) - 1.9) < 1e-6
    assert lr.gain(-math.inf, -23.0, 0.0) == 1.0 and lr.gain(-20.0, None, 0.5) == 1.0 and lr.gain(-20.0, math.nan, 0.5) == 1.0


# ------------------------------------------------------------------------------------------------ the C ABI
def test_bindings_exist_and_match_the_header(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert re.search(r"#define MTTS_ABI_VERSION 2\b", header) and lib.mtts_abi_version() == 2     # entries are only added
    assert re.search(r"#define MTTS_IMAGE_REVISION 7\b", header)
    tile = int(re.search(r"#define MTTS_LOUDNESS_TILE (\d+)", header).group(1))
    chunks = int(re.search(r"#define MTTS_LOUDNESS_CHUNKS (\d+)", header).group(1))
    L = sub("loudness")
    assert lib.mtts_loudness_tile() == tile == L.TILE == chunks * lib.mtts_loudness_chunk(24000)
    for fs in (8000, 16000, 22000, 24000, 44100, 48000, 96000, 192000, 8300, 25700):
        c = lib.mtts_loudness_chunk(fs)
        assert c == lr.chunk_of(fs) == L.chunk(fs) and (fs // 100) % c == 0 and 1 <= c <= 256
    assert lib.mtts_loudness_chunk(24000) == 240 and lib.mtts_loudness_chunk(8000) == 80


@pytest.mark.parametrize("fs", [8000, 24000, 44100, 48000, 192000])
def test_library_coefficients_are_the_restated_ones(lib, fs):
    out = (C.c_double * 10)()
    assert lib.mtts_loudness_coefficients(fs, out) == 0
    worst = max(abs(a - b) for a, b in zip(list(out), lr.coefficients(fs)))
    assert worst <= 1e-14, worst
    if fs == 48000:
        got = list(out)[:5] + list(out)[8:]
        assert max(abs(g - t) for g, t in zip(got, TABLE)) <= 1e-12


def test_loudness_refuses_what_the_host_can_see(lib):
    # (audio, ld, lengths, B, rate, target, ceiling, apply, lufs, gain, peak, ws, ws_bytes, stream): never launched, refused before
    ok = (0x100000, 1024, 0x200000, 2, 24000, None, 0.95, 1, 0x300000, 0x400000, 0x500000, 0x600000, 1 << 20, None)
    for i in (0, 2, 8, 9, 10, 11):                               # every pointer but the targets, which may be null
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_loudness(*bad) == -1 and b"null" in lib.mtts_last_error()
    for B in (0, 65536):
        bad = list(ok); bad[3] = B
        assert lib.mtts_loudness(*bad) == -1 and b"B must" in lib.mtts_last_error()
    for ld in (0, 1022, -4):
        bad = list(ok); bad[1] = ld
        assert lib.mtts_loudness(*bad) == -1 and b"multiple of 4" in lib.mtts_last_error()
    bad = list(ok); bad[1] = (1 << 30) + 4
    assert lib.mtts_loudness(*bad) == -1 and b"2^30" in lib.mtts_last_error()
    for rate in (7900, 24050, 192100, 0):
        bad = list(ok); bad[4] = rate
        assert lib.mtts_loudness(*bad) == -1 and b"sample_rate" in lib.mtts_last_error()
        assert lib.mtts_loudness_workspace_bytes(1024, 2, rate) == -1 and lib.mtts_loudness_chunk(rate) == -1
    for i, p in ((0, 0x100004), (11, 0x600008), (8, 0x300004)):
        bad = list(ok); bad[i] = p
        assert lib.mtts_loudness(*bad) == -1 and b"misaligned" in lib.mtts_last_error()
    for ceiling in (0.0, -1.0, math.inf, math.nan):
        bad = list(ok); bad[6] = ceiling
        assert lib.mtts_loudness(*bad) == -1 and b"peak_ceiling" in lib.mtts_last_error()
    bad = list(ok); bad[12] = lib.mtts_loudness_workspace_bytes(1024, 2, 24000) - 1
    assert lib.mtts_loudness(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()
    assert lib.mtts_loudness_status(None, None) == -1 and b"null" in lib.mtts_last_error()
    assert lib.mtts_loudness_coefficients(24000, None) == -1
    # the workspace grows with the row, not with anything else
    small, large = lib.mtts_loudness_workspace_bytes(1024, 2, 24000), lib.mtts_loudness_workspace_bytes(1 << 21, 2, 24000)
    assert 0 < small < large < 64 << 20


def test_python_entries_refuse_before_anything_is_launched():
    import torch
    L = sub("loudness")
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.measure(torch.zeros(1, 8))
    for bad in ("loud", True, [-1.0, "x"]):
        with pytest.raises(TypeError):
            L.targets_per_row(bad, 2)
    for bad in (3.0, math.inf, math.nan, [-23.0, 0.5]):
        with pytest.raises(ValueError):
            L.targets_per_row(bad, 2)
    with pytest.raises(ValueError, match="one per row"):
        L.targets_per_row([-23.0], 2)
    assert L.targets_per_row(None, 3) is None and L.targets_per_row([None, None], 2) is None
    got = L.targets_per_row([-23, None], 2)
    assert got[0] == -23.0 and math.isnan(got[1]) and L.targets_per_row(-16.0, 2) == [-16.0, -16.0]
    for rate in (7000, 24050, 24000.5):
        with pytest.raises(ValueError, match="sample_rate"):
            L.check_rate(rate)

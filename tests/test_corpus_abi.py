"""CPU checks of the corpus-preparation boundary (nothing runs on a GPU): the entries are declared in include/mtts.h, exported by
the built library and bound in _hip.py with the declared number of arguments; ABI and image revision did not move; every entry
refuses what the host can see with -1 and a message; a target that is no multiple of the window raises; the kernels are in the
gfx950 code object without scratch; the NumPy restatements of tests/corpus_restated.py reproduce tests/golden/silence.npz -- the
reference's own numbers -- exactly, and are themselves checked against plain fp64 and math.fsum; the measure table of
tools/prepare_corpus.py has the layout of the reference's recorded print (tests/golden/silence_table.txt)."""
import importlib.util
import inspect
import json
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, sub
import corpus_restated as cr

LLVM = "/opt/rocm/lib/llvm/bin"
PKG = ROOT / "matcha-tts-24k_amd"


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "silence.npz")


def test_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert re.search(r"#define\s+MTTS_ABI_VERSION\s+2\b", header) and re.search(r"#define\s+MTTS_IMAGE_REVISION\s+7\b", header)
    assert lib.mtts_abi_version() == 2                           # entries were only added
    assert "corpus.hip" in sub("_hip").SOURCES
    for word in ("measure_silence.py:66-132", "normalize_silence.py:86-220", "generate_data_statistics.py:120-131", "v[i] = v[i] + v[i ^ o]"):
        assert word in header, word
    assert lib.mtts_mel_stats_chunk() == cr.CHUNK
    for sr in (24000, 44100, 16000, 22050, 8000):
        assert lib.mtts_silence_window(sr) == int(0.01 * sr) == cr.window(sr)


def test_python_signatures():
    corpus = sub("corpus")
    p = inspect.signature(corpus.measure_silence).parameters
    assert list(p)[:5] == ["audio", "lengths", "sample_rate", "effective_db", "absolute_db"]
    assert (p["sample_rate"].default, p["effective_db"].default, p["absolute_db"].default) == (24000, -60.0, -90.0)
    p = inspect.signature(corpus.normalize_silence).parameters
    assert list(p)[:6] == ["audio", "lengths", "leading", "trailing", "threshold_db", "sample_rate"]
    assert (p["leading"].default, p["trailing"].default, p["threshold_db"].default, p["sample_rate"].default) == (None, None, -60.0, 24000)
    p = inspect.signature(corpus.MelStatistics.__init__).parameters
    assert (p["n_mels"].default, p["hop"].default) == (100, 256)
    for name in ("update", "update_mel", "result"):
        assert callable(getattr(corpus.MelStatistics, name))
    p = inspect.signature(corpus.precompute_mels).parameters
    assert list(p)[:5] == ["audio", "lengths", "mel_mean", "mel_std", "hop"] and p["hop"].default == 256
    inf = sub("inference")
    for fn in (inf.MatchaTTSInfer.enroll_voice, inf.MatchaTTSInfer.align, inf.MatchaTTSInfer.score, inf.MatchaTTSInfer.speaker_grad,
               inf.MatchaTTSInfer.finetune_speaker):
        assert inspect.signature(fn).parameters["silence"].default is None, fn


def test_measure_refuses_what_the_host_can_see(lib):
    ok = [0x10000, 1024, 0x20000, 2, 24000, -60.0, -90.0, 0x30000, 0x40000, 1 << 20, None]      # never launched: refused before
    for i in (0, 2, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_silence_measure(*bad) == -1 and b"null" in lib.mtts_last_error()
    for b in (0, -3, 70000):
        bad = list(ok); bad[3] = b
        assert lib.mtts_silence_measure(*bad) == -1 and b"B must" in lib.mtts_last_error()
    for ld in (1022, 0, -4):
        bad = list(ok); bad[1] = ld
        assert lib.mtts_silence_measure(*bad) == -1 and b"16-byte aligned" in lib.mtts_last_error()
    bad = list(ok); bad[0] = 0x10004
    assert lib.mtts_silence_measure(*bad) == -1 and b"16-byte aligned" in lib.mtts_last_error()
    bad = list(ok); bad[4] = 50
    assert lib.mtts_silence_measure(*bad) == -1 and b"sample_rate" in lib.mtts_last_error()
    need = lib.mtts_silence_workspace_bytes(1024, 2, 24000)
    assert need >= 256 + 2 * 5 * 4
    bad = list(ok); bad[9] = need - 257                          # the slack of 256 bytes is not counted on
    assert lib.mtts_silence_measure(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()
    assert lib.mtts_silence_workspace_bytes(0, 2, 24000) == -1 and lib.mtts_silence_workspace_bytes(1024, 0, 24000) == -1
    assert lib.mtts_silence_status(None, None) == -1 and b"null" in lib.mtts_last_error()


def test_normalize_refuses_what_the_host_can_see(lib):
    ok = [0x10000, 1024, 0x20000, 0x30000, 2, 24000, 4800, 19200, 0x40000, 2048, 0x50000, 0x60000, 0x70000, 256, None]
    for i in (0, 2, 3, 8, 10, 11, 12):
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_silence_normalize(*bad) == -1 and b"null" in lib.mtts_last_error()
    bad = list(ok); bad[4] = 0
    assert lib.mtts_silence_normalize(*bad) == -1 and b"B must" in lib.mtts_last_error()
    for i in (1, 9):
        bad = list(ok); bad[i] = 1022
        assert lib.mtts_silence_normalize(*bad) == -1 and b"16-byte aligned" in lib.mtts_last_error()
    bad = list(ok); bad[8] = bad[0]
    assert lib.mtts_silence_normalize(*bad) == -1 and b"not in place" in lib.mtts_last_error()
    for i, t in ((6, 100), (7, 4801), (6, -2), (7, 239)):        # reference normalize_silence.py:139-154
        bad = list(ok); bad[i] = t
        assert lib.mtts_silence_normalize(*bad) == -1 and b"whole multiple" in lib.mtts_last_error(), (i, t)
    bad = list(ok); bad[5] = 44100; bad[6] = 4800                # 4800 is no multiple of 441
    assert lib.mtts_silence_normalize(*bad) == -1 and b"whole multiple" in lib.mtts_last_error()
    bad = list(ok); bad[13] = 16
    assert lib.mtts_silence_normalize(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()


def test_mel_stats_refuses_what_the_host_can_see(lib):
    ok = [0x10000, 100, 37, 0x20000, 5, 0x30000, 0x40000, 0x50000, 0x60000, 1 << 16, None]
    for i in (0, 3, 5, 6, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert lib.mtts_mel_stats(*bad) == -1 and b"null" in lib.mtts_last_error()
    bad = list(ok); bad[4] = 0
    assert lib.mtts_mel_stats(*bad) == -1 and b"B must" in lib.mtts_last_error()
    for i in (1, 2):
        bad = list(ok); bad[i] = 0
        assert lib.mtts_mel_stats(*bad) == -1 and b"at least 1" in lib.mtts_last_error()
    bad = list(ok); bad[9] = 256
    assert lib.mtts_mel_stats(*bad) == -1 and b"workspace too small" in lib.mtts_last_error()
    assert lib.mtts_mel_stats_workspace_bytes(5, 37) >= 256 + 5 * 20
    assert lib.mtts_mel_stats_workspace_bytes(0, 37) == -1 and lib.mtts_mel_stats_workspace_bytes(5, 0) == -1
    assert lib.mtts_mel_stats_status(None, None) == -1


def test_target_that_is_no_multiple_of_the_window_raises(lib):
    corpus = sub("corpus")
    assert corpus.target_samples(0.2, 24000) == 4800 and corpus.target_samples(0.8, 44100) == 35280 and corpus.target_samples(None, 24000) == -1
    assert corpus.target_samples(0.0, 24000) == 0
    for sec, sr in ((0.205, 24000), (0.2004, 24000), (0.001, 44100), (-0.01, 24000)):
        with pytest.raises(ValueError, match="multiple of 10 ms"):
            corpus.target_samples(sec, sr, "trailing")
    import torch
    with pytest.raises(ValueError, match="multiple of 10 ms"):   # refused before anything touches a device
        corpus.normalize_silence([torch.zeros(1000)], leading=0.123)
    with pytest.raises(RuntimeError, match="no CPU path"):
        corpus.mel_sums(torch.zeros(2, 100, 37))


def test_kernels_are_in_the_gfx950_code_object_without_scratch(tmp_path):
    sub("_hip").build()
    obj = PKG / "build" / "corpus.o"
    assert obj.exists(), obj
    fat, co = tmp_path / "corpus.fat", tmp_path / "corpus.co"
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
    for kernel, count in (("sil_rms_kernel", 2), ("sil_scan_kernel", 1), ("sil_norm_kernel", 1), ("mel_part_kernel", 1), ("mel_total_kernel", 1)):
        hits = [k for k in meta if kernel in k]
        assert len(hits) == count, (kernel, sorted(meta))
        assert all(meta[k] == 0 for k in hits), meta


# ------------------------------------------------------------------------------------------------ restatements vs the reference
def test_fixture_has_every_case_and_its_margin(golden, synthetic):
    cases = cr.clips(synthetic)
    assert len(cases) == 9 and any(sr == 44100 for _, sr in cases.values())
    for key in ("bounds", "measured", "pass1", "bounds2", "pass2"):
        assert {f"{key}_{name}" for name in cases} <= set(golden.files)
    assert float(golden["margin"]) > 1e-3                        # no window's RMS near a threshold: fp32 vs fp64 sums cannot flip it
    worst = 1.0
    for x, sr in cases.values():
        rms = cr.window_rms(x, cr.window(sr)).astype(np.float64)
        for t in cr.thresholds(-60.0, -90.0):
            worst = min(worst, float(np.min(np.abs(rms - float(t)) / float(t))))
    assert worst > 1e-3


def test_restatement_reproduces_the_reference_fixture(golden, synthetic):
    for name, (x, sr) in cr.clips(synthetic).items():
        six = cr.measure(x, sr)
        assert six[:2] == golden[f"bounds_{name}"].tolist(), name
        assert six[2:] == golden[f"measured_{name}"].tolist(), name
        y, changed, _ = cr.normalize(x, sr)
        assert [changed, y.size] == golden[f"pass1_{name}"].tolist(), name
        cs, ce = six[:2]
        lead, trail = cr.samples(cr.LEAD_S, sr), cr.samples(cr.TRAIL_S, sr)
        if changed:                                              # zeros + the content's own bits + zeros
            assert not y[:lead].any() and not y[lead + ce - cs:].any() and y[lead:lead + ce - cs].tobytes() == x[cs:ce].tobytes(), name
        z, changed2, b2 = cr.normalize(y, sr)
        assert list(b2) == golden[f"bounds2_{name}"].tolist(), name
        assert [changed2, z.size] == golden[f"pass2_{name}"].tolist(), name


def test_reference_quirks_are_in_the_fixture(golden):
    assert golden["measured_silent"].tolist() == [3120, 3120, 3120, 3120]            # 13 windows of 240 for 3000 samples
    assert golden["bounds_silent"].tolist() == [0, 0]
    assert golden["measured_tail_m70"][2] > golden["measured_tail_m70"][3] > 0       # the -70 dB tail lies between the thresholds
    assert golden["bounds_ends_mid_window"].tolist() == [1200, 6017]
    assert golden["measured_no_silence"].tolist() == [0, 0, 0, 0]
    for name in ("padded", "exact_multiple", "tail_m70", "r44100"):                  # content is a whole number of windows:
        assert int(golden[f"pass1_{name}"][0]) == 1 and int(golden[f"pass2_{name}"][0]) == 0, name   # the second pass is a no-op
    for name in ("short", "ends_mid_window", "silent"):                              # ... and where it is not, it changes again
        assert int(golden[f"pass2_{name}"][0]) == 1, name


def test_window_rms_restatement_against_plain_fp64():
    """Validates the restatement (the tests' oracle), not the library: the documented order against a plain fp64 sum.  Bound:
    the rounding of the result to fp32 (half an ulp, 2^-24 relative) plus the two fp64 sums' own error, at most W 2^-53 relative
    on each non-negative sum (halved by the root), plus the root's and the division's roundings: (W + 4) 2^-52 covers them."""
    rng = np.random.default_rng(3)
    for W, L in ((240, 1000), (441, 2000), (80, 321), (160, 160), (240, 1)):
        x = rng.uniform(-1, 1, L).astype(np.float32)
        got = cr.window_rms(x, W)
        pad = np.zeros(-(-L // W) * W)
        pad[:L] = x
        want = np.sqrt((pad * pad).reshape(-1, W).sum(1) / W)
        assert got.dtype == np.float32 and np.all(np.abs(got - want) <= (2.0 ** -24 + (W + 4) * 2.0 ** -52) * want)


def test_mel_sums_restatement_against_fsum():
    """Validates the restatement (the tests' oracle), not the library: the documented order against math.fsum."""
    rng = np.random.default_rng(4)
    for F, T, n in ((100, 37, 37), (7, 600, 513), (100, 37, 0), (3, 300, 256)):
        mel = rng.normal(-3.0, 2.0, (F, T)).astype(np.float32)
        s, q, flag = cr.mel_sums(mel, n)
        fs, fq, mag_s, mag_q, count = cr.fsum_sums(mel, n)
        assert not flag
        assert abs(s - fs) <= count * 2.0 ** -53 * mag_s and abs(q - fq) <= count * 2.0 ** -53 * mag_q
        padded = np.concatenate([mel, np.full((F, 5), np.nan, dtype=np.float32)], axis=1)          # a NaN beyond n is never read
        assert cr.mel_sums(padded, n) == (s, q, False)
    mel = rng.normal(0, 1, (7, 40)).astype(np.float32)
    mel[3, 11] = np.inf
    assert cr.mel_sums(mel, 40)[2] and not cr.mel_sums(mel, 11)[2]
    mean, std = cr.statistics(-300.0, 1300.0, 10, 10)
    assert mean == -3.0 and math.isclose(std, 2.0)


def test_measure_table_has_the_layout_of_the_references_print():
    """tools/prepare_corpus.py builds its per-speaker table from a column specification; on the recorded durations it must give,
    character for character, what the reference's own routine printed (tests/golden/silence_table.txt)."""
    spec = importlib.util.spec_from_file_location("prepare_corpus", ROOT / "tools" / "prepare_corpus.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    t = json.loads((GOLDEN / "silence_table.json").read_text())
    got = tool.silence_table(t["caption"].split(" (")[0], t["effective"], t["absolute"], t["effective_db"], t["absolute_db"])
    assert "\n" + got + "\n" == (GOLDEN / "silence_table.txt").read_text()
    assert sorted(t["effective"]) == ["0", "17"] and sum(len(v) for v in t["effective"].values()) == 8
    plain = tool.format_table("t", (("a", 3, ""), ("b", 6, ".2f")), [("x", 1.0), ("yy", 22.125)], rule=7)
    assert plain.split("\n") == ["t", "=======", "a   b     ", "-------", "x   1.00  ", "yy  22.12 ", "======="]

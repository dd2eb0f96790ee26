"""CPU checks of the batched waveform tail's boundary (nothing runs on a GPU): the new C entries are declared in include/mtts.h,
exported by the built library and bound in _hip.py with the declared number of arguments; the host-side argument checks answer
through mtts_last_error; the new kernels are in the gfx950 code objects and use no scratch memory; the batcher reads its
switch per instance."""
import re
import subprocess

import pytest

from conftest import ROOT, sub

LLVM = "/opt/rocm/lib/llvm/bin"
PKG = ROOT / "matcha-tts-24k_amd"


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def test_new_entries_are_declared_exported_and_bound_with_matching_arity(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    # every new declaration cites the reference lines it restates, as the other entries do
    assert "vocos_wrapper.py:8-9" in header and "inference.py:260-264" in header and "inference.py:268-287" in header


def test_host_side_argument_checks(lib):
    assert lib.mtts_waveform_workspace_bytes(256 * 95, 4, 24000) > 0
    assert lib.mtts_waveform_workspace_bytes(-1, 4, 24000) == -1
    assert lib.mtts_waveform_workspace_bytes(1000, 4, 50) == -1           # int(0.01 * 50) = 0 samples per window
    # grows with the row length (chunk peaks + window RMS values) and with the batch
    assert lib.mtts_waveform_workspace_bytes(1_800_000, 1, 24000) > lib.mtts_waveform_workspace_bytes(18_000, 1, 24000)
    assert lib.mtts_waveform_workspace_bytes(18_000, 64, 24000) > lib.mtts_waveform_workspace_bytes(18_000, 1, 24000)
    assert lib.mtts_waveform_finish(None, 1024, None, 0, 1, 24000, -60.0, None, None, None, 0, None) == -1
    assert b"mtts_waveform_finish" in lib.mtts_last_error()
    # rows must be 16-byte aligned (the passes move 16 bytes per lane): refused before anything is launched
    assert lib.mtts_waveform_finish(0x1000, 1022, 0x2000, 0, 1, 24000, -60.0, 0x3000, 0x4000, 0x5000, 1 << 20, None) == -1
    assert b"16-byte aligned" in lib.mtts_last_error()
    v = lib.mtts_vocos_create(100, 512, 1536, 8, 1024, 256)
    try:
        plain, ragged = lib.mtts_vocos_workspace_bytes(v, 4, 96), lib.mtts_vocos_ragged_workspace_bytes(v, 4, 96)
        assert plain > 0 and plain <= ragged <= plain + 1024                # the status words, nothing else
        assert lib.mtts_vocos_ragged_workspace_bytes(v, 4, 1) == -1
        assert lib.mtts_vocos_decode_ragged(v, None, None, 4, 96, None, None, 0, None) == -1
        assert b"null lengths" in lib.mtts_last_error()
    finally:
        lib.mtts_vocos_destroy(v)


def kernel_metadata(stem, tmp_path):
    """{kernel symbol: private (scratch) segment bytes} from the gfx950 code object of one translation unit."""
    sub("_hip").build()
    obj = PKG / "build" / f"{stem}.o"
    assert obj.exists(), obj
    fat, co = tmp_path / f"{stem}.fat", tmp_path / f"{stem}.co"
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", str(obj)], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, flags=re.M)             # the kernel's own key (its arguments' sit deeper)
        scratch = re.search(r"^    \.private_segment_fixed_size:\s+(\d+)", block, flags=re.M)
        if name and scratch:
            out[name.group(1)] = int(scratch.group(1))
    return out


@pytest.mark.parametrize("stem,wanted", [
    ("waveform", ["wave_peak_kernel", "wave_scale_rms_kernelILi4E", "wave_scale_rms_kernelILi1E", "wave_trim_kernel"]),
    ("vocos", ["dwconv7_ln_kernelILb1E", "dwconv7_ln_kernelILb0E", "istft_ola_kernelILb1E", "istft_ola_kernelILb0E",
               "vocos_lengths_check_kernel"]),
    ("norm_glue", ["cf_to_cl_kernelILb1E", "cf_to_cl_kernelILb0E"]),
])
def test_new_kernels_are_in_the_gfx950_code_object_without_scratch(stem, wanted, tmp_path):
    meta = kernel_metadata(stem, tmp_path)
    assert meta, "no kernel metadata found"
    for w in wanted:
        hits = [k for k in meta if w in k]
        assert len(hits) == 1, (w, sorted(meta))
        assert meta[hits[0]] == 0, (hits[0], meta[hits[0]])


def test_batcher_reads_its_switch_per_instance(monkeypatch):
    bt = sub("batcher")
    made = []
    for flag, want in ((None, True), ("0", False), ("1", True)):
        if flag is None:
            monkeypatch.delenv("MTTS_WAVE_BATCH", raising=False)
        else:
            monkeypatch.setenv("MTTS_WAVE_BATCH", flag)
        q = bt.FrameBudgetBatcher(model=None, run_batch=lambda batch: [{} for _ in batch])
        made.append(q)
        assert q.wave_batch is want
    assert [q.wave_batch for q in made] == [True, False, True]              # an earlier batcher keeps what it read
    for q in made:
        q.close()


def test_public_python_names():
    inf, voc = sub("inference"), sub("vocoder")
    import inspect
    assert list(inspect.signature(inf.to_waveforms).parameters)[:4] == ["mel", "mel_lengths", "vocoder", "trim"]
    assert inspect.signature(inf.to_waveforms).parameters["trim"].default is True
    assert inspect.signature(voc.Vocos.decode).parameters["lengths"].default is None
    assert inspect.signature(voc.VocosWrapper.forward).parameters["lengths"].default is None

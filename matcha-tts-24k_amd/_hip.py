"""ctypes binding of libmtts_hip.so (C ABI in include/mtts.h) + the in-tree hipcc build.

There is no CPU fallback: every entry point raises if the library is missing or a tensor is not
on a HIP device.  PyTorch is used only for device memory (workspaces, outputs) and the stream.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .hparams import PathHParams

HERE = Path(__file__).resolve().parent
CSRC = HERE / "csrc"
LIB = Path(os.environ["MTTS_HIP_LIB"]) if os.environ.get("MTTS_HIP_LIB") else HERE / "libmtts_hip.so"   # override: A/B of two builds
SOURCES = ["gemm_f32.hip", "attention_f32.hip", "gemm_p16.hip", "tblock_chain.hip", "tblock_chain_h16.hip", "resnet_conv.hip", "norm_glue.hip", "vocos.hip", "waveform.hip", "mel_frontend.hip", "resample.hip", "audio_codec.hip", "flac.hip", "flac_decode.hip", "corpus.hip", "pitch.hip", "wave_join.hip", "timing.hip", "loudness.hip", "style_encoder.hip", "style_grad.hip", "dp_grad.hip", "mas.hip", "score.hip", "spk_grad.hip", "model.hip", "pack.hip", "decoder.hip", "encoder.hip", "unit_entries.hip"]
HEADERS = [CSRC / "kernels.h", CSRC / "device_utils.h", CSRC / "model.h", CSRC / "host.h", HERE.parent / "include" / "mtts.h"]
SOLVERS = {"euler": 0, "midpoint": 1, "rk4": 2}


class MttsConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_feats", "n_spks", "spk_emb_dim", "n_vocab", "enc_channels", "enc_filter", "enc_heads", "enc_layers",
        "enc_kernel", "prenet_layers", "prenet_kernel", "dp_filter", "dp_kernel", "dp_layers", "dec_levels")] + [
        ("dec_channels", C.c_int32 * 4)] + [(n, C.c_int32) for n in (
            "dec_head_dim", "dec_heads", "dec_n_blocks", "dec_mid_blocks")]


class MttsGemmH16Args(C.Structure):
    """include/mtts.h mtts_gemm_h16_args, field for field."""
    _fields_ = [
        ("d_a", C.c_void_p), ("lda", C.c_int32), ("C", C.c_int32), ("c1", C.c_int32), ("d_a_mask", C.c_void_p),
        ("B", C.c_int32), ("T_in", C.c_int32), ("T_out", C.c_int32), ("ntaps", C.c_int32), ("h_tap_off", C.c_void_p),
        ("in_stride", C.c_int32),
        ("d_a_mean", C.c_void_p), ("d_a_rstd", C.c_void_p), ("d_a_part", C.c_void_p), ("a_nparts", C.c_int32),
        ("h_w", C.c_void_p), ("d_bias", C.c_void_p), ("N", C.c_int32),
        ("act", C.c_int32), ("d_p0", C.c_void_p), ("d_p1", C.c_void_p),
        ("d_res", C.c_void_p), ("ldr", C.c_int32),
        ("res16_mode", C.c_int32), ("d_res16_f32", C.c_void_p),
        ("d_out_mask", C.c_void_p), ("out_scale", C.c_float),
        ("d_out16_mask", C.c_void_p),
        ("d_out", C.c_void_p),
        ("d_out16_f32", C.c_void_p), ("out16_preload", C.c_int32),
        ("out_T", C.c_int32), ("out_stride", C.c_int32), ("out_off", C.c_int32),
        ("d_stats_out", C.c_void_p),
        ("d_gn_stats", C.c_void_p), ("gn_groups", C.c_int32), ("d_gn_nrows", C.c_void_p),
        ("d_gnr_y", C.c_void_p), ("d_gnr_stats", C.c_void_p), ("gnr_tile_rows", C.c_int32), ("gnr_groups", C.c_int32),
        ("d_gnr_gamma", C.c_void_p), ("d_gnr_beta", C.c_void_p), ("d_gnr_mask", C.c_void_p), ("gnr_eps", C.c_float),
        ("d_gnr_nextra", C.c_void_p), ("d_gnr_bias_stats", C.c_void_p),
        ("force_bm", C.c_int32),
        ("half16", C.c_int32), ("bf16", C.c_int32),
        ("d_range_flag", C.c_void_p),
        ("wave_rows", C.c_int32), ("tag", C.c_char * 124)]


def _deps(src: Path, seen=None):
    """The source and the local headers it includes, transitively (quoted #include lines)."""
    import re
    seen = set() if seen is None else seen
    if src in seen or not src.exists():
        return seen
    seen.add(src)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', src.read_text(), flags=re.M):
        _deps((src.parent / inc).resolve(), seen)
    return seen


class MttsChainArgs(C.Structure):
    """include/mtts.h mtts_chain_args, field for field."""
    _fields_ = [
        ("d_att", C.c_void_p), ("d_x", C.c_void_p), ("M", C.c_int32), ("C", C.c_int32), ("inner", C.c_int32),
        ("h_w_out", C.c_void_p), ("h_b_out", C.c_void_p), ("h_w1", C.c_void_p), ("h_b1", C.c_void_p), ("h_p0", C.c_void_p), ("h_p1", C.c_void_p),
        ("h_w2", C.c_void_p), ("h_b2", C.c_void_p), ("h_w_qkv", C.c_void_p), ("h_b_qkv", C.c_void_p), ("n_qkv", C.c_int32),
        ("d_out_mask", C.c_void_p), ("qb", C.c_int32), ("ch", C.c_int32), ("pair", C.c_int32),
        ("pad_att", C.c_int32), ("pad_x", C.c_int32), ("pad_out", C.c_int32), ("pad_qkv", C.c_int32),
        ("sentinel", C.c_uint32),
        ("d_range_flag", C.c_void_p),
        ("d_x_out", C.c_void_p), ("d_qkv_out", C.c_void_p),
        ("d_x_out_image", C.c_void_p), ("d_qkv_image", C.c_void_p),
        ("tag", C.c_char * 124)]


class MttsConvGnArgs(C.Structure):
    """include/mtts.h mtts_conv_gn_args, field for field."""
    _fields_ = [
        ("d_x", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("c1", C.c_int32), ("d_w", C.c_void_p),
        ("d_wpacked", C.c_void_p), ("d_bias", C.c_void_p), ("N", C.c_int32),
        ("d_gamma", C.c_void_p), ("d_beta", C.c_void_p), ("d_mask", C.c_void_p), ("d_chbias", C.c_void_p), ("chbias_stride", C.c_int32),
        ("d_nrows", C.c_void_p), ("d_nextra", C.c_void_p), ("d_bias_stats", C.c_void_p), ("eps", C.c_float),
        ("pad_x", C.c_int32), ("pad_out", C.c_int32),
        ("sentinel", C.c_uint32),
        ("d_range_flag", C.c_void_p),
        ("d_out", C.c_void_p),
        ("d_out_image", C.c_void_p),
        ("tag", C.c_char * 124)]


ENTRY_GUARD_ROWS = 64     # include/mtts.h MTTS_ENTRY_GUARD_ROWS

BUILD_MODE = "not built in this process"     # what the last build() call did (printed by __graft_entry__.build)


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile the HIP sources for gfx950 into libmtts_hip.so next to this file (cross-compiles without a GPU).
    Incremental: a translation unit is recompiled when it or a header it includes is newer than its object; the link runs
    when any object is newer than the library.  ``BUILD_MODE`` records what happened (compiled / reused)."""
    global BUILD_MODE
    srcs = [CSRC / s for s in SOURCES]
    if LIB.exists() and not force:
        deps = set(HEADERS)
        for src in srcs:
            deps |= _deps(src.resolve())
        newest = max(p.stat().st_mtime for p in deps)
        if LIB.stat().st_mtime >= newest:
            BUILD_MODE = f"reused {LIB.name} (newer than every source and header)"
            return LIB
    # -ffp-contract=off: keep the reference's rounding points (no silent FMA fusion in the element-wise math).
    # -fno-slp-vectorize: hipcc (ROCm 7.2) otherwise packs adjacent fp32 ops into v_pk_mul_f32 / v_pk_add_f32.  With SLP on,
    #   gemm_f32_kernel<*, *, NORM=true, TERMS=6|2> returns grossly wrong rows (error 0.6 at magnitude 7) when its LayerNorm
    #   statistics come from partial moments (a_part): DETERMINISTIC repro = build with MTTS_SLP=1 and run
    #   tests/test_hip_kernels.py::test_layernorm_stats_travel_through_epilogue[bf16x6|f16x3s] (2 of 75 kernel tests fail, every
    #   run; all other translation units pass with SLP on).  The packed ops sit in the normalise -> split -> LDS-store chain
    #   ((x - mean) * rstd as v_pk_mul_f32 op_sel:[0,1], the split's subtractions as v_pk_add_f32 neg_lo/neg_hi); a scan for
    #   VALU -> DPP wait-state violations found none, the root cause inside the compiler's output is not isolated.  Packed fp32
    #   VALU is an anti-lever beside MFMAs anyway (MI355X_MICROARCH.md cycle table; 29.98 vs 29.8 ms/step), so the flag stays
    #   on for every translation unit.
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    slp = [] if os.environ.get("MTTS_SLP") == "1" else ["-fno-slp-vectorize"]
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", *slp, "-fPIC",
             *os.environ.get("MTTS_HIPCC_EXTRA", "").split()]
    # one translation unit per process (the GEMM files instantiate dozens of kernels each), objects in build/, then one link
    objdir = HERE / "build"
    objdir.mkdir(exist_ok=True)

    compiled = []

    def compile_one(src: Path) -> Path:
        obj = objdir / (src.stem + ".o")
        if obj.exists() and not force and obj.stat().st_mtime >= max(p.stat().st_mtime for p in _deps(src.resolve())):
            return obj
        compiled.append(src.name)
        cmd = [hipcc, *flags, "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src.name}:\n{res.stdout}\n{res.stderr}")
        return obj

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1, 16)) as pool:
        objs = list(pool.map(compile_one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *[str(o) for o in objs], "-o", str(LIB)]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc link failed:\n{res.stdout}\n{res.stderr}")
    BUILD_MODE = f"compiled {', '.join(sorted(compiled)) or 'nothing'} with hipcc --offload-arch=gfx950 and linked {LIB.name}"
    return LIB


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the library and declare every signature of include/mtts.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB.exists():
        raise RuntimeError(f"{LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP path has no CPU fallback)")
    lib = C.CDLL(str(LIB))
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    # argument lists that several entries share, named once
    gemm = [vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, f32, vp, i32]   # d_a .. ldc
    conv_gn = [vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]                    # d_x .. d_chbias
    conv_gn_tail = [vp, vp, vp, f32, vp, vp, vp]                                            # d_nrows .. stream
    chain = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]        # d_att .. d_out_mask
    chain_p16 = chain + [i32, i32, vp, vp, vp, vp]                                          # qb, ch, d_x_out, d_qkv_out, d_scratch, stream
    chain_h16 = chain + [i32, i32, i32, i32, vp, vp, vp, vp]                                # bf16, qb, ch, pf_wgs, ...
    timed = [i32, C.POINTER(C.c_float)]                                                     # repeat, h_ms
    gn_image = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, i32, vp, vp, vp, vp]  # d_y .. d_out16_mask
    gemm_block, chain_block, conv_gn_block = C.POINTER(MttsGemmH16Args), C.POINTER(MttsChainArgs), C.POINTER(MttsConvGnArgs)
    sig = {
        "mtts_abi_version": (i32, []),
        "mtts_last_error": (C.c_char_p, []),
        "mtts_create": (vp, [C.POINTER(MttsConfig)]),
        "mtts_destroy": (None, [vp]),
        "mtts_set_tensor": (i32, [vp, C.c_char_p, vp, i64]),
        "mtts_weights_bytes": (i64, [vp]),
        "mtts_upload_weights": (i32, [vp, vp, i64]),
        "mtts_debug_hold": (i32, [vp, i32]),
        "mtts_weights_signature": (i32, [vp, C.c_char_p, i64]),
        "mtts_export_weights": (i32, [vp, vp, i64, C.POINTER(i32)]),
        "mtts_import_weights": (i32, [vp, vp, i64, i32]),
        "mtts_encoder_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_text_encoder_forward": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i64, vp]),
        "mtts_speaker_embedding": (i32, [vp, i32, vp, i32, vp, vp]),
        "mtts_durations": (i32, [vp, vp, f32, f32, i32, i32, vp, vp, vp, vp]),
        "mtts_durations_per_utterance": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "mtts_durations_given": (i32, [vp, vp, f32, vp, vp, i32, i32, vp, vp, vp, vp]),
        "mtts_durations_shaped": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "mtts_align_pool": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
        "mtts_set_frame_limits": (i32, [vp, vp]),
        "mtts_decoder_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_decoder_forward": (i32, [vp, vp, vp, vp, f32, i32, i32, vp, vp, i64, vp]),
        "mtts_cfm_solve": (i32, [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, i32, f32, f32, vp, i64, vp]),
        "mtts_fold_rows": (i32, [vp, i32, i32]),
        "mtts_cfm_solve_folded": (i32, [vp, vp, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp, i32, f32, f32, vp, i64, vp]),
        "mtts_cfm_step": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i64, vp]),
        "mtts_gemm_packed_bytes": (i64, [i32, i32, i32]),
        "mtts_attention_p16": (i32, [vp, vp, i32, i32, i32, i32, f32, i32, vp, vp, vp]),
        "mtts_gemm_p16_scratch_bytes": (i64, [i32, i32, i32, i32, i32]),
        "mtts_conv_gn_scratch_bytes": (i64, [i32, i32, i32, i32]),
        "mtts_conv_gn": (i32, conv_gn + conv_gn_tail),
        "mtts_conv_gn_rows": (i32, conv_gn + [i32] + conv_gn_tail),
        "mtts_gemm_p16": (i32, gemm + [vp, f32, vp, i32, vp, vp]),
        "mtts_gemm_f32": (i32, gemm + [vp, i32, vp]),
        "mtts_attention_f32": (i32, [vp, vp, i32, i32, i32, i32, f32, i32, vp, vp]),
        "mtts_chain_stream_frags": (i64, [i32, i32, i32, i32]),
        "mtts_chain_plan": (i32, [i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mtts_chain_shape_exists": (i32, [i32, i32, i32]),
        "mtts_tblock_plan": (i32, [i32] * 12 + [C.POINTER(C.c_int)] * 5),
        "mtts_chain_stream_frags_pair": (i64, [i32, i32, i32, i32]),
        "mtts_chain_stream_pack_pair": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "mtts_chain_stream_pack": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "mtts_tblock_chain_scratch_bytes": (i64, [i32, i32, i32, i32, i32]),
        "mtts_tblock_chain": (i32, chain_p16),
        "mtts_tblock_chain_timed": (i32, chain_p16 + timed),
        "mtts_tblock_chain_pair_timed": (i32, chain_p16 + timed),
        "mtts_tblock_chain_args_scratch_bytes": (i64, [chain_block]),
        "mtts_tblock_chain_args_run": (i32, [chain_block, vp, vp]),
        "mtts_conv_gn_args_scratch_bytes": (i64, [conv_gn_block]),
        "mtts_conv_gn_args_run": (i32, [conv_gn_block, vp, vp]),
        "mtts_chain_stream_frags_h16": (i64, [i32, i32, i32, i32]),
        "mtts_chain_stream_pack_h16": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, C.POINTER(C.c_int)]),
        "mtts_tblock_chain_h16_scratch_bytes": (i64, [i32, i32, i32, i32, i32]),
        "mtts_tblock_chain_h16": (i32, chain_h16),
        "mtts_tblock_chain_h16_timed": (i32, chain_h16 + timed),
        "mtts_last_kernel_tag": (C.c_char_p, []),
        "mtts_panel_h16_host": (i32, [vp, i64, i32, vp]),
        "mtts_to_h16_roundtrip": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
        "mtts_gemm_h16_scratch_bytes": (i64, [gemm_block]),
        "mtts_gemm_h16": (i32, [gemm_block, vp, vp]),
        "mtts_gemm_h16_wave_rows": (i32, [i32, i32, i32, i32]),
        "mtts_attention_h16": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, vp, vp, vp, vp]),
        "mtts_groupnorm_h16_scratch_bytes": (i64, [i32, i32, i32, i32]),
        "mtts_groupnorm_mish_h16": (i32, gn_image + [i32, vp, vp, vp, vp, vp]),
        "mtts_to_p16_roundtrip": (i32, [vp, i32, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp]),
        "mtts_gemm_p16_args_scratch_bytes": (i64, [gemm_block]),
        "mtts_gemm_p16_args_run": (i32, [gemm_block, i32, f32, vp, vp]),
        "mtts_attention_p16_run": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, f32, vp, vp, vp, vp]),
        "mtts_groupnorm_p16_scratch_bytes": (i64, [i32, i32, i32, i32]),
        "mtts_groupnorm_mish_p16": (i32, gn_image + [vp, vp, vp, vp, vp]),
        "mtts_gemm_f32_args_scratch_bytes": (i64, [gemm_block]),
        "mtts_gemm_f32_args_run": (i32, [gemm_block, i32, vp, i32, i32, f32, vp, vp]),
        "mtts_attention_f32_run": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, i32, vp, vp]),
        "mtts_groupnorm_mish_f32_run": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]),
        "mtts_channel_layernorm_ld": (i32, [vp, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp, vp, i32, vp]),
        "mtts_row_stats": (i32, [vp, i32, i32, i32, f32, vp, vp, vp]),
        "mtts_channel_layernorm": (i32, [vp, i32, i32, i32, vp, vp, f32, i32, vp, vp, vp, vp]),
        "mtts_groupnorm_scratch_bytes": (i64, [i32, i32, i32]),
        "mtts_groupnorm_mish": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp]),
        "mtts_groupnorm_mish_rows": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp]),
        "mtts_dwconv7_ln": (i32, [vp, vp, vp, vp, vp, f32, i32, i32, i32, vp, vp, vp]),
        "mtts_spec_polar": (i32, [vp, i32, i32, i32, i32, f32, vp]),
        "mtts_istft_ola": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "mtts_ode_combine": (i32, [i32, f32, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp]),
        "mtts_step_tables": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "mtts_time_sinusoid": (i32, [vp, vp, vp, i32, i32, f32, vp, vp]),
        "mtts_rope": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp]),
        "mtts_cf_to_cl": (i32, [vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp]),
        "mtts_cl_to_cf": (i32, [vp, i32, i32, i32, i32, vp, i32, f32, f32, vp]),
        "mtts_slots_to_cl": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp]),
        "mtts_cl_to_slots": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp]),
        "mtts_vocos_create": (vp, [i32, i32, i32, i32, i32, i32]),
        "mtts_vocos_destroy": (None, [vp]),
        "mtts_vocos_set_tensor": (i32, [vp, C.c_char_p, vp, i64]),
        "mtts_vocos_weights_bytes": (i64, [vp]),
        "mtts_vocos_upload_weights": (i32, [vp, vp, i64]),
        "mtts_vocos_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_vocos_decode": (i32, [vp, vp, i32, i32, vp, vp, i64, vp]),
        "mtts_vocos_ragged_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_vocos_decode_ragged": (i32, [vp, vp, vp, i32, i32, vp, vp, i64, vp]),
        "mtts_vocos_ragged_status": (i32, [vp, vp]),
        "mtts_waveform_workspace_bytes": (i64, [i64, i32, i32]),
        "mtts_waveform_finish": (i32, [vp, i64, vp, i32, i32, i32, C.c_double, vp, vp, vp, i64, vp]),
        "mtts_melfe_create": (vp, [i32, i32, i32]),
        "mtts_melfe_destroy": (None, [vp]),
        "mtts_melfe_n_bins": (i32, [vp]),
        "mtts_melfe_basis": (i32, [vp, vp, i64]),
        "mtts_melfe_filterbank": (i32, [vp, vp, i64]),
        "mtts_melfe_workspace_bytes": (i64, [vp, i32, i64, i32]),
        "mtts_melfe_forward": (i32, [vp, vp, i64, vp, i32, i32, f32, f32, vp, i32, vp, vp, i64, vp]),
        "mtts_resampler_create": (vp, [i32, i32, i32, C.c_double]),
        "mtts_resampler_destroy": (None, [vp]),
        "mtts_resample_tile": (i32, []),
        "mtts_resample_factors": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "mtts_resample_out_length": (i64, [vp, i64]),
        "mtts_resample_bank": (i32, [vp, vp, i64]),
        "mtts_resample_workspace_bytes": (i64, [vp, i32, i64]),
        "mtts_resample_forward": (i32, [vp, vp, i64, vp, i32, vp, i64, vp, vp, i64, vp]),
        "mtts_resample_status": (i32, [vp, vp]),
        "mtts_codec_tile": (i32, []),
        "mtts_pcm_encode": (i32, [vp, i64, vp, vp, vp, i32, i32, i64, vp, vp, vp]),
        "mtts_pcm_decode": (i32, [vp, i64, vp, vp, i32, vp, i64, vp, vp]),
        "mtts_pcm_status": (i32, [vp, i32, vp]),
        "mtts_flac_row_bytes": (i64, [i64, i32]),
        "mtts_flac_workspace_bytes": (i64, [i32, i64, i32]),
        "mtts_flac_encode": (i32, [vp, i64, vp, vp, vp, i32, i32, i32, i64, vp, i64, vp, vp, i64, vp]),
        "mtts_flac_encode_lpc": (i32, [vp, i64, vp, vp, vp, i32, i32, i32, i32, i64, vp, i64, vp, vp, i64, vp]),
        "mtts_flac_decode_workspace_bytes": (i64, [i32, i64, i64, i32]),
        "mtts_flac_decode": (i32, [vp, i64, vp, i32, i32, vp, i64, vp, vp, vp, i64, vp]),
        "mtts_flac_parse_host": (i64, [vp, i64, i32, vp, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "mtts_silence_window": (i32, [i32]),
        "mtts_silence_workspace_bytes": (i64, [i64, i32, i32]),
        "mtts_silence_measure": (i32, [vp, i64, vp, i32, i32, C.c_double, C.c_double, vp, vp, i64, vp]),
        "mtts_silence_normalize": (i32, [vp, i64, vp, vp, i32, i32, i64, i64, vp, i64, vp, vp, vp, i64, vp]),
        "mtts_silence_status": (i32, [vp, vp]),
        "mtts_mel_stats_chunk": (i32, []),
        "mtts_mel_stats_workspace_bytes": (i64, [i32, i32]),
        "mtts_mel_stats": (i32, [vp, i32, i32, vp, i32, vp, vp, vp, vp, i64, vp]),
        "mtts_mel_stats_status": (i32, [vp, vp]),
        "mtts_pitch_tile": (i32, []),
        "mtts_pitch_plan": (i32, [i32, i32, C.c_double, C.c_double, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "mtts_pitch_workspace_bytes": (i64, [i64, i32, i32, i32, C.c_double, C.c_double]),
        "mtts_pitch_track": (i32, [vp, i64, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, i64, vp, vp, i64, vp]),
        "mtts_pitch_stats": (i32, [vp, i64, vp, i32, i64, vp, vp, vp, i64, vp]),
        "mtts_pitch_status": (i32, [vp, vp]),
        "mtts_pitch_candidates": (i32, [vp, i64, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp]),
        "mtts_pitch_viterbi_workspace_bytes": (i64, [i64, i32]),
        "mtts_pitch_viterbi": (i32, [vp, vp, vp, vp, vp, vp, i64, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp, i64, vp]),
        "mtts_pitch_fold": (i32, [vp, i64, vp, i32, i32, i32, i32, vp, i32, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_wave_join_workspace_bytes": (i64, [i64, i64]),
        "mtts_wave_join": (i32, [vp, i64, vp, vp, vp, vp, i32, i32, i64, i64, vp, i64, vp, vp, vp, i64, vp]),
        "mtts_wave_join_status": (i32, [vp, vp]),
        "mtts_token_timing_workspace_bytes": (i64, [i64, i64]),
        "mtts_token_timing": (i32, [vp, vp, vp, i32, i32, i32, i64, vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, vp]),
        "mtts_token_timing_status": (i32, [vp, i32, vp]),
        "mtts_wave_breaks": (i32, [vp, i64, vp, i32, i64, i64, vp, i64, vp, i64, vp]),
        "mtts_loudness_chunk": (i32, [i32]),
        "mtts_loudness_tile": (i32, []),
        "mtts_loudness_coefficients": (i32, [i32, C.POINTER(C.c_double)]),
        "mtts_loudness_workspace_bytes": (i64, [i64, i32, i32]),
        "mtts_loudness": (i32, [vp, i64, vp, i32, i32, vp, f32, i32, vp, vp, vp, vp, i64, vp]),
        "mtts_loudness_status": (i32, [vp, vp]),
        "mtts_true_peak_tile": (i32, []),
        "mtts_true_peak_filter": (i32, [i32, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
        "mtts_loudness_r128_workspace_bytes": (i64, [i64, i32, i32]),
        "mtts_loudness_r128": (i32, [vp, i64, vp, i32, i32, vp, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_style_create": (vp, [i32, i32, i32, i32]),
        "mtts_style_destroy": (None, [vp]),
        "mtts_style_set_tensor": (i32, [vp, C.c_char_p, vp, i64]),
        "mtts_style_weights_bytes": (i64, [vp]),
        "mtts_style_upload_weights": (i32, [vp, vp, i64]),
        "mtts_style_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_style_forward": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, i64, vp]),
        "mtts_style_param_count": (i64, [vp]),
        "mtts_style_param_offset": (i64, [vp, C.c_char_p]),
        "mtts_style_grad_weights_bytes": (i64, [vp]),
        "mtts_style_grad_upload_weights": (i32, [vp, vp, i64]),
        "mtts_style_grad_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_style_grad_tape_offset": (i64, [vp, i32, i32, i32]),
        "mtts_style_forward_taped": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, i64, vp]),
        "mtts_style_backward": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_conv_wgrad_chunk_rows": (i32, [i32, i32]),
        "mtts_conv_wgrad_workspace_bytes": (i64, [i32, i32, i32, i32]),
        "mtts_conv_wgrad": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp]),
        "mtts_mas_workspace_bytes": (i64, [i32, i32, i32]),
        "mtts_mas_logprior": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
        "mtts_mas": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        "mtts_mas_status": (i32, [vp, vp]),
        "mtts_decoder_forward_rows": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, i64, vp]),
        "mtts_cfm_loss": (i32, [vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, vp, vp, vp, i64, vp]),
        "mtts_score_workspace_bytes": (i64, [i32, i32, i32]),
        "mtts_score_serial_run": (i32, [i32, i32, i32, i32]),
        "mtts_score_prior_dur": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_score_status": (i32, [vp, vp]),
        "mtts_spk_grad_weights_bytes": (i64, [vp]),
        "mtts_spk_grad_upload_weights": (i32, [vp, vp, i64]),
        "mtts_spk_grad_workspace_bytes": (i64, [vp, i32, i32, i32]),
        "mtts_spk_grad_tape_offset": (i64, [vp, i32, i32, i32, i32]),
        "mtts_spk_grad_rows_offset": (i64, [vp, i32, i32, i32]),
        "mtts_spk_grad": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_spk_grad_status": (i32, [vp, vp]),
        "mtts_dp_param_count": (i64, [vp]),
        "mtts_dp_param_offset": (i64, [vp, C.c_char_p]),
        "mtts_dp_train_weights_bytes": (i64, [vp]),
        "mtts_dp_train_pack": (i32, [vp, vp, vp, i64]),
        "mtts_dp_train_upload": (i32, [vp, vp, vp, i64]),
        "mtts_dp_grad_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_dp_grad_tape_offset": (i64, [vp, i32, i32, i32]),
        "mtts_dp_grad": (i32, [vp, vp, vp, vp, vp, vp, f32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_dp_grad_status": (i32, [vp, vp]),
        "mtts_dp_unit_workspace_bytes": (i64, [i32, i32, i32]),
        "mtts_ln_film_wgrad": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, i64, vp]),
        "mtts_rows_wgrad": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, i64, vp]),
        "mtts_outer_batch_sum": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "mtts_spk_grad_match_workspace_bytes": (i64, [vp, i32, i32]),
        "mtts_spk_grad_match": (i32, [vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
        "mtts_spk_grad_match_status": (i32, [vp, vp]),
        "mtts_match_seeds_scratch_bytes": (i64, [i32, i32]),
        "mtts_match_seeds": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
        "mtts_channel_layernorm_bwd": (i32, [vp, vp, i32, i32, i32, vp, vp, f32, i32, vp, vp, i32, vp, vp, vp, vp]),
        "mtts_attention_rope_bwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp]),
        "mtts_spk_grad_seeds_scratch_bytes": (i64, [i32, i32, i32]),
        "mtts_spk_grad_seeds": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, i64, vp]),
        "mtts_grad_gate": (i32, [vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]),
        "mtts_token_sums": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp]),
        "mtts_gemm_terms": (i32, [vp]),
        "mtts_set_arithmetic": (i32, [vp, i32]),
        "mtts_weights_saturate": (i32, [vp]),
        "mtts_prof_enable": (i32, [vp, i32]),
        "mtts_prof_reset": (i32, [vp]),
        "mtts_prof_records": (i64, [vp, C.POINTER(C.c_double), i64]),
        "mtts_prof_tags": (i64, [vp, C.c_char_p, i64]),
        "mtts_prof_read": (i32, [vp, i32, C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.mtts_abi_version() != 2:
        raise RuntimeError("libmtts_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("mtts: " + load().mtts_last_error().decode("utf-8", "replace"))


def size(n: int) -> int:
    """A count a ``*_bytes`` / ``*_offset`` entry returned: ``n``, or the library's error raised when it is negative."""
    if n < 0:
        check(-1)
    return n


def raise_refused(fn, *args, prefix: str = "") -> None:
    """Call a ``*_status`` entry -- the one entry of a ragged-batch call that waits for the stream -- and raise ``ValueError`` with the
    device's verdict (the first refused row) when there is one."""
    if fn(*args) != 0:
        raise ValueError(prefix + load().mtts_last_error().decode("utf-8", "replace"))


def on_device(t: torch.Tensor) -> bool:
    return t.is_cuda


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of a contiguous HIP tensor (None passes NULL)."""
    if t is None:
        return None
    if not on_device(t):
        raise RuntimeError("mtts: tensor is not on a HIP device; the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("mtts: tensor must be contiguous")
    return t.data_ptr()


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


class Workspaces:
    """GROW-ONLY scratch, one buffer per (kind, stream, device): a serving process sees a new (B, T_pad) with almost every request,
    so buffers keyed by shape would pin HBM without bound.  The C side takes (pointer, byte count) and bump-allocates what the
    call needs from the front.  Concurrent calls on different streams must not share scratch, hence the stream key; a buffer being
    replaced is dropped before its successor is allocated, and its memory stays valid until the work queued on its stream has
    drained (torch's caching allocator frees a block for re-use in stream order).  ``latest(kind)`` is the buffer of this stream's
    latest ``kind`` call, whose header the status and flag readers look at."""

    def __init__(self):
        self._held: Dict[tuple, torch.Tensor] = {}
        self._latest: Dict[tuple, torch.Tensor] = {}

    def get(self, kind: str, need: int, device) -> torch.Tensor:
        """This stream's ``kind`` buffer on ``device`` with at least ``need`` bytes (``need`` < 0: the library's error)."""
        need = size(need)
        key = (kind, stream_ptr(), torch.device(device))
        ws = self._held.get(key)
        if ws is None or ws.numel() < need:
            if ws is not None and self._latest.get(key[:2]) is ws:
                del self._latest[key[:2]]
            ws = None
            self._held.pop(key, None)
            ws = self._held[key] = torch.empty(int(need), dtype=torch.uint8, device=key[2])
        self._latest[key[:2]] = ws
        return ws

    def latest(self, kind: str) -> Optional[torch.Tensor]:
        return self._latest.get((kind, stream_ptr()))

    def note(self, kind: str, ws: torch.Tensor) -> None:
        """Make a caller-owned buffer the latest of this stream (a captured HIP graph runs on its own scratch)."""
        self._latest[(kind, stream_ptr())] = ws

    def clear(self) -> None:
        self._held.clear()
        self._latest.clear()

    def bytes_held(self) -> int:
        return sum(int(w.numel()) for w in self._held.values())


def row_lengths(lengths, B: int, default, device, name: str = "lengths") -> torch.Tensor:
    """``lengths`` (tensor or sequence; None: ``default`` for every row) as int64 [B] on ``device``.  Nothing is read on the host."""
    if lengths is None:
        return torch.full((B,), default, dtype=torch.long, device=device)
    lengths = torch.as_tensor(lengths).to(device=device, dtype=torch.long).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"{name} must have shape ({B},), got {tuple(lengths.shape)}")
    return lengths


def aligned_rows(t: torch.Tensor, quantum: int, what: str, layout: str = "[B, L]") -> Tuple[torch.Tensor, int]:
    """``t`` [B, L] (or [L]) on the device as rows of 16-byte aligned quanta: ``(rows [B, ld], L)`` with ld = L rounded up to
    ``quantum`` elements, zeros beyond L and a 16-byte aligned base; ``t`` itself when it already is that.  ``quantum`` 4: float32
    samples (other dtypes are converted); 16: uint8 bytes (required)."""
    raw = quantum == 16
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or (raw and t.dtype != torch.uint8):
        raise ValueError(f"{what} must be {layout}")
    if not on_device(t):
        raise RuntimeError(f"matcha-tts-24k_amd: {what} is not on a HIP device; there is no CPU path")
    if not raw:
        t = t.detach().to(torch.float32)
    B, L = t.shape
    if B < 1 or L < 1:
        raise ValueError(f"{what} must have at least one row and one {'byte' if raw else 'sample'}")
    if L % quantum or not t.is_contiguous() or t.data_ptr() % 16:
        padded = torch.zeros(B, (L + quantum - 1) // quantum * quantum, dtype=t.dtype, device=t.device)
        padded[:, :L].copy_(t)
        t = padded
    return t, L


class DeviceComponent:
    """What the module mirrors of the library's weighted objects other than the path's context share (``vocoder.Vocos``,
    ``style.StyleEncoder``; mixed in ahead of their ``nn.Module`` base): the handle, its weight image on the device, dirty tracking and
    one grow-only workspace per stream.  A subclass gives ``_abi`` (prefix of its ``_create / _set_tensor / _weights_bytes /
    _upload_weights / _destroy`` functions), ``_what`` (its name in error texts), ``_create_args()`` and calls ``_init_component()``
    at the end of its ``__init__``; ``_tensors()`` is what gets registered (default: the state dict); ``_ws`` is its ``Workspaces``."""
    _abi = ""
    _what = ""

    def _init_component(self):
        for k, v in (("_ctx", None), ("_weights", None), ("_ws", Workspaces()), ("_dirty", True)):
            object.__setattr__(self, k, v)

    def _create_args(self):
        raise NotImplementedError

    def _tensors(self) -> Dict[str, torch.Tensor]:
        return dict(self.state_dict())

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        object.__setattr__(self, "_dirty", True)
        return out

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        object.__setattr__(self, "_dirty", True)
        return r

    def _ready(self):
        lib = load()
        if self._ctx is None:
            ctx = getattr(lib, self._abi + "_create")(*self._create_args())
            if not ctx:
                raise RuntimeError(self._abi + "_create: " + lib.mtts_last_error().decode())
            object.__setattr__(self, "_ctx", ctx)
        if self._dirty:
            p = next(self.parameters())
            if not p.is_cuda:
                raise RuntimeError(f"matcha-tts-24k_amd: the {self._what} must be on a HIP device; there is no CPU path")
            for k, v in self._tensors().items():
                a = np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy())
                check(getattr(lib, self._abi + "_set_tensor")(self._ctx, k.encode(), a.ctypes.data, a.size))
            n = size(getattr(lib, self._abi + "_weights_bytes")(self._ctx))
            w = torch.empty(n, dtype=torch.uint8, device=p.device)
            check(getattr(lib, self._abi + "_upload_weights")(self._ctx, w.data_ptr(), n))
            object.__setattr__(self, "_weights", w)
            self._ws.clear()
            object.__setattr__(self, "_dirty", False)
        return lib

    def __del__(self):
        try:
            if self._ctx:
                getattr(load(), self._abi + "_destroy")(self._ctx)
        except Exception:
            pass


def rope_tables(d: int, n: int = 4000):
    """cos/sin caches exactly as the reference builds them (text_encoder.py:138-146), [n, d] fp32 on the CPU."""
    theta = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    idx = torch.einsum("n,d->nd", torch.arange(n).float(), theta)
    idx2 = torch.cat([idx, idx], dim=1)
    return idx2.cos().contiguous(), idx2.sin().contiguous()


def time_freqs(dim: int) -> torch.Tensor:
    """Frequency table of SinusoidalPosEmb in the reference's fp32 arithmetic (decoder.py:24-26)."""
    import math
    half = dim // 2
    c = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half).float() * -c).contiguous()


class HipModel:
    """One mtts_ctx: packed weights on a device + cached workspaces + the path's entry points on torch tensors."""
    _uids = 0

    def __init__(self, hp: PathHParams, terms: Optional[int] = None):
        """``terms``: GEMM arithmetic (mtts_set_arithmetic); None = the library default (fp16 two-term split, MTTS_GEMM_TERMS)."""
        self.lib = load()
        self.hp = hp
        cfg = MttsConfig()
        e, d = hp.encoder, hp.decoder
        cfg.n_feats, cfg.n_spks, cfg.spk_emb_dim, cfg.n_vocab = hp.n_feats, hp.n_spks, hp.spk_emb_dim, hp.n_vocab
        cfg.enc_channels, cfg.enc_filter, cfg.enc_heads, cfg.enc_layers = e.n_channels, e.filter_channels, e.n_heads, e.n_layers
        cfg.enc_kernel, cfg.prenet_layers, cfg.prenet_kernel = e.kernel_size, e.prenet_layers, e.prenet_kernel_size
        cfg.dp_filter, cfg.dp_kernel, cfg.dp_layers = e.dp_filter_channels, e.dp_kernel_size, e.dp_n_layers
        if len(d.channels) > 4:
            raise ValueError("at most 4 decoder levels")
        cfg.dec_levels = len(d.channels)
        for i, ch in enumerate(d.channels):
            cfg.dec_channels[i] = ch
        cfg.dec_head_dim, cfg.dec_heads, cfg.dec_n_blocks, cfg.dec_mid_blocks = (d.attention_head_dim, d.num_heads, d.n_blocks,
                                                                                d.num_mid_blocks)
        self.ctx = self.lib.mtts_create(C.byref(cfg))
        if not self.ctx:
            raise RuntimeError("mtts_create: " + self.lib.mtts_last_error().decode())
        if terms is not None:
            check(self.lib.mtts_set_arithmetic(self.ctx, int(terms)))
        self.weights: Optional[torch.Tensor] = None
        HipModel._uids += 1
        self.uid = HipModel._uids    # unique per process (id() is re-used after garbage collection)
        self.generation = 0          # bumped by every load_state_dict: whatever captured the weights' address is stale afterwards
        self.device: Optional[torch.device] = None
        self._ws = Workspaces()      # the latest buffer per kind holds that call's header: range flag, pair time-out, verdict
        self._grad_weights: Optional[torch.Tensor] = None   # backward panels of speaker_grad, uploaded on first use ...
        self._grad_generation = -1                          # ... for this weight generation
        self._dp_tensors: Dict[str, torch.Tensor] = {}      # the duration predictor's tensors as loaded (host fp32): dp_params()
        self._dp_buf: Optional[torch.Tensor] = None         # its training component on the device (dp_train_buffer)

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.mtts_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def _set(self, key: str, t: torch.Tensor) -> None:
        a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
        check(self.lib.mtts_set_tensor(self.ctx, key.encode(), a.ctypes.data, a.size))

    def weights_signature(self) -> str:
        """Everything the packed image's layout depends on (mtts_weights_signature): the key of a packed-image cache."""
        buf = C.create_string_buffer(1024)
        size(self.lib.mtts_weights_signature(self.ctx, buf, 1024))
        return buf.value.decode()

    def load_state_dict(self, sd: Dict[str, torch.Tensor], device, cache_dir=None) -> None:
        """Register every tensor of a reference-format state dict (keys of SURVEY appendix A; torch.compile's
        ``_orig_mod.`` infix is ignored), add the host-precomputed tables, pack and upload.
        ``cache_dir`` (a converted checkpoint's directory, checkpoint.py): the packed image is read from / written to a cache
        file there, keyed by the library's layout signature and a digest of the tensors (``checkpoint.packed_cache``)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mtts: weights must live on a HIP device; the HIP path has no CPU fallback")
        for k, v in sd.items():
            k = k.replace("_orig_mod.", "")
            if k in ("mel_mean", "mel_std") or "rope." in k:
                continue
            self._set(k, v)
            if k.startswith(self.DP_PREFIX):
                self._dp_tensors[k] = v.detach().to("cpu", torch.float32).clone()
            if k.endswith("ff.net.0.alpha"):    # SnakeBeta parameters in the reference's own fp32 ops (transformer.py:68-75)
                self._set(k + "_exp", torch.exp(v.detach().float().cpu()))
            elif k.endswith("ff.net.0.beta"):
                self._set(k[:-4] + "inv_beta", 1.0 / (torch.exp(v.detach().float().cpu()) + 0.000000001))
        e = self.hp.encoder
        dh = (e.n_channels + self.hp.spk_emb_dim) // e.n_heads
        cos, sin = rope_tables(int(dh * 0.5))
        self._set("aux.rope_cos", cos)
        self._set("aux.rope_sin", sin)
        self._set("aux.time_freqs", time_freqs(2 * self.hp.n_feats))
        self.cache_hit = False
        cache = None
        if cache_dir is not None:
            from . import checkpoint as ck
            cache = ck.packed_cache(cache_dir, self.weights_signature(), sd)
            image = cache.read()
            if image is not None:
                try:
                    check(self.lib.mtts_import_weights(self.ctx, image["data"].ctypes.data, image["data"].nbytes, int(image["saturates"])))
                    self.cache_hit = True
                except RuntimeError:
                    self.cache_hit = False       # (a stale or foreign file: pack from the tensors below and rewrite it)
        nbytes = size(self.lib.mtts_weights_bytes(self.ctx))
        if cache is not None and not self.cache_hit:
            host = np.empty(nbytes, dtype=np.uint8)
            sat = C.c_int(0)
            check(self.lib.mtts_export_weights(self.ctx, host.ctypes.data, nbytes, C.byref(sat)))
            cache.write(host, bool(sat.value))
        self.weights = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(self.lib.mtts_upload_weights(self.ctx, self.weights.data_ptr(), nbytes))
        self.device = device
        self.generation += 1
        self._ws.clear()

    def _workspace(self, kind: str, a: int, b: int) -> torch.Tensor:
        """This stream's scratch of the encoder ("enc") or the estimator ("dec") for a (B, T) call (``Workspaces``)."""
        fn = self.lib.mtts_decoder_workspace_bytes if kind == "dec" else self.lib.mtts_encoder_workspace_bytes
        return self._ws.get(kind, fn(self.ctx, a, b), self.device)

    def range_flags(self) -> torch.Tensor:
        """Sticky range flags (include/mtts.h "range guard") of this stream's latest encoder and estimator calls as a device
        int32 tensor [2]; non-zero = an operand left the fp16 range and saturated.  Reading it (``.any().item()``) synchronises."""
        z = torch.zeros(1, dtype=torch.int32, device=self.device)
        parts = [z if ws is None else ws[:4].view(torch.int32) for ws in (self._ws.latest("enc"), self._ws.latest("dec"))]
        return torch.cat(parts)

    def pair_timeouts(self) -> torch.Tensor:
        """Second word of this stream's latest estimator workspace header: non-zero = a workgroup of a pair-form chain launch waited in
        vain for its partner (csrc/tblock_chain.hip) -- the call's results are void.  A device int32 tensor [1]."""
        ws = self._ws.latest("dec")
        return torch.zeros(1, dtype=torch.int32, device=self.device) if ws is None else ws[4:8].view(torch.int32)

    def call_flags(self, kind: str) -> Optional[torch.Tensor]:
        """The first two header words (range flag, pair time-out) of this stream's latest ``kind`` ("enc" / "dec") workspace as a device
        int32 view, or None when no such call ran: what a caller accumulates over several calls without reading any of them."""
        ws = self._ws.latest(kind)
        return None if ws is None else ws[:8].view(torch.int32)

    def weights_saturate(self) -> bool:
        return bool(size(self.lib.mtts_weights_saturate(self.ctx)))

    def decoder_workspace_bytes(self, B: int, T: int) -> int:
        return size(self.lib.mtts_decoder_workspace_bytes(self.ctx, int(B), int(T)))

    def note_workspace(self, kind: str, ws: torch.Tensor) -> None:
        """Make ``ws`` the buffer ``range_flags`` reads for this stream (a replayed HIP graph ran on it)."""
        self._ws.note(kind, ws)

    def workspace_bytes_held(self) -> int:
        return self._ws.bytes_held()

    def _status(self, kind: str, fn) -> None:
        ws = self._ws.latest(kind)
        if ws is not None:
            raise_refused(fn, ws.data_ptr(), stream_ptr())

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        if not t.is_cuda:
            raise RuntimeError("mtts: input tensor is not on a HIP device; the HIP path has no CPU fallback")
        return t.detach().to(torch.float32).contiguous()

    # ------------------------------------------------------------------ the path
    def text_encoder(self, x, x_lengths, e_enc, e_dur):
        B, Tx = x.shape
        x = x.detach().to(torch.int64).contiguous()
        x_lengths = x_lengths.detach().to(torch.int64).contiguous()
        e_enc, e_dur = self._f32(e_enc), self._f32(e_dur)
        if e_enc.shape[0] != B:
            e_enc, e_dur = e_enc.expand(B, -1).contiguous(), e_dur.expand(B, -1).contiguous()
        nf = self.hp.n_feats
        mu_x = torch.empty(B, nf, Tx, dtype=torch.float32, device=x.device)
        logw = torch.empty(B, 1, Tx, dtype=torch.float32, device=x.device)
        x_mask = torch.empty(B, 1, Tx, dtype=torch.float32, device=x.device)
        ws = self._workspace("enc", B, Tx)
        check(self.lib.mtts_text_encoder_forward(self.ctx, ptr(x), ptr(x_lengths), ptr(e_enc), ptr(e_dur), B, Tx, ptr(mu_x),
                                                 ptr(logw), ptr(x_mask), ws.data_ptr(), ws.numel(), stream_ptr()))
        return mu_x, logw, x_mask

    def speaker_embedding(self, table: int, ids: torch.Tensor) -> torch.Tensor:
        ids = ids.detach().to(torch.int64).contiguous()
        out = torch.empty(ids.numel(), self.hp.spk_emb_dim, dtype=torch.float32, device=ids.device)
        check(self.lib.mtts_speaker_embedding(self.ctx, table, ptr(ids), ids.numel(), ptr(out), stream_ptr()))
        return out

    def durations(self, logw, x_mask, scale_correction, length_scale):
        """``scale_correction`` / ``length_scale``: floats, or per-utterance sequences / tensors of B values."""
        logw, x_mask = self._f32(logw), self._f32(x_mask)
        B, _, Tx = logw.shape
        dur = torch.empty(B, Tx, dtype=torch.float32, device=logw.device)
        cum = torch.empty(B, Tx, dtype=torch.int32, device=logw.device)
        yfl = torch.empty(B, dtype=torch.int64, device=logw.device)
        if not (isinstance(scale_correction, (int, float)) and isinstance(length_scale, (int, float))):
            def per_utt(v):
                t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
                t = t.expand(B) if t.numel() == 1 else t
                if t.numel() != B:
                    raise ValueError("per-utterance scale factors need one value per utterance")
                return t.to(logw.device).contiguous()
            sc, ls = per_utt(scale_correction), per_utt(length_scale)
            check(self.lib.mtts_durations_per_utterance(ptr(logw), ptr(x_mask), ptr(sc), ptr(ls), B, Tx, ptr(dur), ptr(cum),
                                                        ptr(yfl), stream_ptr()))
            return dur, cum, yfl
        check(self.lib.mtts_durations(ptr(logw), ptr(x_mask), float(scale_correction), float(length_scale), B, Tx, ptr(dur),
                                      ptr(cum), ptr(yfl), stream_ptr()))
        return dur, cum, yfl

    def durations_given(self, given, x_mask, length_scale=1.0, given_rows=None, out=None):
        """Durations the caller brings (``given`` [B, Tx], fine frames, float or int) instead of the predictor's:
        ``clamp_min(round(given * length_scale), 0) * mask`` and the scan of ``durations`` (mtts_durations_given).  ``given_rows``
        (bool / int [B]) + ``out`` (the ``durations`` tensor of a ``durations`` call): rows not marked keep the predictor's."""
        x_mask = self._f32(x_mask)
        B, _, Tx = x_mask.shape
        given = self._f32(given)
        if given.shape != (B, Tx):
            raise ValueError(f"durations must have shape ({B}, {Tx}), got {tuple(given.shape)}")
        rows = None
        if given_rows is not None:
            if out is None:
                raise ValueError("given_rows needs out= (the predictor's durations of the other rows)")
            rows = torch.as_tensor(given_rows).to(device=given.device, dtype=torch.int32).contiguous()
            if rows.shape != (B,):
                raise ValueError("given_rows needs one flag per utterance")
        dur = torch.empty(B, Tx, dtype=torch.float32, device=given.device) if out is None else out
        cum = torch.empty(B, Tx, dtype=torch.int32, device=given.device)
        yfl = torch.empty(B, dtype=torch.int64, device=given.device)
        ls, ls_b = 1.0, None
        if isinstance(length_scale, (int, float)):
            ls = float(length_scale)
        else:
            ls_b = torch.as_tensor(length_scale, dtype=torch.float32).reshape(-1)
            ls_b = (ls_b.expand(B) if ls_b.numel() == 1 else ls_b).to(given.device).contiguous()
            if ls_b.numel() != B:
                raise ValueError("per-utterance scale factors need one value per utterance")
        check(self.lib.mtts_durations_given(ptr(given), ptr(x_mask), ls, ptr(ls_b), ptr(rows), B, Tx, ptr(dur), ptr(cum), ptr(yfl),
                                            stream_ptr()))
        return dur, cum, yfl

    def durations_shaped(self, logw, x_mask, scale_correction=1.0, length_scale=1.0, given=None, given_rows=None, token_scale=None,
                         token_extend=None):
        """Durations shaped per token in one launch (mtts_durations_shaped; include/mtts.h has the arithmetic): ``token_scale``
        [B, Tx] multiplies a token's duration (a rate; exactly 0 drops the token) and ``token_extend`` [B, Tx] adds fine frames to it,
        on predicted rows and on the rows of ``given`` [B, Tx] that ``given_rows`` [B] marks (None: all of them) alike.
        ``scale_correction`` / ``length_scale``: floats or one per utterance.  Host values outside [0, 16] / [-4096, 4096] raise
        ``ValueError`` before anything is launched (``timing.check_shaping``); the kernel clamps what only the device knows."""
        x_mask = self._f32(x_mask)
        B, _, Tx = x_mask.shape
        dev = x_mask.device

        def per_utt(v):
            t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
            t = t.expand(B) if t.numel() == 1 else t
            if t.numel() != B:
                raise ValueError("per-utterance scale factors need one value per utterance")
            return t.to(dev).contiguous()

        def per_token(v, name):
            if v is None:
                return None
            from .timing import check_shaping
            check_shaping(v, name)
            v = self._f32(torch.as_tensor(v).to(dev))
            if v.shape != (B, Tx):
                raise ValueError(f"{name} must have shape ({B}, {Tx}), got {tuple(v.shape)}")
            return v
        s, a = per_token(token_scale, "token_scale"), per_token(token_extend, "token_extend")
        rows = None
        if given is not None:
            given = self._f32(given)
            if given.shape != (B, Tx):
                raise ValueError(f"durations must have shape ({B}, {Tx}), got {tuple(given.shape)}")
            if given_rows is not None:
                rows = torch.as_tensor(given_rows).to(device=dev, dtype=torch.int32).contiguous()
                if rows.shape != (B,):
                    raise ValueError("given_rows needs one flag per utterance")
        elif given_rows is not None:
            raise ValueError("given_rows needs given=")
        logw = None if logw is None else self._f32(logw)
        sc, ls = per_utt(scale_correction), per_utt(length_scale)
        dur = torch.empty(B, Tx, dtype=torch.float32, device=dev)
        cum = torch.empty(B, Tx, dtype=torch.int32, device=dev)
        yfl = torch.empty(B, dtype=torch.int64, device=dev)
        check(self.lib.mtts_durations_shaped(ptr(logw), ptr(x_mask), ptr(sc), ptr(ls), ptr(given), ptr(rows), ptr(s), ptr(a), B, Tx,
                                             ptr(dur), ptr(cum), ptr(yfl), stream_ptr()))
        return dur, cum, yfl

    def mas_logprior(self, mu_x, y, x_lengths, y_lengths):
        """Diagonal-Gaussian log-prior [B, Tx, Tm] of every (token, frame) pair in fp32 (mtts_mas_logprior)."""
        mu_x, y = self._f32(mu_x), self._f32(y)
        B, F, Tx = mu_x.shape
        Tm = y.shape[2]
        if y.shape[:2] != (B, F):
            raise ValueError(f"y must be [{B}, {F}, Tm], got {tuple(y.shape)}")
        xl = x_lengths.detach().to(device=mu_x.device, dtype=torch.int64).contiguous()
        yl = y_lengths.detach().to(device=mu_x.device, dtype=torch.int64).contiguous()
        lp = torch.empty(B, Tx, Tm, dtype=torch.float32, device=mu_x.device)
        check(self.lib.mtts_mas_logprior(ptr(mu_x), ptr(y), ptr(xl), ptr(yl), B, F, Tx, Tm, ptr(lp), stream_ptr()))
        return lp

    def mas(self, x_lengths, y_lengths, lp=None, mu_x=None, y=None, return_path=False, check_lengths=True):
        """Monotonic Alignment Search (mtts_mas) on a given log-prior ``lp`` [B, Tx, Tm], or on ``mu_x`` [B, F, Tx] and ``y``
        [B, F, Tm] through the log-prior kernel.  Returns ``(durations int32 [B, Tx], score [B], path [B, Tx, Tm] or None)``.
        ``check_lengths``: read the device's verdict on the lengths (one synchronisation) and raise ``ValueError``; pass False
        inside a HIP graph capture and call ``mas_status`` after the replay."""
        if lp is not None:
            lp = self._f32(lp)
            B, Tx, Tm = lp.shape
            F, dev = 0, lp.device
        else:
            mu_x, y = self._f32(mu_x), self._f32(y)
            B, F, Tx = mu_x.shape
            Tm, dev = y.shape[2], mu_x.device
            if y.shape[:2] != (B, F):
                raise ValueError(f"y must be [{B}, {F}, Tm], got {tuple(y.shape)}")
        xl = x_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        yl = y_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        if xl.shape != (B,) or yl.shape != (B,):
            raise ValueError("x_lengths and y_lengths need one entry per utterance")
        ws = self._ws.get("mas", self.lib.mtts_mas_workspace_bytes(B, Tx, Tm), dev)
        dur = torch.empty(B, Tx, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)
        path = torch.empty(B, Tx, Tm, dtype=torch.float32, device=dev) if return_path else None
        check(self.lib.mtts_mas(ptr(lp), ptr(mu_x), ptr(y), ptr(xl), ptr(yl), B, F, Tx, Tm, ptr(dur), ptr(path), ptr(score),
                                ws.data_ptr(), ws.numel(), stream_ptr()))
        if check_lengths:
            self.mas_status()
        return dur, score, path

    def mas_status(self) -> None:
        """Wait for this stream's latest ``mas`` call and raise ``ValueError`` naming the first utterance whose lengths the
        device refused (mtts_mas_status)."""
        self._status("mas", self.lib.mtts_mas_status)

    def align_pool(self, mu_x, cum, y_fine_lengths, t_pad: int):
        mu_x = self._f32(mu_x)
        B, nf, Tx = mu_x.shape
        mu_y = torch.empty(B, nf, t_pad, dtype=torch.float32, device=mu_x.device)
        y_mask = torch.empty(B, 1, t_pad, dtype=torch.float32, device=mu_x.device)
        y_len = torch.empty(B, dtype=torch.int64, device=mu_x.device)
        check(self.lib.mtts_align_pool(ptr(mu_x), ptr(cum), ptr(y_fine_lengths), B, nf, Tx, t_pad, ptr(mu_y), ptr(y_mask),
                                       ptr(y_len), stream_ptr()))
        return mu_y, y_mask, y_len

    def set_frame_limits(self, t_len: Optional[torch.Tensor]) -> None:
        """Per-utterance frame limits (int32 [B] on the device, even) for the following estimator calls; None clears."""
        if t_len is not None:
            if t_len.dtype != torch.int32 or not t_len.is_cuda or not t_len.is_contiguous():
                raise RuntimeError("mtts: frame limits must be a contiguous int32 tensor on the HIP device")
        self._t_len = t_len                     # keep it alive: the library stores the pointer
        check(self.lib.mtts_set_frame_limits(self.ctx, None if t_len is None else t_len.data_ptr()))

    def decoder_forward(self, x, mask, mu, t: float):
        x, mask, mu = self._f32(x), self._f32(mask), self._f32(mu)
        B, nf, T = x.shape
        out = torch.empty_like(x)
        ws = self._workspace("dec", B, T)
        check(self.lib.mtts_decoder_forward(self.ctx, ptr(x), ptr(mask), ptr(mu), float(t), B, T, ptr(out), ws.data_ptr(),
                                            ws.numel(), stream_ptr()))
        return out

    def decoder_forward_rows(self, x, mask, mu, t):
        """``Decoder.forward`` with one time per utterance: ``t`` fp32 [B] (a device tensor, or a host sequence that is copied
        over) -- mtts_decoder_forward_rows."""
        x, mask, mu = self._f32(x), self._f32(mask), self._f32(mu)
        B, nf, T = x.shape
        t = torch.as_tensor(t, dtype=torch.float32).detach().to(device=x.device).reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError(f"t needs one time per utterance ({B}), got {t.numel()}")
        out = torch.empty_like(x)
        ws = self._workspace("dec", B, T)
        check(self.lib.mtts_decoder_forward_rows(self.ctx, ptr(x), ptr(mask), ptr(mu), ptr(t), B, T, ptr(out), ws.data_ptr(),
                                                 ws.numel(), stream_ptr()))
        return out

    def cfm_loss(self, x1, mu, mask, noise, t, add_mu: bool, sigma_min: float, return_pred: bool = False):
        """The flow-matching loss's per-utterance sums ``sq_sum`` [B] (mtts_cfm_loss): target rows, one estimator evaluation at
        ``t`` [B], masked squared error against ``u``.  Returns ``(sq_sum, pred or None)``."""
        x1, mu, mask, noise = self._f32(x1), self._f32(mu), self._f32(mask), self._f32(noise)
        B, nf, T = x1.shape
        if mu.shape != x1.shape or noise.shape != x1.shape or mask.shape != (B, 1, T):
            raise ValueError("cfm_loss: x1, mu, noise must be [B, n_feats, T] and mask [B, 1, T]")
        t = torch.as_tensor(t, dtype=torch.float32).detach().to(device=x1.device).reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError(f"t needs one time per utterance ({B}), got {t.numel()}")
        sq = torch.empty(B, dtype=torch.float32, device=x1.device)
        pred = torch.empty_like(x1) if return_pred else None
        ws = self._workspace("dec", B, T)
        check(self.lib.mtts_cfm_loss(self.ctx, ptr(x1), ptr(mu), ptr(mask), ptr(noise), ptr(t), int(bool(add_mu)), float(sigma_min),
                                     B, T, ptr(sq), ptr(pred), ws.data_ptr(), ws.numel(), stream_ptr()))
        return sq, pred

    def score_prior_dur(self, mu_x, logw, durations, y_fine, x_lengths, y_fine_lengths, delta_prior: float, delta_dur: float,
                        return_frames: bool = False, check_lengths: bool = True):
        """Prior and duration Huber sums per utterance (mtts_score_prior_dur).  Returns ``(prior_sum [B], dur_sum [B], prior_frame
        [B, Tm] or None, dur_err [B, Tx] or None)``.  ``check_lengths``: read the device's verdict (one synchronisation) and raise
        ``ValueError``; otherwise call ``score_status`` later."""
        mu_x, logw, y_fine = self._f32(mu_x), self._f32(logw), self._f32(y_fine)
        B, F, Tx = mu_x.shape
        Tm, dev = y_fine.shape[2], mu_x.device
        if y_fine.shape[:2] != (B, F) or logw.numel() != B * Tx:
            raise ValueError(f"score_prior_dur: y_fine must be [{B}, {F}, Tm] and logw [{B}, 1, {Tx}]")
        durations = durations.detach().to(device=dev, dtype=torch.int32).contiguous()
        if durations.shape != (B, Tx):
            raise ValueError(f"durations must have shape ({B}, {Tx}), got {tuple(durations.shape)}")
        xl = x_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        yl = y_fine_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        if xl.shape != (B,) or yl.shape != (B,):
            raise ValueError("x_lengths and y_fine_lengths need one entry per utterance")
        ws = self._ws.get("score", self.lib.mtts_score_workspace_bytes(B, Tx, Tm), dev)
        prior = torch.empty(B, dtype=torch.float32, device=dev)
        dur = torch.empty(B, dtype=torch.float32, device=dev)
        frame = torch.empty(B, Tm, dtype=torch.float32, device=dev) if return_frames else None
        err = torch.empty(B, Tx, dtype=torch.float32, device=dev) if return_frames else None
        check(self.lib.mtts_score_prior_dur(ptr(mu_x), ptr(logw), ptr(durations), ptr(y_fine), ptr(xl), ptr(yl), B, F, Tx, Tm,
                                            float(delta_prior), float(delta_dur), ptr(prior), ptr(dur), ptr(frame), ptr(err),
                                            ws.data_ptr(), ws.numel(), stream_ptr()))
        if check_lengths:
            self.score_status()
        return prior, dur, frame, err

    def score_status(self) -> None:
        """Wait for this stream's latest ``score_prior_dur`` call and raise ``ValueError`` naming the first utterance the device
        refused (mtts_score_status)."""
        self._status("score", self.lib.mtts_score_status)

    def speaker_grad(self, x, x_lengths, e_enc, e_dur, y_fine, y_fine_lengths, delta_prior: float, delta_dur: float, durations=None,
                     check_lengths: bool = True, return_tape: bool = False):
        """Gradients of the per-utterance prior and duration Huber sums with respect to the speaker rows (mtts_spk_grad): a taped
        text-encoder forward, MAS (``durations`` None) or the given int32 ``durations`` [B, Tx], the two sums and the backward walk.
        Returns a dict: ``g_enc``, ``g_dur`` [B, spk_emb_dim], ``prior_sum``, ``dur_sum`` [B], ``durations`` int32 [B, Tx] and, with
        ``return_tape``, views ``mu_x``, ``logw``, ``x_mask`` of this call's workspace (valid until the next call on this stream).
        The backward panels are packed and uploaded on first use per weight generation.  ``check_lengths`` as ``score_prior_dur``."""
        B, Tx = x.shape
        dev = x.device
        x = x.detach().to(torch.int64).contiguous()
        xl = x_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        e_enc, e_dur = self._f32(e_enc), self._f32(e_dur)
        if e_enc.shape[0] != B:
            e_enc, e_dur = e_enc.expand(B, -1).contiguous(), e_dur.expand(B, -1).contiguous()
        y_fine = self._f32(y_fine)
        F, Tm, Sd = self.hp.n_feats, y_fine.shape[2], self.hp.spk_emb_dim
        if y_fine.shape[:2] != (B, F):
            raise ValueError(f"speaker_grad: y_fine must be [{B}, {F}, Tm], got {tuple(y_fine.shape)}")
        yl = y_fine_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        if xl.shape != (B,) or yl.shape != (B,):
            raise ValueError("x_lengths and y_fine_lengths need one entry per utterance")
        if e_enc.shape != (B, Sd) or e_dur.shape != (B, Sd):
            raise ValueError(f"speaker rows must be [{B}, {Sd}]")
        dur_in = None
        if durations is not None:
            dur_in = durations.detach().to(device=dev, dtype=torch.int32).contiguous()
            if dur_in.shape != (B, Tx):
                raise ValueError(f"durations must have shape ({B}, {Tx}), got {tuple(dur_in.shape)}")
        self._grad_panels()
        ws = self._ws.get("spk_grad", self.lib.mtts_spk_grad_workspace_bytes(self.ctx, B, Tx, Tm), self.device)
        g_enc = torch.empty(B, Sd, dtype=torch.float32, device=dev)
        g_dur = torch.empty(B, Sd, dtype=torch.float32, device=dev)
        prior = torch.empty(B, dtype=torch.float32, device=dev)
        dsum = torch.empty(B, dtype=torch.float32, device=dev)
        dur_out = torch.empty(B, Tx, dtype=torch.int32, device=dev)
        check(self.lib.mtts_spk_grad(self.ctx, ptr(x), ptr(xl), ptr(e_enc), ptr(e_dur), ptr(y_fine), ptr(yl), ptr(dur_in), float(delta_prior),
                                     float(delta_dur), B, Tx, Tm, ptr(g_enc), ptr(g_dur), ptr(prior), ptr(dsum), ptr(dur_out),
                                     self._grad_weights.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()))
        if check_lengths:
            self.spk_grad_status()
        out = {"g_enc": g_enc, "g_dur": g_dur, "prior_sum": prior, "dur_sum": dsum, "durations": dur_out}
        if return_tape:
            for which, (name, shape) in enumerate((("mu_x", (B, F, Tx)), ("logw", (B, 1, Tx)), ("x_mask", (B, 1, Tx)))):
                off = size(self.lib.mtts_spk_grad_tape_offset(self.ctx, B, Tx, Tm, which))
                count = B * Tx * (F if which == 0 else 1)
                out[name] = ws[off:off + 4 * count].view(torch.float32).view(shape)
            Hd = self.hp.encoder.n_channels + Sd
            off = size(self.lib.mtts_spk_grad_rows_offset(self.ctx, B, Tx, Tm))
            out["enc_rows"] = ws[off:off + 4 * B * Tx * Hd].view(torch.float32).view(B * Tx, Hd)
        return out

    def spk_grad_status(self) -> None:
        """Wait for this stream's latest ``speaker_grad`` call and raise ``ValueError`` naming the first utterance the device refused
        (mtts_spk_grad_status)."""
        self._status("spk_grad", self.lib.mtts_spk_grad_status)

    def _grad_panels(self) -> torch.Tensor:
        """The backward panels of the speaker-row gradient, packed and uploaded on first use per weight generation."""
        if self._grad_weights is None or self._grad_generation != self.generation:
            nb = size(self.lib.mtts_spk_grad_weights_bytes(self.ctx))
            buf = torch.empty(nb, dtype=torch.uint8, device=self.device)
            check(self.lib.mtts_spk_grad_upload_weights(self.ctx, buf.data_ptr(), nb))
            self._grad_weights, self._grad_generation = buf, self.generation
        return self._grad_weights

    def speaker_grad_match(self, x, x_lengths, e_enc, e_dur, mu_ref, logw_ref, beta_mu: float = 0.002, beta_logw: float = 0.004,
                           check_lengths: bool = True):
        """Style-encoder training's matching loss (mtts_spk_grad_match; reference style_encoder.py:119-143): the text encoder's
        outputs under the PREDICTED rows ``e_enc``, ``e_dur`` [B, spk_emb_dim] against ``mu_ref`` [B, n_feats, Tx] and ``logw_ref``
        [B, 1, Tx] or [B, Tx] (``text_encoder``'s outputs under the real rows), smooth-L1 with the reference's betas.  Returns a dict:
        ``g_enc``, ``g_dur`` [B, spk_emb_dim] = gradients of the per-utterance sums ``ac_sum``, ``rh_sum`` [B].  ``check_lengths``:
        wait for the stream and raise ``ValueError`` naming a refused utterance."""
        B, Tx = x.shape
        dev = x.device
        x = x.detach().to(torch.int64).contiguous()
        xl = x_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        e_enc, e_dur, mu_ref, logw_ref = self._f32(e_enc), self._f32(e_dur), self._f32(mu_ref), self._f32(logw_ref)
        F, Sd = self.hp.n_feats, self.hp.spk_emb_dim
        if xl.shape != (B,):
            raise ValueError("x_lengths needs one entry per utterance")
        if e_enc.shape != (B, Sd) or e_dur.shape != (B, Sd):
            raise ValueError(f"the predicted rows must be [{B}, {Sd}]")
        if mu_ref.shape != (B, F, Tx) or logw_ref.numel() != B * Tx:
            raise ValueError(f"mu_ref must be [{B}, {F}, {Tx}] and logw_ref [{B}, {Tx}]")
        panels = self._grad_panels()
        ws = self._ws.get("spk_grad_match", self.lib.mtts_spk_grad_match_workspace_bytes(self.ctx, B, Tx), self.device)
        out = {k: torch.empty(B, Sd, dtype=torch.float32, device=dev) for k in ("g_enc", "g_dur")}
        out.update({k: torch.empty(B, dtype=torch.float32, device=dev) for k in ("ac_sum", "rh_sum")})
        check(self.lib.mtts_spk_grad_match(self.ctx, ptr(x), ptr(xl), ptr(e_enc), ptr(e_dur), ptr(mu_ref), ptr(logw_ref), float(beta_mu),
                                           float(beta_logw), B, Tx, ptr(out["g_enc"]), ptr(out["g_dur"]), ptr(out["ac_sum"]),
                                           ptr(out["rh_sum"]), panels.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()))
        if check_lengths:
            self._status("spk_grad_match", self.lib.mtts_spk_grad_match_status)
        return out

    # ------------------------------------------------------------------ duration-predictor training (csrc/dp_grad.hip)
    DP_PREFIX = "encoder.proj_w."

    def dp_layout(self):
        """``(key, offset, shape)`` of every duration-predictor parameter inside the flat vector, in state-dict order, keys without
        the ``encoder.proj_w.`` prefix (mtts_dp_param_offset).  Needs no device."""
        e, Sd = self.hp.encoder, self.hp.spk_emb_dim
        F, k, Hd = e.dp_filter_channels, e.dp_kernel_size, e.n_channels + Sd
        shapes = [("spk_proj.weight", (2 * F, Sd)), ("spk_proj.bias", (2 * F,))]
        for i in range(e.dp_n_layers):
            shapes += [(f"conv_layers.{i}.weight", (F, Hd if i == 0 else F, k)), (f"conv_layers.{i}.bias", (F,)),
                       (f"norm_layers.{i}.gamma", (F,)), (f"norm_layers.{i}.beta", (F,))]
        shapes += [("proj.weight", (1, F, 1)), ("proj.bias", (1,))]
        return [(key, size(self.lib.mtts_dp_param_offset(self.ctx, key.encode())), shape) for key, shape in shapes]

    def dp_param_count(self) -> int:
        return size(self.lib.mtts_dp_param_count(self.ctx))

    def dp_params(self):
        """The duration predictor of the loaded weights as ``(flat, layout)``: one flat fp32 host vector of ``dp_param_count()`` floats
        and ``dp_layout()``."""
        if not self._dp_tensors:
            raise RuntimeError("mtts: no weights loaded (load_state_dict)")
        layout = self.dp_layout()
        flat = torch.empty(self.dp_param_count(), dtype=torch.float32)
        for key, off, shape in layout:
            t = self._dp_tensors[self.DP_PREFIX + key]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{self.DP_PREFIX + key} has shape {tuple(t.shape)}, expected {shape}")
            flat[off:off + t.numel()] = t.reshape(-1)
        return flat, layout

    def dp_train_buffer(self, params=None) -> torch.Tensor:
        """Pack the predictor's training component from the flat vector ``params`` (host or device; None: the registered tensors)
        and upload it into this model's training buffer (mtts_dp_train_upload): 2.5 MB at the production size, one host round trip, nothing else is
        repacked.  Returns the device buffer ``dp_grad`` takes."""
        nb = size(self.lib.mtts_dp_train_weights_bytes(self.ctx))
        if self._dp_buf is None or self._dp_buf.numel() != nb or self._dp_buf.device != self.device:
            self._dp_buf = torch.empty(nb, dtype=torch.uint8, device=self.device)
        torch.cuda.current_stream().synchronize()     # an earlier dp_grad on this stream may still read the buffer: the copy waits for nothing
        host = None
        if params is not None:
            host = np.ascontiguousarray(params.detach().to("cpu", torch.float32).numpy().reshape(-1))
            if host.size != self.dp_param_count():
                raise ValueError(f"params must hold {self.dp_param_count()} floats, got {host.size}")
        check(self.lib.mtts_dp_train_upload(self.ctx, None if host is None else host.ctypes.data, self._dp_buf.data_ptr(), nb))
        return self._dp_buf

    def dp_grad(self, x, x_lengths, e_enc, e_dur, durations, delta_dur: float, train_buf: torch.Tensor, check_lengths: bool = True,
                return_tape: bool = False):
        """Gradient of the batch's duration Huber sum with respect to every parameter of the duration predictor packed in
        ``train_buf`` (mtts_dp_grad): frozen encoder forward, predictor forward from ``train_buf`` in native fp32, the walk back and the
        parameter reductions.  Returns a dict: ``grad`` [dp_param_count] (of the SUM over the batch), ``g_dur`` [B, spk_emb_dim],
        ``dur_sum`` [B], ``logw`` [B, 1, Tx] and, with ``return_tape``, ``enc_rows`` [B*Tx, enc_channels + spk_emb_dim], a view of
        this call's workspace.  ``check_lengths``: wait for the stream and raise ``ValueError`` naming a refused utterance."""
        B, Tx = x.shape
        dev = x.device
        x = x.detach().to(torch.int64).contiguous()
        xl = x_lengths.detach().to(device=dev, dtype=torch.int64).contiguous()
        e_enc, e_dur = self._f32(e_enc), self._f32(e_dur)
        if e_enc.shape[0] != B:
            e_enc, e_dur = e_enc.expand(B, -1).contiguous(), e_dur.expand(B, -1).contiguous()
        Sd = self.hp.spk_emb_dim
        if xl.shape != (B,):
            raise ValueError("x_lengths needs one entry per utterance")
        if e_enc.shape != (B, Sd) or e_dur.shape != (B, Sd):
            raise ValueError(f"speaker rows must be [{B}, {Sd}]")
        dur = durations.detach().to(device=dev, dtype=torch.int32).contiguous()
        if dur.shape != (B, Tx):
            raise ValueError(f"durations must have shape ({B}, {Tx}), got {tuple(dur.shape)}")
        ws = self._ws.get("dp_grad", self.lib.mtts_dp_grad_workspace_bytes(self.ctx, B, Tx), self.device)
        grad = torch.empty(self.dp_param_count(), dtype=torch.float32, device=dev)
        g_dur = torch.empty(B, Sd, dtype=torch.float32, device=dev)
        dsum = torch.empty(B, dtype=torch.float32, device=dev)
        logw = torch.empty(B, 1, Tx, dtype=torch.float32, device=dev)
        check(self.lib.mtts_dp_grad(self.ctx, ptr(x), ptr(xl), ptr(e_enc), ptr(e_dur), ptr(dur), float(delta_dur), B, Tx, train_buf.data_ptr(),
                                    ptr(grad), ptr(g_dur), ptr(dsum), ptr(logw), ws.data_ptr(), ws.numel(), stream_ptr()))
        if check_lengths:
            self.dp_grad_status()
        out = {"grad": grad, "g_dur": g_dur, "dur_sum": dsum, "logw": logw}
        if return_tape:
            Hd = self.hp.encoder.n_channels + Sd
            off = size(self.lib.mtts_dp_grad_tape_offset(self.ctx, B, Tx, 0))
            out["enc_rows"] = ws[off:off + 4 * B * Tx * Hd].view(torch.float32).view(B * Tx, Hd)
        return out

    def dp_grad_status(self) -> None:
        """Wait for this stream's latest ``dp_grad`` call and raise ``ValueError`` naming the first utterance the device refused
        (mtts_dp_grad_status)."""
        self._status("dp_grad", self.lib.mtts_dp_grad_status)

    def update_tensors(self, tensors: Dict[str, torch.Tensor]) -> None:
        """Replace some registered tensors (full state-dict keys), then repack and upload the weight image ONCE.  ``generation`` is
        bumped -- captured graphs and the backward panels of ``speaker_grad`` are rebuilt on their next use -- and the image no longer
        counts as read from a packed-image cache."""
        if self.weights is None:
            raise RuntimeError("mtts: no weights loaded (load_state_dict)")
        for k, v in tensors.items():
            self._set(k, v)
            if k.startswith(self.DP_PREFIX):
                self._dp_tensors[k] = v.detach().to("cpu", torch.float32).clone()
        nbytes = size(self.lib.mtts_weights_bytes(self.ctx))
        self.weights = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        check(self.lib.mtts_upload_weights(self.ctx, self.weights.data_ptr(), nbytes))
        self.cache_hit = False
        self.generation += 1
        self._ws.clear()

    def fold_rows(self, y_max: int, align: int) -> int:
        """Rows per utterance the folded estimator needs for valid lengths up to y_max (mtts_fold_rows)."""
        return size(self.lib.mtts_fold_rows(self.ctx, int(y_max), int(align)))

    def cfm_solve(self, x0, mu, mask, t_span, solver: str, add_mu: bool = False, t_out: Optional[int] = None,
                  out_scale: float = 1.0, out_shift: float = 0.0, y_lengths=None, y_max: Optional[int] = None,
                  t_fold: Optional[int] = None, ws: Optional[torch.Tensor] = None):
        """``y_lengths`` (int64 [B] on the device) + ``y_max`` + ``t_fold``: prefix masks on folded padding
        (mtts_cfm_solve_folded; ``mask`` is then not read).  ``ws``: caller-owned scratch (HIP-graph capture: the buffer must
        belong to the graph, not to the per-stream cache)."""
        x0, mu = self._f32(x0), self._f32(mu)
        B, nf, T = x0.shape
        if solver not in SOLVERS:
            raise ValueError(f"unsupported solver {solver!r} (euler, midpoint, rk4)")
        ts = np.ascontiguousarray(torch.as_tensor(t_span).detach().to("cpu", torch.float32).numpy())
        t_out = T if t_out is None else int(t_out)
        out = torch.empty(B, nf, t_out, dtype=torch.float32, device=x0.device)
        if t_fold is not None:
            y_lengths = y_lengths.detach().to(torch.int64).contiguous()
            if ws is None:
                ws = self._workspace("dec", B, int(t_fold))
            else:
                self._ws.note("dec", ws)
            check(self.lib.mtts_cfm_solve_folded(self.ctx, ptr(x0), ptr(mu), ptr(y_lengths), int(y_max), int(bool(add_mu)),
                                                 ts.ctypes.data, len(ts) - 1, SOLVERS[solver], B, T, int(t_fold), ptr(out), t_out,
                                                 float(out_scale), float(out_shift), ws.data_ptr(), ws.numel(), stream_ptr()))
            return out
        mask = self._f32(mask)
        ws = self._workspace("dec", B, T)
        check(self.lib.mtts_cfm_solve(self.ctx, ptr(x0), ptr(mu), ptr(mask), int(bool(add_mu)), ts.ctypes.data, len(ts) - 1,
                                      SOLVERS[solver], B, T, ptr(out), t_out, float(out_scale), float(out_shift),
                                      ws.data_ptr(), ws.numel(), stream_ptr()))
        return out

    def cfm_step(self, z_pool, mu_pool, slots, t0, t1, y_lengths, y_max: int, t_fold: int, solver: str, slots_dev=None,
                 ws: Optional[torch.Tensor] = None) -> None:
        """One solver step of the utterances in ``slots`` (a host sequence of distinct slot indices), each over its own grid
        interval, in place on ``z_pool`` (mtts_cfm_step).  ``z_pool`` / ``mu_pool``: fp32 [S, n_feats, T_cap] on the device.
        ``t0`` / ``t1``: fp32 [B] and ``y_lengths``: int64 [B] on the device, in the order of ``slots``; host sequences are copied
        over.  ``slots_dev``: the int32 [B] device copy of ``slots`` when the caller already has one.  Frame limits
        (``set_frame_limits``) compose as for ``cfm_solve``."""
        if solver not in SOLVERS:
            raise ValueError(f"unsupported solver {solver!r} (euler, midpoint, rk4)")
        for name, pool in (("z_pool", z_pool), ("mu_pool", mu_pool)):
            if pool.dtype != torch.float32 or pool.dim() != 3 or not pool.is_cuda or not pool.is_contiguous():
                raise RuntimeError(f"mtts: {name} must be a contiguous fp32 [S, n_feats, T_cap] tensor on the HIP device")
        if z_pool.shape != mu_pool.shape or z_pool.shape[1] != self.hp.n_feats:
            raise RuntimeError("mtts: z_pool and mu_pool must both be [S, n_feats, T_cap]")
        S, _, T_cap = z_pool.shape
        h_slots = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        B = int(h_slots.shape[0])
        dev = z_pool.device
        if slots_dev is None:
            slots_dev = torch.from_numpy(h_slots).to(dev)

        def on_device(v, dtype):
            v = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v), dtype=dtype)
            v = v.detach().to(device=dev, dtype=dtype).contiguous()
            if v.numel() != B:
                raise ValueError(f"mtts: a step of {B} slots needs {B} values per argument, got {v.numel()}")
            return v
        t0, t1, y_lengths = on_device(t0, torch.float32), on_device(t1, torch.float32), on_device(y_lengths, torch.int64)
        if slots_dev.dtype != torch.int32 or slots_dev.numel() != B:
            raise RuntimeError("mtts: slots_dev must be an int32 tensor with one entry per slot")
        if ws is None:
            ws = self._workspace("dec", B, int(t_fold))
        else:
            self._ws.note("dec", ws)
        check(self.lib.mtts_cfm_step(self.ctx, ptr(z_pool), ptr(mu_pool), S, T_cap, ptr(slots_dev), h_slots.ctypes.data, ptr(t0), ptr(t1),
                                     ptr(y_lengths), int(y_max), SOLVERS[solver], B, int(t_fold), ws.data_ptr(), ws.numel(), stream_ptr()))

    # ------------------------------------------------------------------ measurement
    def gemm_terms(self) -> int:
        return self.lib.mtts_gemm_terms(self.ctx)

    def prof_enable(self, on: bool) -> None:
        check(self.lib.mtts_prof_enable(self.ctx, int(on)))

    def prof_reset(self) -> None:
        check(self.lib.mtts_prof_reset(self.ctx))

    def prof_read(self, klass: int):
        n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        check(self.lib.mtts_prof_read(self.ctx, klass, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return n.value, ms.value, fl.value, by.value


    def prof_records(self, max_records: int = 1 << 16):
        """[(class, ms, flops, bytes)] per launch of the event pass, in launch order."""
        buf = (C.c_double * (4 * max_records))()
        n = size(self.lib.mtts_prof_records(self.ctx, buf, max_records))
        return [(int(buf[4 * i]), buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]) for i in range(n)]

    def prof_tags(self, max_bytes: int = 1 << 24):
        """Kernel instantiation name of each record of ``prof_records`` ("-" where the launcher does not tag)."""
        buf = C.create_string_buffer(max_bytes)
        n = size(self.lib.mtts_prof_tags(self.ctx, buf, max_bytes))
        return buf.value.decode().split("\n")[:n]


# ---------------------------------------------------------------------- host-only plans
def tblock_plan(width: int, inner: int, n_qkv: int, M: int, count: int = 1, *, chain_on: int = 1, chain_ch: int = 256, chain_qb: int = 0,
                chain_pf: int = 16, chain_min_rows: int = 5761, pair_on: int = 1, pair_min_rows: int = 3000):
    """The estimator's launch form of a transformer block's row-local part at the row counts M .. M + count - 1 (mtts_tblock_plan; the
    keyword defaults are those of csrc/model.h ``Switches``; the environment is not read).  Returns ``(ch, form, qb, grid, prefetch)``:
    the packed hidden chunk and four int32 arrays of ``count`` -- form 0 tiled launches, 1 chain launch, 2 its pair form."""
    lib = load()
    out = [np.zeros(count, dtype=np.int32) for _ in range(4)]
    ch = C.c_int(0)
    ip = C.POINTER(C.c_int)
    check(lib.mtts_tblock_plan(width, inner, n_qkv, M, count, chain_on, chain_ch, chain_qb, chain_pf, chain_min_rows, pair_on, pair_min_rows,
                               C.byref(ch), *[a.ctypes.data_as(ip) for a in out]))
    return (ch.value, *out)


# ---------------------------------------------------------------------- single kernels (used by the parity tests)
def gemm_f32(a, w, bias=None, *, B, T_in, T_out=None, tap_off=None, in_stride=1, a_mask=None, a_mean=None, a_rstd=None,
             a_part=None, act=0, p0=None, p1=None, res=None, out_mask=None, out_scale=1.0, stats_out=False, terms=-1):
    """a [B*T_in, C]; w Linear [N, C] or Conv1d [N, C, k]."""
    lib = load()
    N, Cc = w.shape[0], w.shape[1]
    ntaps = w.shape[2] if w.dim() == 3 else 1
    T_out = T_in if T_out is None else T_out
    taps = (C.c_int * ntaps)(*(tap_off if tap_off is not None else [j - ntaps // 2 for j in range(ntaps)]))
    packed = torch.empty(lib.mtts_gemm_packed_bytes(N, Cc, ntaps), dtype=torch.uint8, device=a.device)
    out = torch.empty(B * T_out, N, dtype=torch.float32, device=a.device)
    stats = torch.empty(B * T_out, N // 64, 2, dtype=torch.float32, device=a.device) if stats_out else None
    check(lib.mtts_gemm_f32(ptr(a), a.shape[1], B, T_in, Cc, ntaps, taps, in_stride, T_out, ptr(a_mask), ptr(a_mean), ptr(a_rstd),
                            ptr(a_part), a_part.shape[1] if a_part is not None else 0,
                            ptr(w.contiguous()), packed.data_ptr(), ptr(bias), N, act, ptr(p0), ptr(p1), ptr(res),
                            res.shape[1] if res is not None else 0, ptr(out_mask), float(out_scale), ptr(out), N, ptr(stats), terms,
                            stream_ptr()))
    return (out, stats) if stats_out else out


def gemm_p16(a, w, bias=None, *, B, T_in, T_out=None, tap_off=None, in_stride=1, a_mask=None, a_mean=None, a_rstd=None,
             a_part=None, act=0, p0=None, p1=None, res=None, out_mask=None, out_scale=1.0, stats_out=False, want_f32=True,
             want_p16=False, lscale=2048.0, force_bm=0):
    """P16-operand GEMM (csrc/gemm_p16.hip); a [B*T_in, C] fp32 is converted to its P16 image first.  Returns a dict."""
    lib = load()
    N, Cc = w.shape[0], w.shape[1]
    ntaps = w.shape[2] if w.dim() == 3 else 1
    T_out = T_in if T_out is None else T_out
    taps = (C.c_int * ntaps)(*(tap_off if tap_off is not None else [j - ntaps // 2 for j in range(ntaps)]))
    packed = torch.empty(lib.mtts_gemm_packed_bytes(N, Cc, ntaps), dtype=torch.uint8, device=a.device)
    scratch = torch.empty(lib.mtts_gemm_p16_scratch_bytes(B, T_in, Cc, T_out, N), dtype=torch.uint8, device=a.device)
    out = torch.empty(B * T_out, N, dtype=torch.float32, device=a.device) if want_f32 else None
    out16 = torch.empty(B * T_out, N, dtype=torch.float32, device=a.device) if want_p16 else None
    stats = torch.empty(B * T_out, N // 64, 2, dtype=torch.float32, device=a.device) if stats_out else None
    check(lib.mtts_gemm_p16(ptr(a), a.shape[1], B, T_in, Cc, ntaps, taps, in_stride, T_out, ptr(a_mask), ptr(a_mean), ptr(a_rstd),
                            ptr(a_part), a_part.shape[1] if a_part is not None else 0,
                            ptr(w.contiguous()), packed.data_ptr(), ptr(bias), N, act, ptr(p0), ptr(p1), ptr(res),
                            res.shape[1] if res is not None else 0, ptr(out_mask), float(out_scale), ptr(out), N,
                            ptr(out16), float(lscale), ptr(stats), force_bm, scratch.data_ptr(), stream_ptr()))
    return {"out": out, "out16": out16, "stats": stats}


def _conv_gn_call(entry, x, w, bias, gamma, beta, mask, chbias, B, T, c1, nrows, nextra, bias_stats, eps, pads=None):
    """What the conv_gn helpers share: shapes, the packed-weight buffer, output and scratch, and the call.  ``pads`` None: the positional
    ``entry`` (returns out); else dict(pad_x, pad_out, sentinel): the argument block (returns the block helper's dict)."""
    lib = load()
    N, Cc = w.shape[0], w.shape[1]
    dev = x.device
    wc = w.contiguous()
    packed = torch.empty(lib.mtts_gemm_packed_bytes(N, Cc, 3), dtype=torch.uint8, device=dev)
    out = torch.empty(B * T, N, dtype=torch.float32, device=dev)
    if pads is None:
        scratch = torch.empty(lib.mtts_conv_gn_scratch_bytes(B, T, Cc, N), dtype=torch.uint8, device=dev)
        stride = [chbias.shape[1]] if entry == "mtts_conv_gn_rows" else []
        check(getattr(lib, entry)(ptr(x), B, T, Cc, c1, ptr(wc), packed.data_ptr(), ptr(bias), N, ptr(gamma), ptr(beta), ptr(mask), ptr(chbias),
                                  *stride, ptr(nrows), ptr(nextra), ptr(bias_stats), float(eps), ptr(out), scratch.data_ptr(), stream_ptr()))
        return out
    g = MttsConvGnArgs()
    g.d_x, g.B, g.T, g.C, g.c1, g.N, g.eps = ptr(x), B, T, Cc, c1, N, float(eps)
    g.d_w, g.d_wpacked, g.d_bias, g.d_gamma, g.d_beta, g.d_mask = ptr(wc), packed.data_ptr(), ptr(bias), ptr(gamma), ptr(beta), ptr(mask)
    g.d_chbias, g.chbias_stride = ptr(chbias), (chbias.shape[1] if chbias is not None and chbias.dim() == 2 else 0)
    g.d_nrows, g.d_nextra, g.d_bias_stats = ptr(nrows), ptr(nextra), ptr(bias_stats)
    g.pad_x, g.pad_out, g.sentinel = pads["pad_x"], pads["pad_out"], pads["sentinel"]
    scratch = torch.empty(size(lib.mtts_conv_gn_args_scratch_bytes(C.byref(g))), dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    img = torch.empty(B * T + ENTRY_GUARD_ROWS, 2 * N + pads["pad_out"], dtype=torch.int16, device=dev)
    g.d_range_flag, g.d_out, g.d_out_image = ptr(flag), ptr(out), ptr(img)
    check(lib.mtts_conv_gn_args_run(C.byref(g), scratch.data_ptr(), stream_ptr()))
    torch.cuda.synchronize()
    return {"out": out, "image": img, "flag": flag, "tag": g.tag.decode()}


def conv_gn(x, w, bias, gamma, beta, mask, *, B, T, c1=0, chbias=None, nrows=None, nextra=None, bias_stats=None, eps=1e-5):
    """One-launch Block1D (csrc/resnet_conv.hip): x [B*T, C] fp32, w Conv1d [N, C, 3]; returns Mish(GroupNorm8(conv(x))) * mask
    (+ chbias, * mask) as fp32 [B*T, N], decoded from the P16 image the kernel writes."""
    return _conv_gn_call("mtts_conv_gn", x, w, bias, gamma, beta, mask, chbias, B, T, c1, nrows, nextra, bias_stats, eps)


def conv_gn_rows(x, w, bias, gamma, beta, mask, chbias, *, B, T, c1=0, nrows=None, nextra=None, bias_stats=None, eps=1e-5):
    """``conv_gn`` with one time-embedding bias row per utterance: chbias [B, stride >= N] (mtts_conv_gn_rows)."""
    return _conv_gn_call("mtts_conv_gn_rows", x, w, bias, gamma, beta, mask, chbias, B, T, c1, nrows, nextra, bias_stats, eps)


def conv_gn_args(x, w, bias, gamma, beta, mask, *, B, T, c1=0, chbias=None, nrows=None, nextra=None, bias_stats=None, eps=1e-5,
                 pad_x=0, pad_out=0, sentinel=0x7e00):
    """The one-launch Block1D on its argument block (include/mtts.h mtts_conv_gn_args): ``conv_gn`` / ``conv_gn_rows`` (chbias [N] or
    [B, stride >= N]) with the range flag, padded image rows and the raw output image.  Returns a dict: out (decoded fp32 [B*T, N]),
    image [B*T + guard, 2 N + pad_out] (int16 bits), flag (device uint32 [1], zeroed before the launch) and tag."""
    return _conv_gn_call(None, x, w, bias, gamma, beta, mask, chbias, B, T, c1, nrows, nextra, bias_stats, eps,
                         pads=dict(pad_x=pad_x, pad_out=pad_out, sentinel=sentinel))


def _host(t):
    """Host fp32 array of a tensor (or None) and the pointer ctypes passes for it."""
    if t is None:
        return None, None
    a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
    return a, a.ctypes.data


CHAIN_PANELS = ("h_w_out", "h_b_out", "h_w1", "h_b1", "h_p0", "h_p1", "h_w2", "h_b2", "h_w_qkv", "h_b_qkv")


def _chain_operands(att, x, panels):
    """What the chain helpers share: shapes, the host copies of the ten panels / vectors (``CHAIN_PANELS`` order) and the outputs."""
    M, Cc = x.shape
    inner = att.shape[1] if att is not None else 0
    n_qkv = panels[8].shape[0] if panels[8] is not None else 0
    keep = [_host(t) for t in panels]
    x_out = torch.empty(M, Cc, dtype=torch.float32, device=x.device)
    qkv = torch.empty(M, n_qkv, dtype=torch.float32, device=x.device) if n_qkv else None
    return M, Cc, inner, n_qkv, keep, x_out, qkv


def _chain_call(run, scratch_bytes, what, att, x, panels, out_mask, mid, ch, repeat):
    """A positional ``*_timed`` chain entry: ``mid`` are its arguments between d_out_mask and d_x_out.  Returns (x_out, qkv or None[, ms
    per launch when ``repeat``])."""
    M, Cc, inner, n_qkv, keep, x_out, qkv = _chain_operands(att, x, panels)
    n = scratch_bytes(M, Cc, inner, n_qkv, ch)
    if n < 0:
        raise RuntimeError(what + ": unsupported shape")
    scratch = torch.empty(n, dtype=torch.uint8, device=x.device)
    ms = C.c_float(0.0)
    check(run(ptr(att), ptr(x), M, Cc, inner, *[k[1] for k in keep], n_qkv, ptr(out_mask), *mid, ptr(x_out), ptr(qkv), scratch.data_ptr(),
              stream_ptr(), repeat, C.byref(ms)))
    torch.cuda.synchronize()
    if repeat:
        return x_out, qkv, ms.value
    return x_out, qkv


def tblock_chain(att, x, w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv=None, b_qkv=None, out_mask=None, qb=64, ch=128, repeat=0, pair=False):
    """Row-local chain of a transformer block (csrc/tblock_chain.hip, include/mtts.h mtts_tblock_chain).  att [M, inner] (or None:
    FeedForward only), x [M, C] on the device; panels / vectors anywhere (copied to the host).  Returns (x_out, qkv or None)."""
    lib = load()
    return _chain_call(lib.mtts_tblock_chain_pair_timed if pair else lib.mtts_tblock_chain_timed, lib.mtts_tblock_chain_scratch_bytes,
                       "mtts_tblock_chain", att, x, (w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv, b_qkv), out_mask, (qb, ch), ch, repeat)


def tblock_chain_h16(att, x, w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv=None, b_qkv=None, out_mask=None, bf16=False, qb=64, ch=128,
                     pf_wgs=0, repeat=0):
    """The same chain in the 16-bit storage modes' arithmetic (csrc/tblock_chain_h16.hip, include/mtts.h mtts_tblock_chain_h16): the
    fp32 operands are rounded to fp16 (or bfloat16) images, the kernel's 16-bit outputs come back widened to fp32.  Returns
    (x_out, qkv or None[, ms per launch when ``repeat``])."""
    lib = load()
    return _chain_call(lib.mtts_tblock_chain_h16_timed, lib.mtts_tblock_chain_h16_scratch_bytes, "mtts_tblock_chain_h16", att, x,
                       (w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv, b_qkv), out_mask, (int(bool(bf16)), qb, ch, pf_wgs), ch, repeat)


def tblock_chain_args(att, x, w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv=None, b_qkv=None, out_mask=None, qb=64, ch=128, pair=False,
                      pad_att=0, pad_x=0, pad_out=0, pad_qkv=0, sentinel=0x7e00):
    """The chain on its argument block (include/mtts.h mtts_chain_args): ``tblock_chain`` with the range flag, padded image rows and
    the raw output images.  Returns a dict: x_out, qkv (decoded fp32), x_out_image [M + guard, 2 C + pad_out] and qkv_image
    [M + guard, 2 n_qkv + pad_qkv] (int16 bits, sentinel wherever the kernel did not write), flag (device uint32 [2], zeroed before
    the launch: range word, pair-timeout word) and tag."""
    lib = load()
    M, Cc, inner, n_qkv, keep, x_out, qkv = _chain_operands(att, x, (w_out, b_out, w1, b1, p0, p1, w2, b2, w_qkv, b_qkv))
    g = MttsChainArgs()
    g.d_att, g.d_x, g.M, g.C, g.inner, g.n_qkv = ptr(att), ptr(x), M, Cc, inner, n_qkv
    for name, k in zip(CHAIN_PANELS, keep):
        setattr(g, name, k[1])
    g.d_out_mask, g.qb, g.ch, g.pair = ptr(out_mask), qb, ch, int(bool(pair))
    g.pad_att, g.pad_x, g.pad_out, g.pad_qkv, g.sentinel = pad_att, pad_x, pad_out, pad_qkv, sentinel
    dev = x.device
    scratch = torch.empty(size(lib.mtts_tblock_chain_args_scratch_bytes(C.byref(g))), dtype=torch.uint8, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    x_img = torch.empty(M + ENTRY_GUARD_ROWS, 2 * Cc + pad_out, dtype=torch.int16, device=dev)
    q_img = torch.empty(M + ENTRY_GUARD_ROWS, 2 * n_qkv + pad_qkv, dtype=torch.int16, device=dev) if n_qkv else None
    g.d_range_flag, g.d_x_out, g.d_qkv_out, g.d_x_out_image, g.d_qkv_image = ptr(flag), ptr(x_out), ptr(qkv), ptr(x_img), ptr(q_img)
    check(lib.mtts_tblock_chain_args_run(C.byref(g), scratch.data_ptr(), stream_ptr()))
    torch.cuda.synchronize()
    return {"x_out": x_out, "qkv": qkv, "x_out_image": x_img, "qkv_image": q_img, "flag": flag, "tag": g.tag.decode()}


def last_kernel_tag() -> str:
    """The kernel instantiation the last launcher call on this thread chose (include/mtts.h mtts_last_kernel_tag)."""
    return load().mtts_last_kernel_tag().decode()


def panel_h16_host(panel, bf16=False):
    """Host only: an fp32 array as the 16-bit weight plane of the storage modes (uint16 bits, same shape)."""
    lib = load()
    a = np.ascontiguousarray(panel, dtype=np.float32)
    out = np.empty(a.shape, dtype=np.uint16)
    check(lib.mtts_panel_h16_host(a.ctypes.data, a.size, int(bool(bf16)), out.ctypes.data))
    return out


def _flag(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def to_h16_roundtrip(x, mask=None, *, C_valid=None, ld16=None, bf16=False, Cc=None):
    """fp32 rows -> H16 image -> fp32 rows (include/mtts.h mtts_to_h16_roundtrip).  Returns a dict: ``out`` [M, C] fp32, ``bits``
    [M, ld16] int16 (the image as stored; columns beyond C are untouched 0x7e7e fill), ``flag`` (the range-flag word)."""
    lib = load()
    M = x.shape[0]
    Cc = x.shape[1] if Cc is None else Cc
    C_valid = Cc if C_valid is None else C_valid
    ld16 = Cc if ld16 is None else ld16
    image = torch.full((M, ld16), 0x7e7e, dtype=torch.int16, device=x.device)
    out = torch.empty(M, Cc, dtype=torch.float32, device=x.device)
    flag = _flag(x.device)
    check(lib.mtts_to_h16_roundtrip(ptr(x), x.stride(0), ptr(mask), M, Cc, C_valid, ld16, int(bool(bf16)), ptr(image), ptr(out), ptr(flag),
                                    stream_ptr()))
    return {"out": out, "bits": image, "flag": int(flag.item())}


def gemm_h16(a, w, bias=None, *, B, T_in, T_out=None, tap_off=None, in_stride=1, c1=0, a_mask=None, a_mean=None, a_rstd=None, a_part=None,
             act=0, p0=None, p1=None, res=None, res16=None, inplace=None, out_mask=None, out_scale=1.0, out16_mask=None,
             want_f32=True, want_h16=False, out=None, out16=None, out_T=0, out_stride=1, out_off=0, stats_out=False, gn_groups=0,
             gn_nrows=None, gnr=None, force_bm=0, bf16=False, half16=True):
    """H16 GEMM (csrc/gemm_p16.hip MODE 2 / 3; include/mtts.h mtts_gemm_h16).  a [B*T_in, C] fp32 is rounded to its H16 image first; w
    Linear [N, C] or Conv1d [N, C, k] anywhere.  ``res16``: residual rows that travel as an H16 image; ``inplace``: rows [out rows, N]
    that are BOTH the residual image and the output image (the residual-stream update).  ``out`` / ``out16``: buffers of an earlier
    call to write into (strided output rows).  ``gnr``: dict(y, stats, tile_rows, groups, gamma, beta, mask[, nextra, bias_stats,
    eps]) = the Block1D tail.  Returns a dict: out, out16, stats, gn_stats, wave_rows, tag, flag."""
    return _gemm_block(lambda lib, g, scratch: lib.mtts_gemm_h16(C.byref(g), scratch, stream_ptr()), "mtts_gemm_h16_scratch_bytes", a, w, bias,
                       B=B, T_in=T_in, T_out=T_out, tap_off=tap_off, in_stride=in_stride, c1=c1, a_mask=a_mask, a_mean=a_mean, a_rstd=a_rstd,
                       a_part=a_part, act=act, p0=p0, p1=p1, res=res, res16=res16, inplace=inplace, out_mask=out_mask, out_scale=out_scale,
                       out16_mask=out16_mask, want_f32=want_f32, want16=want_h16, out=out, out16=out16, out_T=out_T, out_stride=out_stride,
                       out_off=out_off, stats_out=stats_out, gn_groups=gn_groups, gn_nrows=gn_nrows, gnr=gnr, force_bm=force_bm, bf16=bf16,
                       half16=half16)


def _gemm_fill(a, w, bias, *, B, T_in, T_out, tap_off, in_stride, c1, a_mask, a_mean, a_rstd, a_part, act, p0, p1, res, out_mask, out_scale,
               out16_mask, out_T, out_stride, out_off, force_bm, rows=ptr):
    """The operand, prologue and epilogue fields of an argument block (include/mtts.h mtts_gemm_h16_args) that every GEMM helper fills the
    same way; ``rows``: how a / res become pointers (``rows_ptr``: row-strided views).  Returns the block, what must stay alive while it is
    used, the output rows, N and the range-flag word."""
    N, Cc = w.shape[0], w.shape[1]
    ntaps = w.shape[2] if w.dim() == 3 else 1
    T_out = T_in if T_out is None else T_out
    taps = (C.c_int32 * ntaps)(*(tap_off if tap_off is not None else [j - ntaps // 2 for j in range(ntaps)]))
    hw, hw_ptr = _host(w)
    g = MttsGemmH16Args()
    g.d_a, g.lda, g.C, g.c1, g.d_a_mask = rows(a), a.stride(0), Cc, c1, ptr(a_mask)
    g.B, g.T_in, g.T_out, g.ntaps, g.h_tap_off, g.in_stride = B, T_in, T_out, ntaps, C.cast(taps, C.c_void_p), in_stride
    g.d_a_mean, g.d_a_rstd, g.d_a_part, g.a_nparts = ptr(a_mean), ptr(a_rstd), ptr(a_part), a_part.shape[1] if a_part is not None else 0
    g.h_w, g.d_bias, g.N = hw_ptr, ptr(bias), N
    g.act, g.d_p0, g.d_p1 = act, ptr(p0), ptr(p1)
    g.d_res, g.ldr = rows(res), res.stride(0) if res is not None else 0
    g.d_out_mask, g.out_scale, g.d_out16_mask = ptr(out_mask), float(out_scale), ptr(out16_mask)
    g.out_T, g.out_stride, g.out_off = out_T, out_stride, out_off
    g.force_bm = force_bm
    flag = _flag(a.device)
    g.d_range_flag = ptr(flag)
    return g, (taps, hw), B * (out_T if out_T else T_out), N, flag


def _gemm_block(run, scratch_fn, a, w, bias, *, res16, inplace, want_f32, want16, out, out16, stats_out, gn_groups, gn_nrows, gnr, bf16, half16,
                **operands):
    """What gemm_h16 and gemm_p16_args share: fill the argument block, allocate outputs and scratch, call ``run(lib, block, scratch_ptr)``."""
    lib = load()
    dev = a.device
    g, alive, rows, N, flag = _gemm_fill(a, w, bias, **operands)
    if out is None and want_f32:
        out = torch.empty(rows, N, dtype=torch.float32, device=dev)
    preload = out16 is not None
    if inplace is not None:
        out16, preload = inplace.clone(), True
        g.res16_mode = 2
    elif res16 is not None:
        g.res16_mode, g.d_res16_f32 = 1, ptr(res16)
    if out16 is None and want16:
        out16 = torch.empty(rows, N, dtype=torch.float32, device=dev)
    g.d_out, g.d_out16_f32, g.out16_preload = ptr(out), ptr(out16), int(preload)
    stats = torch.empty(rows, N // 64, 2, dtype=torch.float32, device=dev) if stats_out else None
    g.d_stats_out = ptr(stats)
    gn_stats = None
    if gn_groups:
        gn_stats = torch.zeros(2 * ((operands["B"] * g.T_out + 31) // 32 + 1) * (N // 64) * 2, 4, dtype=torch.float32, device=dev)
        g.d_gn_stats, g.gn_groups, g.d_gn_nrows = ptr(gn_stats), gn_groups, ptr(gn_nrows)
    if gnr is not None:
        g.d_gnr_y, g.d_gnr_stats, g.gnr_tile_rows, g.gnr_groups = ptr(gnr["y"]), ptr(gnr["stats"]), gnr["tile_rows"], gnr["groups"]
        g.d_gnr_gamma, g.d_gnr_beta, g.d_gnr_mask, g.gnr_eps = ptr(gnr["gamma"]), ptr(gnr["beta"]), ptr(gnr["mask"]), float(gnr.get("eps", 1e-5))
        g.d_gnr_nextra, g.d_gnr_bias_stats = ptr(gnr.get("nextra")), ptr(gnr.get("bias_stats"))
    g.half16, g.bf16 = int(bool(half16)), int(bool(bf16))
    scratch = torch.empty(size(getattr(lib, scratch_fn)(C.byref(g))), dtype=torch.uint8, device=dev)
    check(run(lib, g, scratch.data_ptr()))
    return {"out": out, "out16": out16, "stats": stats, "gn_stats": gn_stats, "wave_rows": g.wave_rows, "tag": g.tag.decode(),
            "flag": int(flag.item())}


def _attention_call(fn, qkv, mask, B, T, H, D, scale, mask_mode, *, klen=(), mode=(), ew=0, slack=0, flag=False, guard=False):
    """What the attention helpers share: (qkv, mask[, klen], B, T, H, D, scale, mask_mode, *mode, out[, flag][, scratch], stream).  ``ew``:
    halves per image element (0: fp32 I/O, no scratch); ``guard``: the output is a ``guarded`` buffer.  Returns (out or buf, flag word)."""
    dev = qkv.device
    out = guarded(B * T, H * D, dev) if guard else torch.empty(B * T, H * D, dtype=torch.float32, device=dev)
    fl = _flag(dev) if flag else None
    scratch = torch.empty(8 * ew * B * T * H * D + slack, dtype=torch.uint8, device=dev) if ew else None
    check(fn(ptr(qkv), ptr(mask), *[ptr(k) for k in klen], B, T, H, D, float(scale), mask_mode, *mode, ptr(out), *([ptr(fl)] if flag else []),
             *([scratch.data_ptr()] if ew else []), stream_ptr()))
    return out, fl


def attention_f32(qkv, mask, B, T, H, D, scale, mask_mode):
    return _attention_call(load().mtts_attention_f32, qkv, mask, B, T, H, D, scale, mask_mode)[0]


def attention_p16(qkv, mask, B, T, H, D, scale, mask_mode):
    return _attention_call(load().mtts_attention_p16, qkv, mask, B, T, H, D, scale, mask_mode, ew=2)[0]


def attention_f32_run(qkv, mask, B, T, H, D, scale, mask_mode=0, *, klen=None):
    """fp32-I/O attention with klen (include/mtts.h mtts_attention_f32_run).  Returns a dict: out ([B*T, H*D] view of buf), buf, tag."""
    buf, _ = _attention_call(load().mtts_attention_f32_run, qkv, mask, B, T, H, D, scale, mask_mode, klen=[klen], guard=True)
    return {"out": buf[:B * T * H * D].view(B * T, H * D), "buf": buf, "tag": last_kernel_tag()}


def attention_h16(qkv, mask, B, T, H, D, scale, mask_mode=0, *, klen=None, bf16=False):
    """H16 attention (csrc/attention_f32.hip HALF / BF; include/mtts.h mtts_attention_h16).  Returns a dict: out, tag, flag."""
    out, flag = _attention_call(load().mtts_attention_h16, qkv, mask, B, T, H, D, scale, mask_mode, klen=[klen], mode=[int(bool(bf16))], ew=1,
                                slack=256, flag=True)
    return {"out": out, "tag": last_kernel_tag(), "flag": int(flag.item())}


def attention_p16_run(qkv, mask, B, T, H, D, scale, mask_mode=0, *, klen=None, fast16=False, out_lscale=2048.0):
    """P16 attention as the decoder launches it (include/mtts.h mtts_attention_p16_run).  Returns a dict: out, tag, flag."""
    out, flag = _attention_call(load().mtts_attention_p16_run, qkv, mask, B, T, H, D, scale, mask_mode, klen=[klen],
                                mode=[int(bool(fast16)), float(out_lscale)], ew=2, slack=256, flag=True)
    return {"out": out, "tag": last_kernel_tag(), "flag": int(flag.item())}


def _groupnorm_call(fn, scratch_bytes, y, gamma, beta, mask, B, T, G, eps, *, chbias=None, pointer=ptr, res=(), mid=(), outs=()):
    """What the GroupNorm + Mish helpers share: (y, gamma, beta, mask[, chbias, stride][, res, ldr], B, T, C, G, eps, *mid, *outs, scratch,
    stream).  ``chbias``: None (the entry takes none) or a one-element list [tensor or None], [B, stride >= C] or [C]."""
    head = []
    for t in chbias or []:
        head += [pointer(t), (t.stride(0) if t is not None and t.dim() == 2 else 0)]
    for t in res:
        head += [pointer(t), (t.stride(0) if t is not None else 0)]
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=y.device)
    check(fn(ptr(y), ptr(gamma), ptr(beta), ptr(mask), *head, B, T, y.shape[1], G, float(eps), *mid, *[ptr(o) for o in outs], scratch.data_ptr(),
             stream_ptr()))


def groupnorm_mish(y, gamma, beta, mask, B, T, G=8, eps=1e-5):
    lib = load()
    out = torch.empty_like(y)
    _groupnorm_call(lib.mtts_groupnorm_mish, lib.mtts_groupnorm_scratch_bytes(B, T, G), y, gamma, beta, mask, B, T, G, eps, outs=[out])
    return out


def groupnorm_mish_rows(y, gamma, beta, mask, chbias, B, T, G=8, eps=1e-5):
    """``groupnorm_mish`` + the time-embedding bias: chbias [B, stride >= C] (one row per utterance) or [C] (one for the batch)."""
    lib = load()
    out = torch.empty_like(y)
    _groupnorm_call(lib.mtts_groupnorm_mish_rows, lib.mtts_groupnorm_scratch_bytes(B, T, G), y, gamma, beta, mask, B, T, G, eps, chbias=[chbias],
                    outs=[out])
    return out


def _groupnorm_image(fn, scratch_fn, mode, y, gamma, beta, mask, B, T, G, chbias, tile_stats, tile_rows, nrows, nextra, bias_stats, out16_mask,
                     want_f32, eps):
    """groupnorm_mish_h16 / groupnorm_mish_p16: an image out, widened or decoded into out16.  ``mode``: [bf16] or []."""
    out = torch.empty_like(y) if want_f32 else None
    out16 = torch.empty_like(y)
    flag = _flag(y.device)
    _groupnorm_call(fn, size(scratch_fn(B, T, y.shape[1], G)), y, gamma, beta, mask, B, T, G, eps, chbias=[chbias],
                    mid=[ptr(tile_stats), tile_rows, ptr(nrows), ptr(nextra), ptr(bias_stats), ptr(out16_mask), *mode], outs=[out, out16, flag])
    return {"out": out, "out16": out16, "flag": int(flag.item())}


def groupnorm_mish_h16(y, gamma, beta, mask, B, T, *, G=8, chbias=None, tile_stats=None, tile_rows=0, nrows=None, nextra=None,
                       bias_stats=None, out16_mask=None, bf16=False, want_f32=True, eps=1e-5):
    """GroupNorm + Mish + mask [+ chbias, mask] with an H16 image out (gn_apply_kernel's H16 store; mtts_groupnorm_mish_h16).
    chbias [B, stride >= C] or [C].  Returns a dict: out (fp32 rows), out16 (the image widened), flag."""
    lib = load()
    return _groupnorm_image(lib.mtts_groupnorm_mish_h16, lib.mtts_groupnorm_h16_scratch_bytes, [int(bool(bf16))], y, gamma, beta, mask, B, T, G,
                            chbias, tile_stats, tile_rows, nrows, nextra, bias_stats, out16_mask, want_f32, eps)


def groupnorm_mish_p16(y, gamma, beta, mask, B, T, *, G=8, chbias=None, tile_stats=None, tile_rows=0, nrows=None, nextra=None,
                       bias_stats=None, out16_mask=None, want_f32=True, eps=1e-5):
    """GroupNorm + Mish + mask [+ chbias, mask] with a P16 image out (gn_apply_kernel's two-plane store; mtts_groupnorm_mish_p16).
    chbias [B, stride >= C] or [C].  Returns a dict: out (fp32 rows), out16 (the image decoded), flag."""
    lib = load()
    return _groupnorm_image(lib.mtts_groupnorm_mish_p16, lib.mtts_groupnorm_p16_scratch_bytes, [], y, gamma, beta, mask, B, T, G,
                            chbias, tile_stats, tile_rows, nrows, nextra, bias_stats, out16_mask, want_f32, eps)


def to_p16_roundtrip(x, mask=None, *, C_valid=None, ld16=None, lscale=2048.0, Cc=None):
    """fp32 rows -> P16 image -> fp32 rows (include/mtts.h mtts_to_p16_roundtrip).  Returns a dict: ``out`` [M, C] fp32, ``bits``
    [M, ld16] int16 (the image as stored: per 32-channel group 32 heads then 32 residuals; halves beyond 2 * C are untouched 0x7e7e
    fill), ``flag`` (the range-flag word)."""
    lib = load()
    M = x.shape[0]
    Cc = x.shape[1] if Cc is None else Cc
    C_valid = Cc if C_valid is None else C_valid
    ld16 = 2 * Cc if ld16 is None else ld16
    image = torch.full((M, ld16), 0x7e7e, dtype=torch.int16, device=x.device)
    out = torch.empty(M, Cc, dtype=torch.float32, device=x.device)
    flag = _flag(x.device)
    check(lib.mtts_to_p16_roundtrip(ptr(x), x.stride(0), ptr(mask), M, Cc, C_valid, ld16, float(lscale), ptr(image), ptr(out), ptr(flag),
                                    stream_ptr()))
    return {"out": out, "bits": image, "flag": int(flag.item())}


def gemm_p16_args(a, w, bias=None, *, B, T_in, T_out=None, tap_off=None, in_stride=1, c1=0, a_mask=None, a_mean=None, a_rstd=None, a_part=None,
                  act=0, p0=None, p1=None, res=None, res16=None, inplace=None, out_mask=None, out_scale=1.0, out16_mask=None,
                  want_f32=True, want_p16=False, out=None, out16=None, out_T=0, out_stride=1, out_off=0, stats_out=False, gn_groups=0,
                  gn_nrows=None, gnr=None, force_bm=0, fast16=False, out_lscale=2048.0, half16=False, bf16=False):
    """P16 GEMM with every epilogue form of the decoder (csrc/gemm_p16.hip MODE 0, MODE 1 with ``fast16``; include/mtts.h
    mtts_gemm_p16_args_run).  Arguments and result as ``gemm_h16`` with P16 images in place of H16 ones; ``out_lscale``: residual scale
    of the output image (2048, or 1 for what the attention kernel reads)."""
    return _gemm_block(lambda lib, g, scratch: lib.mtts_gemm_p16_args_run(C.byref(g), int(bool(fast16)), float(out_lscale), scratch, stream_ptr()),
                       "mtts_gemm_p16_args_scratch_bytes", a, w, bias,
                       B=B, T_in=T_in, T_out=T_out, tap_off=tap_off, in_stride=in_stride, c1=c1, a_mask=a_mask, a_mean=a_mean, a_rstd=a_rstd,
                       a_part=a_part, act=act, p0=p0, p1=p1, res=res, res16=res16, inplace=inplace, out_mask=out_mask, out_scale=out_scale,
                       out16_mask=out16_mask, want_f32=want_f32, want16=want_p16, out=out, out16=out16, out_T=out_T, out_stride=out_stride,
                       out_off=out_off, stats_out=stats_out, gn_groups=gn_groups, gn_nrows=gn_nrows, gnr=gnr, force_bm=force_bm, bf16=bf16,
                       half16=half16)


# ---- the fp32-row flow's unit entries.  Every output buffer is filled with F32_SENTINEL and has F32_GUARD floats behind its last row,
# so a caller can see every element a launch did not write.
F32_GUARD = 64
F32_SENTINEL = -7.0e33


def rows_ptr(t):
    """Device pointer of fp32 rows that may be a row-strided view (unit stride inside a row); None passes NULL."""
    if t is None:
        return None
    if not on_device(t) or t.stride(-1) != 1:
        raise RuntimeError("mtts: rows must be on a HIP device with unit stride inside a row")
    return t.data_ptr()


def guarded(rows, ld, device):
    """flat fp32 buffer of rows * ld + F32_GUARD sentinels"""
    return torch.full((rows * ld + F32_GUARD,), F32_SENTINEL, dtype=torch.float32, device=device)


def gemm_f32_args(a, w, bias=None, *, terms, B, T_in, T_out=None, tap_off=None, in_stride=1, c1=0, a1=None, a_mask=None, a_mean=None,
                  a_rstd=None, a_part=None, act=0, p0=None, p1=None, res=None, out_mask=None, out_scale=1.0, out16_mask=None, want_f32=True,
                  want_p16=False, into=None, ldc=0, out_T=0, out_stride=1, out_off=0, stats_out=False, force_bm=0, out_lscale=2048.0):
    """gemm_f32_kernel as the fp32-row flow launches it (include/mtts.h mtts_gemm_f32_args_run).  a [B*T_in, >= C - c1 (or C)] fp32 rows
    (a row-strided view is passed with its stride), a1 the second segment's rows or None (the last c1 columns of a); w Linear [N, C] or
    Conv1d [N, C, k] anywhere; res a [rows, >= N] view.  ``into``: the result of an earlier call whose buffers this launch writes into
    (strided output rows).  Returns a dict: out ([rows, N] view of buf), buf (flat, rows * ld + guard), ld, out16 (decoded image), image
    (raw, int16 [rows + guard rows, 2 N]), stats, stats_buf, tag, flag."""
    lib = load()
    dev = a.device
    g, alive, rows, N, flag = _gemm_fill(a, w, bias, B=B, T_in=T_in, T_out=T_out, tap_off=tap_off, in_stride=in_stride, c1=c1, a_mask=a_mask,
                                         a_mean=a_mean, a_rstd=a_rstd, a_part=a_part, act=act, p0=p0, p1=p1, res=res, out_mask=out_mask,
                                         out_scale=out_scale, out16_mask=out16_mask, out_T=out_T, out_stride=out_stride, out_off=out_off,
                                         force_bm=force_bm, rows=rows_ptr)
    ld = ldc if ldc else N
    buf = into["buf"] if into is not None else (guarded(rows, ld, dev) if want_f32 else None)
    out16 = torch.full((rows, N), F32_SENTINEL, dtype=torch.float32, device=dev) if want_p16 else None
    g.d_out, g.d_out16_f32 = ptr(buf), ptr(out16)
    stats_buf = None
    if stats_out:
        stats_buf = into["stats_buf"] if into is not None else guarded(rows, 2 * (N // 64), dev)
    g.d_stats_out = ptr(stats_buf)
    n = size(lib.mtts_gemm_f32_args_scratch_bytes(C.byref(g)))
    scratch = torch.empty(n + 256, dtype=torch.uint8, device=dev)
    check(lib.mtts_gemm_f32_args_run(C.byref(g), int(terms), rows_ptr(a1), a1.stride(0) if a1 is not None else 0, int(ldc), float(out_lscale),
                                     scratch.data_ptr(), stream_ptr()))
    image = None
    if want_p16:
        off = (-scratch.data_ptr()) % 256
        image = scratch[off:off + (rows + 64) * 2 * N * 2].view(torch.int16).view(rows + 64, 2 * N).clone()
    return {"out": buf[:rows * ld].view(rows, ld)[:, :N] if buf is not None else None, "buf": buf, "ld": ld, "out16": out16, "image": image,
            "stats": stats_buf[:rows * 2 * (N // 64)].view(rows, N // 64, 2) if stats_buf is not None else None, "stats_buf": stats_buf,
            "tag": g.tag.decode(), "flag": int(flag.item())}


def groupnorm_mish_f32_run(y, gamma, beta, mask, B, T, *, G=8, chbias=None, res=None, nrows=None, nextra=None, bias_stats=None,
                           stats_out=False, eps=1e-5):
    """gn_partial + gn_apply with the fp32 store (include/mtts.h mtts_groupnorm_mish_f32_run).  chbias [B, stride >= C] or [C]; res a
    [B*T, >= C] view.  Returns a dict: out ([B*T, C] view of buf), buf, stats, stats_buf."""
    lib = load()
    Cc = y.shape[1]
    buf = guarded(B * T, Cc, y.device)
    stats_buf = guarded(B * T, 2 * (Cc // 64), y.device) if stats_out else None
    _groupnorm_call(lib.mtts_groupnorm_mish_f32_run, size(lib.mtts_groupnorm_scratch_bytes(B, T, G)) + 256, y, gamma, beta, mask, B, T, G, eps,
                    chbias=[chbias], pointer=rows_ptr, res=[res], mid=[ptr(nrows), ptr(nextra), ptr(bias_stats)], outs=[buf, stats_buf])
    return {"out": buf[:B * T * Cc].view(B * T, Cc), "buf": buf,
            "stats": stats_buf[:B * T * 2 * (Cc // 64)].view(B * T, Cc // 64, 2) if stats_out else None, "stats_buf": stats_buf}


def _layernorm_call(x, ldx, B, T, Cc, gamma, beta, eps, act, film, mask, y, ldy):
    """``mtts_channel_layernorm_ld`` is ``mtts_channel_layernorm`` with leading dimensions; the plain entry keeps its own export."""
    lib = load()
    if ldx is None:
        check(lib.mtts_channel_layernorm(ptr(x), B, T, Cc, ptr(gamma), ptr(beta), float(eps), act, ptr(film), ptr(mask), ptr(y), stream_ptr()))
    else:
        check(lib.mtts_channel_layernorm_ld(rows_ptr(x), ldx, B, T, Cc, ptr(gamma), ptr(beta), float(eps), act, ptr(film), ptr(mask), ptr(y), ldy,
                                            stream_ptr()))
    return y


def channel_layernorm_ld(x, B, T, Cc, gamma, beta, *, eps=1e-5, act=0, film=None, mask=None, ldy=None):
    """Channel LayerNorm on rows of wider buffers (include/mtts.h mtts_channel_layernorm_ld).  x a [B*T, >= C] view.  Returns a dict:
    out ([B*T, C] view of buf), buf, ld."""
    ldy = Cc if ldy is None else ldy
    buf = _layernorm_call(x, x.stride(0), B, T, Cc, gamma, beta, eps, act, film, mask, guarded(B * T, ldy, x.device), ldy)
    return {"out": buf[:B * T * ldy].view(B * T, ldy)[:, :Cc], "buf": buf, "ld": ldy}


def channel_layernorm(x, gamma, beta, B, T, *, act=0, film=None, mask=None, eps=1e-5):
    """x [B*T, C] rows; film [B, 2C] = gamma | beta of the DurationPredictor's speaker FiLM; mask [B*T]."""
    return _layernorm_call(x, None, B, T, x.shape[1], gamma, beta, eps, act, film, mask, torch.empty_like(x), None)


def row_stats(x, eps=1e-5):
    lib = load()
    M, Cc = x.shape
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    check(lib.mtts_row_stats(ptr(x), M, Cc, Cc, eps, ptr(mean), ptr(rstd), stream_ptr()))
    return mean, rstd


def channel_layernorm_bwd(x, dy, gamma, beta, B, T, *, act=0, film=None, mask=None, gate=0, eps=1e-5):
    """Backward of ``channel_layernorm`` (mtts_channel_layernorm_bwd): returns ``(dx [B*T, C], dfilm [B, 2C] or None)``."""
    lib = load()
    dx = torch.empty_like(x)
    Cc = x.shape[1]
    dfilm = torch.empty(B, 2 * Cc, dtype=torch.float32, device=x.device) if film is not None else None
    scratch = torch.empty(B * T * Cc, dtype=torch.float32, device=x.device) if film is not None else None
    check(lib.mtts_channel_layernorm_bwd(ptr(x), ptr(dy), B, T, Cc, ptr(gamma), ptr(beta), float(eps), act, ptr(film), ptr(mask), gate,
                                         ptr(dx), ptr(dfilm), ptr(scratch), stream_ptr()))
    return dx, dfilm


def attention_rope_bwd(qkv, o, do, lengths, B, T, H, D, scale, cos, sin):
    """Backward of the encoder's rotary SDPA (mtts_attention_rope_bwd): ``qkv`` [B*T, 3*H*D] rows after the rotation -> the gradient
    with respect to q | k | v before it."""
    lib = load()
    dqkv = torch.empty_like(qkv)
    scratch = torch.empty(B * H * T * 3, dtype=torch.float32, device=qkv.device)
    lengths = lengths.detach().to(device=qkv.device, dtype=torch.int64).contiguous()
    check(lib.mtts_attention_rope_bwd(ptr(qkv), ptr(o), ptr(do), ptr(lengths), B, T, H, D, float(scale), ptr(cos), ptr(sin), ptr(dqkv),
                                      ptr(scratch), stream_ptr()))
    return dqkv


def spk_grad_seeds(mu_x, logw, durations, y_fine, x_lengths, y_fine_lengths, w_proj, delta_prior, delta_dur, *, seed_mu, seed_logw):
    """The two Huber seeds of ``mtts_spk_grad`` on given buffers (mtts_spk_grad_seeds).  ``seed_mu`` (>= B*Tx*round_up(F, 4) floats) and
    ``seed_logw`` (>= B*Tx*Fd floats) are the caller's, so that a test can fill them first.  Returns the scratch, whose header
    ``mtts_score_status`` reads."""
    lib = load()
    B, F, Tx = mu_x.shape
    Tm, Fd = y_fine.shape[2], w_proj.numel()
    scratch = torch.zeros(size(lib.mtts_spk_grad_seeds_scratch_bytes(B, Tx, Tm)), dtype=torch.uint8, device=mu_x.device)
    check(lib.mtts_spk_grad_seeds(ptr(mu_x), ptr(logw), ptr(durations), ptr(y_fine), ptr(x_lengths), ptr(y_fine_lengths), ptr(w_proj), B, F, Tx,
                                  Tm, Fd, float(delta_prior), float(delta_dur), ptr(seed_mu), ptr(seed_logw), scratch.data_ptr(), scratch.numel(),
                                  stream_ptr()))
    return scratch


def grad_gate(g, ldg, M, Cc, mode, ref, *, mask=None):
    """``gate_kernel`` in place on the flat buffer ``g`` (rows of ``ldg`` floats) against ``ref`` [M, ldref] (mtts_grad_gate)."""
    scratch = torch.empty(M * 2 * Cc, dtype=torch.float16, device=ref.device) if mode == 2 else None
    check(load().mtts_grad_gate(ptr(g), ldg, M, Cc, mode, ptr(ref), ref.shape[1], ptr(mask), ptr(scratch), stream_ptr()))
    return g


def token_sums(src, col0, Cc, B, T, dst, ldd, dcol0, *, lengths=None, verdict=None, accumulate=0):
    """``colsum_kernel`` with every argument (mtts_token_sums): ``src`` [B*T, ld] rows, ``dst`` a flat buffer of rows of ``ldd`` floats."""
    check(load().mtts_token_sums(ptr(src), src.shape[1], col0, Cc, B, T, ptr(lengths), ptr(verdict), ptr(dst), ldd, dcol0, accumulate, stream_ptr()))
    return dst


# ---- the kernels that are not GEMMs (csrc/vocos.hip, csrc/norm_glue.hip): thin wrappers of their unit entries.  Buffers a kernel
# writes can be passed in (``out=`` / ``dst``), so that a test can fill them with a sentinel first.
def dwconv7_ln(x, w7, bias, gamma, beta, B, T, *, eps=1e-6, lengths=None, out=None):
    """x [B*T, C] rows, w7 [7, C] (tap-major); lengths int64 [B] or None.  Returns y [B*T, C]."""
    y = torch.empty_like(x) if out is None else out
    check(load().mtts_dwconv7_ln(ptr(x), ptr(w7), ptr(bias), ptr(gamma), ptr(beta), float(eps), B, T, x.shape[1], ptr(lengths), ptr(y),
                                 stream_ptr()))
    return y


def spec_polar(x, nbins, off, clip=1e2):
    """In place on x [M, ld]: columns (k, off + k) hold (log-magnitude, phase) and become (Re, Im)."""
    check(load().mtts_spec_polar(ptr(x), x.shape[0], x.shape[1], nbins, off, float(clip), stream_ptr()))
    return x


def istft_ola(frames, window, B, T, hop, *, lengths=None, out=None):
    """frames [B*T, n_fft] (already windowed once), window [n_fft] -> audio [B, hop * (T - 1)]."""
    n_fft = frames.shape[1]
    audio = torch.empty(B, hop * (T - 1), dtype=torch.float32, device=frames.device) if out is None else out
    check(load().mtts_istft_ola(ptr(frames), ptr(window), B, T, n_fft, hop, ptr(lengths), ptr(audio), stream_ptr()))
    return audio


def ode_combine(stage, dt, y, k1, k2=None, k3=None, k4=None, *, C, out, T=0):
    """Rows [M, ld] (ld = each tensor's second dimension; k1..k4 share one); ``dt`` a float, or a device tensor [M / T] of one dt
    per utterance.  ``out`` may be ``y``."""
    per_utt = torch.is_tensor(dt)
    check(load().mtts_ode_combine(stage, 0.0 if per_utt else float(dt), ptr(dt) if per_utt else None, T, ptr(y), y.shape[1], ptr(k1),
                                  ptr(k2), ptr(k3), ptr(k4), k1.shape[1], ptr(out), out.shape[1], y.shape[0], C, stream_ptr()))
    return out


def step_tables(t0, t1, mask, stages, out=None):
    """t0, t1 [B], mask [B, T] -> (tv [stages * B], dt_b [B], rs_full [B*T], rs_half [B*T]); ``out``: those four buffers."""
    B, T = mask.shape
    dev = mask.device
    tv, dt_b, rs_full, rs_half = out if out is not None else (
        torch.empty(stages * B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
        torch.empty(B * T, dtype=torch.float32, device=dev), torch.empty(B * T, dtype=torch.float32, device=dev))
    check(load().mtts_step_tables(ptr(t0), ptr(t1), ptr(mask), B, T, stages, ptr(tv), ptr(dt_b), ptr(rs_full), ptr(rs_half), stream_ptr()))
    return tv, dt_b, rs_full, rs_half


def time_sinusoid(freqs, t, scale=1000.0, out=None):
    """freqs [half] on the device; ``t`` a CPU tensor (the host form, at most 256 times) or a device tensor (the device form).
    Returns [nt, 2 * half] = sin | cos."""
    nt, half = t.numel(), freqs.numel()
    emb = torch.empty(nt, 2 * half, dtype=torch.float32, device=freqs.device) if out is None else out
    if t.is_cuda:
        check(load().mtts_time_sinusoid(ptr(freqs), None, ptr(t), nt, half, float(scale), ptr(emb), stream_ptr()))
    else:
        t = t.detach().to(torch.float32).contiguous()
        check(load().mtts_time_sinusoid(ptr(freqs), t.data_ptr(), None, nt, half, float(scale), ptr(emb), stream_ptr()))
    return emb


def rope(qkv, B, T, H, D, d_rope, cos, sin):
    """In place on qkv [B*T, 3*H*D]; cos / sin [>= T, d_rope]."""
    check(load().mtts_rope(ptr(qkv), B, T, H, D, d_rope, ptr(cos), ptr(sin), stream_ptr()))
    return qkv


def cf_to_cl(src, dst, *, T=None, col_off=0, add=None, lengths=None):
    """src [B, C, T_src] (+ add) -> dst [B*T, ld] at columns [col_off, col_off + C); T defaults to T_src."""
    B, Cc, T_src = src.shape
    T = T_src if T is None else T
    check(load().mtts_cf_to_cl(ptr(src), ptr(add), B, Cc, T, T_src, ptr(dst), dst.shape[1], col_off, ptr(lengths), stream_ptr()))
    return dst


def cl_to_cf(src, dst, *, T, scale=1.0, shift=0.0):
    """src [B*T, ld] -> dst [B, C, T_out] = src * scale + shift."""
    B, Cc, T_out = dst.shape
    check(load().mtts_cl_to_cf(ptr(src), src.shape[1], B, Cc, T, ptr(dst), T_out, float(scale), float(shift), stream_ptr()))
    return dst


def slots_to_cl(pool, slots, dst, *, T, col_off=0):
    """pool [S, C, T_pool], slots int32 [B] -> dst [B*T, ld] at columns [col_off, col_off + C)."""
    S, Cc, T_pool = pool.shape
    check(load().mtts_slots_to_cl(ptr(pool), ptr(slots), S, T_pool, slots.numel(), Cc, T, ptr(dst), dst.shape[1], col_off, stream_ptr()))
    return dst


def cl_to_slots(src, pool, slots, *, T):
    """src [B*T, ld] -> pool [S, C, T_pool] at the slots of int32 [B]."""
    S, Cc, T_pool = pool.shape
    check(load().mtts_cl_to_slots(ptr(src), src.shape[1], slots.numel(), Cc, T, ptr(pool), ptr(slots), S, T_pool, stream_ptr()))
    return pool

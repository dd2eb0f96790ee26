"""Time the pitch entries (profiles/r30_pitch.md): ``mtts_pitch_track`` and ``mtts_pitch_stats`` alone, by HIP events (warm, then the
median of ``--repeats`` calls), on a batch of 32 clips of 10 s at 24 kHz with the default parameters and on one such clip; the same
analysis by the fp64 restatement (tests/pitch_restated.py) on the host for one clip, and the device's largest deviation from it
beside the derived budget.  Prints one JSON line.

    python tools/pitch_time.py [--repeats 20] [--seconds 10]
    python tools/pitch_time.py --kernels        # only a few calls on each shape: for a kernel trace
"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "matcha-tts-24k_amd"
FS = 24000


def summary(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def clip(i: int, seconds: float) -> np.ndarray:
    """A five-harmonic voice that glides between 100 + 5 i and 220 + 5 i Hz twice a second, with noise 40 dB below it."""
    rng = np.random.default_rng(i)
    n = int(seconds * FS) + 37 * i
    t = np.arange(n) / FS
    f = 160.0 + 5.0 * i + 60.0 * np.sin(2 * np.pi * 0.5 * t)
    phase = 2 * np.pi * np.cumsum(f) / FS
    x = sum(a * np.sin((h + 1) * phase + 0.3 * h) for h, a in enumerate((1.0, 0.6, 0.4, 0.25, 0.15)))
    x *= 0.3 / np.sqrt(np.mean(x * x))
    return (x + 0.003 * rng.standard_normal(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required")
    hip = importlib.import_module(PKG + "._hip")
    P = importlib.import_module(PKG + ".pitch")
    lib = hip.load()
    hop, window, min_lag, max_lag = P.plan(FS)
    out = {"tool": "pitch_time", "repeats": args.repeats, "sample_rate": FS, "hop": hop, "max_lag": max_lag, "shapes": {}}
    clips = [clip(i, args.seconds) for i in range(32)]
    for name, B in (("batch32", 32), ("one", 1)):
        rows = clips[:B]
        ld = (max(len(r) for r in rows) + 3) // 4 * 4
        host = np.zeros((B, ld), dtype=np.float32)
        for b, r in enumerate(rows):
            host[b, :len(r)] = r
        audio = torch.from_numpy(host).cuda()
        d_len = torch.tensor([len(r) for r in rows], device="cuda")
        T = P.n_frames(ld, hop, window, max_lag)
        f0, aper = torch.empty(B, T, device="cuda"), torch.empty(B, T, device="cuda")
        frames = torch.empty(B, dtype=torch.long, device="cuda")
        ws = torch.empty(lib.mtts_pitch_workspace_bytes(ld, B, FS, hop, 60.0, 500.0), dtype=torch.uint8, device="cuda")
        hz, counts = torch.empty(B, 4, device="cuda"), torch.empty(B, 3, dtype=torch.long, device="cuda")
        ws2 = torch.empty(256, dtype=torch.uint8, device="cuda")
        calls = {"mtts_pitch_track": lambda: hip.check(lib.mtts_pitch_track(
                     audio.data_ptr(), ld, d_len.data_ptr(), B, FS, hop, 60.0, 500.0, 0.15, f0.data_ptr(), aper.data_ptr(), T, frames.data_ptr(),
                     ws.data_ptr(), ws.numel(), hip.stream_ptr())),
                 "mtts_pitch_stats": lambda: hip.check(lib.mtts_pitch_stats(
                     f0.data_ptr(), T, frames.data_ptr(), B, 47, hz.data_ptr(), counts.data_ptr(), ws2.data_ptr(), 256, hip.stream_ptr()))}
        res = {"rows": B, "samples_per_row": len(rows[0]), "frames_per_row": T, "workspace_mb": round(ws.numel() / 1e6, 1)}
        for key, fn in calls.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            if args.kernels:
                continue
            ev = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            res[key + "_ms"] = summary([a.elapsed_time(b) for a, b in ev])
        # multiply-adds of the block sums: every block of every clip, every lag, every sample of the block
        blocks = int((frames.clamp(min=1) + 7).sum())
        res["block_sum_multiply_adds"] = blocks * max_lag * hop
        out["shapes"][name] = res
        if B == 1 and not args.kernels and (ROOT / "tests" / "pitch_restated.py").exists():
            sys.path.insert(0, str(ROOT / "tests"))
            import pitch_restated as pr
            t0 = time.perf_counter()
            ref = pr.analyse(rows[0], FS, hop)
            host_s = time.perf_counter() - t0
            n = int(frames[0])
            a = aper[0, :n].cpu().numpy().astype(np.float64)
            ok = ref["margin"] > 0
            rel = np.abs(a - ref["aperiodicity"])[ok] / ref["aperiodicity"][ok]
            out["fp64_restatement"] = {"host_seconds_one_clip": round(host_s, 3), "frames": n, "decidable": int(ok.sum()),
                                       "worst_relative_aperiodicity_error": float(rel.max()), "derived_budget": pr.rel_budget(hop),
                                       "worst_absolute_aperiodicity_error": float(np.abs(a - ref["aperiodicity"])[ok].max()),
                                       "voiced_equal_on_decidable": bool(np.array_equal((f0[0, :n].cpu().numpy() > 0)[ok], ref["voiced"][ok]))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

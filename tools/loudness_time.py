"""Time the loudness stage (profiles/r19_loudness.md): `inference.to_waveforms` with and without ``loudness=`` on the two shapes that
matter -- a batch of 32 utterances of 10 s, and one row of 1.8 M samples -- by a host clock around calls that end in the
device-to-host copies, alternated; and `loudness.normalize` alone on audio of the same shapes by HIP events.  Synthetic Vocos
weights, random mels in the log-mel range.  Prints one JSON line.

    python tools/loudness_time.py [--repeats 20]
    python tools/loudness_time.py --kernels        # only a few normalize calls on each shape: for a kernel trace
"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "matcha-tts-24k_amd"
SHAPES = (("batch32_10s", 32, 938), ("long1_75s", 1, 7032))       # (name, rows, mel frames at hop 256)


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required")
    inf = importlib.import_module(PKG + ".inference")
    syn = importlib.import_module(PKG + ".synthetic")
    LD = importlib.import_module(PKG + ".loudness")
    out = {"tool": "loudness_time", "repeats": args.repeats, "shapes": {}}
    vocoder = None if args.kernels else inf.load_vocoder("vocos", state_dict=syn.make_vocos_state_dict(seed=11))
    g = torch.Generator().manual_seed(1)
    for name, B, T in SHAPES:
        n = 256 * (T - 1)
        ld = (n + 3) // 4 * 4
        audio = (torch.randn(B, ld, generator=g) * 0.09).cuda()
        lengths = torch.full((B,), n, dtype=torch.long, device="cuda")
        targets = (-23.0, -26.0)                                  # alternated: the gain is never 1, the apply pass always runs
        for i in range(3):
            LD.normalize(audio, lengths, targets[i % 2], check=False)
        torch.cuda.synchronize()
        if args.kernels:
            continue
        ev = []
        for i in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            LD.normalize(audio, lengths, targets[i % 2], check=False)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        res = {"rows": B, "samples_per_row": n, "normalize_ms": stats([a.elapsed_time(b) for a, b in ev])}
        mel = (torch.randn(B, 100, T, generator=g) * 2.0 - 4.0).cuda()
        lens = torch.full((B,), T, dtype=torch.long, device="cuda")
        calls = {"plain": lambda: inf.to_waveforms(mel, lens, vocoder), "loudness": lambda: inf.to_waveforms(mel, lens, vocoder, loudness=-23.0)}
        for fn in calls.values():
            fn()
        t = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[k].append((time.perf_counter() - t0) * 1e3)
        res["to_waveforms_ms"] = {k: stats(v) for k, v in t.items()}
        out["shapes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Time and characterise the R 128 stage (profiles/r21_r128.md): `loudness.normalize` with and without ``true_peak=`` (``mtts_loudness``
against ``mtts_loudness_r128``) by HIP events, alternated, on the two shapes of profiles/r19_loudness.md; the overshoot that is left
after the rate conversion; and the reading of the 12-tap estimator on sines against a long interpolation.  Prints one JSON line.

    python tools/r128_time.py [--repeats 20]
    python tools/r128_time.py --kernels        # a few calls on each shape and on a 25-minute row: for a kernel trace
    python tools/r128_time.py --estimator      # host only: the estimator's error across the band
"""
import argparse
import importlib
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "matcha-tts-24k_amd"
SHAPES = (("batch32_10s", 32, 239872), ("long1_75s", 1, 1799936))      # (name, rows, samples per row): 75 s has 720 short-term blocks
LONG = ("long1_1503s", 1, 36069600)                                    # 25 minutes: 15 000 short-term blocks


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def am_noise(n, seed, rms=0.09, fs=24000):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (rng.standard_normal(n) * rms * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t))).astype(np.float32)


def estimator(LD):
    """A sine of amplitude 1 at f, phase swept: the 12-tap reading against a 129-tap Kaiser-windowed sinc at 32 times the rate."""
    fs = 24000
    F, h = LD.true_peak_filter(fs)
    h = h.numpy()
    up, half = 32, 64
    k = np.arange(-half * up, half * up + 1)
    long = np.sinc(k / up) * np.kaiser(len(k), 12.0)
    out = {}
    for rel in (0.05, 0.1, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45):
        over, under, worst_sample = -math.inf, math.inf, math.inf
        for phase in np.linspace(0.0, np.pi, 16, endpoint=False):
            x = np.sin(2.0 * np.pi * rel * np.arange(2048) + phase).astype(np.float32)
            pad = np.concatenate([np.zeros(5, np.float32), x, np.zeros(6, np.float32)])
            win = np.lib.stride_tricks.sliding_window_view(pad, 12)[200:-200]
            short = max(float(np.abs(x).max()), max(float(np.abs((win * h[p]).sum(axis=1)).max()) for p in range(1, F)))
            z = np.zeros(len(x) * up)
            z[::up] = x
            fine = np.convolve(z, long, mode="same")[300 * up:-300 * up]
            diff = 20 * math.log10(short) - 20 * math.log10(float(np.abs(fine).max()))
            over, under = max(over, diff), min(under, diff)
            worst_sample = min(worst_sample, 20 * math.log10(float(np.abs(x[200:-200]).max())) - 20 * math.log10(float(np.abs(fine).max())))
        out[str(rel)] = {"over_read_db": round(over, 3), "under_read_db": round(under, 3), "sample_peak_under_read_db": round(worst_sample, 3)}
    # a sine that starts and stops inside the row: the reading at the row's two ends, where the 12 taps see the step
    x = np.sin(2.0 * np.pi * 0.25 * np.arange(2048) + np.pi / 4.0).astype(np.float32)
    pad = np.concatenate([np.zeros(5, np.float32), x, np.zeros(6, np.float32)])
    win = np.lib.stride_tricks.sliding_window_view(pad, 12)
    out["truncated_quarter_rate_sine_db"] = round(20 * math.log10(max(float(np.abs((win * h[p]).sum(axis=1)).max()) for p in range(1, F))), 3)
    return out


def overshoot(LD, R):
    """Rows brought towards -8 LUFS with and without ``true_peak=-1``, then converted: the sample peak of what is delivered, in dB
    relative to the -1 dBTP ceiling."""
    fs = 24000
    rows = [am_noise(fs, seed) for seed in (10, 11, 12, 13, 14, 15, 16, 17)]
    host = np.stack(rows)
    lengths = torch.full((len(rows),), fs, dtype=torch.long, device="cuda")
    out = {}
    for name, kw in (("with_true_peak_-1", dict(true_peak=-1.0)), ("without", {})):
        audio = torch.from_numpy(host.copy()).cuda()
        LD.normalize(audio, lengths, -8.0, check=False, **kw)
        res = {"24000": round(float(20 * torch.log10(audio.abs().max(dim=1).values).max()) + 1.0, 3),
               "true_peak_24000": round(float(LD.dbtp(LD.meter(audio, lengths)["true_peak"]).max()) + 1.0, 3)}
        for rate in (8000, 48000):
            conv, n = R.resample(audio, lengths, fs, rate, check=False)
            peaks = conv.abs().max(dim=1).values
            res[str(rate)] = round(float(20 * torch.log10(peaks).max()) + 1.0, 3)
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--estimator", action="store_true")
    args = ap.parse_args()
    LD = importlib.import_module(PKG + ".loudness")
    if args.estimator:
        print(json.dumps({"tool": "r128_time", "estimator": estimator(LD)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required")
    R = importlib.import_module(PKG + ".resample")
    out = {"tool": "r128_time", "repeats": args.repeats, "shapes": {}}
    g = torch.Generator().manual_seed(1)
    for name, B, n in SHAPES + ((LONG,) if args.kernels else ()):
        audio = (torch.randn(B, n, generator=g) * 0.09).cuda()
        lengths = torch.full((B,), n, dtype=torch.long, device="cuda")
        targets = (-23.0, -26.0)                                  # alternated: the gain is never 1, the apply pass always runs
        calls = {"loudness": lambda t: LD.normalize(audio, lengths, t, check=False),
                 "r128": lambda t: LD.normalize(audio, lengths, t, check=False, true_peak=-1.0, return_meter=True)}
        for i in range(3):
            for fn in calls.values():
                fn(targets[i % 2])
        torch.cuda.synchronize()
        if args.kernels:
            continue
        ev = {k: [] for k in calls}
        for i in range(args.repeats):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(targets[i % 2])
                e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        out["shapes"][name] = {"rows": B, "samples_per_row": n, **{k + "_ms": stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}}
    if not args.kernels:
        out["overshoot_db_over_ceiling"] = overshoot(LD, R)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

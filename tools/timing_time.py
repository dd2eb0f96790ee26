#!/usr/bin/env python3
"""Times of token timing on one GPU (profiles/r22_timing.md): ``to_waveforms`` at 32 rows of 128 tokens without the new arguments,
with ``return_marks`` and with one break per row, and the three new entries as calls.

    python tools/timing_time.py [--tree DIR] [--repeats 20]      # call times, profiler off; --tree: another checkout (the parent commit)
    python tools/timing_time.py --kernels                       # three calls of each new entry and nothing else (for a kernel trace)

Random Vocos weights and a random mel: no files.  ``--tree DIR`` imports the package from DIR instead of this checkout; a tree
without ``timing.py`` is timed without the new arguments only.  Host clock around calls that end in a device synchronise; five runs
of ``--repeats`` calls each, the median of each run.  One JSON line goes to stdout."""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

PKG = "matcha-tts-24k_amd"
B, TX = 32, 128


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    sub = lambda name: importlib.import_module(f"{PKG}.{name}")
    inf, voc, syn, hip = sub("inference"), sub("vocoder"), sub("synthetic"), sub("_hip")
    hip.load()
    timed = (Path(args.tree) / PKG / "timing.py").exists()
    rng = np.random.default_rng(1)
    dur = rng.integers(3, 9, (B, TX))
    x_len = rng.integers(96, TX + 1, B)
    x_len[0] = TX
    for b in range(B):
        dur[b, x_len[b]:] = 0
    cum = np.cumsum(dur, 1)
    frames = (cum[:, -1] + 1) // 2
    T = int(frames.max())
    g = torch.Generator().manual_seed(3)
    mel = (torch.randn(B, 100, T, generator=g) * 2.0 - 4.0).cuda()
    lens = torch.tensor(frames).cuda()
    ends = dict(token_ends=torch.tensor(cum, dtype=torch.int32).cuda(), x_lengths=torch.tensor(x_len).cuda())
    out = {"tree": args.tree, "timed": timed, "shape": dict(B=B, Tx=TX, T=T, samples=256 * (T - 1))}

    if timed:
        tm = sub("timing")
        model = hip.HipModel(sub("hparams").tiny())              # durations need no weights
        logw = torch.randn(B, 1, TX, generator=g).cuda()
        mask = torch.ones(B, 1, TX).cuda()
        s, a = torch.rand(B, TX, generator=g).cuda() * 2, torch.zeros(B, TX).cuda()
        audio = torch.randn(B, 256 * (T - 1), generator=g).cuda() * 0.1
        keep = 256 * (lens - 1)
        brk = [[(int(n) // 2, 7200)] for n in x_len]
        plan_of = lambda breaks: tm.token_marks(ends["token_ends"], ends["x_lengths"], keep, breaks, keep_max=audio.shape[1], check=False)
        entries = {
            "durations_shaped": lambda: model.durations_shaped(logw, mask, 1.0, 1.0, token_scale=s, token_extend=a),
            "durations (per utterance, the yardstick)": lambda: model.durations(logw, mask, [1.0] * B, [1.0] * B),
            "token_marks, no breaks": lambda: plan_of(None),
            "token_marks, one break per row": lambda: plan_of(brk),
        }
        plan = plan_of(brk)[2]
        entries["apply_breaks"] = lambda: tm.apply_breaks(audio, plan, 120)
    if args.kernels:
        if not timed:
            raise SystemExit("--kernels needs a tree with timing.py")
        for fn in entries.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        print(json.dumps(out))
        return 0

    wrapper = voc.load_model("cuda", state_dict=syn.make_vocos_state_dict(seed=11))
    cases = {"plain": {}}
    if timed:
        cases["return_marks"] = dict(return_marks=True, **ends)
        cases["one break per row"] = dict(breaks=[[(int(n) // 2, 300.0)] for n in x_len], return_marks=True, **ends)

    def run(kw, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf.to_waveforms(mel, lens, wrapper, **kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts
    out["to_waveforms_ms"] = {}
    for name, kw in cases.items():
        run(kw, 5)
        out["to_waveforms_ms"][name] = [round(statistics.median(run(kw, args.repeats)), 4) for _ in range(5)]
    if timed:
        def events(fn, n=50):
            for _ in range(5):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / n * 1e3, 2)
        out["entry_us_per_call"] = {name: events(fn) for name, fn in entries.items()}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    with torch.inference_mode():
        sys.exit(main())

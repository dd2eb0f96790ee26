#!/usr/bin/env python3
"""FLAC in, timed: ``recordings()`` for B clips of 10 s at 24 kHz handed over as ``FlacClip`` files against the same clips as
``Encoded("pcm16")``, alternating, and the two decode calls alone by device events (profiles/r27_flac_in.md).

    python tools/flac_time_in.py [--batch 32] [--repeats 20] [--seconds 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/flac_time_in.py --repeats 3     # kernel times, a run of its own

The clip is written by the recipe writer of tests/flac_in_restated.py the way libFLAC writes speech: block 4096, LPC order 8 from a
least-squares fit, precision 12, partition order 4, one Rice parameter per partition.  Prints one JSON line."""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
PKG = "matcha-tts-24k_amd"


def clip(seconds: float):
    """``(stream bytes, int16 words)`` of a speech-like signal."""
    import flac_in_restated as fi
    n, bs, shift = int(24000 * seconds), 4096, 10
    t = np.arange(n) / 24000.0
    x = 0.3 * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) * np.sin(2 * np.pi * 180 * t) + 0.1 * np.sin(2 * np.pi * 1900 * t)
    q = np.clip(np.rint((x + 0.002 * np.random.default_rng(0).standard_normal(n)) * 32768), -32768, 32767).astype(np.int64)
    m = min(n - 8, 50000)
    fit = np.linalg.lstsq(np.stack([q[7 - j:7 - j + m] for j in range(8)], axis=1).astype(np.float64), q[8:8 + m].astype(np.float64), rcond=None)[0]
    coefs = np.clip(np.rint(fit * (1 << shift)), -2048, 2047).astype(int)
    frames = [{"samples": q[j:j + bs], "sub": {"kind": "lpc", "coefs": coefs, "precision": 12, "shift": shift, "po": 4 if j + bs <= n else 0}}
              for j in range(0, n, bs)]
    return fi.write_stream(frames, rate=24000)[0], q.astype("<i2")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("a HIP device is required: there is no CPU path, and a CPU time says nothing")
    ac, inf = importlib.import_module(PKG + ".audio_codec"), importlib.import_module(PKG + ".inference")
    data, words = clip(args.seconds)
    B, n = args.batch, words.size
    flac = [ac.read_flac(data) for _ in range(B)]
    pcm = [ac.Encoded(words.tobytes(), "pcm16", 24000) for _ in range(B)]

    def run(clips):
        wave, lengths = inf.recordings(clips, "cuda", None)
        torch.cuda.synchronize()
        return wave, lengths

    (wf, lf), (wp, lp) = run(flac), run(pcm)
    assert lf == lp == [n] * B and torch.equal(wf.view(torch.int32), wp.view(torch.int32)), "FLAC and PCM16 rows differ"
    for _ in range(3):
        run(flac), run(pcm)
    ms = {"flac": [], "pcm16": []}
    for _ in range(args.repeats):
        for name, clips in (("flac", flac), ("pcm16", pcm)):
            t0 = time.perf_counter()
            run(clips)
            ms[name].append((time.perf_counter() - t0) * 1e3)

    def events(call):
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return out

    rows, prow = ac._rows_of_bytes([c.tensor() for c in flac], "cuda"), ac._rows_of_bytes([c.tensor() for c in pcm], "cuda")
    ms["decode_flac"] = events(lambda: ac.decode_flac(rows, [len(data)] * B, ld=n, check=False))
    ms["decode_pcm16"] = events(lambda: ac.decode(prow, [n] * B, "pcm16", check=False, ld=n))
    print(json.dumps({"batch": B, "samples": n, "repeats": args.repeats, "stream_bytes": len(data),
                      "h2d_bytes": {"flac": int(rows.numel()), "pcm16": int(prow.numel())},
                      **{k + "_ms": {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Time the waveform tail of one batcher batch on its own: the per-request loop (Vocos decode on each exact-length mel, peak
normalisation, trim, copy; what MTTS_WAVE_BATCH=0 runs) against `inference.to_waveforms` (ragged decode + finish, one copy).
Host wall time around work that ends in the device-to-host copies, alternated, synthetic Vocos weights and random mels in the
log-mel range; prints one JSON line.

    python tools/wave_tail.py --batch 26 --frames 920 --spread 0.35 --repeats 20
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=26)
    ap.add_argument("--frames", type=int, default=920, help="frames of the longest utterance")
    ap.add_argument("--spread", type=float, default=0.35, help="the shortest utterance is (1 - spread) of the longest")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required")
    inf = importlib.import_module(PKG + ".inference")
    syn = importlib.import_module(PKG + ".synthetic")
    vocoder = inf.load_vocoder("vocos", state_dict=syn.make_vocos_state_dict(seed=11))
    g = torch.Generator().manual_seed(args.seed)
    B, T = args.batch, args.frames
    lens = [T] + [int(T * (1.0 - args.spread * float(torch.rand(1, generator=g)))) for _ in range(B - 1)]
    mel = (torch.randn(B, 100, T, generator=g) * 2.0 - 4.0).cuda()
    lens_dev = torch.tensor(lens).cuda()

    def loop():
        return [inf.trim_trailing_silence(inf._waveform_on_device(mel[b:b + 1, :, :n], vocoder).squeeze()).cpu() for b, n in enumerate(lens)]

    def batched():
        return inf.to_waveforms(mel, lens_dev, vocoder)

    a, b = loop(), batched()                                     # warm-up of every shape, and the agreement of the two
    err = max(float((x - y).abs().max()) if x.numel() else 0.0 for x, y in zip(a, b))
    same_len = all(x.shape == y.shape for x, y in zip(a, b))
    t = {"loop": [], "batched": []}
    for _ in range(args.repeats):
        for name, fn in (("loop", loop), ("batched", batched)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    print(json.dumps({"tool": "wave_tail", "batch": B, "frames_max": T, "frames_total": sum(lens), "frames_padded": B * T,
                      "repeats": args.repeats, "loop_ms_median": round(med["loop"], 3), "batched_ms_median": round(med["batched"], 3),
                      "loop_ms_min": round(min(t["loop"]), 3), "batched_ms_min": round(min(t["batched"]), 3),
                      "same_lengths": same_len, "max_abs_diff": err}))


if __name__ == "__main__":
    main()

"""Time the FLAC stage of the waveform tail (``audio_codec.encode_flac``: three launches) against the PCM16 launch it stands beside
(``audio_codec.encode``) and the Vocos decode it follows, at the benchmark's tail shape: B rows of a 128-token utterance (320 mel
frames, 81,920 samples at 24 kHz) and one such row alone.  Device events around ``--repeats`` calls of each, the three alternated;
the signal is speech-like (a modulated 180 Hz tone, a 1.9 kHz partial, a noise floor), the Vocos weights synthetic.  Also the bytes
each form copies to the host, and the whole tail (``to_waveforms``) by a host clock with ``encoding="pcm16"`` and ``"flac"``.  Prints
one JSON line.  ``--lpc N``: the same table with ``encode_flac(lpc_order=N)`` beside the FIXED call.

    python tools/flac_time.py --batch 32 --repeats 200
    python tools/flac_time.py --batch 32 --repeats 200 --lpc 12
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


def speech_like(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 24000.0
    rows = []
    for b in range(B):
        f0 = 150.0 + 60.0 * float(torch.rand(1, generator=g))
        x = 0.3 * (1 + 0.5 * torch.sin(2 * torch.pi * 3 * t)) * torch.sin(2 * torch.pi * f0 * t) + 0.1 * torch.sin(2 * torch.pi * 1900 * t)
        rows.append((x + 0.002 * torch.randn(L, generator=g, dtype=torch.float64)).float())
    return torch.stack(rows)


def events_ms(fns, repeats):
    """Median milliseconds per call of each function by device events, the functions alternated."""
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}, {k: round(min(v), 4) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--lpc", type=int, default=0, metavar="N", help="also time and size encode_flac(lpc_order=N) beside the FIXED call")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required")
    inf = importlib.import_module(PKG + ".inference")
    syn = importlib.import_module(PKG + ".synthetic")
    ac = importlib.import_module(PKG + ".audio_codec")
    wf = importlib.import_module(PKG + ".waveform")
    vocoder = inf.load_vocoder("vocos", state_dict=syn.make_vocos_state_dict(seed=11))
    model = vocoder.model if hasattr(vocoder, "model") else vocoder
    out = {"tool": "flac_time", "frames": args.frames, "block_size": args.block_size, "repeats": args.repeats, "shapes": {}}
    for B in sorted({args.batch, 1}, reverse=True):
        L = 256 * args.frames
        audio = speech_like(B, L, 7).cuda()
        mel = (torch.randn(B, 100, args.frames, generator=torch.Generator().manual_seed(3)) * 2.0 - 4.0).cuda()
        lens = torch.full((B,), args.frames, dtype=torch.long, device="cuda")
        fns = {"pcm16": lambda: ac.encode(audio, None, "pcm16"), "flac": lambda: ac.encode_flac(audio, None, 24000, block_size=args.block_size),
               "vocos_decode": lambda: model.decode(mel, lens, check=False)}
        if args.lpc:
            fns["flac_lpc"] = lambda: ac.encode_flac(audio, None, 24000, block_size=args.block_size, lpc_order=args.lpc)
        for fn in fns.values():                                    # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        med, least = events_ms(fns, args.repeats)
        data, nbytes = ac.encode_flac(audio, None, 24000, block_size=args.block_size, check=True)
        nbytes = nbytes.tolist()
        tail = {}
        forms = {"pcm16": dict(encoding="pcm16"), "flac": dict(encoding="flac")}
        if args.lpc:
            forms["flac_lpc"] = dict(encoding="flac", flac_lpc=args.lpc)
        for enc in list(forms) * 2:                                # the whole tail, host clock around work that ends in the copies
            wf.tail(mel, lens, vocoder, **forms[enc])                # (to_waveforms is this call; flac_lpc is tail's own option)
            torch.cuda.synchronize()
            ts = []
            for _ in range(max(10, args.repeats // 10)):
                t0 = time.perf_counter()
                wf.tail(mel, lens, vocoder, **forms[enc])
                ts.append((time.perf_counter() - t0) * 1e3)
            tail.setdefault(enc, []).append(round(sorted(ts)[len(ts) // 2], 3))
        out["shapes"][f"B{B}"] = {"samples_per_row": L, "ms_median": med, "ms_min": least, "pcm16_bytes": 2 * L * B, "flac_bytes": sum(nbytes),
                                  "flac_copied_bytes": max(nbytes) * B, "ratio": round(sum(nbytes) / (2 * L * B), 4),
                                  "to_waveforms_ms_median": tail}
        if args.lpc:
            lpc_bytes = ac.encode_flac(audio, None, 24000, block_size=args.block_size, check=True, lpc_order=args.lpc)[1].tolist()
            out["shapes"][f"B{B}"].update(lpc_order=args.lpc, flac_lpc_bytes=sum(lpc_bytes), flac_lpc_copied_bytes=max(lpc_bytes) * B,
                                          lpc_ratio=round(sum(lpc_bytes) / (2 * L * B), 4), lpc_against_fixed=round(sum(lpc_bytes) / sum(nbytes), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

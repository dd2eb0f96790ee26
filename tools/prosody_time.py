"""Time the prosody entries (profiles/r31_prosody.md) beside ``mtts_pitch_track``, by HIP events around the C entries alone (warm,
then the median of ``--repeats`` calls, the entries taking turns inside every repeat so that a busy neighbour hits all alike), on
the batch of tools/pitch_time.py -- 32 clips of 10 s at 24 kHz, default parameters -- and on one such clip: ``mtts_pitch_track``
("yin"), ``mtts_pitch_candidates``, ``mtts_pitch_viterbi``, the two together ("viterbi" as a whole) and ``mtts_pitch_fold`` on 120
tokens per clip with the audio.  Also how often the two trackers differ on these clips.  Prints one JSON line.

    python tools/prosody_time.py [--repeats 20] [--seconds 10]
"""
import argparse
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
PKG = "matcha-tts-24k_amd"
FS = 24000
TOKENS = 120


def main():
    from pitch_time import clip, summary
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required")
    hip = importlib.import_module(PKG + "._hip")
    P = importlib.import_module(PKG + ".pitch")
    lib = hip.load()
    hop, window, min_lag, max_lag = P.plan(FS)
    out = {"tool": "prosody_time", "repeats": args.repeats, "sample_rate": FS, "hop": hop, "max_lag": max_lag, "tokens": TOKENS, "shapes": {}}
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
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="cuda")      # noqa: E731
        f0, aper, frames = new(B, T), new(B, T), new(B, dtype=torch.long)
        f0v, aperv, state = new(B, T), new(B, T), new(B, T, dtype=torch.int8)
        period, mass, depth = new(B, T, 8), new(B, T, 8), new(B, T, 8)
        count, unvoiced, floor = new(B, T, dtype=torch.int32), new(B, T), new(B, T)
        ws = new(lib.mtts_pitch_workspace_bytes(ld, B, FS, hop, 60.0, 500.0), dtype=torch.uint8)
        wsv = new(lib.mtts_pitch_viterbi_workspace_bytes(T, B), dtype=torch.uint8)
        wsf = new(256, dtype=torch.uint8)
        # 120 tokens per clip: equal shares of the clip
        edges = torch.stack([torch.linspace(0, len(r), TOKENS + 1).round().long() for r in rows]).cuda()
        marks = torch.stack([edges[:, :-1], edges[:, 1:]], 2).contiguous()
        x_len = torch.full((B,), TOKENS, dtype=torch.long, device="cuda")
        counts, hz, ms = new(B, TOKENS, 2, dtype=torch.int32), new(B, TOKENS, 3), new(B, TOKENS, dtype=torch.float64)
        s = hip.stream_ptr

        def yin():
            hip.check(lib.mtts_pitch_track(audio.data_ptr(), ld, d_len.data_ptr(), B, FS, hop, 60.0, 500.0, 0.15, f0.data_ptr(), aper.data_ptr(), T,
                                           frames.data_ptr(), ws.data_ptr(), ws.numel(), s()))

        def cands():
            hip.check(lib.mtts_pitch_candidates(audio.data_ptr(), ld, d_len.data_ptr(), B, FS, hop, 60.0, 500.0, 0.15, period.data_ptr(), mass.data_ptr(),
                                                depth.data_ptr(), count.data_ptr(), unvoiced.data_ptr(), floor.data_ptr(), T, frames.data_ptr(),
                                                ws.data_ptr(), ws.numel(), s()))

        def path():
            hip.check(lib.mtts_pitch_viterbi(period.data_ptr(), mass.data_ptr(), depth.data_ptr(), count.data_ptr(), unvoiced.data_ptr(), floor.data_ptr(),
                                             T, frames.data_ptr(), B, FS, 2.0, 0.5, f0v.data_ptr(), aperv.data_ptr(), state.data_ptr(), wsv.data_ptr(),
                                             wsv.numel(), s()))

        def both():
            cands()
            path()

        def fold():
            hip.check(lib.mtts_pitch_fold(f0v.data_ptr(), T, frames.data_ptr(), B, hop, window, max_lag, marks.data_ptr(), TOKENS, x_len.data_ptr(),
                                          audio.data_ptr(), ld, d_len.data_ptr(), counts.data_ptr(), hz.data_ptr(), ms.data_ptr(), wsf.data_ptr(), 256, s()))

        calls = {"mtts_pitch_track": yin, "mtts_pitch_candidates": cands, "mtts_pitch_viterbi": path, "candidates_then_viterbi": both,
                 "mtts_pitch_fold": fold}
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in calls}
        for _ in range(args.repeats):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[key].append((e0, e1))
        torch.cuda.synchronize()
        res = {"rows": B, "samples_per_row": len(rows[0]), "frames_per_row": T, "viterbi_workspace_mb": round(wsv.numel() / 1e6, 2)}
        for key, pairs in ev.items():
            res[key + "_ms"] = summary([a.elapsed_time(b) for a, b in pairs])
        n = int(frames.clamp(min=0).sum())
        live = torch.arange(T, device="cuda")[None] < frames[:, None]
        res["frames"] = n
        res["frames_voiced_yin"] = int(((f0 > 0) & live).sum())
        res["frames_voiced_path"] = int(((f0v > 0) & live).sum())
        res["frames_where_voicing_differs"] = int((((f0 > 0) != (f0v > 0)) & live).sum())
        both_v = (f0 > 0) & (f0v > 0) & live
        res["frames_more_than_50_cents_apart"] = int((both_v & ((1200.0 * torch.log2(f0.clamp(min=1.0) / f0v.clamp(min=1.0))).abs() > 50.0)).sum())
        res["candidates_per_frame_max"] = int(count.max())
        res["tokens_with_a_voiced_frame"] = int((counts[..., 1] > 0).sum())
        out["shapes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Forced alignment of phoneme ids to recordings: per-token durations and the measured scale_correction of a voice.

    python tools/align.py --matcha CKPT --ids-file FILE [--speaker N] [--out align.npz] clip1.wav clip2.wav ...
    python tools/align.py --marks ...                                                     # also when each token is spoken in its clip
    python tools/align.py --marks --pitch ...                                             # and each token's pitch and energy
    python tools/align.py --synthetic 32 [--tokens 128 --frames 1500] [--repeat 200]      # no files: random weights, planted durations

FILE holds one line of whitespace-separated phoneme ids per clip (the phonemiser is outside this package: ``process_text`` of the
reference installation produces them).  Clips are PCM wav at any sample rate, read as tools/enroll.py reads them.  Prints, per clip,
each token's duration in fine frames (hop 128) and milliseconds beside the predictor's, and ``scale_correction`` = aligned total /
predicted total; the .npz holds ``durations``, ``predicted_durations``, ``scale_correction``, ``score``, ``mel_fine_lengths``.

``--synthetic N``: N utterances of ``--tokens`` tokens on random prod-shaped weights; the fine mel is the model's own ``mu_x``
expanded by planted durations (drawn to sum to ``--frames``) plus a little noise; whether the planted durations come back is
reported (on random weights neighbouring tokens can be near-equal).  With ``--repeat R`` the
call ``align(mel_fine=...)`` and the search alone (``HipModel.mas`` on the same ``mu_x`` / mel) are timed with device events after
a warm-up, alternating in one process with a torch-op-loop restatement of the same search on the device (one dependent step per
frame, a few launches each) whose durations must equal the kernel's.  One JSON line with the numbers goes to stdout."""
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
HOP_MS = 128 / 24000 * 1e3


@torch.inference_mode()
def mas_op_loop(lp, x_lengths, y_lengths):
    """The same search written with torch ops on the device, the way a user without the kernel would: lp [B, Tx, Tm] ->
    durations int32 [B, Tx].  One add / maximum / where group per frame forward, one gather group per frame backward."""
    B, Tx, Tm = lp.shape
    neg = torch.tensor(-1e9, device=lp.device)
    xs = torch.arange(Tx, device=lp.device)[None]
    xl, yl = x_lengths[:, None], y_lengths[:, None]
    v = torch.where(xs == 0, lp[:, :, 0], neg)
    came = torch.zeros(B, Tm, Tx, dtype=torch.bool, device=lp.device)
    pad = neg.expand(B, 1)
    for y in range(1, Tm):
        left = torch.cat([pad, v[:, :-1]], 1)
        came[:, y] = left > v
        new = lp[:, :, y] + torch.maximum(v, left)
        inside = (xs >= xl - (yl - y)) & (xs <= y) & (xs < xl)
        v = torch.where((y < yl) & inside, new, torch.where(y < yl, neg, v))
    x = (x_lengths - 1).clone()
    dur = torch.zeros(B, Tx, dtype=torch.int32, device=lp.device)
    one = torch.ones(B, 1, dtype=torch.int32, device=lp.device)
    for y in range(Tm - 1, -1, -1):
        live = y < y_lengths
        dur.scatter_add_(1, x[:, None], one * live[:, None].to(torch.int32))
        if y > 0:
            step = came[:, y].gather(1, x[:, None])[:, 0] & (x > 0) & live
            x = x - step.to(x.dtype)
    return dur


def timed(fn, repeat):
    """Milliseconds per call by device events around ``repeat`` calls (the caller has warmed up)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / repeat


def synthetic_run(args, inf) -> int:
    hparams, synthetic = importlib.import_module(PKG + ".hparams"), importlib.import_module(PKG + ".synthetic")
    dev = torch.device("cuda")
    hp = hparams.prod_v20(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to(dev).eval()
    B, Tx, Tm = args.synthetic, args.tokens, args.frames
    if Tm < Tx:
        raise SystemExit("--frames must be at least --tokens")
    x, x_len, spk = synthetic.make_inputs(hp, B, Tx, seed=1234)
    x, x_len, spk = x.to(dev), x_len.to(dev), spk.to(dev)
    mu_x = model.synthesise(x[:, :Tx], x_len, 1, speaker=spk, debug=True)["mu_x"]
    rng = np.random.default_rng(0)
    planted = np.ones((B, Tx), dtype=np.int64)
    for b in range(B):                                         # Tm frames over Tx tokens, at least one each
        np.add.at(planted[b], rng.integers(0, Tx, size=Tm - Tx), 1)
    d_planted = torch.from_numpy(planted).to(dev)
    y = torch.stack([torch.repeat_interleave(mu_x[b], d_planted[b], dim=1) for b in range(B)])
    y = y + 0.05 * torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y_len = torch.full((B,), Tm, dtype=torch.long, device=dev)
    out = model.align(x, x_len, mel_fine=y, mel_fine_lengths=y_len, speaker=spk)
    hip = model.hip
    lp = hip.mas_logprior(mu_x, y, x_len, y_len)
    loop = mas_op_loop(lp, x_len, y_len)
    res = {"B": B, "Tx": Tx, "Tm": Tm, "repeat": args.repeat,
           "planted_recovered": bool(torch.equal(out["durations"].long(), d_planted)),
           "op_loop_equal": bool(torch.equal(loop, out["durations"])),
           "scale_correction_mean": float(out["scale_correction"].mean())}
    if args.repeat > 1:
        def call_align():
            model.align(x, x_len, mel_fine=y, mel_fine_lengths=y_len, speaker=spk)

        def call_mas():
            hip.mas(x_len, y_len, mu_x=mu_x, y=y, check_lengths=False)

        def call_loop():
            mas_op_loop(lp, x_len, y_len)
        for fn in (call_align, call_mas, call_loop):            # warm-up of every shape the timed window uses
            fn()
        torch.cuda.synchronize()
        loop_rep = max(1, min(args.repeat // 50, 4))
        rounds = {"align_ms": [], "mas_ms": [], "op_loop_ms": []}
        for _ in range(3):                                      # alternate, so a busy neighbour hits all three alike
            rounds["align_ms"].append(timed(call_align, args.repeat))
            rounds["mas_ms"].append(timed(call_mas, args.repeat))
            rounds["op_loop_ms"].append(timed(call_loop, loop_rep))
        for k, vals in rounds.items():
            res[k] = min(vals)
            res[k + "_rounds"] = [round(v, 4) for v in vals]
        res["op_loop_over_mas"] = res["op_loop_ms"] / res["mas_ms"]
        res["note"] = ("align_ms: text encoder + log-prior + search + the status read, per call; mas_ms: log-prior + search "
                       "(3 launches), no host read; op_loop_ms: the torch-op restatement of the search alone on a ready log-prior")
    print(json.dumps(res))
    return 0 if res["op_loop_equal"] else 1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("wavs", nargs="*")
    ap.add_argument("--matcha", help="Matcha checkpoint (Lightning .ckpt or converted directory)")
    ap.add_argument("--ids-file", help="one line of phoneme ids per clip")
    ap.add_argument("--speaker", type=int, default=0)
    ap.add_argument("--out", default="align.npz")
    from enroll import add_silence_argument, silence_of
    add_silence_argument(ap)
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic utterances on random weights instead of files")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--repeat", type=int, default=1, help="time the call this many times per round (synthetic mode)")
    ap.add_argument("--marks", action="store_true", help="also print when each token is spoken in its recording (seconds at 24 kHz; timing.token_marks)")
    ap.add_argument("--pitch", action="store_true", help="with --marks: median / first / last Hz and energy of each token (pitch.track_viterbi, pitch.fold)")
    args = ap.parse_args()
    inf = importlib.import_module(PKG + ".inference")
    if args.synthetic:
        return synthetic_run(args, inf)
    if not (args.matcha and args.ids_file and args.wavs):
        ap.error("give --matcha, --ids-file and at least one wav (or --synthetic N)")
    from enroll import read_wavs
    ids = [[int(t) for t in line.split()] for line in Path(args.ids_file).read_text().splitlines() if line.strip()]
    if len(ids) != len(args.wavs):
        ap.error(f"{args.ids_file} has {len(ids)} lines for {len(args.wavs)} clips")
    model = inf.load_matcha("matcha", args.matcha)
    dev = next(model.parameters()).device
    clips, rates = read_wavs(args.wavs)
    x = torch.zeros(len(ids), max(len(r) for r in ids), dtype=torch.long)
    for b, r in enumerate(ids):
        x[b, :len(r)] = torch.tensor(r)
    x_len = torch.tensor([len(r) for r in ids])
    out = model.align(x.to(dev), x_len.to(dev), audio=clips, speaker=args.speaker, silence=silence_of(args), sample_rate=rates)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for b, path in enumerate(args.wavs):
        n = len(ids[b])
        print(f"[align] {path}: {int(host['mel_fine_lengths'][b])} frames, scale_correction {host['scale_correction'][b]:.4f}")
        for i in range(n):
            d = int(host["durations"][b, i])
            print(f"    token {i:4d} id {ids[b][i]:4d}: {d:4d} frames {d * HOP_MS:8.1f} ms   (predicted {host['predicted_durations'][b, i]:.2f})")
    print(f"[align] scale_correction over {len(ids)} clips: {host['durations'].sum() / host['predicted_durations'].sum():.4f}")
    if args.marks:
        # the marks of a recording: its measured durations through the kernel that marks synthesised audio, keep = the clip's length
        # (with --silence the clip was reshaped on the device: its length is then that of its fine mel)
        tm = importlib.import_module(PKG + ".timing")
        each = rates if isinstance(rates, (list, tuple)) else [rates] * len(clips)
        if silence_of(args) is None:
            keep = [int(round(len(c) * 24000 / int(r))) for c, r in zip(clips, each)]
        else:
            keep = [tm.FINE_HOP * int(v) for v in host["mel_fine_lengths"]]
        cum = torch.cumsum(out["durations"].to(torch.int32), 1).to(torch.int32)
        marks, _, _ = tm.token_marks(cum, x_len, keep)
        folded = None
        if args.pitch:
            # the clips as the alignment saw them (24 kHz, silence reshaped), tracked at the fine-mel hop and folded onto the marks
            pitch = importlib.import_module(PKG + ".pitch")
            wave, n24 = inf.recordings(list(clips), dev, rates, None, silence_of(args))
            tracked = pitch.track_viterbi(wave, n24, 24000, hop=tm.FINE_HOP)
            ends = torch.as_tensor(n24, device=marks.device).long()[:, None, None]     # (with --silence keep is whole frames: not past the clip)
            inside = torch.where(marks >= 0, torch.minimum(marks, ends), marks)
            folded = {k: v.cpu().numpy() for k, v in pitch.fold(tracked, inside, x_len, audio=wave, lengths=n24).items()}
        for b, row in enumerate(tm.marks_rows(marks.cpu())):
            print(f"[align] {args.wavs[b]}: marks")
            for i, (t0, t1) in enumerate(row):
                tail = ""
                if folded is not None:
                    tail = (f"   {folded['median_hz'][b, i]:7.1f} Hz ({folded['first_hz'][b, i]:7.1f} .. {folded['last_hz'][b, i]:7.1f}), "
                            f"{int(folded['voiced'][b, i])}/{int(folded['frames'][b, i])} voiced, {folded['energy_db'][b, i]:6.1f} dB")
                print(f"    token {i:4d} id {ids[b][i]:4d}: {t0:9.4f} s .. {t1:9.4f} s{tail}")
        host["marks"] = marks.cpu().numpy()
        if folded is not None:
            host.update({"token_" + k: v for k, v in folded.items()})
    np.savez(args.out, **host)
    return 0


if __name__ == "__main__":
    sys.exit(main())

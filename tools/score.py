#!/usr/bin/env python3
"""How well does a model, with a voice, explain recordings: duration, prior and flow-matching loss per file.

    python tools/score.py --matcha CKPT --ids-file FILE [--speaker N] [--t-grid 8] [--out score.npz] clip1.wav clip2.wav ...
    python tools/score.py --matcha CKPT --ids-file FILE --style-encoder SE --enroll a.wav b.wav -- clip1.wav ...
    python tools/score.py --synthetic 32 [--tokens 128] [--repeat 20]          # no files: random weights, planted durations

FILE holds one line of whitespace-separated phoneme ids per clip (the phonemiser is outside this package).  Clips are any-rate
PCM wav, read as tools/enroll.py reads them.  The voice is table speaker ``--speaker``, or the row a style encoder gives the
``--enroll`` clips (``MatchaTTSInfer.enroll_voice``).  ``diff_loss`` is averaged over ``--t-grid`` times (k + 0.5) / K with ONE
seeded noise draw, so two voices or two checkpoints are compared on the same estimate.  Prints a table of the three losses per
file (each file's sum over its own count) and the batch figures with the reference's normalisation (matcha/models/matcha_tts.py:
128,145, flow_matching.py:105); the .npz holds every tensor ``MatchaTTSInfer.score`` returns.  A mis-transcribed row shows as an
outlier in ``prior_loss`` and in the MAS score per frame.

``--synthetic N``: N utterances of ``--tokens`` tokens on random prod-shaped weights, the recording built from the model's own
``mu_x`` with 5 frames per token; ``--repeat R`` times the call and prints one JSON line."""
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
sys.path.insert(0, str(ROOT / "tools"))
PKG = "matcha-tts-24k_amd"


def t_grid(k: int, B: int) -> torch.Tensor:
    return ((torch.arange(k, dtype=torch.float32) + 0.5) / k)[:, None].expand(k, B).contiguous()


def synthetic_run(args, inf) -> int:
    hparams, synthetic = importlib.import_module(PKG + ".hparams"), importlib.import_module(PKG + ".synthetic")
    dev = torch.device("cuda")
    hp = hparams.prod_v20(n_spks=2)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.to(dev).eval()
    B, Tx, per = args.synthetic, args.tokens, 5
    x, x_len, spk = synthetic.make_inputs(hp, B, Tx, seed=1234)
    x, x_len, spk = x.to(dev), x_len.to(dev), spk.to(dev)
    mu_x = model.synthesise(x, x_len, 1, speaker=spk, debug=True)["mu_x"]
    g = torch.Generator(device=dev).manual_seed(1)
    y_fine = torch.repeat_interleave(mu_x, per, dim=2)
    y_fine = y_fine + 0.3 * torch.randn(y_fine.shape, device=dev, generator=g)
    y = torch.nn.functional.avg_pool1d(y_fine, 3, 2, 1)
    noise = torch.randn(y.shape, device=dev, generator=g)
    kw = dict(mel=y, mel_fine=y_fine, speaker=spk, t=t_grid(args.t_grid, B), noise=noise)
    out = model.score(x, x_len, **kw)
    res = {"B": B, "Tx": Tx, "Tm": int(y_fine.shape[2]), "t_grid": args.t_grid,
           "planted_recovered": bool((out["durations"] == per).all()),
           "dur_loss": float(out["dur_loss"]), "prior_loss": float(out["prior_loss"]), "diff_loss": float(out["diff_loss"].mean())}
    if args.repeat > 1:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.repeat):
            model.score(x, x_len, **kw)
        torch.cuda.synchronize()
        res["score_ms"] = (time.perf_counter() - t0) * 1e3 / args.repeat
    print(json.dumps(res))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("wavs", nargs="*")
    ap.add_argument("--matcha", help="Matcha checkpoint (Lightning .ckpt or converted directory)")
    ap.add_argument("--ids-file", help="one line of phoneme ids per clip")
    ap.add_argument("--speaker", type=int, default=0)
    ap.add_argument("--style-encoder", help="style-encoder checkpoint: score under the voice of the --enroll clips")
    ap.add_argument("--enroll", nargs="+", default=[], help="clips of the voice to enrol (needs --style-encoder)")
    ap.add_argument("--t-grid", type=int, default=8, help="flow-matching times per file")
    ap.add_argument("--seed", type=int, default=0, help="seed of the one noise draw")
    ap.add_argument("--out", default="score.npz")
    from enroll import add_silence_argument, silence_of
    add_silence_argument(ap)
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic utterances on random weights instead of files")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=1, help="time the call this many times (synthetic mode)")
    args = ap.parse_args()
    if args.t_grid < 1:
        ap.error("--t-grid must be at least 1")
    inf = importlib.import_module(PKG + ".inference")
    if args.synthetic:
        return synthetic_run(args, inf)
    if not (args.matcha and args.ids_file and args.wavs):
        ap.error("give --matcha, --ids-file and at least one wav (or --synthetic N)")
    if bool(args.enroll) != bool(args.style_encoder):
        ap.error("--enroll and --style-encoder go together")
    from enroll import read_wavs
    ids = [[int(t) for t in line.split()] for line in Path(args.ids_file).read_text().splitlines() if line.strip()]
    if len(ids) != len(args.wavs):
        ap.error(f"{args.ids_file} has {len(ids)} lines for {len(args.wavs)} clips")
    model = inf.load_matcha("matcha", args.matcha)
    dev = next(model.parameters()).device
    voice = {"speaker": args.speaker}
    if args.enroll:
        style = importlib.import_module(PKG + ".style")
        enrol_clips, enrol_rates = read_wavs(args.enroll)
        voice = {"speaker_embeddings": model.enroll_voice(enrol_clips, style.load_style_encoder(args.style_encoder), silence=silence_of(args),
                                                                 sample_rate=enrol_rates)}
    clips, rates = read_wavs(args.wavs)
    silence = silence_of(args)
    if silence is not None:                    # here, not as score(silence=...): the noise below is drawn for the normalised lengths
        wave, kept = inf.recordings(clips, dev, rates, silence=silence)
        clips, rates = [wave[b, :n] for b, n in enumerate(kept)], [24000] * len(kept)
    B = len(ids)
    x = torch.zeros(B, max(len(r) for r in ids), dtype=torch.long)
    for b, r in enumerate(ids):
        x[b, :len(r)] = torch.tensor(r)
    x_len = torch.tensor([len(r) for r in ids])
    T = inf.fix_len_compatibility(max(-(-24000 * c.numel() // r) // inf.STD_RES_HOP_LENGTH + 1 for c, r in zip(clips, rates)))
    noise = torch.randn(B, model.hp.n_feats, T, generator=torch.Generator().manual_seed(args.seed))
    out = model.score(x.to(dev), x_len.to(dev), audio=clips, t=t_grid(args.t_grid, B), noise=noise.to(dev), sample_rate=rates, **voice)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    diff = host["diff_loss_per_utterance"].mean(0)
    print(f"{'file':40s} {'frames':>7s} {'dur_loss':>10s} {'prior_loss':>11s} {'diff_loss':>10s} {'mas/frame':>10s}")
    for b, path in enumerate(args.wavs):
        frames = int(host["mel_fine_lengths"][b])
        print(f"{Path(path).name[:40]:40s} {frames:7d} {host['dur_loss_per_utterance'][b]:10.5f} {host['prior_loss_per_utterance'][b]:11.5f} "
              f"{diff[b]:10.5f} {host['mas_score'][b] / frames:10.3f}")
    print(f"{'batch (reference normalisation)':40s} {int(host['mel_fine_lengths'].sum()):7d} {float(host['dur_loss']):10.5f} "
          f"{float(host['prior_loss']):11.5f} {float(host['diff_loss'].mean()):10.5f}")
    np.savez(args.out, **host)
    return 0


if __name__ == "__main__":
    sys.exit(main())

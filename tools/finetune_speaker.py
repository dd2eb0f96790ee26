#!/usr/bin/env python3
"""Fine-tune one voice's two speaker rows on its recordings, on the device (``MatchaTTSInfer.finetune_speaker``).

    python tools/finetune_speaker.py --matcha CKPT --ids-file FILE [--speaker N | --voice voice.npz] [--steps 200] [--lr 5e-5]
                                     [--batch-size 16] [--out voice_ft] clip1.wav clip2.wav ...
    python tools/finetune_speaker.py --synthetic-model tiny --ids-file FILE clip1.wav ...      # random weights (trials, tests)

FILE holds one line of whitespace-separated phoneme ids per clip (the phonemiser is outside this package).  Clips are any-rate
PCM wav, read as tools/enroll.py reads them.  The start is table speaker ``--speaker`` or the rows of a ``--voice`` file (the .npz
of tools/enroll.py: ``e_enc``, ``e_dur``).  What is trained and how follows the reference's matcha/finetune_speaker.py: everything
frozen but the two rows, Adam on the duration + prior loss, alignment searched anew every step; dropout is off here and the
flow-matching loss, which cannot move the rows, is not evaluated.  Prints the loss history and writes ``OUT_enc.npy`` and
``OUT_dur.npy`` ([spk_emb_dim] each): the rows for ``synthesise(speaker_embeddings=...)``, a batcher request or ``add_speaker``."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
PKG = "matcha-tts-24k_amd"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("wavs", nargs="+")
    ap.add_argument("--matcha", help="Matcha checkpoint (Lightning .ckpt or converted directory)")
    ap.add_argument("--synthetic-model", choices=["tiny", "prod"], help="random weights of that architecture instead of --matcha")
    ap.add_argument("--ids-file", required=True, help="one line of phoneme ids per clip")
    ap.add_argument("--speaker", type=int, default=0, help="table row to start from")
    ap.add_argument("--voice", help=".npz with e_enc / e_dur to start from (tools/enroll.py)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--batch-size", type=int, default=0, help="utterances per step (0: all)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the batch order")
    ap.add_argument("--print-every", type=int, default=10)
    ap.add_argument("--out", default="voice_ft", help="prefix of the two .npy files")
    from enroll import add_silence_argument, silence_of
    add_silence_argument(ap)
    args = ap.parse_args()
    if bool(args.matcha) == bool(args.synthetic_model):
        ap.error("give either --matcha or --synthetic-model")
    inf = importlib.import_module(PKG + ".inference")
    from enroll import read_wavs
    ids = [[int(t) for t in line.split()] for line in Path(args.ids_file).read_text().splitlines() if line.strip()]
    if len(ids) != len(args.wavs):
        ap.error(f"{args.ids_file} has {len(ids)} lines for {len(args.wavs)} clips")
    if args.synthetic_model:
        hparams, synthetic = importlib.import_module(PKG + ".hparams"), importlib.import_module(PKG + ".synthetic")
        hp = hparams.tiny(n_spks=2) if args.synthetic_model == "tiny" else hparams.prod_v20(n_spks=2)
        model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        model.load_state_dict(synthetic.make_state_dict(hp, seed=7, duration_recipe=False), strict=True)
        model = model.to("cuda").eval()
    else:
        model = inf.load_matcha("matcha", args.matcha)
    dev = next(model.parameters()).device
    start = {"speaker": args.speaker}
    if args.voice:
        v = np.load(args.voice)
        start = {"speaker_embeddings": (torch.from_numpy(v["e_enc"]).to(dev), torch.from_numpy(v["e_dur"]).to(dev))}
    clips, rates = read_wavs(args.wavs)
    B = len(ids)
    x = torch.zeros(B, max(len(r) for r in ids), dtype=torch.long)
    for b, r in enumerate(ids):
        x[b, :len(r)] = torch.tensor(r)
    x_len = torch.tensor([len(r) for r in ids])
    e_enc, e_dur, history = model.finetune_speaker(x.to(dev), x_len.to(dev), audio=clips, steps=args.steps, lr=args.lr,
                                                   batch_size=args.batch_size or None, shuffle_seed=args.seed, silence=silence_of(args), sample_rate=rates, **start)
    print(f"{'step':>6s} {'dur_loss':>10s} {'prior_loss':>11s}")
    every = max(args.print_every, 1)
    for k, (d, p) in enumerate(zip(history["dur_loss"], history["prior_loss"])):
        if k % every == 0 or k == len(history["dur_loss"]) - 1:
            print(f"{k:6d} {d:10.5f} {p:11.5f}")
    np.save(args.out + "_enc.npy", e_enc[0].cpu().numpy())
    np.save(args.out + "_dur.npy", e_dur[0].cpu().numpy())
    print(f"[finetune_speaker] {B} clips, {args.steps} steps -> {args.out}_enc.npy, {args.out}_dur.npy")
    return 0


if __name__ == "__main__":
    sys.exit(main())

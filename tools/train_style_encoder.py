#!/usr/bin/env python3
"""Train the style encoder on a prepared corpus, on the device (``style.StyleTrainer``).

    python tools/train_style_encoder.py --matcha CKPT --ids-file FILE [--style DIR] [--epochs 1] [--batch-size 32] [--lr 1e-4]
                                        [--out style_encoder_trained] MEL_DIR
    python tools/train_style_encoder.py --synthetic-model tiny --ids-file FILE MEL_DIR         # random weights (trials, tests)

MEL_DIR is what ``tools/prepare_corpus.py mels`` wrote: ``<rel>.fine.npy`` per clip, the normalised fine mel [n_mels, T].  FILE
holds one line per clip: ``<rel> <speaker id> <phoneme id> <phoneme id> ...``, whitespace-separated (the phonemiser is outside
this package); the speaker id is the row of the Matcha checkpoint's speaker tables whose voice the clip is.  What is trained and how
follows the reference's matcha/models/style_encoder.py:75-160: Matcha frozen in eval(), the text encoder's outputs under the predicted
rows matched against those under the real rows with smooth-L1, AdamW (configs/model/optimizer/adamw.yaml) on every style parameter.
``--style`` continues from a converted style encoder (``checkpoint.convert_style_checkpoint`` or an earlier ``--out``); without it
the encoder starts from torch's default initialisation with ``--seed``.  Prints the loss history and writes ``--out``: the directory
``style.load_style_encoder`` (and so ``enroll_voice``) reads, with the optimiser state beside the weights."""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "matcha-tts-24k_amd"


def read_rows(ids_file):
    rows = []
    for line in Path(ids_file).read_text().splitlines():
        f = line.split()
        if not f:
            continue
        if len(f) < 3:
            raise ValueError(f"{ids_file}: a line needs a clip, a speaker id and at least one phoneme id: {line!r}")
        rows.append((f[0], int(f[1]), [int(t) for t in f[2:]]))
    return rows


def batches_of(rows, mel_dir, batch_size, n_feats):
    """Padded batches in file order: (x, x_lengths, mel_fine, mel_fine_lengths, spks) on the host."""
    for at in range(0, len(rows), batch_size):
        part = rows[at:at + batch_size]
        mels = [np.load(Path(mel_dir) / (rel + ".fine.npy")) for rel, _, _ in part]
        for (rel, _, _), m in zip(part, mels):
            if m.ndim != 2 or m.shape[0] != n_feats:
                raise ValueError(f"{rel}.fine.npy has shape {m.shape}, expected ({n_feats}, T)")
        x = torch.zeros(len(part), max(len(ids) for _, _, ids in part), dtype=torch.long)
        mel = torch.zeros(len(part), n_feats, max(m.shape[1] for m in mels))
        for b, ((_, _, ids), m) in enumerate(zip(part, mels)):
            x[b, :len(ids)] = torch.tensor(ids)
            mel[b, :, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
        yield (x, torch.tensor([len(ids) for _, _, ids in part]), mel, torch.tensor([m.shape[1] for m in mels]),
               torch.tensor([spk for _, spk, _ in part]))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mel_dir")
    ap.add_argument("--matcha", help="Matcha checkpoint (Lightning .ckpt or converted directory)")
    ap.add_argument("--synthetic-model", choices=["tiny", "prod"], help="random weights of that architecture instead of --matcha")
    ap.add_argument("--ids-file", required=True, help="one line per clip: <rel> <speaker id> <phoneme ids ...>")
    ap.add_argument("--style", help="converted style encoder to continue from")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=0, help="stop after this many steps (0: all epochs)")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0, help="seed of the initialisation")
    ap.add_argument("--print-every", type=int, default=10)
    ap.add_argument("--out", default="style_encoder_trained")
    args = ap.parse_args()
    if bool(args.matcha) == bool(args.synthetic_model):
        ap.error("give either --matcha or --synthetic-model")
    inf, style = importlib.import_module(PKG + ".inference"), importlib.import_module(PKG + ".style")
    if args.synthetic_model:
        hparams, synthetic = importlib.import_module(PKG + ".hparams"), importlib.import_module(PKG + ".synthetic")
        hp = hparams.tiny(n_spks=2) if args.synthetic_model == "tiny" else hparams.prod_v20(n_spks=2)
        model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        model.load_state_dict(synthetic.make_state_dict(hp, seed=7, duration_recipe=False), strict=True)
        model = model.to("cuda").eval()
    else:
        model = inf.load_matcha("matcha", args.matcha)
    hp = model.hp
    if args.style:
        enc = style.load_style_encoder(args.style)
    else:
        torch.manual_seed(args.seed)
        enc = style.StyleEncoder(hp.n_feats, args.hidden, args.layers, hp.spk_emb_dim).to("cuda").eval()
    rows = read_rows(args.ids_file)
    if not rows:
        ap.error(f"{args.ids_file} names no clip")
    trainer = style.StyleTrainer(model, enc, lr=args.lr, weight_decay=args.weight_decay)
    batches = list(batches_of(rows, args.mel_dir, max(args.batch_size, 1), hp.n_feats))
    if args.max_steps:
        plan = [batches[i % len(batches)] for i in range(min(args.max_steps, args.epochs * len(batches)))]
        history = trainer.fit(plan, 1)
    else:
        history = trainer.fit(batches, args.epochs)
    print(f"{'step':>6s} {'acoustic':>11s} {'rhythm':>11s} {'dist_enc':>10s} {'dist_dur':>10s}")
    n, every = len(history["acoustic_loss"]), max(args.print_every, 1)
    for k in range(n):
        if k % every == 0 or k == n - 1:
            print(f"{k:6d} {history['acoustic_loss'][k]:11.6f} {history['rhythm_loss'][k]:11.6f} {history['emb_dist_enc'][k]:10.5f} "
                  f"{history['emb_dist_dur'][k]:10.5f}")
    out = trainer.save(args.out)
    print(f"[train_style_encoder] {len(rows)} clips, {n} steps -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

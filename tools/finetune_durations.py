#!/usr/bin/env python3
"""Train the duration predictor on recordings, on the device (``duration.DurationTrainer``), everything else frozen.

    python tools/finetune_durations.py --matcha CKPT --ids-file FILE [--speaker N | --voice voice.npz] [--epochs 10] [--lr 5e-5]
                                       [--batch-size 16] [--out durations_ft] clip1.wav clip2.fine.npy ...
    python tools/finetune_durations.py --synthetic-model tiny --ids-file FILE clip1.wav ...      # random weights (trials, tests)

FILE holds one line of whitespace-separated phoneme ids per clip (the phonemiser is outside this package).  A clip is an any-rate
PCM wav, read as tools/enroll.py reads them, or a ``.fine.npy`` cache of ``tools/prepare_corpus.py mels`` (the normalised fine mel
[n_mels, T]).  The voice is table speaker ``--speaker`` or the rows of a ``--voice`` file (the .npz of tools/enroll.py).  The clips
are aligned ONCE with the model as it is (``model.align``: the reference searches the alignment under no_grad, and the predictor does
not take part in it), the durations are cached in ``OUT/durations.npz`` and reused by a later run, the predictor is trained for
``--epochs`` passes with AdamW in the reference's two parameter groups, and the tensors are written to ``OUT`` (safetensors under
their state-dict keys, plus the optimiser state).  Dropout is off here; the reference trains the predictor with dropout."""
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


def align_all(model, x, x_len, paths, voice, silence, dev):
    """Durations int32 [N, Tx] of every clip: the wavs in one ``align`` call, the mel caches in another."""
    from enroll import read_wavs
    N, Tx = x.shape
    dur = torch.zeros(N, Tx, dtype=torch.int32)
    wav = [i for i, p in enumerate(paths) if not p.endswith(".fine.npy")]
    npy = [i for i, p in enumerate(paths) if p.endswith(".fine.npy")]
    if wav:
        clips, rates = read_wavs([paths[i] for i in wav])
        out = model.align(x[wav].to(dev), x_len[wav].to(dev), audio=clips, sample_rate=rates, silence=silence, **voice)
        dur[wav] = out["durations"].cpu()
    if npy:
        mels = [np.load(paths[i]) for i in npy]
        T = max(m.shape[1] for m in mels)
        fine = torch.zeros(len(npy), mels[0].shape[0], T)
        for k, m in enumerate(mels):
            fine[k, :, :m.shape[1]] = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
        lens = torch.tensor([m.shape[1] for m in mels])
        out = model.align(x[npy].to(dev), x_len[npy].to(dev), mel_fine=fine.to(dev), mel_fine_lengths=lens.to(dev), **voice)
        dur[npy] = out["durations"].cpu()
    return dur


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("clips", nargs="+", help="wav files or .fine.npy mel caches")
    ap.add_argument("--matcha", help="Matcha checkpoint (Lightning .ckpt or converted directory)")
    ap.add_argument("--synthetic-model", choices=["tiny", "prod"], help="random weights of that architecture instead of --matcha")
    ap.add_argument("--ids-file", required=True, help="one line of phoneme ids per clip")
    ap.add_argument("--speaker", type=int, default=0, help="table row of the voice")
    ap.add_argument("--voice", help=".npz with e_enc / e_dur of the voice (tools/enroll.py)")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--batch-size", type=int, default=0, help="utterances per step (0: all)")
    ap.add_argument("--print-every", type=int, default=10)
    ap.add_argument("--out", default="durations_ft", help="output directory")
    from enroll import add_silence_argument, silence_of
    add_silence_argument(ap)
    args = ap.parse_args()
    if bool(args.matcha) == bool(args.synthetic_model):
        ap.error("give either --matcha or --synthetic-model")
    inf = importlib.import_module(PKG + ".inference")
    duration = importlib.import_module(PKG + ".duration")
    ids = [[int(t) for t in line.split()] for line in Path(args.ids_file).read_text().splitlines() if line.strip()]
    if len(ids) != len(args.clips):
        ap.error(f"{args.ids_file} has {len(ids)} lines for {len(args.clips)} clips")
    if args.synthetic_model:
        hparams, synthetic = importlib.import_module(PKG + ".hparams"), importlib.import_module(PKG + ".synthetic")
        hp = hparams.tiny(n_spks=2) if args.synthetic_model == "tiny" else hparams.prod_v20(n_spks=2)
        model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        model.load_state_dict(synthetic.make_state_dict(hp, seed=7, duration_recipe=False), strict=True)
        model = model.to("cuda").eval()
    else:
        model = inf.load_matcha("matcha", args.matcha)
    dev = next(model.parameters()).device
    voice = {"speaker": args.speaker}
    if args.voice:
        v = np.load(args.voice)
        voice = {"speaker_embeddings": (torch.from_numpy(v["e_enc"]).to(dev).reshape(1, -1), torch.from_numpy(v["e_dur"]).to(dev).reshape(1, -1))}
    N = len(ids)
    x = torch.zeros(N, max(len(r) for r in ids), dtype=torch.long)
    for b, r in enumerate(ids):
        x[b, :len(r)] = torch.tensor(r)
    x_len = torch.tensor([len(r) for r in ids])
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    cache = out / "durations.npz"
    dur = None
    if cache.exists():
        c = np.load(cache)
        if c["durations"].shape == tuple(x.shape) and np.array_equal(c["x"], x.numpy()):
            dur = torch.from_numpy(c["durations"])
            print(f"[finetune_durations] durations read from {cache}")
    if dur is None:
        dur = align_all(model, x, x_len, list(args.clips), voice, silence_of(args), dev)
        np.savez(cache, durations=dur.numpy(), x=x.numpy(), x_lengths=x_len.numpy())
    trainer = duration.DurationTrainer(model, lr=args.lr, weight_decay=args.weight_decay)
    bs = args.batch_size or N
    batches = []
    for at in range(0, N, bs):
        sel = slice(at, at + bs)
        n = int(x_len[sel].max())
        batches.append(dict(x=x[sel, :n].contiguous(), x_lengths=x_len[sel], durations=dur[sel, :n].contiguous(), **voice))
    history = trainer.fit(batches, epochs=args.epochs)["dur_loss"]
    print(f"{'step':>6s} {'dur_loss':>10s}")
    every = max(args.print_every, 1)
    for k, d in enumerate(history):
        if k % every == 0 or k == len(history) - 1:
            print(f"{k:6d} {d:10.5f}")
    trainer.save(out)
    print(f"[finetune_durations] {N} clips, {len(history)} steps -> {out / duration.DURATION_WEIGHTS}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

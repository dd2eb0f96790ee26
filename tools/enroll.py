#!/usr/bin/env python3
"""Enrol a voice from wav files: clips -> (e_enc, e_dur) speaker rows, the reference's matcha/add_speaker.py on the device.

    python tools/enroll.py --matcha CKPT --style-encoder CKPT_OR_DIR --out voice.npz clip1.wav clip2.wav ...
    python tools/enroll.py --synthetic 10          # ten synthetic 5 s clips on random weights (profiling / smoke, no files needed)
    python tools/enroll.py ... --silence 0.2 0.8   # first give every clip exactly 0.2 s / 0.8 s of leading / trailing silence

Clips are PCM wav (8 / 16 / 32 bit) at any sample rate, read with the standard library's ``wave`` module; of a multi-channel file
channel 0 is used (the reference's ``audio[0]``), and clips that are not at 24 kHz are converted on the device.  The output .npz
holds ``e_enc`` and ``e_dur`` ([spk_emb_dim] each): pass them as ``synthesise(speaker_embeddings=...)``, as a batcher
request's ``speaker_embedding``, or to ``MatchaTTSInfer.add_speaker``."""
import argparse
import importlib
import sys
import wave
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "matcha-tts-24k_amd"


def read_wav(path):
    """``(samples: 1-D float32 tensor in [-1, 1], sample rate)`` of a PCM wav file; channel 0 of a multi-channel file.  A file whose
    format the stdlib ``wave`` module refuses (G.711 mu-law / A-law: "unknown format: 7") is read by ``audio_codec.read_wav`` and
    comes back as an ``Encoded`` clip, still bytes, which the model's recording entries decode on the device; so does a FLAC file
    (one that starts with ``fLaC``), as an ``audio_codec.FlacClip``."""
    with open(str(path), "rb") as f:
        if f.read(4) == b"fLaC":
            clip = importlib.import_module(PKG + ".audio_codec").read_flac(path)
            return clip, int(clip.sample_rate)
    try:
        with wave.open(str(path), "rb") as w:
            rate, channels = w.getframerate(), w.getnchannels()
            width, raw = w.getsampwidth(), w.readframes(w.getnframes())
    except wave.Error as e:
        if "unknown format" not in str(e):
            raise
        enc = importlib.import_module(PKG + ".audio_codec").read_wav(path)
        return enc, int(enc.sample_rate)
    if width == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError(f"{path}: unsupported PCM sample width {width}")
    return torch.from_numpy(a[::channels].copy()), int(rate)


def read_wavs(paths):
    """``(clips, rates)`` of several files, as the ``audio=`` / ``sample_rate=`` arguments of the model's methods take them."""
    pairs = [read_wav(p) for p in paths]
    return [c for c, _ in pairs], [r for _, r in pairs]


def add_silence_argument(ap) -> None:
    ap.add_argument("--silence", nargs=2, metavar=("LEAD", "TRAIL"),
                    help="normalise every clip's leading / trailing silence to exactly these seconds (multiples of 0.01; 'none' leaves "
                         "that end as it is) on the device before the mel front end, as the reference's normalize_silence.py does to its corpus")


def silence_of(args):
    """``--silence LEAD TRAIL`` as the ``silence=`` argument of the model's methods (None without the option)."""
    if not args.silence:
        return None
    return tuple(None if v.lower() == "none" else float(v) for v in args.silence)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("wavs", nargs="*")
    ap.add_argument("--matcha", help="Matcha checkpoint (Lightning .ckpt or converted directory): supplies mel_mean / mel_std")
    ap.add_argument("--style-encoder", help="style-encoder checkpoint (.ckpt or converted directory)")
    ap.add_argument("--out", default="voice.npz")
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic 5 s clips on random weights instead of files")
    ap.add_argument("--repeat", type=int, default=1, help="run the enrolment this many times (profiling)")
    add_silence_argument(ap)
    args = ap.parse_args()
    inf = importlib.import_module(PKG + ".inference")
    style = importlib.import_module(PKG + ".style")
    if args.synthetic:
        hparams, synthetic = importlib.import_module(PKG + ".hparams"), importlib.import_module(PKG + ".synthetic")
        hp = hparams.prod_v20(n_spks=2)
        model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
        model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
        model = model.to("cuda").eval()
        torch.manual_seed(0)
        enc = style.StyleEncoder(**style.DEFAULT_CFG).to("cuda").eval()
        t = torch.arange(5 * 24000, dtype=torch.float32) / 24000.0
        clips = [(0.4 * torch.sin(2 * np.pi * (120.0 + 20.0 * i) * t) + 0.05 * torch.randn(t.numel())).clamp(-1, 1) for i in range(args.synthetic)]
        rates = 24000
    else:
        if not (args.matcha and args.style_encoder and args.wavs):
            ap.error("give --matcha, --style-encoder and at least one wav (or --synthetic N)")
        model = inf.load_matcha("matcha", args.matcha)
        enc = style.load_style_encoder(args.style_encoder)
        clips, rates = read_wavs(args.wavs)
    for _ in range(max(args.repeat, 1)):
        e_enc, e_dur = model.enroll_voice(clips, enc, silence=silence_of(args), sample_rate=rates)
    torch.cuda.synchronize()
    np.savez(args.out, e_enc=e_enc[0].cpu().numpy(), e_dur=e_dur[0].cpu().numpy())
    print(f"[enroll] {len(clips)} clips -> {args.out}: e_enc |max| {e_enc.abs().max().item():.4f}, e_dur |max| {e_dur.abs().max().item():.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

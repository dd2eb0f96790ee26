#!/usr/bin/env python3
"""A text longer than one utterance to one wav file: sentences as rows of one ragged batch, joined on the device.

    python tools/speak_long.py speak --matcha CKPT --vocos CKPT TEXT.txt OUT.wav [--voice 0 --speed 1.0 --steps 4 --sample-rate 24000 --loudness LUFS --true-peak DB]
    python tools/speak_long.py speak --matcha CKPT --vocos CKPT --segments-file FILE OUT.wav
    python tools/speak_long.py time [--sentences 20 --tokens 100 --repeat 10] [--utterance | --kernels]     # random weights, no files

``speak`` cuts TEXT.txt with ``longform.split_text`` and phonemizes each sentence with the reference installation's phonemizer
(``process_text``) when that imports.  Where it does not, ``--segments-file`` takes the text already cut and phonemized: one
segment per line, whitespace-separated phoneme ids, then ``|`` and the pause behind it in milliseconds (``12 7 33 | 300``), as
tools/align.py takes ids.  The document goes through ``FrameBudgetBatcher.submit_document``; OUT.wav is RIFF PCM16 (an OUT.flac: FLAC) at
``--sample-rate``, encoded on the device.  ``--captions FILE.vtt|.srt`` writes one cue per sentence from the result's ``segments``;
``--marks FILE.json`` writes when each token (and, with the phonemizer here, each word) is spoken, in seconds of the 24 kHz join.  ``--loudness LUFS`` brings the joined document to that integrated loudness (ITU-R BS.1770,
one gain for the document, the sample peak held at 0.95) on the device, ahead of the rate conversion.  The sentences' times are printed.

``time``: a document of ``--sentences`` sentences of about ``--tokens`` tokens on random prod-shaped weights (a text of about
sentences x tokens characters), timed per call with a host clock around calls that end in the result on the host, alternating
  document   one ``submit_document`` (PCM16 encoded on the device), with
  separate   what a caller does without it: the same sentences as separate requests of one batch, the waveforms joined with
             the same pauses and encoded to PCM16 on the host (NumPy), and, with ``--utterance`` and up to 4000 tokens,
  utterance  all the tokens as ONE utterance (informational: another computation, quadratic in frames).
``--kernels`` instead runs ``inference.join_waveforms`` alone on the two shapes of profiles/r18_longform.md (for a kernel trace)
and prints the bytes the join has to move.  One JSON line with the numbers goes to stdout."""
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
PKG = "matcha-tts-24k_amd"


def sub(name):
    return importlib.import_module(f"{PKG}.{name}")


def read_segments(path):
    """``--segments-file``: [(ids, pause_ms)]."""
    out = []
    for n, line in enumerate(Path(path).read_text().splitlines(), 1):
        if not line.strip():
            continue
        ids, _, pause = line.partition("|")
        try:
            out.append(([int(v) for v in ids.split()], float(pause) if pause.strip() else 0.0))
        except ValueError as e:
            raise SystemExit(f"{path}:{n}: expected 'id id id ... | pause_ms' ({e})")
    return out


def speak(args) -> int:
    inf, bt, sv, AC = sub("inference"), sub("batcher"), sub("serving"), sub("audio_codec")
    if (args.text is None) == (args.segments_file is None):
        raise SystemExit("give TEXT.txt or --segments-file FILE (one of them)")
    model = inf.load_matcha("matcha", args.matcha)
    vocoder = inf.load_vocoder("vocos", checkpoint=args.vocos)
    p = sv.request_params(args.voice, args.speed, args.steps, args.solver)
    if args.segments_file is not None:
        pieces = read_segments(args.segments_file)
        ids, pauses = [s for s, _ in pieces], [ms for _, ms in pieces]
        texts, groups = [f"segment {n + 1}" for n in range(len(ids))], None
    else:
        try:
            inf.process_text("test", p.language)
        except RuntimeError as e:
            raise SystemExit(f"{e}\n(no phonemizer here: cut and phonemize elsewhere and pass --segments-file)")
        pieces = sub("longform").split_text(Path(args.text).read_text(), max_chars=args.max_chars, language=p.language)
        spoken = [inf.process_text(s, p.language) for s, _ in pieces]
        ids = [r["x_phone_ids"] for r in spoken]
        pauses = [ms for _, ms in pieces]
        texts = [s for s, _ in pieces]
        # one symbol per id: the words are the runs between the phonemizer's spaces
        groups = [sub("timing").word_groups(list(r["x_phones"])) if len(r["x_phones"]) == len(r["x_phone_ids"]) else None for r in spoken]
        groups = groups if all(g is not None for g in groups) else None
    if not ids:
        raise SystemExit("nothing to speak")
    extra = {} if args.loudness is None else {"loudness": args.loudness}
    if args.true_peak is not None:
        if args.loudness is None:
            raise SystemExit("--true-peak limits the gain towards --loudness: name a target too")
        extra["true_peak"] = args.true_peak
    if args.captions is not None and Path(args.captions).suffix.lower() not in (".vtt", ".srt"):
        raise SystemExit("--captions writes WebVTT (.vtt) or SubRip (.srt)")
    if args.marks is not None:
        extra["marks"] = True
        if groups is not None:
            extra["word_groups"] = groups
    flac = Path(args.out).suffix.lower() == ".flac"                   # OUT.flac: the document as one FLAC stream, encoded on the device
    if args.flac_lpc:
        if not flac:
            raise SystemExit("--flac-lpc belongs to an OUT.flac")
        extra["flac_lpc"] = args.flac_lpc
    with bt.FrameBudgetBatcher(model, max_batch=max(32, len(ids)), max_tokens=max(8192, len(ids) * max(len(s) for s in ids)),
                               vocoder=vocoder, fade_ms=args.fade_ms) as q:
        res = q.submit_document(ids, pauses, speaker=p.speaker, voice_mix=p.voice_mix, solver=p.solver, n_timesteps=p.n_timesteps,
                                scale_correction=p.scale_correction, length_scale=p.length_scale, sample_rate=args.sample_rate,
                                encoding="flac" if flac else "pcm16", level=args.level, **extra).result()
    Path(args.out).write_bytes(sv.response_body(res, "flac" if flac else "wav", args.sample_rate))
    for n, (t0, t1) in enumerate(res["segments"]):
        print(f"{n:4d}  {t0:9.3f} s .. {t1:9.3f} s")
    if args.captions is not None:
        tm = sub("timing")
        cues = [(t0, t1, text) for (t0, t1), text in zip(res["segments"], texts)]
        Path(args.captions).write_text(tm.webvtt(cues) if Path(args.captions).suffix.lower() == ".vtt" else tm.srt(cues))
        print(f"wrote {args.captions}: {len(cues)} cues")
    if args.marks is not None:
        Path(args.marks).write_text(json.dumps({"sample_rate": 24000, "sentences": texts, "segments": res["segments"], **res["marks"]}))
        print(f"wrote {args.marks}: marks of {sum(len(t) for t in res['marks']['tokens'])} tokens")
    if "loudness" in res:
        print(f"loudness {res['loudness']:.2f} LUFS as synthesised, gain {res['gain']:.4f} towards {args.loudness:.2f} LUFS")
    if "true_peak" in res:
        print(f"true peak {res['true_peak']:.2f} dBTP as synthesised (ceiling {args.true_peak:.2f} dBTP), loudness range {res['lra']:.2f} LU")
    size = f"{res['audio'].numel()} bytes of FLAC" if flac else f"{res['audio'].numel() // 2} samples"
    print(f"wrote {args.out}: {size} at {args.sample_rate} Hz, {len(ids)} sentences")
    return 0


def host_join_pcm16(waves, gaps):
    """What a caller does without the device join: concatenate with silences, then s16le as every reader of this project scales it."""
    parts = []
    for n, w in enumerate(waves):
        parts.append(w.numpy())
        if n + 1 < len(waves):
            parts.append(np.zeros(gaps[n], dtype=np.float32))
    y = np.concatenate(parts) * np.float32(32768.0)
    return np.clip(np.rint(y), -32768, 32767).astype("<i2").tobytes()


def clock(fn, repeat):
    """Milliseconds of each of ``repeat`` calls by a host clock; every call ends with its result on the host."""
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def time_kernels(args) -> int:
    inf = sub("inference")
    rows_s = 4.0
    out = {}
    for name, docs, per in (("32 rows of 4 s in 4 documents", 4, 8), ("8 documents of 20 sentences", 8, 20)):
        B, ld = docs * per, int(rows_s * 24000)
        g = torch.Generator().manual_seed(1)
        lengths = [int(v) for v in torch.randint(int(0.6 * ld), ld + 1, (B,), generator=g)]
        audio = (torch.randn(B, ld, generator=g) * 0.1).cuda()
        scale = torch.rand(B, generator=g).mul(0.5).add(0.5).cuda()
        gaps = [7200] * B
        d_len = torch.tensor(lengths).cuda()
        for _ in range(3):
            joined, out_len, _ = inf.join_waveforms(audio, d_len, [per] * docs, gaps, fade=120, scale=scale, check=False)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.repeat):
            inf.join_waveforms(audio, d_len, [per] * docs, gaps, fade=120, scale=scale, check=False)
        b.record()
        b.synchronize()
        moved = 4 * (sum(lengths) + joined.numel())              # kept samples read + G * out_ld written
        out[name] = {"B": B, "G": docs, "ld": ld, "out_ld": joined.shape[1], "bytes": moved, "call_ms_events": a.elapsed_time(b) / args.repeat,
                     "joined_s": [round(int(v) / 24000, 2) for v in out_len.tolist()]}
        print(f"{name}: {moved / 1e6:.1f} MB to move, {out[name]['call_ms_events']:.4f} ms per join_waveforms call (device events, "
              f"{args.repeat} calls; the call's allocations and the two small uploads included)")
    print(json.dumps({"join_kernels": out}))
    return 0


def time_run(args) -> int:
    if args.kernels:
        return time_kernels(args)
    inf, bt, hparams, synthetic = sub("inference"), sub("batcher"), sub("hparams"), sub("synthetic")
    hp = hparams.prod_v20(n_spks=10)
    model = inf.MatchaTTSInfer(**hp.as_reference_kwargs())
    model.load_state_dict(synthetic.make_state_dict(hp, seed=7), strict=True)
    model = model.cuda().eval()
    vocoder = sub("vocoder").load_model("cuda", state_dict=synthetic.make_vocos_state_dict(seed=11))
    rng = np.random.RandomState(3)
    sizes = [int(v) for v in rng.randint(int(0.6 * args.tokens), int(1.4 * args.tokens) + 1, size=args.sentences)]
    ids = [synthetic.make_inputs(hp, 1, n, seed=200 + i)[0][0].tolist() for i, n in enumerate(sizes)]
    pauses = [300.0] * len(ids)
    gaps = [7200] * len(ids)
    kw = dict(speaker=3, solver="midpoint", n_timesteps=args.steps)
    one = [t for s in ids for t in s]
    fits = args.utterance and len(one) <= 4000
    # max_batch = the sentences: the worker starts as soon as they are all there, a document's rows or the separate requests alike
    with bt.FrameBudgetBatcher(model, max_batch=len(ids), max_tokens=max(8192, len(ids) * max(sizes), len(one)), max_wait_ms=50.0,
                               vocoder=vocoder) as q:
        def document():
            return q.submit_document(ids, pauses, encoding="pcm16", level="sentence", **kw).result()

        def separate():
            futs = [q.submit(s, **kw) for s in ids]
            return host_join_pcm16([f.result()["audio"] for f in futs], gaps)

        def utterance():
            return q.submit(one, encoding="pcm16", **kw).result()

        d, s = document(), separate()                            # warm-up of every shape, and the two ways side by side
        if fits:
            utterance()
        n_doc, n_sep = d["audio"].numel() // 2, len(s) // 2
        before = q.batches_run
        t_doc, t_sep, t_one = [], [], []
        for _ in range(args.repeat):                             # alternating within one process
            t_doc += clock(document, 1)
            t_sep += clock(separate, 1)
            if fits:
                t_one += clock(utterance, 1)
        batches = q.batches_run - before
    res = {"sentences": len(ids), "tokens": len(one), "steps": args.steps, "audio_s": n_doc / 24000, "samples_document": n_doc,
           "samples_separate": n_sep, "batches_run": batches, "document_ms": t_doc, "separate_ms": t_sep, "utterance_ms": t_one or None}
    for name, t in (("document", t_doc), ("separate", t_sep), ("utterance", t_one)):
        if t:
            print(f"{name:10s} median {np.median(t):9.2f} ms   min {min(t):9.2f}   max {max(t):9.2f}   ({len(t)} calls)")
        else:
            print(f"{name:10s} not measured" + ("" if args.utterance else " (--utterance)"))
    print(json.dumps({"speak_long_time": res}))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    cmds = ap.add_subparsers(dest="cmd", required=True)
    sp = cmds.add_parser("speak", help="a text file (or a file of phonemized segments) to a wav file")
    sp.add_argument("text", nargs="?", default=None)
    sp.add_argument("out")
    sp.add_argument("--segments-file")
    sp.add_argument("--matcha", required=True)
    sp.add_argument("--vocos", required=True)
    sp.add_argument("--voice", default="0")
    sp.add_argument("--speed", type=float, default=1.0)
    sp.add_argument("--steps", type=int, default=4)
    sp.add_argument("--solver", default="midpoint")
    sp.add_argument("--sample-rate", type=int, default=24000)
    sp.add_argument("--max-chars", type=int, default=300)
    sp.add_argument("--fade-ms", type=float, default=5.0)
    sp.add_argument("--level", choices=("document", "sentence"), default="document")
    sp.add_argument("--flac-lpc", type=int, default=0, metavar="N", help="an OUT.flac also tries linear prediction up to order N (1..12): fewer bytes")
    sp.add_argument("--loudness", type=float, default=None, metavar="LUFS", help="integrated loudness of the joined document, e.g. -16, -19, -23")
    sp.add_argument("--true-peak", type=float, default=None, metavar="DB", help="ceiling in dBTP on the true peak of the levelled document, e.g. -1")
    sp.add_argument("--captions", default=None, metavar="FILE.vtt|.srt", help="one cue per sentence, from the result's segments")
    sp.add_argument("--marks", default=None, metavar="FILE.json", help="token (and word) marks in seconds of the 24 kHz join")
    tm = cmds.add_parser("time", help="per-call times on random weights")
    tm.add_argument("--sentences", type=int, default=20)
    tm.add_argument("--tokens", type=int, default=100)
    tm.add_argument("--steps", type=int, default=4)
    tm.add_argument("--repeat", type=int, default=10)
    tm.add_argument("--kernels", action="store_true")
    tm.add_argument("--utterance", action="store_true", help="also time all the tokens as one utterance (informational)")
    args = ap.parse_args()
    with torch.inference_mode():
        return speak(args) if args.cmd == "speak" else time_run(args)


if __name__ == "__main__":
    sys.exit(main())

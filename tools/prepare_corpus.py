#!/usr/bin/env python3
"""Prepare a corpus directory for training, on the device: what the reference's matcha/utils/measure_silence.py,
normalize_silence.py, generate_data_statistics.py and precompute_mels.py do, as subcommands over batches of clips.

    python tools/prepare_corpus.py measure   -i configs/data/corpus-24k.yaml
    python tools/prepare_corpus.py normalize -i configs/data/corpus-24k.yaml --target_leading_silence 0.2 --target_trailing_silence 0.8
    python tools/prepare_corpus.py stats     -i configs/data/corpus-24k.yaml
    python tools/prepare_corpus.py mels      -i configs/data/corpus-24k.yaml
    python tools/prepare_corpus.py loudness  -i configs/data/corpus-24k.yaml
    python tools/prepare_corpus.py pitch     -i configs/data/corpus-24k.yaml
    python tools/prepare_corpus.py measure --synthetic 4 [--root DIR]     # no files needed: a small corpus is written first
    python tools/prepare_corpus.py time --synthetic 32 [--seconds 10] [--repeat 20]     # per-call times, nothing is written

The data YAML is read with ``yaml`` (the reference's keys: train_filelist_path, valid_filelist_path, sample_rate, n_fft,
n_feats, hop_length, win_length, data_statistics {mel_mean, mel_std}, mel_dir; relative paths are relative to the working
directory).  Filelists hold ``rel|speaker|lang|text`` lines, wavs are at ``<filelist dir>/wav/<rel>.wav`` (PCM, read with
tools/enroll.py's ``read_wav``; a ``<rel>.flac`` beside a missing wav is read in its place, decoded on the device).  Clips are sorted by length and processed ``--batch`` at a time, so a batch holds clips of
similar length.

measure    one table per end (leading, trailing) with a row per speaker of the train filelist: count, mean and standard
           deviation in ms at the effective and at the absolute threshold, laid out as the reference prints them
           (``SILENCE_TABLE``; tests/golden/silence_table.txt is the reference's own print).
normalize  rewrites every wav in place with the standard ``wave`` module: the file's own frames [content_start, content_end)
           between the target counts of zero frames, so sample width, channels and content samples are kept bit for bit;
           bounds, lengths and the changed flag come from the device.  ``--report FILE`` writes them as JSON.
stats      prints the ``data_statistics:`` block for the YAML.
mels       writes ``<mel_dir>/<rel>.npy`` (n_mels, T) and ``.fine.npy`` at half the hop, ``metadata.json`` and, if any file
           failed, ``failures.txt``, in the layout the reference's trainer reads; files that are already there are kept.
loudness   prints integrated loudness (LUFS, ITU-R BS.1770 gating), sample peak, true peak (dBTP) and loudness range (LU) of every file of the train and validation
           filelists and the corpus median, and marks files more than ``--loudness_margin`` dB from it: recordings that are far too
           quiet or too hot.  Nothing is rewritten: the mel statistics are computed without a level change.
pitch      one table row per speaker over both filelists: clips, median F0, range in semitones, and the mean final rise (median of
           the last 0.25 s of voicing against the clip's median, in semitones) over the rows whose text ends in ``?`` and over the
           rest, with their difference: which speakers raise a question and which stay flat (the reference's
           documentation/pitch_raise_transfer.md, steps 1-2).
time       HIP-event times of the device calls on N synthetic clips of ``--seconds`` (median, min .. max of ``--repeat``), and
           the wall time of the NumPy restatement (tests/corpus_restated.py) of the same batch; profiles/r14_corpus.md.
"""
import argparse
import importlib
import json
import statistics
import sys
import tempfile
import time
import wave
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
PKG = "matcha-tts-24k_amd"


def load_config(path: Path) -> dict:
    import yaml
    with open(path, "r", encoding="utf-8") as f:
        return yaml.safe_load(f)


def resolve(p) -> Path:
    p = Path(str(p))
    return p if p.is_absolute() else (Path.cwd() / p).resolve()


def entries(filelists):
    """[(rel, speaker, wav path)] of the filelists that exist, in file order."""
    out = []
    for fl in filelists:
        if fl is None or not fl.is_file():
            continue
        for line in fl.read_text(encoding="utf-8").splitlines():
            parts = line.strip().split("|")
            if not line.strip() or len(parts) < 2:
                continue
            wav = (fl.parent / "wav" / (parts[0] + ".wav")).resolve()
            flac = wav.with_suffix(".flac")                        # a FLAC file stands in for a missing wav of the same name
            out.append((parts[0], parts[1], flac if flac.exists() and not wav.exists() else wav))
    return out


def batches(items, size):
    """Present wavs, read and sorted by length, ``size`` at a time: (items, clips, rates)."""
    from enroll import read_wav
    loaded = []
    for it in items:
        if not it[2].exists():
            print(f"[prepare_corpus] skipped, no such file: {it[2]}")
            continue
        clip, rate = read_wav(it[2])
        loaded.append((it, clip, rate))
    loaded.sort(key=lambda t: t[1].numel())
    for i in range(0, len(loaded), size):
        chunk = loaded[i:i + size]
        yield [c[0] for c in chunk], [c[1] for c in chunk], [c[2] for c in chunk]


def synthetic_clip(i: int, body_seconds: float, rng) -> np.ndarray:
    """A sine plus noise between silent ends whose lengths depend on i (float64 in [-1, 1])."""
    body = int(24000 * body_seconds) + 37 * i
    t = np.arange(body) / 24000.0
    speech = 0.4 * np.sin(2 * np.pi * (120.0 + 20.0 * i) * t) + 0.05 * rng.standard_normal(body)
    return np.concatenate([np.zeros(1000 + 700 * i), speech, np.zeros(3000 + 2500 * (i % 2) + 111 * i)])


def write_synthetic(root: Path, n: int) -> Path:
    """A corpus of n 16-bit clips (two speakers) with uneven silence at both ends, its filelists and data YAML under ``root``."""
    cfg = root / "data.yaml"
    if cfg.exists():
        return cfg
    rng = np.random.default_rng(0)
    lines = []
    for i in range(n):
        spk = i % 2
        pcm = synthetic_clip(i, 0.6 + 0.15 * i, rng)
        rel = f"{spk}/{i:04d}"
        path = root / "wav" / (rel + ".wav")
        path.parent.mkdir(parents=True, exist_ok=True)
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(24000)
            w.writeframes(np.clip(np.round(pcm * 32767.0), -32768, 32767).astype("<i2").tobytes())
        lines.append(f"{rel}|{spk}|en-us|synthetic utterance {i}")
    (root / "train.csv").write_text("\n".join(lines[:max(1, n - 1)]) + "\n", encoding="utf-8")
    (root / "valid.csv").write_text("\n".join(lines[max(1, n - 1):]) + "\n", encoding="utf-8")
    cfg.write_text(f"train_filelist_path: {root / 'train.csv'}\nvalid_filelist_path: {root / 'valid.csv'}\nsample_rate: 24000\nn_fft: 1024\n"
                   f"n_feats: 100\nhop_length: 256\nwin_length: 1024\nf_min: 0\nf_max: 12000\nmel_backend: vocos\n"
                   f"data_statistics:\n  mel_mean: -5.5\n  mel_std: 2.0\nmel_dir: {root / 'mel'}\n", encoding="utf-8")
    return cfg


# ---------------------------------------------------------------------------------------------------------------- measure
# The layout of the per-speaker table: (heading, field width, format of a value).  Cells are left-aligned in their field and
# joined by one space; the rules above and below are RULE characters wide.
SILENCE_TABLE = (("Speaker", 10, ""), ("Count", 8, "d"), ("Effective Mean", 16, ".1f"), ("Effective Std", 16, ".1f"),
                 ("Absolute Mean", 16, ".1f"), ("Absolute Std", 16, ".1f"))
RULE = 98


def format_table(caption: str, columns, rows, rule: int = RULE) -> str:
    """A captioned text table: caption, a heavy rule, the headings, a light rule, one line per row, a heavy rule."""
    def line(cells):
        return " ".join(cell.ljust(width) for cell, (_, width, _) in zip(cells, columns))
    body = [line([format(v, spec) for v, (_, _, spec) in zip(row, columns)]) for row in rows]
    return "\n".join([caption, "=" * rule, line([name for name, _, _ in columns]), "-" * rule, *body, "=" * rule])


def silence_table(what: str, effective, absolute, effective_db: float, absolute_db: float) -> str:
    """The table of one end: ``effective`` / ``absolute`` map a speaker to that end's silences in seconds."""
    rows = []
    for spk in sorted(effective):
        e, a = np.asarray(effective[spk]) * 1000.0, np.asarray(absolute[spk]) * 1000.0
        rows.append((spk, len(e), e.mean(), e.std(), a.mean(), a.std()))
    return format_table(f"{what} (effective: {effective_db} dB, absolute: {absolute_db} dB)", SILENCE_TABLE, rows)


def cmd_measure(args, cfg, corpus) -> int:
    dbs = (args.effective_silence_threshold, args.absolute_silence_threshold)
    speakers, seconds = [], []                                       # one entry per file: speaker, the four durations
    for its, clips, rates in batches(entries([resolve(cfg["train_filelist_path"])]), args.batch):
        for rate in sorted(set(rates)):                              # the 10 ms window follows each file's own rate
            rows = [i for i, r in enumerate(rates) if r == rate]
            got = corpus.measure_silence([clips[i] for i in rows], None, rate, *dbs)["seconds"].cpu().numpy()
            speakers += [its[i][1] for i in rows]
            seconds.append(got[:, 2:6])
    print(f"[prepare_corpus] measured {len(speakers)} files")
    if not speakers:
        return 0
    seconds = np.concatenate(seconds)
    by = {spk: seconds[[s == spk for s in speakers]] for spk in set(speakers)}
    for what, eff, ab in (("Leading silence per speaker, ms", 0, 1), ("Trailing silence per speaker, ms", 2, 3)):
        print()
        print(silence_table(what, {k: v[:, eff] for k, v in by.items()}, {k: v[:, ab] for k, v in by.items()}, *dbs))
    return 0


# ---------------------------------------------------------------------------------------------------------------- loudness
def loudness_report(rows, margin: float) -> str:
    """``rows``: [(rel, lufs, peak)] or [(rel, lufs, peak, true_peak, lra)].  One line per file -- with the longer rows also the true
    peak in dBTP and the loudness range in LU --, then the median over the files with a finite loudness; a file further than
    ``margin`` dB from it, or with no block above the absolute gate, is marked."""
    finite = [r[1] for r in rows if np.isfinite(r[1])]
    median = statistics.median(finite) if finite else float("nan")
    lines = []
    for rel, lufs, peak, *more in rows:
        mark = "" if np.isfinite(lufs) and abs(lufs - median) <= margin else "   <-- silent" if not np.isfinite(lufs) else \
            f"   <-- {lufs - median:+.1f} dB from the median"
        r128 = f"   true peak {20.0 * np.log10(more[0]) if more[0] > 0 else -np.inf:7.2f} dBTP   range {more[1]:5.2f} LU" if more else ""
        lines.append(f"{rel:<24} {lufs:8.2f} LUFS   peak {peak:.4f}{r128}{mark}")
    lines.append(f"[prepare_corpus] {len(rows)} files, {len(finite)} with a finite loudness, median {median:.2f} LUFS")
    return "\n".join(lines)


def cmd_loudness(args, cfg, corpus) -> int:
    valid = cfg.get("valid_filelist_path") or None
    items = entries([resolve(cfg["train_filelist_path"]), resolve(valid) if valid else None])
    rows = []
    for its, clips, rates in batches(items, args.batch):
        for rate in sorted(set(rates)):                              # the K-weighting follows each file's own rate
            sel = [i for i, r in enumerate(rates) if r == rate]
            got = corpus.measure_loudness([clips[i] for i in sel], None, rate)
            lufs, peak, tp, lra = (got[k].cpu().tolist() for k in ("lufs", "peak", "true_peak", "lra"))
            rows += [(its[i][0], lufs[k], peak[k], tp[k], lra[k]) for k, i in enumerate(sel)]
    rows.sort(key=lambda r: r[0])
    print(loudness_report(rows, args.loudness_margin))
    return 0


# ---------------------------------------------------------------------------------------------------------------- pitch
PITCH_TABLE = (("Speaker", 10, ""), ("Count", 8, "d"), ("Median Hz", 12, ".1f"), ("Range st", 12, ".2f"), ("Rise ? st", 12, ".2f"),
               ("Rise rest st", 14, ".2f"), ("Difference st", 14, ".2f"))


def pitch_table(rows) -> str:
    """``rows``: [(speaker, median_hz, range_st, final_rise_st, text ends in "?")], one per clip.  One line per speaker: clips, the
    median of the clips' medians, the mean range, the mean final rise over the questions and over the rest, and their difference;
    clips without a voiced frame (NaN) are left out of a mean, and a mean over nothing is NaN."""
    def mean(values):
        v = np.asarray([x for x in values if np.isfinite(x)], dtype=np.float64)
        return float(v.mean()) if v.size else float("nan")
    lines = []
    for spk in sorted({r[0] for r in rows}):
        mine = [r for r in rows if r[0] == spk]
        med = [r[1] for r in mine if np.isfinite(r[1])]
        up, rest = mean(r[3] for r in mine if r[4]), mean(r[3] for r in mine if not r[4])
        lines.append((spk, len(mine), float(np.median(med)) if med else float("nan"), mean(r[2] for r in mine), up, rest, up - rest))
    return format_table("Pitch per speaker (final rise: last 0.25 s of voicing against the clip's median)", PITCH_TABLE, lines)


def cmd_pitch(args, cfg, corpus) -> int:
    valid = cfg.get("valid_filelist_path") or None
    lists = [resolve(cfg["train_filelist_path"]), resolve(valid) if valid else None]
    question = {}
    for fl in lists:                                                 # rel -> the row's text ends in a question mark
        if fl is not None and fl.is_file():
            for line in fl.read_text(encoding="utf-8").splitlines():
                parts = line.strip().split("|")
                if len(parts) >= 2:
                    question[parts[0]] = parts[-1].rstrip().endswith("?") if len(parts) >= 4 else False
    rows = []
    for its, clips, rates in batches(entries(lists), args.batch):
        for rate in sorted(set(rates)):                              # hop and lags follow each file's own rate
            sel = [i for i, r in enumerate(rates) if r == rate]
            got = corpus.measure_pitch([clips[i] for i in sel], None, rate, method="viterbi" if args.viterbi else "yin")
            med, rng, rise = (got[k].cpu().tolist() for k in ("median_hz", "range_st", "final_rise_st"))
            rows += [(its[i][1], med[k], rng[k], rise[k], question.get(its[i][0], False)) for k, i in enumerate(sel)]
    print(f"[prepare_corpus] pitch of {len(rows)} files, {sum(r[4] for r in rows)} of them questions")
    if args.viterbi:
        print("[prepare_corpus] tracked by the shortest path through YIN's candidates (pitch.track_viterbi)")
    if rows:
        print()
        print(pitch_table(rows))
    return 0


# ---------------------------------------------------------------------------------------------------------------- normalize
def rewrite_wav(path: Path, cs: int, ce: int, lead: int, trail: int, L: int) -> int:
    """The file's own frames [cs, ce) between ``lead`` / ``trail`` zero frames (-1: that end's own frames); returns the frame count."""
    with wave.open(str(path), "rb") as w:
        params, raw = w.getparams(), w.readframes(w.getnframes())
    fs = params.sampwidth * params.nchannels
    if len(raw) // fs != L:
        raise RuntimeError(f"{path}: {len(raw) // fs} frames on disk, {L} measured")
    quiet = (b"\x80" if params.sampwidth == 1 else b"\x00") * fs       # 8-bit PCM is unsigned
    head = raw[:cs * fs] if lead < 0 else quiet * lead
    tail = raw[ce * fs:] if trail < 0 else quiet * trail
    data = head + raw[cs * fs:ce * fs] + tail
    with wave.open(str(path), "wb") as w:
        w.setparams(params)
        w.writeframes(data)
    return len(data) // fs


def cmd_normalize(args, cfg, corpus) -> int:
    targets = (args.target_leading_silence, args.target_trailing_silence)
    if targets == (None, None):
        print("[prepare_corpus] normalize needs --target_leading_silence and / or --target_trailing_silence")
        return 2
    valid = cfg.get("valid_filelist_path") or None
    items = entries([resolve(cfg["train_filelist_path"]), resolve(valid) if valid else None])
    report = {}
    for its, clips, rates in batches(items, args.batch):
        for rate in sorted(set(rates)):
            rows = [i for i, r in enumerate(rates) if r == rate]
            lead, trail = (corpus.target_samples(t, rate, end) for t, end in zip(targets, ("leading", "trailing")))
            _, out_len, info = corpus.normalize_silence([clips[i] for i in rows], None, *targets, args.threshold_db, rate)
            host = {k: info[k].cpu().tolist() for k in ("bounds", "changed", "leading_delta", "trailing_delta")}
            for k, (i, n) in enumerate(zip(rows, out_len.tolist())):
                rel, _, path = its[i]
                cs, ce = host["bounds"][k][:2]
                if host["changed"][k] and path.suffix == ".flac":
                    raise RuntimeError(f"{path}: normalize rewrites wav files in place; a FLAC file is read, not rewritten")
                if host["changed"][k] and rewrite_wav(path, cs, ce, lead, trail, clips[i].numel()) != n:
                    raise RuntimeError(f"{path}: the frames written and the device's rebuilt length {n} differ")
                report[rel] = {"changed": bool(host["changed"][k]), "content_start": cs, "content_end": ce, "length": int(clips[i].numel()),
                               "new_length": int(n), "leading_delta": host["leading_delta"][k], "trailing_delta": host["trailing_delta"][k]}
    ends = []
    for end in ("leading", "trailing"):
        d = np.array([e[end + "_delta"] for e in report.values()])
        ends.append(f"{end} +{int((d > 0).sum())} / -{int((d < 0).sum())}")
    print(f"[prepare_corpus] normalized {len(report)} files, {sum(e['changed'] for e in report.values())} rewritten; padded / trimmed: " + ", ".join(ends))
    if args.report:
        Path(args.report).write_text(json.dumps(report, indent=2), encoding="utf-8")
    return 0


# ---------------------------------------------------------------------------------------------------------------- stats / mels
def both_filelists(cfg):
    lists = [resolve(cfg["train_filelist_path"]), resolve(cfg["valid_filelist_path"])]
    for fl in lists:
        if not fl.exists():
            raise FileNotFoundError(f"no filelist at {fl}")
    return lists


def at_rate(its, rates, sr, failed):
    """Indices of the clips at the corpus rate; the others are recorded as failures."""
    for i, r in enumerate(rates):
        if r != sr:
            failed.append((str(its[i][2]), f"{its[i][2]} is at {r} Hz, the data config says {sr} Hz"))
    return [i for i, r in enumerate(rates) if r == sr]


def cmd_stats(args, cfg, corpus) -> int:
    sr = int(cfg["sample_rate"])
    stats = corpus.MelStatistics(n_mels=int(cfg["n_feats"]), hop=int(cfg["hop_length"]), sample_rate=sr, n_fft=int(cfg["n_fft"]))
    failed = []
    for its, clips, rates in batches(entries(both_filelists(cfg)), args.batch):
        keep = at_rate(its, rates, sr, failed)
        if not keep:
            continue
        seen = stats.seen
        stats.update([clips[i] for i in keep])
        failed += [(str(its[keep[j - seen]][2]), msg) for j, msg in stats.failures if j >= seen]
    print(f"[prepare_corpus] statistics over {stats.ok} files, {stats.total_frames} frames; {len(failed)} left out")
    for path, msg in failed[:20]:
        print(f"  left out: {msg}")
    if stats.ok == 0:
        raise RuntimeError("no file could be used for the statistics")
    res = stats.result()
    print("\ndata_statistics:")
    print(f"  mel_mean: {res['mel_mean']}")
    print(f"  mel_std: {res['mel_std']}")
    return 0


def cmd_mels(args, cfg, corpus) -> int:
    ds = cfg.get("data_statistics") or {}
    if "mel_mean" not in ds or "mel_std" not in ds:
        raise KeyError("the data YAML has no data_statistics.mel_mean / mel_std (run `stats` first)")
    lists = both_filelists(cfg)
    mel_dir = resolve(cfg["mel_dir"])
    mel_dir.mkdir(parents=True, exist_ok=True)
    sr, hop, n_mels, n_fft = int(cfg["sample_rate"]), int(cfg["hop_length"]), int(cfg["n_feats"]), int(cfg["n_fft"])
    mean, std = float(ds["mel_mean"]), float(ds["mel_std"])
    items = entries(lists)
    todo = [it for it in items if not ((mel_dir / (it[0] + ".npy")).exists() and (mel_dir / (it[0] + ".fine.npy")).exists())]
    processed, failed = 0, []
    for its, clips, rates in batches(todo, args.batch):
        keep = at_rate(its, rates, sr, failed)
        if not keep:
            continue
        out = corpus.precompute_mels([clips[i] for i in keep], None, mean, std, hop, sr, n_fft, n_mels)
        mel, fine = out["mel"].cpu().numpy(), out["mel_fine"].cpu().numpy()
        n, nf, ok = out["mel_lengths"].tolist(), out["mel_fine_lengths"].tolist(), out["ok"].tolist()
        for k, i in enumerate(keep):
            rel, _, path = its[i]
            if not ok[k]:
                failed.append((str(path), f"a mel of {path} holds a NaN or an Inf"))
                continue
            dst = mel_dir / (rel + ".npy")
            dst.parent.mkdir(parents=True, exist_ok=True)
            np.save(dst, np.ascontiguousarray(mel[k, :, :n[k]]))
            np.save(dst.with_suffix(".fine.npy"), np.ascontiguousarray(fine[k, :, :nf[k]]))
            processed += 1
    # metadata.json and failures.txt: the keys and the tab-separated lines the reference writes beside its mels
    f_max = float(cfg["f_max"]) if cfg.get("f_max") is not None else None
    params = {"sample_rate": sr, "n_fft": n_fft, "n_mels": n_mels, "hop_length": hop, "win_length": int(cfg.get("win_length", n_fft)),
              "f_min": float(cfg.get("f_min", 0.0)), "f_max": f_max}
    meta = {"data_config": str(args.config), **params, "mel_backend": cfg.get("mel_backend", "vocos"), "mel_extractor_params": params,
            "mel_mean": mean, "mel_std": std, "num_files": len(items), "num_ok": processed, "num_fail": len(failed),
            "filelists": [str(p) for p in lists]}
    (mel_dir / "metadata.json").write_text(json.dumps(meta, indent=2), encoding="utf-8")
    if failed:
        (mel_dir / "failures.txt").write_text("".join(f"{p}\t{m}\n" for p, m in failed), encoding="utf-8")
    print(f"[prepare_corpus] mels: {processed} written, {len(items) - len(todo)} already there, {len(failed)} failed -> {mel_dir}")
    return 0


# ---------------------------------------------------------------------------------------------------------------- time
def cmd_time(args, corpus) -> int:
    """Per-call times on ``--synthetic`` clips of ``--seconds`` at 24 kHz, as a markdown table."""
    M = importlib.import_module(PKG + ".mel")
    rng = np.random.default_rng(0)
    rows = [synthetic_clip(i, args.seconds, rng).astype(np.float32) for i in range(args.synthetic)]
    B, lens = len(rows), [len(r) for r in rows]
    host = np.zeros((B, (max(lens) + 3) // 4 * 4), dtype=np.float32)
    for b, r in enumerate(rows):
        host[b, :len(r)] = r
    audio, d_len = torch.from_numpy(host).cuda(), torch.tensor(lens, device="cuda")
    mel, mel_len = M.extract(audio, lens, 256, 0.0, 1.0)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(args.repeat, 1)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})"

    print(f"B = {B} clips of about {args.seconds} s: audio {audio.numel() * 4 / 1e6:.1f} MB, hop-256 mel {list(mel.shape)} {mel.numel() * 4 / 1e6:.1f} MB")
    print("| call | ms |\n|---|---|")
    for name, fn in (("corpus.measure_silence", lambda: corpus.measure_silence(audio, d_len, check=False)),
                     ("corpus.normalize_silence, 0.2 s / 0.8 s", lambda: corpus.normalize_silence(audio, d_len, 0.2, 0.8, check=False)),
                     ("corpus.mel_sums on the hop-256 mel", lambda: corpus.mel_sums(mel, mel_len, check=False)),
                     ("mel front end at hop 256, un-normalised", lambda: M.extract(audio, lens, 256, 0.0, 1.0)),
                     ("corpus.precompute_mels", lambda: corpus.precompute_mels(audio, d_len, -5.5, 2.0)),
                     ("corpus.measure_pitch", lambda: corpus.measure_pitch(audio, d_len, check=False))):
        print(f"| `{name}` | {timed(fn)} |")
    hip = importlib.import_module(PKG + "._hip")
    lib, ld = hip.load(), audio.shape[1]
    six = torch.empty(B, 6, dtype=torch.long, device="cuda")
    ws = torch.empty(lib.mtts_silence_workspace_bytes(ld, B, 24000), dtype=torch.uint8, device="cuda")
    ld_out = (ld + 4800 + 19200 + 3) // 4 * 4
    out, out_len = torch.empty(B, ld_out, device="cuda"), torch.empty(B, dtype=torch.long, device="cuda")
    changed = torch.empty(B, dtype=torch.int32, device="cuda")
    for name, fn in (("mtts_silence_measure alone", lambda: hip.check(lib.mtts_silence_measure(
                          audio.data_ptr(), ld, d_len.data_ptr(), B, 24000, -60.0, -90.0, six.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr()))),
                     ("mtts_silence_normalize alone", lambda: hip.check(lib.mtts_silence_normalize(
                          audio.data_ptr(), ld, d_len.data_ptr(), six.data_ptr(), B, 24000, 4800, 19200, out.data_ptr(), ld_out, out_len.data_ptr(),
                          changed.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr())))):
        print(f"| `{name}` | {timed(fn)} |")
    if (ROOT / "tests" / "corpus_restated.py").exists():             # the same batch on the host, for scale
        sys.path.insert(0, str(ROOT / "tests"))
        import corpus_restated as cr
        t0 = time.perf_counter()
        want = [cr.measure(r, 24000) for r in rows]
        t1 = time.perf_counter()
        for r, w in zip(rows, want):
            cr.rebuild(r, w[0], w[1], 4800, 19200)
        t2 = time.perf_counter()
        mel_host, ml = mel.cpu().numpy(), mel_len.tolist()
        t3 = time.perf_counter()
        sums = [cr.mel_sums(mel_host[b], ml[b]) for b in range(B)]
        t4 = time.perf_counter()
        print(f"| NumPy restatement on the host, wall: measure / rebuild / mel sums | {1e3 * (t1 - t0):.1f} / {1e3 * (t2 - t1):.1f} / {1e3 * (t4 - t3):.1f} |")
        got = corpus.mel_sums(mel, mel_len)
        same = corpus.measure_silence(audio, d_len)["samples"].cpu().tolist() == want and all(
            float(got["sum"][b]) == sums[b][0] and float(got["sum_sq"][b]) == sums[b][1] for b in range(B))
        print(f"device results equal the restatement: {same}")
        return 0 if same else 1
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=["measure", "normalize", "stats", "mels", "loudness", "pitch", "time"])
    ap.add_argument("-i", "--data-config", help="data YAML (e.g. configs/data/corpus-24k.yaml)")
    ap.add_argument("--synthetic", type=int, default=0, help="write and use a synthetic corpus of N clips instead of -i")
    ap.add_argument("--root", help="where --synthetic keeps its corpus (default: a temporary directory); reused when it is already there")
    ap.add_argument("--batch", type=int, default=32, help="clips per device call")
    ap.add_argument("--effective_silence_threshold", type=float, default=-60.0)
    ap.add_argument("--absolute_silence_threshold", type=float, default=-90.0)
    ap.add_argument("--target_leading_silence", type=float, default=None, help="seconds, a multiple of 10 ms")
    ap.add_argument("--target_trailing_silence", type=float, default=None, help="seconds, a multiple of 10 ms")
    ap.add_argument("--threshold_db", type=float, default=-60.0)
    ap.add_argument("--loudness_margin", type=float, default=6.0, help="loudness: mark files further than this many dB from the median")
    ap.add_argument("--report", help="normalize: write per-file bounds and deltas as JSON")
    ap.add_argument("--viterbi", action="store_true", help="pitch: smooth octave errors (pitch.track_viterbi) instead of plain YIN")
    ap.add_argument("--seconds", type=float, default=10.0, help="time: length of the synthetic clips' content")
    ap.add_argument("--repeat", type=int, default=20, help="time: timed calls")
    args = ap.parse_args()
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    if args.command == "time" and args.synthetic < 1:
        ap.error("time needs --synthetic N")
    if not torch.cuda.is_available():
        raise RuntimeError("prepare_corpus needs a HIP device (there is no CPU path)")
    corpus = importlib.import_module(PKG + ".corpus")
    if args.command == "time":
        return cmd_time(args, corpus)
    keep = None
    if args.synthetic:
        if args.root is None:
            keep = tempfile.TemporaryDirectory()
        root = Path(args.root or keep.name).resolve()
        root.mkdir(parents=True, exist_ok=True)
        args.config = write_synthetic(root, args.synthetic)
    elif args.data_config:
        args.config = Path(args.data_config).resolve()
    else:
        ap.error("give -i DATA_YAML or --synthetic N")
    cfg = load_config(args.config)
    rc = {"measure": cmd_measure, "normalize": cmd_normalize, "stats": cmd_stats, "mels": cmd_mels, "loudness": cmd_loudness, "pitch": cmd_pitch}[args.command](args, cfg, corpus)
    if keep is not None:
        keep.cleanup()
    return rc


if __name__ == "__main__":
    sys.exit(main())

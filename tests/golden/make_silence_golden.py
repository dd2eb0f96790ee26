#!/usr/bin/env python3
"""Write tests/golden/silence.npz by running the REFERENCE's own silence utilities on the seeded clips of
tests/corpus_restated.py.

    python tests/golden/make_silence_golden.py /path/to/reference

Runs only where a checkout of the reference is at hand.  Its matcha/utils/measure_silence.py and normalize_silence.py are loaded
unmodified; torchaudio, which they import for file access alone, is replaced by a stand-in module whose ``load`` and ``save``
serve tensors from a dict.  Recorded per case (the clips themselves are regenerated from seeds, nothing else is stored):
  bounds_<case>    (content_start, content_end) of _find_content_bounds at -60 dB
  measured_<case>  measure_silence at (-60, -90) dB: leading_eff, leading_abs, trailing_eff, trailing_abs, in samples
  pass1_<case>     normalize_silence(0.2 s, 0.8 s): (changed, output length)
  bounds2_<case>, pass2_<case>   the same for a second pass over the first pass's output
  margin           the smallest relative distance of any window's RMS (both passes) to either threshold
and, for the layout of ``tools/prepare_corpus.py measure``, silence_table.txt: what the reference's own table routine prints
for the per-speaker durations in silence_table.json (the 24 kHz cases dealt to two speakers; caption and thresholds as given
there).
"""
import contextlib
import importlib.util
import io
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.dont_write_bytecode = True

import corpus_restated as cr  # noqa: E402

FILES = {}            # path -> (tensor [1, L], sample rate)


def stand_in_torchaudio():
    ta = types.ModuleType("torchaudio")
    ta.load = lambda path: (FILES[str(path)][0].clone(), FILES[str(path)][1])

    def save(path, tensor, sr):
        FILES[str(path)] = (tensor.clone(), int(sr))
    ta.save = save
    sys.modules["torchaudio"] = ta


def load(ref: Path, name: str):
    spec = importlib.util.spec_from_file_location("ref_" + name, ref / "matcha" / "utils" / (name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def margin(x: np.ndarray, sr: int) -> float:
    rms = cr.window_rms(x, cr.window(sr)).astype(np.float64)
    return min(float(np.min(np.abs(rms - float(t)) / float(t))) for t in cr.thresholds(-60.0, -90.0)) if rms.size else 1.0


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    ref = Path(sys.argv[1])
    stand_in_torchaudio()
    ms, ns = load(ref, "measure_silence"), load(ref, "normalize_silence")
    import importlib
    synthetic = importlib.import_module("matcha-tts-24k_amd.synthetic")
    out, worst = {}, 1.0
    for name, (x, sr) in cr.clips(synthetic).items():
        src, p1, p2 = Path(f"{name}.wav"), Path(f"{name}.pass1.wav"), Path(f"{name}.pass2.wav")
        FILES[str(src)] = (torch.from_numpy(x)[None], sr)
        out[f"bounds_{name}"] = np.array(ns._find_content_bounds(torch.from_numpy(x), sr, -60.0), dtype=np.int64)
        out[f"measured_{name}"] = np.array([int(round(v * sr)) for v in ms.measure_silence(src, -60.0, -90.0)], dtype=np.int64)
        worst = min(worst, margin(x, sr))
        changed = ns.normalize_silence(src, p1, cr.LEAD_S, cr.TRAIL_S, -60.0)[0]
        if not changed:
            FILES[str(p1)] = FILES[str(src)]
        y = FILES[str(p1)][0][0]
        out[f"pass1_{name}"] = np.array([int(changed), y.numel()], dtype=np.int64)
        worst = min(worst, margin(y.numpy(), sr))
        out[f"bounds2_{name}"] = np.array(ns._find_content_bounds(y, sr, -60.0), dtype=np.int64)
        changed2 = ns.normalize_silence(p1, p2, cr.LEAD_S, cr.TRAIL_S, -60.0)[0]
        if not changed2:
            FILES[str(p2)] = FILES[str(p1)]
        out[f"pass2_{name}"] = np.array([int(changed2), FILES[str(p2)][0].shape[1]], dtype=np.int64)
        print(f"{name:16s} sr={sr} L={x.size:6d} bounds={out[f'bounds_{name}'].tolist()} measured={out[f'measured_{name}'].tolist()} "
              f"pass1={out[f'pass1_{name}'].tolist()} bounds2={out[f'bounds2_{name}'].tolist()} pass2={out[f'pass2_{name}'].tolist()}")
    assert worst > 1e-3, ("a window's RMS lies within 1e-3 relative of a threshold: pick other seeds", worst)
    out["margin"] = np.array(worst)
    np.savez(HERE / "silence.npz", **out)
    print(f"margin {worst:.3f}; wrote {HERE / 'silence.npz'}")
    # the reference's printed table for known durations (seconds): a text fixture of its layout
    names = [k for k, (_, sr) in cr.clips(synthetic).items() if sr == 24000]
    table = {"caption": "Trailing silence per speaker, ms", "effective_db": -60.0, "absolute_db": -90.0, "effective": {}, "absolute": {}}
    for i, name in enumerate(names):
        spk = ("0", "17")[i % 2]
        table["effective"].setdefault(spk, []).append(int(out[f"measured_{name}"][2]) / 24000)
        table["absolute"].setdefault(spk, []).append(int(out[f"measured_{name}"][3]) / 24000)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ms._print_silence_table(table["caption"], table["effective"], table["absolute"], table["effective_db"], table["absolute_db"])
    (HERE / "silence_table.json").write_text(json.dumps(table, indent=1) + "\n", encoding="utf-8")
    (HERE / "silence_table.txt").write_text(buf.getvalue(), encoding="utf-8")
    print(buf.getvalue())
    return 0


if __name__ == "__main__":
    sys.exit(main())

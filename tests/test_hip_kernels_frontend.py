"""Kernel-level fp64 parity of the recording side: the log-mel front end (csrc/mel_frontend.hip: mel_dft_kernel,
mel_filterbank_kernel) in two stages, and the style encoder's rows (csrc/style_encoder.hip: style_prep_kernel, the conv GEMMs,
style_pool_proj_kernel).

One rule, no free constant: e_hip <= 8 * e_cpu32 + floor.  e_hip is the device's error against the fp64 restatement
(tests/enroll_restated.py, written from the published definitions), e_cpu32 the error of THE SAME OPERATION IN THE SAME FORM in fp32
torch on the CPU, floor one fp32 ulp of the scale the error is divided by.  The 8 is 4 for the 22-bit operands of the fp16 two-term
split against fp32's 24 bits, times 2 for another summation order (tests/test_hip_spk_grad.py reads it the same way).
  * Stage 1, magnitudes: read from the workspace (MelFrontEnd.magnitudes), every bin, DC and Nyquist included.  The fp32 form is
    frames (reflect-padded, unfolded) times the fp32 basis table the library exports, then sqrt(re^2 + im^2) -- a matrix product like
    the kernel's, not torch.stft in fp32, whose FFT has a smaller error growth.  Errors are per frame, divided by the frame's largest
    fp64 magnitude; floor = 2^-23.
  * Stage 2, filterbank + log + normalisation: the input is the device's own magnitudes, so stage 1's error does not enter.  In the
    linear domain (normalisation undone, exp) every band is compared, per frame divided by the frame's largest band, floor 2^-23.  In
    the log domain the bands of at least 1e-3 of the frame's largest are compared as they are (a difference of logarithms is already
    relative), floor one ulp of the largest value compared.  Bands of filters without support are exact.
  * Style rows: per row, divided by the row's largest fp64 entry, floor 2^-23; the fp32 form is R.style_rows in fp32.
Everything else is bitwise: padded columns, rows beyond a clip, the two staging paths (16-byte vector load / four scalar loads with
reflection) against each other, the bias row of an empty clip, the empty group.  Audio beyond lengths[b] and mel frames beyond a
row's length are NaN, and the samples a clip loses to the trim to a multiple of hop are ordinary noise: neither may reach an output.

Every figure is printed (and appended to $MTTS_FRONTEND_REPORT: the source of profiles/r17_frontend_parity.md) before it is
asserted."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import sub
import enroll_restated as R

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MTTS_FRONTEND_REPORT")
NAN = float("nan")
SENT = -12345.0
ULP1 = 2.0 ** -23            # one fp32 ulp of 1: the floor of an error that is divided by its scale


def note(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


def ulp32(m):
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 2.0 ** -149


def rule(name, e_hip, e_cpu, floor):
    note(f"FRONTEND-PARITY {name} | {e_hip:.3e} | {e_cpu:.3e} | {floor:.3e} | ratio {e_hip / max(e_cpu, 1e-300):.2f}")
    assert math.isfinite(e_hip) and e_hip <= 8 * e_cpu + floor, f"{name}: e_hip {e_hip:.3e} e_cpu32 {e_cpu:.3e} floor {floor:.3e}"


@pytest.fixture(scope="module")
def mel():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("mel")


@pytest.fixture(scope="module")
def style():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return sub("style")


# ------------------------------------------------------------------------------------------------ the front end's cases
# name: (n_fft, hop, sample_rate, n_mels, [(samples, kind)] of one ragged call)
CASES = {
    # one N tile, two k-steps; 48 and 49 -> 48 samples: every frame reflects at both ends; 47 filters narrower than one bin
    "64/16": (64, 16, 24000, 100, [(48, "noise"), (200, "noise"), (33 + 16, "noise")]),
    "64/64": (64, 64, 24000, 20, [(200, "noise"), (64, "noise")]),                         # hop = n_fft
    "512/160": (512, 160, 16000, 80, [(417, "noise"), (2000, "noise")]),                   # nbp 288, Np 640, trimmed tail
    "1024/256": (1024, 256, 24000, 100, [(768, "noise"), (5000, "noise")]),                # n_fft / 2 < L < n_fft
    "1024/128": (1024, 128, 24000, 100, [(640, "noise"), (3001, "noise")]),                # the same at the fine hop
    # 100 = 4 * 25 IS a multiple of 4: with an aligned buffer every interior row still takes the vector load.  Its own ld (2222, two
    # mod 4) moves row 1 to the scalar path; 1024/150 below is the hop that is no multiple of 4
    "1024/100": (1024, 100, 24000, 100, [(1300, "noise"), (2222, "noise")]),
    "1024/150": (1024, 150, 24000, 100, [(1300, "noise"), (2222, "noise")]),               # odd frames start 2 mod 4: scalar interior
    # an odd hop and an odd trimmed length (1400 -> 11 * 125 = 1375 = 3 mod 4): the only way to `j + 3 == L` on an aligned address.  j is
    # t * hop - n_fft / 2 + 4 i and L a multiple of hop, so with an even hop j + 3 is odd and L even whatever the row's base; here frame
    # 8 of row 0 meets it at j = 1372, and a vector load there would fetch sample 1375 (trimmed off, ordinary noise) for sample 1373
    "1024/125": (1024, 125, 24000, 100, [(1400, "noise"), (2222, "noise")]),
    "2048/512": (2048, 512, 24000, 100, [(1536, "noise"), (6000, "noise")]),               # LDS above 48 KiB, dead wave of the last N tile
    "2048/300": (2048, 300, 44100, 128, [(5000, "noise")]),                                # another sample rate and filter count
    # strong-bin and weak-bin regimes; 2 x 36 frames = two M tiles
    "1024/256 sweep+voiced": (1024, 256, 24000, 100, [(9000, "sweep"), (9100, "voiced")]),
}
_clips, _refs, _runs = {}, {}, {}


def clips_of(case):
    if case not in _clips:
        _clips[case] = [R.synthetic_clip(n, 40 + 7 * len(case) + i, kind) for i, (n, kind) in enumerate(CASES[case][4])]
    return _clips[case]


def front_end(mel, case):
    n_fft, _, sr, n_mels, _ = CASES[case]
    return mel.front_end(sr, n_fft, n_mels)


def mag_refs(mel, case):
    """Per clip (fp64 magnitudes, fp32 matrix-form magnitudes) [frames, bins]; computed once, shared, never changed."""
    if case not in _refs:
        n_fft, hop = CASES[case][:2]
        basis32 = torch.from_numpy(front_end(mel, case).basis())
        _refs[case] = [(R.stft_mag(c, hop, n_fft), R.stft_mag(c, hop, n_fft, basis32)) for c in clips_of(case)]
    return _refs[case]


def batch(clips, pad=0, base=0):
    """The clips as rows of a [B, ld] device buffer, ld = the longest clip rounded up to a multiple of 4, plus `pad`; everything
    beyond a clip is NaN; the buffer starts `base` floats after a 16-byte boundary."""
    lengths = [int(c.numel()) for c in clips]
    ld = (max(lengths) + 3) // 4 * 4 + pad
    flat = torch.full((base + len(clips) * ld,), NAN)
    rows = flat[base:].view(len(clips), ld)
    for b, c in enumerate(clips):
        rows[b, :lengths[b]] = c
    dev = flat.cuda()
    assert dev.data_ptr() % 16 == 0
    return dev[base:].view(len(clips), ld), lengths


def run(fe, clips, hop, mean=0.0, std=1.0, pad=0, base=0):
    """-> (mel [B, n_mels, T_max], frames [B], magnitudes [B, T_max, padded bins]) on the host."""
    audio, lengths = batch(clips, pad, base)
    out, n = fe.extract(audio, lengths, hop, mean, std)
    mag = fe.magnitudes(padded=True).clone()
    torch.cuda.synchronize()
    return out.cpu(), n.cpu().tolist(), mag.cpu()


def run_case(mel, case, variant="aligned", mean=0.0, std=1.0):
    """aligned: every row starts on a 16-byte boundary.  misaligned: ld = 3 mod 4, so row 1 starts 3 and row 2 starts 2 floats past
    one and their interior takes the four scalar loads; a single clip starts 3 floats past a boundary instead."""
    key = (case, variant, mean, std)
    if key not in _runs:
        clips = clips_of(case)
        pad, base = (0, 0) if variant == "aligned" else ((3, 0) if len(clips) > 1 else (3, 3))
        _runs[key] = run(front_end(mel, case), clips, CASES[case][1], mean, std, pad, base)
    return _runs[key]


# ------------------------------------------------------------------------------------------------ stage 1: magnitudes
@pytest.mark.parametrize("variant", ["aligned", "misaligned"])
@pytest.mark.parametrize("case", list(CASES))
def test_magnitudes_against_fp64(mel, case, variant):
    n_fft, hop = CASES[case][:2]
    fe = front_end(mel, case)
    nb = fe.n_bins
    out, n, mag = run_case(mel, case, variant)
    clips = clips_of(case)
    assert n == [c.numel() // hop + 1 for c in clips]
    assert mag.shape == (len(clips), max(n), (nb + 31) // 32 * 32)
    assert (mag[:, :, nb:] == 0).all()                                  # the padded columns are exactly zero
    e_hip = e_cpu = 0.0
    for b, (ref, c32) in enumerate(mag_refs(mel, case)):
        assert ref.shape == (n[b], nb)
        got = mag[b, :n[b], :nb]
        assert torch.isfinite(got).all() and torch.isfinite(out[b, :, :n[b]]).all()      # no NaN from beyond the clip
        assert (mag[b, n[b]:] == 0).all() and (out[b, :, n[b]:] == 0).all()             # rows without a frame
        scale = ref.amax(1, keepdim=True)
        e_hip = max(e_hip, ((got.double() - ref).abs() / scale).max().item())
        e_cpu = max(e_cpu, ((c32.double() - ref).abs() / scale).max().item())
    rule(f"magnitudes {case} {variant}", e_hip, e_cpu, ULP1)


ALIGN = {"1024/256": [(768, "noise"), (5000, "noise"), (1300, "noise")], "64/16": [(48, "noise"), (200, "noise"), (33 + 16, "noise")],
         "1024/125": [(1400, "noise"), (2222, "noise"), (1300, "noise")]}


@pytest.mark.parametrize("key", list(ALIGN))
def test_row_alignment_changes_no_bit(mel, key):
    """ld = 0, 1, 2, 3 mod 4 with B = 3: rows 1 and 2 start at every offset from a 16-byte boundary and whole rows move from the vector
    load to the four scalar loads.  Both loads fetch the same samples.  At the odd hop 125 the frames of one row alternate between the
    two loads and the clip of 1375 samples has `j + 3 == L` on an aligned address when it is a batch of one."""
    n_fft, hop = (int(v) for v in key.split("/"))
    fe = mel.front_end(24000, n_fft, 100)
    clips = [R.synthetic_clip(n, 70 + i, kind) for i, (n, kind) in enumerate(ALIGN[key])]
    solo = [run(fe, [c], hop, -4.0, 2.0) for c in clips]
    for pad in range(4):
        out, n, mag = run(fe, clips, hop, -4.0, 2.0, pad=pad)
        for b, (s_out, s_n, s_mag) in enumerate(solo):
            assert n[b] == s_n[0]
            assert torch.equal(mag[b, :n[b]], s_mag[0]), (pad, b)
            assert torch.equal(out[b, :, :n[b]], s_out[0]), (pad, b)


@pytest.mark.parametrize("case", ["64/16", "512/160", "2048/512"])
def test_nothing_is_written_outside_the_documented_regions(mel, case):
    """The C entry on buffers filled with a sentinel: the workspace beyond mag [B * T_max][nbp] and the floats behind mel and the
    frame counts are untouched (B * T_max is no multiple of the 64-row tile; at n_fft 512 and 2048 the last N tile has columns
    beyond nbp), and what it wrote is what extract() returns."""
    hip = sub("_hip")
    n_fft, hop, _, n_mels, _ = CASES[case]
    fe = front_end(mel, case)
    clips = clips_of(case)
    want_out, want_n, want_mag = run_case(mel, case)
    audio, lengths = batch(clips)
    B, t_max, nbp = len(clips), max(want_n), want_mag.shape[2]
    assert (B * t_max) % 64
    ws = torch.full((B * t_max * nbp + 64,), SENT, device="cuda")
    out = torch.full((B * n_mels * t_max + 64,), SENT, device="cuda")
    cnt = torch.full((B + 8,), -77, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lengths, dtype=torch.int64, device="cuda")
    hip.check(fe.lib.mtts_melfe_forward(fe.ctx, hip.ptr(audio), audio.shape[1], hip.ptr(d_len), B, hop, 0.0, 1.0, hip.ptr(out), t_max,
                                        hip.ptr(cnt), ws.data_ptr(), B * t_max * nbp * 4, hip.stream_ptr()))
    torch.cuda.synchronize()
    assert (ws[B * t_max * nbp:] == SENT).all() and (out[B * n_mels * t_max:] == SENT).all() and (cnt[B:] == -77).all()
    assert cnt[:B].tolist() == want_n
    assert torch.equal(ws[:B * t_max * nbp].view(B, t_max, nbp).cpu(), want_mag)
    assert torch.equal(out[:B * n_mels * t_max].view(B, n_mels, t_max).cpu(), want_out)


# ------------------------------------------------------------------------------------------------ stage 2: filterbank, log, normalisation
def floor_value(mean, std):
    """(log(1e-7) - mean) / std as fp32 rounds it: the constant, its logarithm, the difference and the quotient each rounded once."""
    lg = np.float32(np.log(np.float64(np.float32(1e-7))))
    return float((lg - np.float32(mean)) / np.float32(std))


@pytest.mark.parametrize("norm", [(0.0, 1.0), (-4.0, 2.0)])
@pytest.mark.parametrize("case", list(CASES))
def test_filterbank_log_normalisation_against_fp64(mel, case, norm):
    n_fft, hop, sr, n_mels, _ = CASES[case]
    mean, std = norm
    fe = front_end(mel, case)
    nb = fe.n_bins
    out, n, mag = run_case(mel, case, "aligned", mean, std)
    assert max(n) % 16                                                  # the last tile of 16 frames is partly used
    fb64 = torch.from_numpy(R.htk_fbanks(nb, sr, n_mels))
    fb32 = torch.from_numpy(fe.filterbank())
    empty = fb64.sum(0) == 0
    assert torch.equal(empty, fb32.sum(0) == 0)
    if case == "64/16":
        assert int(empty.sum()) == 47
    e_log = c_log = e_lin = c_lin = top = 0.0
    for b in range(len(n)):
        m32 = mag[b, :n[b], :nb]
        got = out[b, :, :n[b]].t().double()
        ref = R.mel_from_mag(m32.double(), fb64, mean, std)
        c32 = R.mel_from_mag(m32, fb32, mean, std).double()
        assert torch.isfinite(got).all()
        assert (out[b, :, n[b]:] == 0).all()
        assert (out[b, empty, :n[b]] == floor_value(mean, std)).all()   # no support: exactly the clamp
        lin = torch.clamp(m32.double() @ fb64, min=1e-7)
        peak = lin.amax(1, keepdim=True)
        strong = lin >= 1e-3 * peak
        e_log = max(e_log, (got - ref).abs()[strong].max().item())
        c_log = max(c_log, (c32 - ref).abs()[strong].max().item())
        top = max(top, ref.abs()[strong].max().item())
        e_lin = max(e_lin, (((got * std + mean).exp() - lin).abs() / peak).max().item())
        c_lin = max(c_lin, (((c32 * std + mean).exp() - lin).abs() / peak).max().item())
    rule(f"log-mel {case} mean {mean} std {std}", e_log, c_log, ulp32(top))
    rule(f"linear mel {case} mean {mean} std {std}", e_lin, c_lin, ULP1)


# ------------------------------------------------------------------------------------------------ the style encoder
STYLE_CFGS = [(4, 36, 1, 5), (20, 260, 2, 16), (100, 256, 4, 96), (100, 512, 2, 7)]      # (n_feats, hidden, layers, E)
STYLE_T = [1, 2, 3, 5, 33, 70]
_style = {}


def style_model(style, cfg):
    if cfg not in _style:
        torch.manual_seed(17 + cfg[1])
        m = style.StyleEncoder(*cfg)
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.endswith("bias"):
                    p.add_(0.1 * torch.randn_like(p))            # biases that cannot be mistaken for one another or for zero
        _style[cfg] = ({k: v.clone() for k, v in m.state_dict().items()}, m.cuda().eval())
    return _style[cfg]


def style_inputs(n_feats, T, lengths, seed):
    x = torch.randn(len(lengths), n_feats, T, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lengths):
        x[b, :, n:] = NAN                                        # the padded part is never read as data
    return x


def row_errors(got, ref, c32):
    scale = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / scale, (c32.double() - ref).abs().max().item() / scale


@pytest.mark.parametrize("T", STYLE_T)
@pytest.mark.parametrize("cfg", STYLE_CFGS)
def test_style_rows_against_fp64(style, cfg, T):
    """T < 4 leaves time slices of the pooling empty; hidden 36 and 260 are no multiple of 64, 512 needs two channel trips; 2E = 10
    and 14 are no multiple of the 16 projecting waves; n_feats 4 and T < 32 are below one tile of the transposing kernel."""
    sd, model = style_model(style, cfg)
    lengths = sorted({T, 1, 0, T // 2 + 1}, reverse=True)
    x = style_inputs(cfg[0], T, lengths, 1000 + T)
    e_enc, e_dur = (t.cpu() for t in model(x.cuda(), lengths=lengths))
    assert e_enc.shape == e_dur.shape == (len(lengths), cfg[3])
    e_hip = e_cpu = 0.0
    for b, n in enumerate(lengths):
        clean = torch.nan_to_num(x[b])
        ref = R.style_rows(sd, clean, n)
        c32 = R.style_rows(sd, clean, n, dtype=torch.float32)
        for got, r, c in zip((e_enc[b], e_dur[b]), ref, c32):
            assert torch.isfinite(got).all()
            eh, ec = row_errors(got, r, c)
            e_hip, e_cpu = max(e_hip, eh), max(e_cpu, ec)
        if n == 0:                                               # pooled is exactly 0: the row is the two biases
            assert torch.equal(e_enc[b], sd["proj_enc.bias"]) and torch.equal(e_dur[b], sd["proj_dur.bias"])
    rule(f"style rows cfg {cfg} T={T}", e_hip, e_cpu, ULP1)


@pytest.mark.parametrize("T", [3, 33])
@pytest.mark.parametrize("cfg", STYLE_CFGS)
def test_style_groups_against_fp64(style, cfg, T):
    """A group of one clip, a group of three (one of them empty) and a group without clips, against the fp64 mean of the fp64 rows;
    the unit is the fp32 mean of the fp32 rows."""
    sd, model = style_model(style, cfg)
    lengths, group = [T, 1, 0, T // 2 + 1], [2, 0, 2, 2]
    x = style_inputs(cfg[0], T, lengths, 2000 + T)
    g_enc, g_dur = (t.cpu() for t in model(x.cuda(), lengths=lengths, group=group, n_groups=3))
    assert g_enc.shape == g_dur.shape == (3, cfg[3])
    rows64 = [R.style_rows(sd, torch.nan_to_num(x[b]), n) for b, n in enumerate(lengths)]
    rows32 = [R.style_rows(sd, torch.nan_to_num(x[b]), n, dtype=torch.float32) for b, n in enumerate(lengths)]
    e_hip = e_cpu = 0.0
    for g in (0, 2):
        idx = [b for b, v in enumerate(group) if v == g]
        for h, got in enumerate((g_enc[g], g_dur[g])):
            assert torch.isfinite(got).all()
            ref = torch.stack([rows64[b][h] for b in idx]).mean(0)
            c32 = torch.stack([rows32[b][h] for b in idx]).mean(0)
            eh, ec = row_errors(got, ref, c32)
            e_hip, e_cpu = max(e_hip, eh), max(e_cpu, ec)
    assert (g_enc[1] == 0).all() and (g_dur[1] == 0).all()      # a voice without clips
    rule(f"style groups cfg {cfg} T={T}", e_hip, e_cpu, ULP1)

"""CPU checks of the unit entries of the kernels that are not GEMMs (csrc/unit_entries.hip: mtts_dwconv7_ln, mtts_spec_polar,
mtts_istft_ola, mtts_ode_combine, mtts_step_tables, mtts_time_sinusoid, mtts_rope and the four layout moves; nothing runs on a
GPU): the binding itself is checked for every entry in test_abi.py; here: every refusal
that can be decided on the host returns -1 with a message before anything is launched (the buffers named here are never touched);
and the restatements the GPU file measures against (tests/glue_restated.py) agree with independent torch code: torch.istft,
F.conv1d + F.layer_norm, the oracle's rotary function and alignment, a textbook 3/8-rule step."""
import ctypes as C
import math
import re

import pytest
import torch
import torch.nn.functional as F

import glue_restated as G
from conftest import ROOT, sub

NEW = ["mtts_dwconv7_ln", "mtts_spec_polar", "mtts_istft_ola", "mtts_ode_combine", "mtts_step_tables", "mtts_time_sinusoid", "mtts_rope",
       "mtts_cf_to_cl", "mtts_cl_to_cf", "mtts_slots_to_cl", "mtts_cl_to_slots"]
FAKE = 0x1000          # a non-null "pointer" for buffers a refused call must not touch
ISTFT_SHAPES = [(16, 4, 2), (16, 4, 9), (32, 8, 7), (64, 32, 5), (64, 16, 3), (16, 8, 2)]


@pytest.fixture(scope="module")
def hip():
    h = sub("_hip")
    h.build()
    h.load()
    return h


@pytest.fixture(scope="module")
def lib(hip):
    return hip.load()


def test_new_entries_are_declared_exported_and_bound_with_matching_arity_and_types(hip, lib):
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    header = (ROOT / "include" / "mtts.h").read_text()
    for name in NEW:
        assert callable(getattr(hip, name[len("mtts_"):]))
    assert lib.mtts_abi_version() == 2
    assert re.search(r"#define\s+MTTS_ABI_VERSION\s+2\b", header) and re.search(r"#define\s+MTTS_IMAGE_REVISION\s+7\b", header)


def refused(lib, rc, needle):
    assert rc == -1
    assert needle.encode() in lib.mtts_last_error(), lib.mtts_last_error()


def test_vocos_tail_entries_refuse_on_the_host(lib):
    dw = lambda **k: lib.mtts_dwconv7_ln(k.get("x", FAKE), k.get("w", FAKE), k.get("b", FAKE), k.get("g", FAKE), k.get("be", FAKE), 1e-6,
                                         k.get("B", 2), k.get("T", 5), k.get("C", 64), None, k.get("y", FAKE), None)
    for name in ("x", "w", "b", "g", "be", "y"):
        refused(lib, dw(**{name: None}), "null buffer")
    refused(lib, dw(B=0), "empty batch")
    refused(lib, dw(T=0), "empty batch")
    for c in (0, 66, 2052, 4096):
        refused(lib, dw(C=c), "multiple of 4, at most 2048")
    sp = lambda x=FAKE, M=3, ld=72, nb=33, off=36: lib.mtts_spec_polar(x, M, ld, nb, off, 100.0, None)
    refused(lib, sp(x=None), "null buffer")
    refused(lib, sp(M=0), "empty")
    refused(lib, sp(nb=0), "empty")
    refused(lib, sp(off=32), "overlap or leave the row")          # the phase half begins inside the magnitude half
    refused(lib, sp(ld=68), "overlap or leave the row")           # off + nbins = 69 > ld
    ola = lambda **k: lib.mtts_istft_ola(k.get("fr", FAKE), k.get("w", FAKE), k.get("B", 2), k.get("T", 4), k.get("n", 16), k.get("hop", 4),
                                         None, k.get("a", FAKE), None)
    for name in ("fr", "w", "a"):
        refused(lib, ola(**{name: None}), "null buffer")
    refused(lib, ola(B=0), "empty batch")
    refused(lib, ola(T=1), "at least 2 frames")
    refused(lib, ola(hop=0), "hop must divide")
    refused(lib, ola(hop=5), "hop must divide")
    refused(lib, ola(n=0), "hop must divide")


def test_solver_glue_entries_refuse_on_the_host(lib):
    oc = lambda **k: lib.mtts_ode_combine(k.get("stage", 4), 0.1, k.get("dtb"), k.get("T", 5), k.get("y", FAKE), k.get("ldy", 40),
                                          k.get("k1", FAKE), k.get("k2", FAKE), k.get("k3", FAKE), k.get("k4", FAKE), k.get("ldk", 48),
                                          k.get("out", FAKE + 0x100000), k.get("ldo", 44), k.get("M", 10), k.get("C", 37), None)
    refused(lib, oc(stage=5), "stage is 0 .. 4")
    refused(lib, oc(stage=-1), "stage is 0 .. 4")
    for name in ("y", "k1", "k2", "k3", "k4", "out"):
        refused(lib, oc(**{name: None}), "null buffer")
    refused(lib, oc(stage=2, k2=None, k3=None, k4=None), "null buffer")
    refused(lib, oc(stage=3, k3=None, k4=None), "null buffer")
    refused(lib, oc(M=0), "empty state")
    refused(lib, oc(C=0), "empty state")
    for name in ("ldy", "ldk", "ldo"):
        refused(lib, oc(**{name: 36}), "smaller than C")
    refused(lib, oc(out=FAKE, ldo=44), "in place needs ldo == ldy")
    refused(lib, oc(dtb=FAKE, T=0), "per-utterance dt")
    refused(lib, oc(dtb=FAKE, T=3), "per-utterance dt")            # 3 does not divide M = 10
    st = lambda **k: lib.mtts_step_tables(k.get("t0", FAKE), k.get("t1", FAKE), k.get("m", FAKE), k.get("B", 3), k.get("T", 7), k.get("st", 4),
                                          k.get("tv", FAKE), k.get("dt", FAKE), k.get("rf", FAKE), k.get("rh", FAKE), None)
    for name in ("t0", "t1", "m", "tv", "dt", "rf", "rh"):
        refused(lib, st(**{name: None}), "null buffer")
    refused(lib, st(B=0), "empty batch")
    refused(lib, st(T=0), "empty batch")
    for stages in (0, 3, 5):
        refused(lib, st(st=stages), "stages is 1")
    ts = lambda **k: lib.mtts_time_sinusoid(k.get("f", FAKE), k.get("ht", FAKE), k.get("dt"), k.get("nt", 4), k.get("half", 8), 1000.0,
                                            k.get("o", FAKE), None)
    refused(lib, ts(f=None), "null buffer")
    refused(lib, ts(o=None), "null buffer")
    refused(lib, ts(ht=None), "one of the two")
    refused(lib, ts(dt=FAKE), "one of the two")
    refused(lib, ts(nt=0), "empty table")
    refused(lib, ts(half=0), "empty table")
    refused(lib, ts(nt=257), "at most 256 host times")
    ro = lambda **k: lib.mtts_rope(k.get("q", FAKE), k.get("B", 2), k.get("T", 5), k.get("H", 2), k.get("D", 8), k.get("dr", 4),
                                   k.get("c", FAKE), k.get("s", FAKE), None)
    for name in ("q", "c", "s"):
        refused(lib, ro(**{name: None}), "null buffer")
    for name in ("B", "T", "H", "D"):
        refused(lib, ro(**{name: 0}), "empty batch")
    for dr in (0, 3, 10):
        refused(lib, ro(dr=dr), "d_rope must be even and within the head")


def test_layout_entries_refuse_on_the_host(lib):
    cf = lambda **k: lib.mtts_cf_to_cl(k.get("src", FAKE), None, k.get("B", 3), k.get("C", 33), k.get("T", 31), k.get("Ts", 34), k.get("dst", FAKE),
                                       k.get("ld", 41), k.get("co", 4), None, None)
    refused(lib, cf(src=None), "null buffer")
    refused(lib, cf(dst=None), "null buffer")
    for name in ("B", "C", "T"):
        refused(lib, cf(**{name: 0}), "empty batch")
    refused(lib, cf(Ts=30), "T_src is shorter than T")
    refused(lib, cf(ld=36), "smaller than col_off + C")            # 4 + 33 = 37
    refused(lib, cf(co=-1), "smaller than col_off + C")
    cl = lambda **k: lib.mtts_cl_to_cf(k.get("src", FAKE), k.get("ld", 41), k.get("B", 3), k.get("C", 33), k.get("T", 31), k.get("dst", FAKE),
                                       k.get("To", 29), 2.5, -5.5, None)
    refused(lib, cl(src=None), "null buffer")
    refused(lib, cl(dst=None), "null buffer")
    for name in ("B", "C", "T"):
        refused(lib, cl(**{name: 0}), "empty batch")
    refused(lib, cl(To=0), "T_out must be within")
    refused(lib, cl(To=32), "T_out must be within")
    refused(lib, cl(ld=32), "ld is smaller than C")
    s2c = lambda **k: lib.mtts_slots_to_cl(k.get("pool", FAKE), k.get("sl", FAKE), k.get("S", 5), k.get("Tp", 33), k.get("B", 3), k.get("C", 33),
                                           k.get("T", 31), k.get("dst", FAKE), k.get("ld", 41), k.get("co", 4), None)
    for name in ("pool", "sl", "dst"):
        refused(lib, s2c(**{name: None}), "null buffer")
    for name in ("S", "B", "C", "T"):
        refused(lib, s2c(**{name: 0}), "empty batch or pool")
    refused(lib, s2c(Tp=30), "longer than T_pool")
    refused(lib, s2c(ld=36), "smaller than col_off + C")
    c2s = lambda **k: lib.mtts_cl_to_slots(k.get("src", FAKE), k.get("ld", 41), k.get("B", 3), k.get("C", 33), k.get("T", 31), k.get("pool", FAKE),
                                           k.get("sl", FAKE), k.get("S", 5), k.get("Tp", 33), None)
    for name in ("src", "pool", "sl"):
        refused(lib, c2s(**{name: None}), "null buffer")
    for name in ("S", "B", "C", "T"):
        refused(lib, c2s(**{name: 0}), "empty batch or pool")
    refused(lib, c2s(Tp=30), "longer than T_pool")
    refused(lib, c2s(ld=32), "ld is smaller than C")


# ------------------------------------------------------------------------------------------------ the restatements
def rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("n_fft,hop,T", ISTFT_SHAPES)
def test_overlap_add_with_irfft_times_window_is_torch_istft(n_fft, hop, T):
    nb = n_fft // 2 + 1
    spec = torch.complex(rand(2, nb, T, seed=n_fft + T), rand(2, nb, T, seed=n_fft + T + 1))
    window = torch.hann_window(n_fft, dtype=torch.float64)
    ref = torch.istft(spec, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True)
    frames = torch.fft.irfft(spec.transpose(1, 2), n=n_fft, dim=2) * window            # [B, T, n_fft]
    out, env = G.istft_ola(frames, window, hop)
    assert out.shape == ref.shape == (2, hop * (T - 1))
    assert (env > 1e-11).all()
    assert (out - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())


def test_overlap_add_ragged_rows_are_their_own_plain_result_and_hop_equal_n_fft_keeps_the_sum():
    window = torch.hann_window(32, dtype=torch.float64)
    frames = rand(6, 7, 32, seed=3)
    lengths = [7, 4, 2, 1, 0, 9]
    out, _ = G.istft_ola(frames, window, 8, lengths)
    for b, n in enumerate(lengths):
        n = max(0, min(n, 7))
        Lb = 8 * max(n - 1, 0)
        if n >= 2:
            own, _ = G.istft_ola(frames[b:b + 1, :n], window, 8)
            assert torch.equal(out[b, :Lb], own[0])
        assert (out[b, Lb:] == 0).all()
    # hop = n_fft: every sample has one frame; where the periodic hann window is zero (pos % 16 == 0) the sum is kept undivided
    w16 = torch.hann_window(16, dtype=torch.float64)
    fr = rand(1, 4, 16, seed=4)
    out, env = G.istft_ola(fr, w16, 16)
    assert out.shape == (1, 48) and (env[0, 8::16] <= 1e-11).all() and (env > 1e-11).sum().item() == 45
    assert torch.equal(out[0, 8::16], fr[0, 1:, 0])
    s = 3                                                   # pos = 11, frame 0, sample 11
    assert out[0, s].item() == (fr[0, 0, 11] / w16[11] ** 2).item()


@pytest.mark.parametrize("C,B,T", [(4, 1, 1), (68, 3, 5), (16, 2, 9)])
def test_conv_norm_is_conv1d_groups_plus_layer_norm(C, B, T):
    x, w7 = rand(B, T, C, seed=1), rand(7, C, seed=2)
    bias, gamma, beta = rand(C, seed=3), rand(C, seed=4), rand(C, seed=5)
    ref = F.conv1d(x.transpose(1, 2), w7.t().reshape(C, 1, 7), bias, padding=3, groups=C).transpose(1, 2)
    ref = F.layer_norm(ref, (C,), gamma, beta, eps=1e-6)
    out = G.dwconv7_ln(x, w7, bias, gamma, beta, 1e-6)
    assert (out - ref).abs().max().item() < 1e-11
    lengths = [T, max(T - 4, 0), 1][:B]
    rag = G.dwconv7_ln(x, w7, bias, gamma, beta, 1e-6, lengths)
    for b, n in enumerate(lengths):
        if n:
            own = F.layer_norm(F.conv1d(x[b:b + 1, :n].transpose(1, 2), w7.t().reshape(C, 1, 7), bias, padding=3, groups=C).transpose(1, 2),
                               (C,), gamma, beta, eps=1e-6)
            assert (rag[b, :n] - own[0]).abs().max().item() < 1e-11
        assert torch.isnan(rag[b, n:]).all()


def test_polar_is_the_oracle_head_arithmetic():
    x = rand(5, 72, seed=6) * 3.0
    x[0, 0] = 7.0                                           # exp(7) is clipped at 100
    out = G.spec_polar(x, 33, 36)
    mag = torch.clip(torch.exp(x[:, :33]), max=1e2)
    spec = mag * (torch.cos(x[:, 36:69]) + 1j * torch.sin(x[:, 36:69]))
    assert torch.equal(out[:, :33], spec.real) and torch.equal(out[:, 36:69], spec.imag)
    assert torch.equal(out[:, 33:36], x[:, 33:36]) and torch.equal(out[:, 69:], x[:, 69:])
    assert abs(out[0, 0].item() / math.cos(x[0, 36].item()) - 100.0) < 1e-12


@pytest.mark.parametrize("B,T,H,D,d", [(2, 5, 2, 8, 4), (1, 70, 3, 64, 32), (2, 9, 1, 6, 6)])
def test_rope_is_the_oracle_rotary_function(oracle, B, T, H, D, d):
    qkv = rand(B * T, 3 * H * D, seed=T)
    cos, sin = oracle.rope_tables(d, T, torch.float64)
    out = G.rope(qkv, B, T, H, D, d, cos, sin).view(B, T, 3, H, D)
    x = qkv.view(B, T, 3, H, D)
    for sec in (0, 1):
        ref = oracle.apply_rope(x[:, :, sec].permute(0, 2, 1, 3), d).permute(0, 2, 1, 3)
        assert (out[:, :, sec] - ref).abs().max().item() < 1e-14
    assert torch.equal(out[:, :, 2], x[:, :, 2])


def test_rk4_stages_chained_are_a_textbook_three_eighths_step():
    """y' = A y + c t on 37 components: k1..k4 of the 3/8 rule with the textbook tableau, against the four stage combinations."""
    A, c, y = rand(37, 37, seed=7) * 0.3, rand(37, seed=8), rand(10, 37, seed=9)
    f = lambda t, v: v @ A.t() + c * t
    t0, h = 0.3, 0.1
    k1 = f(t0, y)
    k2 = f(t0 + h / 3, y + h * k1 / 3)
    k3 = f(t0 + 2 * h / 3, y + h * (-k1 / 3 + k2))
    k4 = f(t0 + h, y + h * (k1 - k2 + k3))
    ref = y + h * (k1 + 3 * k2 + 3 * k3 + k4) / 8
    dt = torch.tensor(h, dtype=torch.float64)
    tv, dtb, _, _ = G.step_tables(torch.tensor([t0], dtype=torch.float64), torch.tensor([t0 + h], dtype=torch.float64),
                                  torch.ones(1, 1, dtype=torch.float64), 4)
    g1 = f(tv[0].item(), y)
    g2 = f(tv[1].item(), G.ode_combine(1, dt, y, g1))
    g3 = f(tv[2].item(), G.ode_combine(2, dt, y, g1, g2))
    g4 = f(tv[3].item(), G.ode_combine(3, dt, y, g1, g2, g3))
    out = G.ode_combine(4, dt, y, g1, g2, g3, g4)
    assert (out - ref).abs().max().item() < 1e-14 and abs(dtb.item() - h) < 1e-16
    assert torch.equal(G.ode_combine(0, dt, y, k1), y + h * k1)
    # a coefficient slip is far outside that bound: 1/2 in place of 1/3 in stage 1
    bad = f(tv[1].item(), y + h * g1 * 0.5)
    assert (bad - g2).abs().max().item() > 1e-4
    # per-utterance dt as a column
    col = torch.tensor([[0.1]] * 5 + [[-0.25]] * 5, dtype=torch.float64)
    rows = G.ode_combine(4, col, y, g1, g2, g3, g4)
    assert torch.equal(rows[:5], out[:5]) and torch.equal(rows[5:], G.ode_combine(4, torch.tensor(-0.25, dtype=torch.float64), y, g1, g2, g3, g4)[5:])


def test_step_tables_and_sinusoid_follow_the_oracle(oracle):
    t0, t1 = torch.tensor([0.0, 0.3, 0.9]), torch.tensor([1.0, 0.4, 1.0])
    mask = (torch.arange(7)[None, :] < torch.tensor([7, 3, 0])[:, None]).float()
    for stages, want in ((1, [t0]), (2, [t0, t0 + 0.5 * (t1 - t0)]), (4, [t0, t0 + (t1 - t0) / 3, t0 + (t1 - t0) * 2 / 3, t1])):
        tv, dt, rf, rh = G.step_tables(t0, t1, mask, stages)
        assert tv.shape == (stages * 3,) and (tv - torch.cat(want)).abs().max().item() < 2e-7
        assert torch.equal(dt, t1 - t0) and torch.equal(rf.view(3, 7), mask * dt[:, None]) and torch.equal(rh.view(3, 7), mask * (0.5 * dt)[:, None])
    hipmod = sub("_hip")
    t = torch.tensor([0.0, 1e-4, 0.37, 0.5, 0.999, 1.0])
    emb = G.sinusoid(G.sinusoid_arg(hipmod.time_freqs(128), t, 1000.0))
    assert torch.equal(emb, oracle.sinusoidal_pos_emb(t, 128, 1000.0))


@pytest.mark.parametrize("C,T", [(1, 1), (31, 33), (33, 31)])
def test_layout_moves_invert_each_other(C, T):
    B, ld = 3, C + 8
    src = rand(B, C, T + 3, seed=C)
    rows = G.cf_to_cl(src, torch.full((B * T, ld), -7.0, dtype=torch.float64), T, col_off=4)
    assert torch.equal(rows.view(B, T, ld)[:, :, 4:4 + C], src[:, :, :T].transpose(1, 2)) and (rows[:, :4] == -7).all() and (rows[:, 4 + C:] == -7).all()
    assert torch.equal(G.cl_to_cf(rows[:, 4:].contiguous(), B, C, T, T), src[:, :, :T])
    rag = G.cf_to_cl(src, torch.full((B * T, ld), -7.0, dtype=torch.float64), T, col_off=4, lengths=[T, T // 2, 1]).view(B, T, ld)
    assert (rag[1, T // 2:, 4:4 + C] == 0).all() and torch.equal(rag[1, :T // 2, 4:4 + C], src[1, :, :T // 2].t())
    pool = rand(5, C, T + 2, seed=C + 1)
    slots = [3, -1, 5]
    got = G.slots_to_cl(pool, slots, torch.full((B * T, ld), -7.0, dtype=torch.float64), T, col_off=4).view(B, T, ld)
    assert torch.equal(got[0, :, 4:4 + C], pool[3, :, :T].t()) and (got[1:, :, 4:4 + C] == 0).all()
    back = G.cl_to_slots(got.view(B * T, ld)[:, 4:].contiguous(), torch.full_like(pool, 9.0), slots, T)
    assert torch.equal(back[3, :, :T], pool[3, :, :T]) and (back[3, :, T:] == 9).all() and (back[[0, 1, 2, 4]] == 9).all()


def test_alignment_restated_is_the_oracle_on_zero_free_durations_and_skips_empty_tokens(oracle):
    g = torch.Generator().manual_seed(5)
    B, Tx, nf = 3, 37, 20
    x_len = torch.tensor([37, 20, 1])
    x_mask = oracle.sequence_mask(x_len, Tx).unsqueeze(1).double()
    dur = torch.randint(1, 9, (B, Tx), generator=g).double() * x_mask.squeeze(1)
    mu_x = torch.randn(B, nf, Tx, generator=g, dtype=torch.float64) * x_mask
    mu_y_ref, y_mask_ref, y_len_ref, _, t_pad = oracle.align_and_pool(mu_x, dur, x_mask)
    mu_y, y_mask, y_len = G.align_pool(mu_x, dur, t_pad)
    assert torch.equal(y_len, y_len_ref) and torch.equal(y_mask, y_mask_ref) and (mu_y - mu_y_ref).abs().max().item() < 1e-14
    wide, wide_mask, _ = G.align_pool(mu_x, dur, t_pad + 3)             # a longer pad: the same frames, then zeros
    assert torch.equal(wide[:, :, :t_pad], mu_y) and (wide[:, :, t_pad:] == 0).all() and (wide_mask[:, :, t_pad:] == 0).all()
    # tokens of zero frames are skipped: the result is that of the same row with them removed
    d0 = torch.tensor([[2.0, 0.0, 0.0, 3.0, 0.0, 1.0]], dtype=torch.float64)
    m0 = rand(1, 4, 6, seed=1)
    a, _, la = G.align_pool(m0, d0, 6)
    b, _, lb = G.align_pool(m0[:, :, [0, 3, 5]], d0[:, [0, 3, 5]], 6)
    assert torch.equal(a, b) and la.tolist() == lb.tolist() == [3]
    # and the oracle's own path takes zero durations the same way
    ref0 = oracle.align_and_pool(m0, d0, torch.ones(1, 1, 6, dtype=torch.float64))
    assert ref0[4] == 6 and (a - ref0[0]).abs().max().item() < 1e-14

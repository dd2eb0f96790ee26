"""GPU parity of the four small kernels of the speaker-row gradient (csrc/spk_grad.hip) through their unit entries, at sizes the whole
gradient tests do not reach: seed_mu_kernel / seed_logw_kernel (mtts_spk_grad_seeds), gate_kernel in its three modes (mtts_grad_gate)
and colsum_kernel with every argument (mtts_token_sums).  The yardsticks are tests/spk_grad_restated.py, anchored on the CPU by
tests/test_spk_grad_abi.py (the seeds against torch.autograd of the restated losses).

Every tolerance is one of
  * bit equality with a documented order: seed_mu (per token a serial fp32 sum over its frames in frame order), the token sums (four
    phases t = p, p + 4, ..., combined as ((p0 + p1) + p2) + p3), the ReLU gates (a decision, no arithmetic);
  * a derived rounding bound: seed_mu against fp64 within (n + 1) 2^-24 sum|terms| (n frames: one rounding per difference, n - 1
    additions, the sign is exact); the token sums within fp64_bound(ceil(n / 4), n) sum|terms| of tests/test_hip_spk_grad.py;
  * e_hip <= 8 e_cpu32 + floor per element, e_cpu32 the fp32 CPU twin's error against fp64 and the floor derived from the roundings
    of the expression (spk_grad_restated.seed_logw_floor, silu_gate_floor): seed_logw and the SiLU' gate, whose logf / expf differ
    between the device and the CPU's libm.
Nothing is taken from what the device returns.  Every output buffer is filled with a sentinel first and has guard floats behind it.
Every figure is printed (and appended to $MTTS_SPK_GRAD_REPORT: profiles/r32_grad_parity.md) before it is asserted."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import sub
import spk_grad_restated as G

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MTTS_SPK_GRAD_REPORT")
SENT = 7.75e33           # sentinel: what no kernel of this file writes
GUARD = 64               # floats behind every output
U = 2.0 ** -24
DELTA_PRIOR, DELTA_DUR = 0.15625, 0.3125        # 5 / 32 and 5 / 16: |difference| == delta can be hit with representable values


def note(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    h = sub("_hip")
    h.load()
    return h


def fp64_bound(r, n):
    return 2 * (r + math.log2(max(n / r, 1.0)) + 4) * 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def guarded(n, dev="cuda"):
    return torch.full((n + GUARD,), SENT, dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ seeds
def seeds_case(kind):
    """big: B = 6, F = 20, x_len = [1024, 261, 257, 256, 5, 1] -- all 256 scan threads carry data, a wave boundary of the scan falls at
    token 256, the token loop of seed_mu_kernel iterates four times; utterance 0 has zero durations and one long run, utterance 1 sums
    to exactly Tm, utterance 2's durations do not sum to its y_len (refused).  pad: F = 6, so seed_mu has two padding columns.
    Durations beyond x_len are garbage the kernels must not read as data."""
    rng = np.random.default_rng(5 if kind == "big" else 6)
    F, Fd = (20, 70) if kind == "big" else (6, 5)
    x_len = [1024, 261, 257, 256, 5, 1] if kind == "big" else [9, 4, 1, 6]
    B, Tx = len(x_len), max(x_len)
    dur = np.full((B, Tx), 7, dtype=np.int64)
    for b, n in enumerate(x_len):
        dur[b, :n] = rng.integers(0, 5, size=n)
        dur[b, n - 1] += 1
    dur[0, 300 % x_len[0]] = 400 if kind == "big" else 9        # one long run
    dur[0, 1:4] = 0                                              # tokens without a frame
    for b, n in enumerate(x_len):                                # (every utterance has at least as many frames as tokens)
        dur[b, n - 1] += max(0, n - int(dur[b, :n].sum()))
    Tm = (int(dur[0, :x_len[0]].sum()) + 40) // 4 * 4
    dur[1, 2] += Tm - int(dur[1, :x_len[1]].sum())              # utterance 1 sums to exactly Tm
    y_len = np.array([int(dur[b, :n].sum()) for b, n in enumerate(x_len)], dtype=np.int64)
    assert y_len[1] == Tm and y_len.max() == Tm
    y_len[2] += 1                                                # refused: the durations do not sum to y_len
    mu = rng.standard_normal((B, F, Tx)).astype(np.float32)
    logw = np.zeros((B, Tx), dtype=np.float32)
    y = rng.standard_normal((B, F, Tm)).astype(np.float32)       # (frames beyond an utterance: data nobody may add)
    for b, n in enumerate(x_len):
        d = dur[b, :n]
        total = int(d.sum())
        # differences exactly +-delta: mu = 0.5 and y = 0.5 +- 5 / 32 in the features 0 and 1 of every third token
        mu[b, :2, :n:3] = 0.5
        y[b, :, :total] = np.repeat(mu[b, :, :n], d, axis=1) + (0.15 * rng.standard_normal((F, total))).astype(np.float32)
        start = np.cumsum(d) - d
        for x in range(0, n, 3):
            y[b, 0, start[x]:start[x] + d[x]] = np.float32(0.5 + DELTA_PRIOR)
            y[b, 1, start[x]:start[x] + d[x]] = np.float32(0.5 - DELTA_PRIOR)
        target = np.log(np.float32(2) + d.astype(np.float32))
        logw[b, :n] = target + (0.3 * rng.standard_normal(n)).astype(np.float32)
        exact = (np.arange(n) % 5 == 0) & ((d == 0) | (d == 2))          # log 2 and log 4 minus 5 / 16 are exact in fp32
        logw[b, :n][exact] = target[exact] - np.float32(DELTA_DUR)
        logw[b, n:] = 3.0
    assert (np.float32(0.5 + DELTA_PRIOR) - np.float32(0.5) == np.float32(DELTA_PRIOR))
    w = rng.standard_normal(Fd).astype(np.float32)
    return dict(mu=mu, logw=logw, dur=dur, y=y, x_len=x_len, y_len=y_len, w=w, B=B, F=F, Tx=Tx, Tm=Tm, Fd=Fd)


def run_seeds(hip, c, rows=None):
    sel = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(np.asarray(a)[rows]))
    B = len(sel(np.asarray(c["x_len"])))
    ldm = (c["F"] + 3) // 4 * 4
    n_mu, n_lw = B * c["Tx"] * ldm, B * c["Tx"] * c["Fd"]
    seed_mu, seed_lw = guarded(n_mu), guarded(n_lw)
    t = lambda a: torch.from_numpy(sel(a)).cuda().contiguous()
    held = [t(c["mu"]), t(c["logw"]), t(c["dur"].astype(np.int32)), t(c["y"]), t(np.asarray(c["x_len"], dtype=np.int64)), t(c["y_len"]),
            torch.from_numpy(c["w"]).cuda()]
    scratch = hip.spk_grad_seeds(*held, DELTA_PRIOR, DELTA_DUR, seed_mu=seed_mu, seed_logw=seed_lw)
    torch.cuda.synchronize()
    for name, buf, n in (("seed_mu", seed_mu, n_mu), ("seed_logw", seed_lw, n_lw)):
        assert (buf[n:] == SENT).all(), f"{name}: written past the end"
        assert not (buf[:n] == SENT).any(), f"{name}: an element was not written"
    return seed_mu[:n_mu].cpu().numpy().reshape(B * c["Tx"], ldm), seed_lw[:n_lw].cpu().numpy().reshape(B * c["Tx"], c["Fd"]), scratch


@pytest.mark.parametrize("kind", ["big", "pad"])
def test_seed_kernels_against_the_restated_seeds(hip, kind):
    c = seeds_case(kind)
    B, F, Tx, Fd = c["B"], c["F"], c["Tx"], c["Fd"]
    args = (c["mu"], c["logw"], c["dur"], c["y"], c["x_len"], c["y_len"], c["w"], DELTA_PRIOR, DELTA_DUR)
    ref, twin = G.seeds(*args), G.seeds(*args, dtype=np.float32)
    # conditions on the inputs, in fp64, before the device is looked at
    assert ref["verdict"] == [0, 0, 2] + [0] * (B - 3)
    note(f"seeds {kind}: clamped share of the terms mu {ref['clamped_mu']:.3f}, logw {ref['clamped_logw']:.3f}")
    assert 0.1 <= ref["clamped_mu"] <= 0.9 and 0.1 <= ref["clamped_logw"] <= 0.9
    live = ref["n"] > 0
    edge_mu = (np.abs(ref["seed_mu"][:, :2]) == ref["n"][:, None] * DELTA_PRIOR) & live[:, None]
    edge_lw = np.abs(twin["diff"]) == np.float32(DELTA_DUR)     # (in the fp32 order: the target is logf's value)
    assert edge_mu.sum() >= B and edge_lw.sum() >= (3 if kind == "big" else 0)          # |difference| == delta occurs
    assert (ref["n"].reshape(B, Tx)[0, 1:4] == 0).all()
    got_mu, got_lw, scratch = run_seeds(hip, c)
    with pytest.raises(ValueError, match="utterance 2 .*durations that sum to"):
        hip.raise_refused(hip.load().mtts_score_status, scratch.data_ptr(), hip.stream_ptr())
    # seed_mu: the documented fp32 order bit for bit, and the serial-sum bound against fp64
    same = bits(got_mu) == bits(twin["seed_mu"])
    err = np.abs(got_mu.astype(np.float64) - ref["seed_mu"])
    bound = (ref["n"][:, None] + 1) * U * ref["abs_mu"]
    worst = float((err / np.maximum(bound, 1e-300)).max())
    note(f"seed_mu {kind}: {int((~same).sum())} of {same.size} elements differ from the fp32 order; max|err| vs fp64 {err.max():.3e}, "
         f"worst err / bound {worst:.3f} (bound (n + 1) u sum|terms|, n up to {int(ref['n'].max())})")
    assert same.all() and (err <= bound).all()
    # seed_logw: 8 x the CPU twin's error + the derived floor, per element
    e_hip = np.abs(got_lw.astype(np.float64) - ref["seed_logw"])
    e_cpu = np.abs(twin["seed_logw"].astype(np.float64) - ref["seed_logw"])
    bar = 8 * e_cpu + G.seed_logw_floor(ref, c["w"])
    note(f"seed_logw {kind}: max e_hip {e_hip.max():.3e}, max e_cpu32 {e_cpu.max():.3e}, worst e_hip / (8 e_cpu32 + floor) "
         f"{float((e_hip / np.maximum(bar, 1e-300)).max()):.3f}")
    assert (e_hip <= bar).all()
    # exact zeros: tokens beyond an utterance, the padding columns, tokens without a frame, the refused utterance.  seed_mu's are the
    # zero fill's bytes; a seed_logw zero is the product 0 * w_proj[c], whose sign is w_proj's
    mu3, lw3 = got_mu.reshape(B, Tx, -1), got_lw.reshape(B, Tx, Fd)
    for b, n in enumerate(c["x_len"]):
        assert (bits(mu3[b, n:]) == 0).all() and (lw3[b, n:] == 0).all(), b
    assert (bits(mu3[:, :, F:]) == 0).all() and (bits(mu3[2]) == 0).all() and (lw3[2] == 0).all()
    assert (mu3[0, 1:4] == 0).all()                              # (minus an empty sum: -0.0, as the fp32 order has it)
    assert np.abs(mu3[[0, 1] + list(range(3, B))]).max() > 0 and np.abs(lw3[0]).max() > 0
    # the neighbours of the refused utterance: the bits of a run without it
    keep = [b for b in range(B) if b != 2]
    solo_mu, solo_lw, scratch = run_seeds(hip, c, rows=keep)
    hip.raise_refused(hip.load().mtts_score_status, scratch.data_ptr(), hip.stream_ptr())        # nothing refused
    assert (bits(solo_mu.reshape(B - 1, Tx, -1)) == bits(mu3[keep])).all() and (bits(solo_lw.reshape(B - 1, Tx, Fd)) == bits(lw3[keep])).all()


# ------------------------------------------------------------------------------------------------ gates
SPECIAL = [0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -40, 2.0 ** -36, 1.5 * 2.0 ** -36, 2.0 ** -30, 2.0 ** -25, 2.0 ** -24, -(2.0 ** -149),
           -(2.0 ** -36), -(2.0 ** -25), 1.0 + 2.0 ** -11 + 2.0 ** -13, 0.1, 65504.0, 70000.0, -70000.0]


def gate_case(C, M, seed):
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(M, C, generator=g)
    ref[torch.rand(M, C, generator=g) < 0.1] *= 2.0 ** -30       # a tenth of the values far below the fp16 head's range
    ref[torch.rand(M, C, generator=g) < 0.05] *= 2.0 ** -45      # and some below both planes
    for i, v in enumerate(SPECIAL):                              # every special value in a first, a middle and the last row
        for row in (0, M // 2, M - 1):
            ref[row, (3 * i + row) % C] = v
    grad = torch.randn(M, C, generator=g)
    mask = (torch.arange(M) % 3 != 1).float()                    # rows 1, 4, 7, ... masked
    return ref, grad, mask


def run_gate(hip, mode, ref, grad, mask, ldg, ldref):
    M, C = ref.shape
    buf = guarded(M * ldg)
    body = buf[:M * ldg].view(M, ldg)
    body[:, :C] = grad.cuda()
    wide = torch.full((M, ldref), 3.0e30, device="cuda")         # (the pad columns hold a positive value: a wrong stride switches gates on)
    wide[:, :C] = ref.cuda()
    hip.grad_gate(buf, ldg, M, C, mode, wide, mask=None if mask is None else mask.cuda())
    torch.cuda.synchronize()
    assert (buf[M * ldg:] == SENT).all() and (body[:, C:] == SENT).all(), "written outside the rows' C columns"
    return body[:, :C].cpu()


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("mode,C", [(1, 80), (2, 96), (2, 1152)])
def test_relu_gates_are_exact(hip, mode, C, masked):
    """Mode 1 against ref > 0, mode 2 against the restated rule on the restated split: bit for bit.  Mode 2 differs from ref > 0 on
    exactly the positive inputs that flush in both planes."""
    M = 37
    ref, grad, mask = gate_case(C, M, seed=C + mode)
    mask = mask if masked else None
    on, flushed = G.relu_gate(ref, mode, mask)
    plain, _ = G.relu_gate(ref, 1, mask)
    import p16_restated as P
    h, l = P.split(ref if mask is None else ref * mask[:, None])
    h, l = h.float(), l.float()
    if mode == 2:                                                # conditions on the inputs
        assert flushed.sum() >= 3 and ((h > ref) & (l < 0) & on).any() and ((h == 0) & (l > 0) & on).sum() >= 3
        assert torch.equal(on, plain & ~flushed)
    assert (ref[plain] == 2.0 ** -149).any() and (bits(ref.numpy()) == -2 ** 31).any() and 0.2 < on.float().mean() < 0.6
    got = run_gate(hip, mode, ref, grad, mask, ldg=C + 5, ldref=C + 4)
    want = torch.where(on, grad, torch.zeros_like(grad))
    wrong = bits(got.numpy()) != bits(want.numpy())
    diff_plain = int(((got != 0) != plain).sum())
    note(f"gate mode {mode} C={C} {'masked' if masked else 'unmasked'}: {int(wrong.sum())} of {wrong.size} elements differ from the rule; "
         f"{diff_plain} differ from ref > 0 ({int(flushed.sum())} positive inputs flush in both planes)")
    assert not wrong.any()
    assert diff_plain == (int(flushed.sum()) if mode == 2 else 0)
    if masked:
        assert (got[mask == 0] == 0).all()


@pytest.mark.parametrize("C", [80, 96])
def test_silu_gate_against_fp64(hip, C):
    M = 37
    g = torch.Generator().manual_seed(C)
    ref = 3 * torch.randn(M, C, generator=g)
    ref[0, :6] = torch.tensor([0.0, -0.0, 12.0, -12.0, 2.0 ** -30, -1.2784645])       # (the last: where silu' crosses zero)
    grad = torch.randn(M, C, generator=g)
    want = G.silu_gate(grad, ref)
    twin = G.silu_gate(grad, ref, torch.float32)
    got = run_gate(hip, 0, ref, grad, None, ldg=C + 5, ldref=C + 3)
    e_hip, e_cpu = (got.double() - want).abs(), (twin.double() - want).abs()
    bar = 8 * e_cpu + G.silu_gate_floor(grad, ref)
    note(f"gate mode 0 C={C}: max e_hip {e_hip.max().item():.3e}, max e_cpu32 {e_cpu.max().item():.3e}, worst e_hip / (8 e_cpu32 + floor) "
         f"{(e_hip / bar.clamp(min=1e-300)).max().item():.3f}")
    assert (e_hip <= bar).all()


# ------------------------------------------------------------------------------------------------ token sums
@pytest.mark.parametrize("T", [1, 3, 4, 5, 261])
@pytest.mark.parametrize("C", [96, 36, 64, 65])
def test_token_sums_against_the_restated_order(hip, C, T):
    """lengths 0, 1, T, T + 3 (clamped) and -2 (clamped), a refused utterance, without lengths, accumulate 0 and 1, column offsets on both
    sides and rows wider than needed."""
    lengths = [0, 1, T, T + 3, -2, T]
    verdict = [0, 0, 0, 0, 0, 2]
    B, col0, dcol0 = len(lengths), 3, 5
    ld, ldd = col0 + C + 7, dcol0 + C + 2
    g = torch.Generator().manual_seed(1000 * C + T)
    src = torch.randn(B * T, ld, generator=g) * torch.exp2(torch.randint(-6, 7, (B * T, 1), generator=g).float())
    prev = torch.randn(B, ldd, generator=g)
    d_src = src.cuda()
    d_len = torch.tensor(lengths, dtype=torch.long, device="cuda")
    d_ver = torch.tensor([[v, 9] for v in verdict], dtype=torch.int32, device="cuda")
    r = -(-T // 4)                                                # a phase's serial run (a shorter utterance's is shorter)
    for tag, ln, vd, acc in (("plain", None, None, 0), ("ragged", lengths, verdict, 0), ("ragged+acc", lengths, verdict, 1), ("acc", None, None, 1)):
        buf = guarded(B * ldd)
        body = buf[:B * ldd].view(B, ldd)
        if acc:
            body[:, dcol0:dcol0 + C] = prev[:, dcol0:dcol0 + C].cuda()
        hip.token_sums(d_src, col0, C, B, T, buf, ldd, dcol0, lengths=d_len if ln else None, verdict=d_ver if vd else None, accumulate=acc)
        torch.cuda.synchronize()
        assert (buf[B * ldd:] == SENT).all() and (body[:, :dcol0] == SENT).all() and (body[:, dcol0 + C:] == SENT).all(), tag
        got = body[:, dcol0:dcol0 + C].cpu().numpy()
        want32, mag = G.token_sums(src.numpy(), col0, C, B, T, lengths=ln, verdict=vd)
        want64, _ = G.token_sums(src.numpy(), col0, C, B, T, lengths=ln, verdict=vd, dtype=np.float64)
        bound = fp64_bound(r, T) * mag
        if acc:                                                  # one more fp32 addition, onto what the buffer held
            p = prev[:, dcol0:dcol0 + C].numpy()
            want32 = p + want32
            want64 = p.astype(np.float64) + want64
            bound = bound + U * (np.abs(p) + mag)
        same = bits(got) == bits(want32)
        err = np.abs(got.astype(np.float64) - want64)
        note(f"token sums C={C} T={T} {tag}: {int((~same).sum())} of {same.size} differ from the fp32 order; worst err / bound vs fp64 "
             f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert same.all() and (err <= bound).all(), tag
        if ln:
            assert (got[[0, 4, 5]] == (prev[:, dcol0:dcol0 + C].numpy()[[0, 4, 5]] if acc else 0)).all()

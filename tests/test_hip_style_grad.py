"""Parameter gradients of the style encoder on the GPU (csrc/style_grad.hip): the conv weight-gradient kernel against fp64, the taped
forward bit for bit against mtts_style_forward, the backward given the device's own tape against the fp64 restatement, and the whole
parameter gradient against fp64 autograd from the inputs (tests/style_grad_restated.py).

Bounds.
  * Weight-gradient kernel, per element: fp64_bound(r, n) sum|terms| with fp64_bound of tests/test_hip_spk_grad.py, n = B T rows and
    r = the kernel's longest serial accumulation.  The rows are cut into chunks of CHUNK(B, T) = 256 max(1, ceil(B T / 4096)) rows; a
    workgroup feeds ALL rows of its chunk, in row order, into one accumulator of v_mfma_f32_32x32x2_f32 -- an fp32 FMA chain, one
    rounding per term -- and a second kernel adds the chunks in chunk order: r = CHUNK + (chunks - 1).  The bias gradient adds a
    chunk's rows in four interleaved phases, combines them with three additions and then adds the chunks: r = CHUNK / 4 + 3 + chunks - 1.
  * Backward given the tape: the same form at every step, with the bound of a step's inputs carried through the absolute values of
    its factors (style_grad_restated.backward_from_tape).
  * Whole gradient: per tensor err = max|g - g64| / max|g64| <= 8 max(err32, e_fwd); err32 the same quantity for float32 CPU
    autograd, e_fwd the relative error of mtts_style_forward's rows against fp64 on the same inputs (the forward carries 22-bit
    operands); 8 = 4 for operand width x 2 for summation order.
  * Exact cases (sections 1b and 3): small-integer operands whose sums of absolute terms stay below 2^24, checked on the inputs
    before any device call (style_grad_restated.fp32_is_exact_on).  fp32 then has nothing to round in any order, and the device must
    equal the fp64 restatement element for element: torch.equal, no tolerance.  At 19 200 rows the first bound above is about one
    whole term wide (1.55e-4 sum|terms|), so only these cases see a single dropped, doubled or mis-masked row for certain; what they
    cannot see -- where and how the kernel rounds -- stays with the bounded cases, which run at the same shapes
    (profiles/r33_style_grad_shapes.md).
Nothing here is taken from what the device returns.  Every figure is printed (and appended to $MTTS_STYLE_GRAD_REPORT) before it is
asserted."""
import os

import pytest
import torch

from conftest import sub
import style_grad_restated as R

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("MTTS_STYLE_GRAD_REPORT")
SENT = 7.75e33           # sentinel: what no kernel of this file writes
GUARD = 64               # floats behind every output


def note(line):
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


def CHUNK(B, T):
    """Rows per chunk of the reduction: a function of the shape alone."""
    return 256 * max(1, -(-(B * T) // 4096))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def hip(dev):
    h = sub("_hip")
    h.load()
    return h


def make(cfg, seed, dev):
    torch.manual_seed(seed)
    m = sub("style").StyleEncoder(*cfg)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(dev).eval(), sd


def inputs(n_feats, T, lengths, seed):
    mel = torch.randn(len(lengths), n_feats, T, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lengths):
        mel[b, :, n:] = float("nan")          # the padded part is never read as data
    return mel


# ------------------------------------------------------------------------------------------------ 1. the weight-gradient kernel
def run_wgrad(hip, dev, dz, x, lengths, cin, cout):
    """One mtts_conv_wgrad call on sentinel-filled outputs with guard floats behind them -> dw, db, the partial results."""
    lib = hip.load()
    B, T, ldx = x.shape
    need = lib.mtts_conv_wgrad_workspace_bytes(B, T, cin, cout)
    chunks = -(-(B * T) // CHUNK(B, T))
    assert need == 4 * chunks * (5 * cout * cin + cout)
    n_w = cout * cin * 5
    dw = torch.full((n_w + GUARD,), SENT, device=dev)
    db = torch.full((cout + GUARD,), SENT, device=dev)
    ws = torch.full((need // 4 + GUARD,), SENT, device=dev)
    d_dz, d_x = dz.to(dev).contiguous(), x.to(dev).contiguous()
    d_len = None if lengths is None else torch.tensor(lengths, dtype=torch.long, device=dev)
    hip.check(lib.mtts_conv_wgrad(hip.ptr(d_dz), hip.ptr(d_x), hip.ptr(d_len), B, T, cin, ldx, cout, hip.ptr(dw), hip.ptr(db),
                                  ws.data_ptr(), need, hip.stream_ptr()))
    torch.cuda.synchronize()
    for name, buf, n in (("dw", dw, n_w), ("db", db, cout), ("partials", ws, need // 4)):
        assert (buf[n:] == SENT).all(), f"{name}: written past the end"
        assert not (buf[:n] == SENT).any() and torch.isfinite(buf[:n]).all(), f"{name}: an element was not written"
    return dw[:n_w].cpu().reshape(cout, cin, 5), db[:cout].cpu(), ws[:need // 4].cpu()


def check_wgrad(tag, dw, db, dz, x, lengths, cin):
    B, T, _ = x.shape
    full = lengths if lengths is not None else [T] * B
    want, mag = R.conv_wgrad(dz, x[:, :, :cin], full)
    m = R.prefix_mask(full, T)[:, :, None]
    dzm = torch.nan_to_num(dz.double()) * m
    bound_w = R.fp64_bound(R.wgrad_serial_run(B, T), B * T) * mag
    bound_b = R.fp64_bound(R.bias_serial_run(B, T), B * T) * dzm.abs().sum((0, 1))
    err_w, err_b = (dw.double() - want).abs(), (db.double() - dzm.sum((0, 1))).abs()
    worst_w = (err_w / bound_w.clamp(min=1e-300)).max().item() if mag.max() > 0 else 0.0
    worst_b = (err_b / bound_b.clamp(min=1e-300)).max().item() if dzm.abs().max() > 0 else 0.0
    note(f"conv_wgrad {tag}: max|err| {err_w.max().item():.3e} (of max|dW| {want.abs().max().item():.3e}), worst err / bound {worst_w:.3f}; "
         f"bias {err_b.max().item():.3e}, worst err / bound {worst_b:.3f}")
    assert (err_w <= bound_w).all() and (err_b <= bound_b).all()


ROWS = [(5, 51, [51, 0, 1, 2, 30], -1), (4, 64, [64, 2, 0, 1], 0), (1, 257, [257], 1), (5, 103, [103, 0, 1, 2, 77], 259)]


@pytest.mark.parametrize("B,T,lengths,over", ROWS, ids=["chunk-1", "chunk", "chunk+1", "2chunks+3"])
@pytest.mark.parametrize("cin,cout", [(100, 256), (256, 256), (20, 32), (4, 4)])
def test_conv_wgrad_against_fp64(hip, dev, cin, cout, B, T, lengths, over):
    """Row counts around the chunk length (255, 256, 257 and 2 x 256 + 3 rows), lengths 0, 1, 2 (shorter than the tap span) and T,
    channel counts that are no multiple of the 64-wide tile and as small as 4, NaN wherever nothing may be read as data (frames at
    t >= len_b of both operands, the padding columns of X)."""
    assert CHUNK(B, T) == 256 == R.chunk_rows(B, T) and B * T == 256 + over
    g = torch.Generator().manual_seed(1000 * cin + cout + T)
    ldx = cin + 4
    x = torch.randn(B, T, ldx, generator=g)
    dz = torch.randn(B, T, cout, generator=g)
    x[:, :, cin:] = float("nan")
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")
        dz[b, n:] = float("nan")
    dw, db, part = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
    check_wgrad(f"({cin}, {cout}) B={B} T={T}", dw, db, dz, x, lengths, cin)
    dw2, db2, part2 = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(part, part2)      # two calls: the same bits


@pytest.mark.parametrize("cin,cout", [(100, 256), (4, 4)])
def test_conv_wgrad_clips_adjacent_in_memory_do_not_see_each_other(hip, dev, cin, cout):
    """Two full-length clips, lengths given and not given: row T - 1 of clip 0 and row 0 of clip 1 are neighbours in memory and hold
    values 1e4 times the rest in X.  A tap that crossed the boundary would add terms 1e4 / bound times larger than the bound."""
    B, T = 2, 130                                    # 260 rows: the clip boundary (row 130) and the chunk boundary (row 256) differ
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(B, T, cin, generator=g)
    dz = torch.randn(B, T, cout, generator=g)
    x[0, T - 2:] *= 1e4
    x[1, :2] *= 1e4
    for lengths in ([T, T], None):
        dw, db, _ = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
        check_wgrad(f"boundary ({cin}, {cout}) lengths={'given' if lengths else 'null'}", dw, db, dz, x, lengths, cin)


# ------------------------------------------------------------------------------------------------ 1b. beyond one chunk length
# The row counts of training (style_grad_restated.WGRAD_ROWS: 4096 .. 19 200 rows, chunk lengths 256 .. 1280, up to 16 chunks) and clips
# shorter than the tap span.  At these sizes the bound above is wider than one whole term, so every shape is ALSO run on small
# integers, where fp32 has nothing to round: there the device must give the fp64 restatement itself, chunk by chunk and in total.
def normal_wgrad_case(B, T, lengths, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, cin + 4, generator=g)
    dz = torch.randn(B, T, cout, generator=g)
    x[:, :, cin:] = float("nan")
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")
        dz[b, n:] = float("nan")
    return dz, x


def check_wgrad_exact(tag, hip, dev, B, T, lengths, cin, cout, seed):
    """Integer operands: every chunk's partial result left in the workspace, dw and db equal the fp64 restatement exactly."""
    full = lengths if lengths is not None else [T] * B
    dz, x = R.integer_wgrad_case(B, T, full, cin, cout, seed)
    sums = R.wgrad_abs_sums(dz, x[:, :, :cin], full)
    assert R.fp32_is_exact_on(sums, dz, x), sums                                  # the condition on the inputs, before any device call
    chunk = R.chunk_rows(B, T)
    want_w, _, want_b, _ = R.conv_wgrad_by_chunk(dz, x[:, :, :cin], full, chunk)
    chunks = want_w.shape[0]
    dw, db, part = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
    n_w = chunks * 5 * cout * cin
    part_w = part[:n_w].reshape(chunks, 5, cout, cin).permute(0, 2, 3, 1).double()
    part_b = part[n_w:].reshape(chunks, cout).double()
    bad_w = [c for c in range(chunks) if not torch.equal(part_w[c], want_w[c])]
    bad_b = [c for c in range(chunks) if not torch.equal(part_b[c], want_b[c])]
    d_w, d_b = (dw.double() - want_w.sum(0)).abs().max().item(), (db.double() - want_b.sum(0)).abs().max().item()
    note(f"conv_wgrad integers {tag}: chunk {chunk} x {chunks}, largest sum of |terms| dW {sums['dW']:.0f} bias {sums['d bias']:.0f}, "
         f"max|dW| {want_w.sum(0).abs().max().item():.0f}; max|dW - fp64| {d_w:g}, max|db - fp64| {d_b:g}, chunks with a wrong partial: "
         f"dW {bad_w} bias {bad_b}")
    assert not bad_w and not bad_b, f"wrong partial results in chunks {bad_w} (dW) {bad_b} (bias)"
    assert torch.equal(dw.double(), want_w.sum(0)) and torch.equal(db.double(), want_b.sum(0)), "exact partials, a wrong sum over the chunks"
    dw2, db2, part2 = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(part, part2)      # two calls: the same bits


def check_wgrad_bounded(tag, hip, dev, B, T, lengths, cin, cout, seed):
    """Unit-normal operands: the bound of the file's head with the serial runs at the real chunk length."""
    dz, x = normal_wgrad_case(B, T, lengths if lengths is not None else [T] * B, cin, cout, seed)
    dw, db, part = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
    check_wgrad(tag, dw, db, dz, x, lengths, cin)
    dw2, db2, part2 = run_wgrad(hip, dev, dz, x, lengths, cin, cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(part, part2)


def chunk_of(hip, B, T):
    ch = hip.load().mtts_conv_wgrad_chunk_rows(B, T)
    assert ch == CHUNK(B, T) == R.chunk_rows(B, T)
    return ch


WGRAD_IDS = [f"{rows}rows-{cin}x{cout}" for rows, cin, cout in R.WGRAD_CASES]


@pytest.mark.parametrize("rows,cin,cout", R.WGRAD_CASES, ids=WGRAD_IDS)
def test_conv_wgrad_training_rows_exact_on_integers(hip, dev, rows, cin, cout):
    """4096 rows (16 chunks of 256), 4097 (the last of 9 chunks holds one row), 8192 (16 of 512), 8193 (the last chunk ends in a slab
    of one row; clip boundaries on no slab or chunk boundary) and 19 200 = 32 x 600, the measured training step (15 chunks of 1280).
    Lengths T, 0, 1, 2 and draws between where the batch has room for them (4097 rows are one clip; 8193 are T, 2, T)."""
    B, T, lengths = R.WGRAD_ROWS[rows]
    assert B * T == rows and chunk_of(hip, B, T) == {4096: 256, 4097: 512, 8192: 512, 8193: 768, 19200: 1280}[rows]
    check_wgrad_exact(f"({cin}, {cout}) B={B} T={T}", hip, dev, B, T, lengths, cin, cout, rows + cin)


@pytest.mark.parametrize("rows,cin,cout", R.WGRAD_CASES, ids=WGRAD_IDS)
def test_conv_wgrad_training_rows_against_fp64(hip, dev, rows, cin, cout):
    B, T, lengths = R.WGRAD_ROWS[rows]
    assert B * T == rows and chunk_of(hip, B, T) == {4096: 256, 4097: 512, 8192: 512, 8193: 768, 19200: 1280}[rows]
    check_wgrad_bounded(f"({cin}, {cout}) B={B} T={T} chunk {R.chunk_rows(B, T)}", hip, dev, B, T, lengths, cin, cout, rows + cout)


@pytest.mark.parametrize("B,T,cin,cout", R.SHORT_CASES, ids=[f"{B}x{T}-{cin}x{cout}" for B, T, cin, cout in R.SHORT_CASES])
def test_conv_wgrad_clips_shorter_than_the_tap_span(hip, dev, B, T, cin, cout):
    """Clips of T = 1, 2, 3 frames, lengths drawn from 0 .. T and, with no lengths given, all full: every tap but the centre one
    leaves a 1-frame clip, and one 4-row stride of the bias kernel crosses up to four clips.  Exact on integers, bounded on normals."""
    assert chunk_of(hip, B, T) == 256 and B * T > 256
    for lengths, how in ((R.short_lengths(B, T), "given"), (None, "null")):
        tag = f"short ({cin}, {cout}) B={B} T={T} lengths={how}"
        check_wgrad_exact(tag, hip, dev, B, T, lengths, cin, cout, B)
        check_wgrad_bounded(tag, hip, dev, B, T, lengths, cin, cout, B + 1)


# ------------------------------------------------------------------------------------------------ 2. the tape
CONFIGS = {"prod": (100, 256, 4, 96), "tiny": (20, 32, 2, 16)}


@pytest.mark.parametrize("size", ["prod", "tiny"])
def test_taped_forward_is_the_forward_bit_for_bit(dev, size):
    cfg = CONFIGS[size]
    model, _ = make(cfg, 5, dev)
    lengths, T = [120, 57, 0, 3], 120
    mel = inputs(cfg[0], T, lengths, 6).to(dev)
    e_enc, e_dur = model(mel, lengths=lengths)
    t_enc, t_dur = model.forward_taped(mel, lengths=lengths)
    assert torch.equal(e_enc, t_enc) and torch.equal(e_dur, t_dur)
    # the tape: the masked input rows are the mel itself, nothing of an empty clip or beyond a clip's length is non-zero
    m = R.prefix_mask(lengths, T, torch.float32)
    x0 = model.tape(0).reshape(4, T, -1).cpu()
    assert torch.equal(x0[:, :, :cfg[0]], torch.nan_to_num(mel.cpu()).transpose(1, 2) * m[:, :, None])
    for l in range(cfg[2]):
        h = model.tape(1 + l).reshape(4, T, cfg[1]).cpu()
        assert torch.isfinite(h).all() and (h >= 0).all() and (h * (1 - m[:, :, None]) == 0).all() and h[0].max() > 0
    pooled = model.tape(cfg[2] + 1).cpu()
    assert (pooled[2] == 0).all() and torch.isfinite(pooled).all()
    assert torch.equal(model.tape(cfg[2] + 2).reshape(4, T).cpu(), m)


# ------------------------------------------------------------------------------------------------ 3. the backward given the tape
def read_tape(model, cfg, B, T):
    x0 = model.tape(0).reshape(B, T, -1)[:, :, :cfg[0]].cpu()
    hs = [model.tape(1 + l).reshape(B, T, cfg[1]).cpu() for l in range(cfg[2])]
    return x0, hs, model.tape(cfg[2] + 1).cpu()


def split(model, flat):
    out = {}
    for k, off, shape in model.parameter_layout():
        n = 1
        for d in shape:
            n *= d
        out[k] = flat[off:off + n].reshape(shape).cpu()
    return out


@pytest.mark.parametrize("size", ["prod", "tiny"])
def test_backward_given_the_tape_against_fp64(dev, size):
    """The restatement takes the device's own activations as constants, so no ReLU gate differs between the two sides; every element of
    every parameter tensor then stays within the carried bound."""
    check_backward_given_the_tape(dev, size, size, [70, 33, 0, 2], 70)


def test_backward_given_the_tape_against_fp64_at_a_training_batch(dev):
    """The same body at tiny, B = 32, T = 150: 4800 rows, 10 chunks of 512, ragged lengths with 0 and 2 among them."""
    lengths = R.ragged(32, 150, 4)
    assert 0 in lengths and 2 in lengths and R.chunk_rows(32, 150) == 512
    check_backward_given_the_tape(dev, "tiny", "tiny B=32 T=150", lengths, 150)


def check_backward_given_the_tape(dev, size, tag, lengths, T):
    cfg = CONFIGS[size]
    model, sd = make(cfg, 7, dev)
    B = len(lengths)
    mel = inputs(cfg[0], T, lengths, 8).to(dev)
    g = torch.Generator().manual_seed(9)
    g_enc, g_dur = torch.randn(B, cfg[3], generator=g), torch.randn(B, cfg[3], generator=g)
    model.forward_taped(mel, lengths=lengths)
    flat = model.backward(g_enc.to(dev), g_dur.to(dev))
    again = model.backward(g_enc.to(dev), g_dur.to(dev))
    assert torch.equal(flat, again) and torch.isfinite(flat).all()
    got = split(model, flat)
    want, bounds = R.backward_from_tape(sd, *read_tape(model, cfg, B, T), lengths, g_enc, g_dur)
    for k in R.param_names(cfg[2]):
        err = (got[k].double() - want[k]).abs()
        worst = (err / bounds[k].clamp(min=1e-300)).max().item()
        note(f"style backward from tape [{tag}] {k}: max|err| {err.max().item():.3e} of max|g| {want[k].abs().max().item():.3e}, "
             f"worst err / bound {worst:.3f}")
        assert (err <= bounds[k]).all(), k


def write_tape(model, cfg, B, T, x0, hs, pooled, lengths):
    """Overwrite what forward_taped kept, in the workspace tensor the module holds, at mtts_style_grad_tape_offset: the masked input
    rows (padding columns zero), every layer's ReLU output, the pooled rows, the prefix mask."""
    hipm = sub("_hip")
    ws = model._tape[3]
    L = cfg[2]
    ldx = (cfg[0] + 3) // 4 * 4
    regions = {0: torch.nn.functional.pad(x0, (0, ldx - cfg[0])), L + 1: pooled, L + 2: R.prefix_mask(lengths, T, torch.float32)}
    regions.update({1 + l: hs[l] for l in range(L)})
    with torch.inference_mode():
        for which, t in regions.items():
            off = hipm.size(hipm.load().mtts_style_grad_tape_offset(model._ctx, B, T, which))
            ws[off:off + 4 * t.numel()].view(torch.float32).copy_(t.reshape(-1).to(ws.device))
    for which, t in regions.items():
        assert torch.equal(model.tape(which).cpu().reshape(-1), t.reshape(-1)), which


@pytest.mark.parametrize("size", ["prod", "tiny"])
def test_backward_on_an_integer_tape_is_exact(dev, size):
    """mtts_style_backward on a HAND-WRITTEN integer tape (style_grad_restated.integer_tape_case), 4800 rows in 10 chunks of 512, a
    batch of 32 (tiny) and of 8 (prod): sparse weights in {-1, 0, 1}, integer activations, lengths in {0, 1, 2, 4 .. 128} and
    upstream rows that are multiples of them, so that every quantity of the chain -- projection gradients, d pooled, the mean pool's
    factor, every gate, data gradient, weight and bias gradient -- is an integer whose terms' absolute values add up to less than
    2^24.  fp32 has nothing to round: every element of every parameter gradient equals the fp64 restatement."""
    cfg, B, T, lengths = R.TAPE_CASES[size]
    assert cfg == CONFIGS[size]
    sd, x0, hs, pooled, g_enc, g_dur = R.integer_tape_case(cfg, B, T, lengths, 5)
    sums = R.tape_abs_sums(sd, x0, hs, pooled, lengths, g_enc, g_dur)
    assert R.fp32_is_exact_on(sums, *sd.values(), x0, *hs, pooled, g_enc, g_dur), sums     # the condition on the inputs, before any device call
    want, _ = R.backward_from_tape(sd, x0, hs, pooled, lengths, g_enc, g_dur)
    model = sub("style").StyleEncoder(*cfg)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    model.forward_taped(torch.zeros(B, cfg[0], T, device=dev), lengths=lengths)      # allocates the workspace, uploads the weights
    write_tape(model, cfg, B, T, x0, hs, pooled, lengths)
    flat = model.backward(g_enc.to(dev), g_dur.to(dev))
    again = model.backward(g_enc.to(dev), g_dur.to(dev))
    got = split(model, flat)
    note(f"style backward on an integer tape [{size}] B={B} T={T}: largest sum of |terms| {max(sums.values()):.0f} "
         f"({max(sums, key=sums.get)}) of 2^24 = {R.EXACT_BELOW:.0f}")
    wrong = []
    for k in R.param_names(cfg[2]):
        diff = (got[k].double() - want[k]).abs()
        note(f"style backward on an integer tape [{size}] {k}: max|g| {want[k].abs().max().item():.0f}, elements that differ "
             f"{int((diff != 0).sum())} of {diff.numel()}, max|g - fp64| {diff.max().item():g}")
        if not torch.equal(got[k].double(), want[k]):
            wrong.append(k)
    assert not wrong, wrong
    assert torch.equal(flat, again)


def test_an_empty_clip_contributes_exactly_zero(dev):
    """Upstream gradients on the empty clip alone: its rows are the projections' biases, so the two bias gradients are its upstream
    rows and every other gradient is exactly zero."""
    cfg = CONFIGS["tiny"]
    model, _ = make(cfg, 7, dev)
    lengths, T = [70, 33, 0, 2], 70
    mel = inputs(cfg[0], T, lengths, 8).to(dev)
    g_enc, g_dur = torch.zeros(4, cfg[3]), torch.zeros(4, cfg[3])
    g_enc[2], g_dur[2] = torch.randn(cfg[3], generator=torch.Generator().manual_seed(1)), torch.randn(cfg[3], generator=torch.Generator().manual_seed(2))
    model.forward_taped(mel, lengths=lengths)
    got = split(model, model.backward(g_enc.to(dev), g_dur.to(dev)))
    for k, v in got.items():
        if k == "proj_enc.bias":
            assert torch.equal(v, g_enc[2])
        elif k == "proj_dur.bias":
            assert torch.equal(v, g_dur[2])
        else:
            assert (v == 0).all(), k


# ------------------------------------------------------------------------------------------------ 4. the whole parameter gradient
WHOLE = {"prod": (300, [300, 157, 2]), "tiny": (70, [70, 33, 0])}


@pytest.mark.parametrize("size", ["prod", "tiny"])
def test_whole_parameter_gradient_against_fp64_autograd(dev, size):
    cfg = CONFIGS[size]
    T, lengths = WHOLE[size]
    B = len(lengths)
    model, sd = make(cfg, 11, dev)
    mel = inputs(cfg[0], T, lengths, 12)
    g = torch.Generator().manual_seed(13)
    g_enc, g_dur = torch.randn(B, cfg[3], generator=g), torch.randn(B, cfg[3], generator=g)
    clean = torch.nan_to_num(mel)
    g64, e64 = R.style_param_grads(sd, clean, lengths, g_enc, g_dur)
    g32, _ = R.style_param_grads(sd, clean, lengths, g_enc, g_dur, dtype=torch.float32)
    rows = model(mel.to(dev), lengths=lengths)                         # the parent's forward entry
    e_fwd = max((r.cpu().double() - e).abs().max().item() / e.abs().max().item() for r, e in zip(rows, e64))
    t_rows = model.forward_taped(mel.to(dev), lengths=lengths)
    assert torch.equal(t_rows[0], rows[0]) and torch.equal(t_rows[1], rows[1])
    got = split(model, model.backward(g_enc.to(dev), g_dur.to(dev)))
    note(f"style gradient [{size}] e_fwd {e_fwd:.3e}")
    failed = []
    for k in R.param_names(cfg[2]):
        top = g64[k].abs().max().item()
        err = (got[k].double() - g64[k]).abs().max().item() / top
        err32 = (g32[k].double() - g64[k]).abs().max().item() / top
        bound = 8 * max(err32, e_fwd)
        note(f"style gradient [{size}] {k}: err {err:.3e}, err32 {err32:.3e}, bound {bound:.3e}")
        if not err <= bound:
            failed.append(k)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ 5. the matching loss
BETA_MU, BETA_LOGW = 0.002, 0.004           # the reference's (style_encoder.py:133-139)


def test_match_seed_and_sum_kernels_against_fp64(hip, dev):
    """The seed and sum kernels on given buffers: differences in the linear region, the saturated region and at |d| == beta exactly
    (reference value 0, so the fp32 subtraction is exact), lengths Tx, 65, 1 and a refused 0.  Per element: a seed is one rounded
    subtraction and one rounded division, |err| <= 3 u |seed|; times the projection weight, one more rounding.  The sums: every term
    carries at most 4 roundings, and they are added with serial runs of r = ceil(Tx / 256) + ceil(F / 64) (a thread's tokens, then a
    lane's features; the butterflies and the four waves are the log term) for mu and ceil(Tx / 64) for logw."""
    lib = hip.load()
    B, F, Tx, Fd = 4, 100, 300, 5
    lengths = [300, 65, 1, 0]
    g = torch.Generator().manual_seed(21)
    out = {}
    for name, shape, beta in (("mu", (B, F, Tx), BETA_MU), ("logw", (B, Tx), BETA_LOGW)):
        ref = torch.randn(shape, generator=g)
        kind = torch.randint(0, 3, shape, generator=g)
        sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
        d = torch.where(kind == 0, 0.9 * beta * torch.rand(shape, generator=g), beta * (1.5 + 50 * torch.rand(shape, generator=g))) * sign
        val = ref + d
        exact = kind == 2
        ref[exact] = 0.0
        val[exact] = (torch.tensor(beta, dtype=torch.float32) * sign)[exact]
        out[name] = (val, ref)
    w_proj = torch.randn(Fd, generator=g)
    d_len = torch.tensor(lengths, dtype=torch.long, device=dev)
    bufs = {k: torch.full(s, SENT, device=dev) for k, s in (("seed_mu", (B * Tx, F)), ("seed_logw", (B * Tx, Fd)), ("ac", (B,)), ("rh", (B,)))}
    scratch = torch.empty(lib.mtts_match_seeds_scratch_bytes(B, F), dtype=torch.uint8, device=dev)
    held = [t.to(dev).contiguous() for t in (out["mu"][0], out["mu"][1], out["logw"][0], out["logw"][1], w_proj)]     # (alive across the call)
    hip.check(lib.mtts_match_seeds(hip.ptr(held[0]), hip.ptr(held[1]), hip.ptr(held[2]), hip.ptr(held[3]),
                                   hip.ptr(d_len), hip.ptr(held[4]), B, F, Tx, Fd, BETA_MU, BETA_LOGW, hip.ptr(bufs["seed_mu"]),
                                   hip.ptr(bufs["seed_logw"]), hip.ptr(bufs["ac"]), hip.ptr(bufs["rh"]), scratch.data_ptr(), hip.stream_ptr()))
    torch.cuda.synchronize()
    ok = torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=torch.float64)            # the utterance of length 0 is refused: zeros
    mask = R.prefix_mask(lengths, Tx) * ok[:, None]
    b_mu, b_lw = float(torch.tensor(BETA_MU, dtype=torch.float32)), float(torch.tensor(BETA_LOGW, dtype=torch.float32))
    d_mu = (out["mu"][0].double() - out["mu"][1].double()) * mask[:, None, :]
    d_lw = (out["logw"][0].double() - out["logw"][1].double()) * mask
    for d, beta in ((d_mu, b_mu), (d_lw, b_lw)):                             # the condition on the inputs: all three regimes occur
        live = d[d != 0].abs()
        assert (live < beta).any() and (live > beta).any() and (live == beta).any()
    seed_mu = R.smooth_l1_seed(d_mu, b_mu).permute(0, 2, 1).reshape(B * Tx, F)
    seed_lw = R.smooth_l1_seed(d_lw, b_lw).reshape(B * Tx, 1) * w_proj.double()[None, :]
    for name, got, want, k in (("seed_mu", bufs["seed_mu"], seed_mu, 3), ("seed_logw", bufs["seed_logw"], seed_lw, 4)):
        err = (got.cpu().double() - want).abs()
        note(f"match {name}: max|err| {err.max().item():.3e}, worst err / bound {(err / (k * R.U * want.abs()).clamp(min=1e-300)).max().item():.3f}")
        assert (err <= k * R.U * want.abs()).all(), name
    ac = R.smooth_l1_terms(d_mu, b_mu).sum((1, 2))
    rh = R.smooth_l1_terms(d_lw, b_lw).sum(1)
    for name, got, want, r, n in (("ac_sum", bufs["ac"], ac, -(-Tx // 256) + -(-F // 64), F * Tx), ("rh_sum", bufs["rh"], rh, -(-Tx // 64), Tx)):
        err = (got.cpu().double() - want).abs()
        bound = (R.fp64_bound(r, n) + 4 * R.U) * want
        note(f"match {name}: {got.cpu().tolist()} err {err.tolist()} bound {bound.tolist()}")
        assert (err <= bound).all() and got[3] == 0, name


def make_tts(hp, sd, dev):
    m = sub("inference").MatchaTTSInfer(**hp.as_reference_kwargs())
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module", params=["tiny", "prod"])
def tts(request, hparams, synthetic, dev):
    hp = hparams.tiny(n_spks=3) if request.param == "tiny" else hparams.prod_v20(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)      # a duration projection that is not zero: logw depends on e_dur
    return request.param, hp, sd, make_tts(hp, sd, dev)


X_LENGTHS = [14, 9, 1, 12, 5]


X_LONG = [261, 130, 1, 64]         # 1044 rows: nine 128-row GEMM tiles, a partly live third attention-backward workgroup, tokens beyond 256


def match_case(hp, sd, synthetic, seed=41, lengths=X_LENGTHS):
    x, x_len, spk = synthetic.make_inputs(hp, len(lengths), max(lengths), seed=seed, lengths=lengths)
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(len(lengths), hp.spk_emb_dim, generator=g), torch.randn(len(lengths), hp.spk_emb_dim, generator=g))
    return x, x_len, spk, pred


def test_match_gradient_against_fp64_autograd(tts, synthetic, oracle, dev):
    """End to end through model.style_match_grad, random (unit normal) predicted rows, the restatement on the device's own mu_ref /
    logw_ref as constants; the 8 x err32 rule of tests/test_hip_spk_grad.py.

    The condition on the inputs, checked in fp64: at least 95 % of the seeds of either loss are saturated.  A seed in the linear
    region is (out - ref) / beta: it turns the forward's rounding error -- of any arithmetic, the CPU's fp32 included -- into a
    gradient error 1 / beta = 250 .. 500 times larger, and err32 then records fp32's luck at that token, not the unit of the
    backward's error.  (Rows drawn at the speaker table's scale, 0.53, left one of the 41 logw seeds of the tiny model linear: err32
    of g_dur was 7.1e-7 against the device's reference outputs and 5.8e-6 against the oracle's own, the device's 5.7e-6 -- a logw
    off by 2e-8 -- and the ratio 8.05.)  The linear region and |d| == beta are held per element by the seed-kernel test above."""
    size, hp, sd, model = tts
    check_match_gradient(size, hp, sd, model, match_case(hp, sd, synthetic), oracle, dev)


def test_match_gradient_against_fp64_autograd_beyond_one_tile(hparams, synthetic, oracle, dev):
    """The same check with the same bounds on the tiny model at lengths [261, 130, 1, 64].  Seed 41, the short case's: in fp64 on the
    CPU (the oracle's own outputs under the real rows as the constants) 0.996 of the mu seeds and 0.996 of the logw seeds are
    saturated; the test asserts the condition again on the device's constants."""
    hp = hparams.tiny(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    check_match_gradient("tiny long", hp, sd, make_tts(hp, sd, dev), match_case(hp, sd, synthetic, lengths=X_LONG), oracle, dev)


def check_match_gradient(size, hp, sd, model, case, oracle, dev):
    x, x_len, spk, pred = case
    got = model.style_match_grad(x.to(dev), x_len.to(dev), (pred[0].to(dev), pred[1].to(dev)), speaker=spk.to(dev))
    mu_ref, logw_ref = got["mu_ref"].cpu(), got["logw_ref"].cpu()
    ref = R.match_grad(oracle, sd, hp, x, x_len, pred[0], pred[1], mu_ref, logw_ref, BETA_MU, BETA_LOGW)
    cpu32 = R.match_grad(oracle, sd, hp, x, x_len, pred[0], pred[1], mu_ref, logw_ref, BETA_MU, BETA_LOGW, dtype=torch.float32)
    mask = R.prefix_mask(x_len, x.shape[1])[:, None, :].bool()
    sat = ((ref["mu_x"] - mu_ref.double()).abs() >= BETA_MU)[mask.expand_as(ref["mu_x"])].double().mean().item()
    sat_w = ((ref["logw"] - logw_ref.double().reshape(ref["logw"].shape)).abs() >= BETA_LOGW)[mask].double().mean().item()
    note(f"match gradient {size}: saturated share of the seeds mu {sat:.3f}, logw {sat_w:.3f}")
    assert sat >= 0.95 and sat_w >= 0.95
    tokens = float(x_len.sum())
    for name, total in (("acoustic_loss", ref["ac_sum"].sum() / tokens), ("rhythm_loss", ref["rh_sum"].sum() / tokens)):
        note(f"match gradient {size} {name}: device {got[name].item():.6e}, fp64 {total.item():.6e}")
    worst = []
    for name in ("g_enc", "g_dur"):
        err32 = float(R.row_error(cpu32[name], ref[name]).max())
        err = float(R.row_error(got[name], ref[name]).max())
        note(f"match gradient vs fp64 {size} {name}: err32 {err32:.3e}, device {err:.3e}, ratio {err / err32:.2f} (bound 8)")
        worst.append((name, err, err32))
    for name, total in (("ac_sum", ref["ac_sum"]), ("rh_sum", ref["rh_sum"])):
        err32 = float(((cpu32[name].double() - total).abs() / total.abs()).max())
        err = float(((got[name].cpu().double() - total).abs() / total.abs()).max())
        note(f"match sums vs fp64 {size} {name}: err32 {err32:.3e}, device {err:.3e}")
        worst.append((name, err, err32))
    for name, err, err32 in worst:
        assert err <= 8 * err32, (size, name, err, err32)
    e_enc, e_dur = sd["speaker_embeddings_enc.weight"][spk], sd["speaker_embeddings_dur.weight"][spk]
    assert abs(got["emb_dist_enc"].item() - (pred[0] - e_enc).pow(2).mean(1).sqrt().mean().item()) <= 1e-5
    assert abs(got["emb_dist_dur"].item() - (pred[1] - e_dur).pow(2).mean(1).sqrt().mean().item()) <= 1e-5


def test_match_is_exactly_zero_at_the_real_rows(tts, synthetic, dev):
    """Predicted rows equal to the real rows: the taped forward is mtts_text_encoder_forward's bits, so every difference, both sums and
    both gradients are exactly zero."""
    size, hp, sd, model = tts
    x, x_len, spk, _ = match_case(hp, sd, synthetic)
    real = (sd["speaker_embeddings_enc.weight"][spk].to(dev), sd["speaker_embeddings_dur.weight"][spk].to(dev))
    got = model.style_match_grad(x.to(dev), x_len.to(dev), real, speaker=spk.to(dev))
    for k in ("g_enc", "g_dur", "ac_sum", "rh_sum"):
        assert (got[k] == 0).all(), k
    assert got["acoustic_loss"].item() == 0 and got["rhythm_loss"].item() == 0 and got["emb_dist_enc"].item() == 0


def match_device(model, dev, x, x_len, spk, pred, sd, rows=None, **kw):
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    n = int(sel(x_len).max()) if rows is not None else x.shape[1]
    hipm = model.hip
    xs, xl = sel(x)[:, :n].contiguous().to(dev), sel(x_len).to(dev)
    e_enc, e_dur = sel(sd["speaker_embeddings_enc.weight"][spk]).to(dev), sel(sd["speaker_embeddings_dur.weight"][spk]).to(dev)
    mu_ref, logw_ref, _ = hipm.text_encoder(xs, xl.clamp(1, n), e_enc, e_dur)
    return hipm.speaker_grad_match(xs, xl, sel(pred[0]).to(dev), sel(pred[1]).to(dev), mu_ref, logw_ref, BETA_MU, BETA_LOGW, **kw)


def test_match_rows_do_not_depend_on_the_batch(tts, synthetic, dev):
    size, hp, sd, model = tts
    x, x_len, spk, pred = match_case(hp, sd, synthetic, seed=43)
    whole = {k: v.clone() for k, v in match_device(model, dev, x, x_len, spk, pred, sd).items()}
    again = match_device(model, dev, x, x_len, spk, pred, sd)
    for k in ("g_enc", "g_dur", "ac_sum", "rh_sum"):
        assert torch.equal(whole[k], again[k]), k
    assert whole["g_enc"].abs().max() > 0 and whole["g_dur"].abs().max() > 0
    for b in range(len(X_LENGTHS)):
        solo = match_device(model, dev, x, x_len, spk, pred, sd, rows=[b])
        for k in ("g_enc", "g_dur", "ac_sum", "rh_sum"):
            assert torch.equal(solo[k][0], whole[k][b]), (k, b)


def test_match_refused_row_is_named_and_the_others_are_unaffected(tts, synthetic, dev):
    size, hp, sd, model = tts
    x, x_len, spk, pred = match_case(hp, sd, synthetic, seed=43)
    good = {k: v.clone() for k, v in match_device(model, dev, x, x_len, spk, pred, sd).items()}
    for bad in (0, x.shape[1] + 1):
        broken = x_len.clone()
        broken[1] = bad
        out = match_device(model, dev, x, broken, spk, pred, sd, check_lengths=False)
        with pytest.raises(ValueError, match="utterance 1 has x_length = %d" % bad):
            model.hip._status("spk_grad_match", model.hip.lib.mtts_spk_grad_match_status)
        keep = [b for b in range(len(X_LENGTHS)) if b != 1]
        for k in ("g_enc", "g_dur", "ac_sum", "rh_sum"):
            assert (out[k][1] == 0).all(), k
            assert torch.equal(out[k][keep], good[k][keep]), k
    with pytest.raises(ValueError, match="utterance 1 "):
        broken = x_len.clone()
        broken[1] = 0
        model.style_match_grad(x.to(dev), broken.to(dev), (pred[0].to(dev), pred[1].to(dev)), speaker=spk.to(dev))


# ------------------------------------------------------------------------------------------------ 6. the trainer
STYLE_TINY = (20, 32, 2, 16)


def train_batches(hp, synthetic, steps=5):
    """One small ragged batch per step: texts of 3 utterances with the fine mels of their clips (random mels: the encoder sees them
    through its own convolutions, nothing else reads them)."""
    out = []
    for k in range(steps):
        x, x_len, spk = synthetic.make_inputs(hp, 3, 11, seed=60 + k, lengths=[11, 6, 1])
        mel_len = torch.tensor([50, 33, 2])
        mel = torch.randn(3, hp.n_feats, 50, generator=torch.Generator().manual_seed(70 + k))
        for b, n in enumerate(mel_len.tolist()):
            mel[b, :, n:] = 0.0
        out.append((x, x_len, mel, mel_len, spk))
    return out


def test_trainer_steps_follow_the_restated_fp64_loop(hparams, synthetic, oracle, dev, tmp_path):
    """Five StyleTrainer.step calls on the tiny model against the restated fp64 loop (torch autograd through the oracle, the restated
    AdamW): the loss history, and every parameter tensor's total update after the fifth step.

    Tolerance: the margin of the whole-gradient test, 8 max(err32, e_fwd), PER STEP, COMPOUNDED: err32_j is the error at step j of the
    same restated loop run in float32 on the CPU (for a loss |l - l64| / l64, for a tensor max|dp - dp64| / max|dp64| of its update
    dp = p_j - p_0), e_fwd the relative error of the device's style rows against fp64 before the first step, and the device must
    stay within prod_{j <= k} (1 + 8 max(err32_j, e_fwd)) - 1 at step k.  Nothing in it comes from the device's training run."""
    style = sub("style")
    hp = hparams.tiny(n_spks=3)
    sd = synthetic.make_state_dict(hp, seed=7, duration_recipe=False)
    model = make_tts(hp, sd, dev)
    assert STYLE_TINY[0] == hp.n_feats and STYLE_TINY[3] == hp.spk_emb_dim
    enc, style_sd = make(STYLE_TINY, 17, dev)
    batches = train_batches(hp, synthetic)
    h64, t64 = R.train_loop(oracle, sd, hp, style_sd, batches)
    h32, t32 = R.train_loop(oracle, sd, hp, style_sd, batches, dtype=torch.float32)
    e64 = R.style_forward({k: v.double() for k, v in style_sd.items()}, batches[0][2], batches[0][3])
    rows = enc(batches[0][2].to(dev), lengths=batches[0][3].to(dev))
    e_fwd = max((r.cpu().double() - e).abs().max().item() / e.abs().max().item() for r, e in zip(rows, e64))
    trainer = style.StyleTrainer(model, enc)
    log = [trainer.step(*b) for b in batches]
    names = ("acoustic_loss", "rhythm_loss", "emb_dist_enc", "emb_dist_dur")
    got = torch.stack([torch.stack([r[k] for k in names]) for r in log]).cpu().double()
    note(f"trainer: e_fwd {e_fwd:.3e}")
    failed = []
    for i, name in enumerate(names[:2]):
        tol = 1.0
        for j in range(5):
            err32 = abs(h32[j][i] - h64[j][i]) / h64[j][i]
            tol *= 1 + 8 * max(err32, e_fwd)
            err = abs(got[j, i].item() - h64[j][i]) / h64[j][i]
            note(f"trainer step {j} {name}: device {got[j, i].item():.8e}, fp64 {h64[j][i]:.8e}, err {err:.3e}, err32 {err32:.3e}, bound {tol - 1:.3e}")
            if not err <= tol - 1:
                failed.append((name, j))
    for i in (2, 3):
        assert abs(got[0, i].item() - h64[0][i]) <= 1e-5 * h64[0][i], names[i]
    final = {k: v.detach().cpu().double() for k, v in trainer.views.items()}
    for k in R.param_names(STYLE_TINY[2]):
        p0 = style_sd[k].double()
        tol = 1.0
        for j in range(5):
            top = (t64[j][k] - p0).abs().max().item()
            tol *= 1 + 8 * max((t32[j][k].double() - t64[j][k]).abs().max().item() / top, e_fwd)
        top = (t64[4][k] - p0).abs().max().item()
        err = (final[k] - t64[4][k]).abs().max().item() / top
        err32 = (t32[4][k].double() - t64[4][k]).abs().max().item() / top
        note(f"trainer after 5 steps {k}: max|update| {top:.3e}, err {err:.3e}, err32 {err32:.3e}, bound {tol - 1:.3e}")
        if not err <= tol - 1:
            failed.append((k, 5))
    assert not failed, failed
    # the saved directory gives the trainer's forward bits, and loads where enroll_voice looks for an encoder
    out = trainer.save(tmp_path / "trained")
    assert (out / style.STYLE_OPTIMIZER).exists()
    again = style.load_style_encoder(out, device=dev)
    mel, mel_len = batches[0][2].to(dev), batches[0][3].to(dev)
    a, b = enc(mel, lengths=mel_len), again(mel, lengths=mel_len)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    state = torch.load(out / style.STYLE_OPTIMIZER, map_location="cpu", weights_only=False)
    assert state["steps"] == 5 and state["optimizer"]["state"][0]["exp_avg"].numel() == trainer.flat.numel()


def test_train_style_encoder_tool_runs_two_steps(hparams, dev, tmp_path):
    """tools/train_style_encoder.py on a three-clip corpus in the layout `tools/prepare_corpus.py mels` writes; what it saves loads."""
    import subprocess
    import sys
    import numpy as np
    from conftest import ROOT
    hp = hparams.tiny(n_spks=2)
    rng = np.random.default_rng(5)
    lines = []
    for i, (frames, spk, n_ids) in enumerate(((40, 0, 7), (25, 1, 4), (61, 0, 9))):
        rel = f"spk{spk}/clip{i}"
        (tmp_path / "mels" / f"spk{spk}").mkdir(parents=True, exist_ok=True)
        np.save(tmp_path / "mels" / (rel + ".fine.npy"), rng.standard_normal((hp.n_feats, frames)).astype(np.float32))
        lines.append(" ".join([rel, str(spk)] + [str(int(t)) for t in rng.integers(1, hp.n_vocab, size=n_ids)]))
    (tmp_path / "ids.txt").write_text("\n".join(lines) + "\n")
    out = tmp_path / "trained"
    res = subprocess.run([sys.executable, str(ROOT / "tools" / "train_style_encoder.py"), "--synthetic-model", "tiny", "--ids-file",
                          str(tmp_path / "ids.txt"), "--hidden", "32", "--layers", "2", "--batch-size", "2", "--out", str(out),
                          str(tmp_path / "mels")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "2 steps" in res.stdout
    enc = sub("style").load_style_encoder(out, device=dev)
    assert enc.cfg == dict(n_feats=hp.n_feats, hidden_channels=32, n_layers=2, spk_emb_dim=hp.spk_emb_dim)
    e_enc, e_dur = enc(torch.randn(1, hp.n_feats, 30, device=dev))
    assert torch.isfinite(e_enc).all() and torch.isfinite(e_dur).all()

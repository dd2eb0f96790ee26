"""The streams the FLAC-in tests share, built once with the recipe writer of ``flac_in_restated``: ``good()`` is the case list (name ->
stream bytes), ``refused()`` the refusal list (name -> (stream bytes, ld or None)), ``expected()`` the restated decoder's answer for
every good stream.  The CPU tests run them through ``mtts_flac_parse_host``, the GPU tests through ``mtts_flac_decode``."""
import functools

import numpy as np

from conftest import GOLDEN
import flac_in_restated as fi
import flac_restated as fr


def walk(n, bps, seed, step=None):
    """A random walk inside ``bps`` bits: small differences, the whole range visited."""
    rng, lim = np.random.default_rng(seed), 1 << (bps - 1)
    step = step or max(lim >> 7, 2)
    x = np.cumsum(rng.integers(-step, step + 1, n)) + rng.integers(-lim // 2, lim // 2)
    return np.clip(x, -lim, lim - 1).astype(np.int64)


FIX2 = {"kind": "fixed", "order": 2}


TRUTH = {}                                      # name -> int64 [channels, total]: what the recipes of ``good()`` were given


def stream(name, frames, **kw) -> bytes:
    channels = kw.get("channels", 1)
    TRUTH[name] = (np.concatenate([np.atleast_2d(np.asarray(f["samples"], dtype=np.int64)) for f in frames], axis=1) if frames
                   else np.zeros((channels, 0), dtype=np.int64))
    return fi.write_stream(frames, **kw)[0]


def small_frame(value=-3, n=16, number=0) -> bytes:
    """A complete, valid mono 16-bit frame (CONSTANT), for hiding in places the walk never visits."""
    return fi.frame_bytes({"samples": np.full(n, value), "sub": {"kind": "constant"}}, number, 24000, 16, 24000)


@functools.lru_cache(maxsize=None)
def good() -> dict:
    rng = np.random.default_rng(2027)
    out = {}
    # block sizes, each stream closed by a last frame of 1 sample
    for bs in (16, 192, 256, 576, 4608):
        x = walk(2 * bs + 1 if bs < 4608 else bs + 1, 16, bs)
        frames = [{"samples": x[j:j + bs], "sub": {"kind": "verbatim"} if j + bs > len(x) else FIX2 if bs > 16 else {"kind": "fixed", "order": 4}}
                  for j in range(0, len(x), bs)]
        out[f"block_{bs}"] = stream(f"block_{bs}", frames, rate=(24000, 44100, 8000, 11025, 96000)[bs % 5])
    # LPC: order 32 on a block of 32 (no residual; precision 15, shift 14) and order 1 (precision 1, shift 0)
    x = walk(64, 16, 1)
    out["lpc_small"] = stream("lpc_small", [
        {"samples": x[:32], "sub": {"kind": "lpc", "coefs": rng.integers(-16384, 16384, 32), "precision": 15, "shift": 14, "params": [0]}},
        {"samples": x[32:], "sub": {"kind": "lpc", "coefs": [-1], "precision": 1, "shift": 0}}])
    # order 32 on 4096; partition order 8 at 4096 with order 16 (the first partition is empty); a last frame of 1 sample
    x = walk(2 * 4096 + 1, 16, 2)
    out["lpc_4096"] = stream("lpc_4096", [
        {"samples": x[:4096], "sub": {"kind": "lpc", "coefs": rng.integers(-2048, 2048, 32), "precision": 12, "shift": 10, "method": 1, "po": 3}},
        {"samples": x[4096:8192], "sub": {"kind": "lpc", "coefs": rng.integers(-128, 128, 16), "precision": 8, "shift": 6, "po": 8}},
        {"samples": x[8192:], "sub": {"kind": "verbatim"}}])
    # full-scale 24-bit samples under coefficients at the ends of 15 bits: the sum needs 43 bits
    x = np.where(np.arange(96) % 3 == 0, -(1 << 23), (1 << 23) - 1)
    coefs = np.where(x[:32] < 0, -16384, 16383)[::-1]
    out["lpc_wide"] = stream("lpc_wide", [{"samples": x, "sub": {"kind": "lpc", "coefs": coefs, "precision": 15, "shift": 14, "method": 1,
                                                               "params": [("esc", 31)]}}], bps=24, rate=48000)
    # Rice parameters 0 and 14 (method 0) and 30 (method 1)
    x = rng.integers(-2, 3, 96)
    out["rice_k"] = stream("rice_k", [
        {"samples": x[:32], "sub": {"kind": "fixed", "order": 0, "params": [0]}},
        {"samples": walk(32, 16, 3), "sub": {"kind": "fixed", "order": 1, "params": [14], "po": 2}},
        {"samples": x[64:], "sub": {"kind": "fixed", "order": 0, "method": 1, "params": [30]}}])
    # escapes with raw widths 0 and 18, at 20 bits
    out["escape"] = stream("escape", [
        {"samples": np.full(32, 7), "sub": {"kind": "fixed", "order": 1, "params": [("esc", 0)]}},
        {"samples": rng.integers(-(1 << 17), 1 << 17, 32), "sub": {"kind": "fixed", "order": 0, "po": 1, "params": [("esc", 18), 12]}}], bps=20)
    # wasted bits 1 and 15
    out["wasted"] = stream("wasted", [
        {"samples": walk(32, 15, 4) * 2, "sub": {**FIX2, "wasted": 1}},
        {"samples": rng.integers(-1, 1, 32) * 32768, "sub": {"kind": "verbatim", "wasted": 15}}])
    # CONSTANT and VERBATIM at every sample size
    for bps in (8, 12, 16, 20, 24):
        lim = 1 << (bps - 1)
        out[f"plain_{bps}"] = stream(f"plain_{bps}", [
            {"samples": np.full(16, -lim), "sub": {"kind": "constant"}},
            {"samples": np.r_[lim - 1, -lim, rng.integers(-lim, lim, 14)], "sub": {"kind": "verbatim"}}], bps=bps, rate=16000)
    # the three stereo modes at the extremes, odd and even sums
    left = np.r_[32767, -32768, 32767, -32768, 1, 2, -1, -2, walk(8, 16, 5)]
    right = np.r_[-32768, 32767, 32767, -32768, 2, 2, -2, -1, walk(8, 16, 6)]
    subs = [{"kind": "fixed", "order": 1}, {"kind": "verbatim"}]
    out["stereo"] = stream("stereo", [{"samples": [left, right], "stereo": m, "sub": subs if j % 2 else subs[::-1]}
                                     for j, m in enumerate(("ls", "sr", "ms", None))], channels=2, rate=16000)
    # 8 independent channels
    out["eight"] = stream("eight", [{"samples": [walk(16, 16, 10 + c) for c in range(8)], "sub": [FIX2, {"kind": "verbatim"}] * 4},
                                    {"samples": [walk(5, 16, 20 + c) for c in range(8)], "sub": {"kind": "fixed", "order": 1}}], channels=8)
    # fixed numbering across 127 -> 128
    x = walk(129 * 16, 16, 7)
    out["numbers"] = stream("numbers", [{"samples": x[j:j + 16], "sub": {"kind": "fixed", "order": 1}} for j in range(0, len(x), 16)])
    # variable blocking, mixed sizes
    sizes, x = (16, 700, 192, 33, 4096, 1), walk(16 + 700 + 192 + 33 + 4096 + 1, 16, 8)
    cuts = np.cumsum((0,) + sizes)
    out["variable"] = stream("variable", [{"samples": x[a:b], "sub": FIX2 if b - a > 2 else {"kind": "verbatim"}, "variable": True, **({"rcode": 0} if a else {})}
                                       for a, b in zip(cuts[:-1], cuts[1:])], rate=22050)
    # metadata ahead of the frames; one PADDING block holds a byte-exact valid frame
    x = walk(80, 16, 9)
    blocks = [(1, bytes(37)), (2, b"mtts" + bytes(range(20))), (3, bytes(18 * 3)), (4, (4).to_bytes(4, "little") + b"test" + bytes(4)),
              (1, b"\xff\xf8" + small_frame() + small_frame(5, 16, 1) + bytes(3))]
    out["metadata"] = stream("metadata", [{"samples": x[j:j + 16], "sub": FIX2} for j in range(0, 80, 16)], blocks=blocks)
    # a VERBATIM payload that embeds a complete valid frame with both CRCs right
    inner = small_frame(9, 16, 1) + small_frame(11, 16, 2)
    inner += bytes(len(inner) % 2)
    words = np.frombuffer(inner, dtype=">i2").astype(np.int64)
    x = np.r_[walk(4, 16, 11), words, walk(32 - 4 - len(words), 16, 12)]
    out["embedded"] = stream("embedded", [{"samples": x[:16], "sub": {"kind": "verbatim"}}, {"samples": x[16:], "sub": {"kind": "verbatim"}}])
    assert inner in out["embedded"]
    out["empty"] = stream("empty", [])
    return out


@functools.lru_cache(maxsize=None)
def own() -> dict:
    """Streams of the project's own encoder (restated) and the RFC's first example file."""
    out = {"rfc_example1": (GOLDEN / "rfc9639_example1.flac").read_bytes()}
    for bs in fr.BLOCK_SIZES:
        for n in (0, 1, bs - 1, bs, bs + 1):
            out[f"own_{bs}_{n}"] = fr.encode(walk(n, 16, bs + n) if n else [], 24000 if bs != 512 else 11025, bs)
    return out


@functools.lru_cache(maxsize=None)
def expected() -> dict:
    return {name: fi.decode(data) for name, data in {**good(), **own()}.items()}


def base_frames(n=4, bs=64, seed=30):
    x = walk(n * bs, 16, seed)
    return [{"samples": x[j * bs:(j + 1) * bs], "sub": FIX2} for j in range(n)]


@functools.lru_cache(maxsize=None)
def refused() -> dict:
    """name -> (stream, ld or None): every one a stream the contract refuses (``ld``: the row capacity that makes it so)."""
    frames = base_frames()
    ok, spans = fi.write_stream(frames)
    flip = lambda data, at, bit=0x10: data[:at] + bytes([data[at] ^ bit]) + data[at + 1:]
    s1, l1 = spans[1]
    s3, l3 = spans[3]
    out = {
        "crc16_flip": flip(ok, s1 + l1 - 1),
        "crc8_flip": flip(ok, s1 + 6),
        "payload_flip": flip(ok, s1 + l1 // 2),
        "truncated_1": ok[:-1],
        "truncated_half": ok[:s3 + l3 // 2],
        "frame_removed": ok[:s1] + ok[s1 + l1:],
        "duplicate_number": fi.write_stream(frames, numbers=[0, 1, 1, 3])[0],
        "total_plus_1": fi.write_stream(frames, total=257)[0],
        "total_minus_1": fi.write_stream(frames, total=255)[0],
        "unknown_total": fi.write_stream(frames, total=0)[0],
        "sample_size_code": fi.write_stream([{**f, "scode": 5} if j == 2 else f for j, f in enumerate(frames)])[0],
        "block_above_max": fi.write_stream(frames, max_bs=8192)[0],
        "lpc_precision_1111": fi.write_stream(frames[:3] + [{"samples": frames[3]["samples"], "sub": {
            "kind": "lpc", "coefs": [3, -1], "precision": 4, "shift": 1, "precision_code": 15}}])[0],
        "partition_not_dividing": fi.write_stream(frames[:3] + [{"samples": frames[3]["samples"][:48], "sub": {**FIX2, "po": 5}}])[0],
        "partition_below_order": fi.write_stream(frames[:3] + [{"samples": frames[3]["samples"], "sub": {
            "kind": "lpc", "coefs": [1] * 8, "precision": 4, "shift": 3, "po": 4}}])[0],
        "zero_tail": ok[:s3 + l3 // 2] + bytes(64),
        "metadata_runs_off": (lambda s: s[:43] + b"\xff\xff\xff" + s[46:])(fi.write_stream(frames, blocks=[(1, bytes(8))])[0]),
        "no_streaminfo": b"fLaC" + bytes([0x81, 0, 0, 34]) + ok[8:],
        "type_127": fi.write_stream(frames, blocks=[(127, bytes(4))])[0],
        "variable_mixed": fi.write_stream([{**f, "variable": j == 2} for j, f in enumerate(frames)], numbers=[0, 1, 128, 3])[0],
        "short_in_the_middle": fi.write_stream([{**f, "samples": f["samples"][:32]} if j == 1 else f for j, f in enumerate(frames)])[0],
    }
    out = {k: (v, None) for k, v in out.items()}
    out["bytes_0"], out["bytes_3"], out["bytes_41"] = (b"", None), (ok[:3], None), (ok[:41], None)
    out["total_above_ld"] = (ok, 252)
    return out

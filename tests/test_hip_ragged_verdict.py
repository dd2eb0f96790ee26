"""The ragged-batch verdict (csrc/device_utils.h ``first_refused_row``) with more rows than the verdict workgroup has threads, so
that the strided scan takes a second trip: every entry that calls it, at B = its workgroup's thread count + 1 and the smallest
shapes it accepts.  The entries are called through the C ABI so that every output buffer can be filled with a sentinel first.
Nothing here provokes a fault: refused lengths are clamped before they index anything, which is the contract under test."""

import numpy as np
import pytest
import torch

from conftest import sub

pytestmark = pytest.mark.gpu

SMALL = dict(n_mels=20, dim=68, inter=136, layers=2, n_fft=64, hop=16)             # tests/test_hip_vocos.py's second configuration
SENTINEL = {torch.float32: -7.25, torch.float64: -7.25, torch.int32: -77, torch.int64: -77}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("a HIP device is required for -m gpu tests (no CPU fallback exists)")
    return torch.device("cuda")


def filled(dev, dtype, *shape):
    return torch.full(shape, SENTINEL[dtype], dtype=dtype, device=dev)


def i64(dev, values):
    return torch.tensor(values, dtype=torch.int64, device=dev)


class Entry:
    """One entry: ``run(lengths) -> outputs`` (device tensors with the batch in front, written by the call into sentinel-filled
    buffers) after which ``status()`` is the entry's synchronising verdict; ``good`` lengths every row accepts, ``bad(row)`` a length
    the entry refuses (another one per row: the report must carry the first refused row's own) and ``names(row, length)`` what the
    error says about it."""
    B = 257

    def __init__(self, dev):
        self.dev, self.hip = dev, sub("_hip")
        self.lib, self.stream = self.hip.load(), self.hip.stream_ptr()
        self.rng = np.random.default_rng(self.B)

    def verdict(self):
        rc = self.status()
        return rc, self.lib.mtts_last_error().decode()

    def workspace(self, nbytes):
        assert nbytes > 0
        return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)


class Mas(Entry):
    B, Tx, Tm = 65, 2, 4

    def __init__(self, dev):
        super().__init__(dev)
        self.lp = torch.from_numpy(self.rng.standard_normal((self.B, self.Tx, self.Tm)).astype(np.float32)).to(dev)
        self.y_len = [int(v) for v in self.rng.integers(2, self.Tm + 1, self.B)]
        self.good = [int(v) for v in self.rng.integers(1, 3, self.B)]                      # x_length in {1, 2} <= y_length
        self.ws = self.workspace(self.lib.mtts_mas_workspace_bytes(self.B, self.Tx, self.Tm))

    def bad(self, row):
        return -row

    def names(self, row, length):
        return f"mtts_mas: utterance {row} has x_length = {length}, y_length = {self.y_len[row]} "

    def run(self, x_len):
        B, Tx, Tm, d = self.B, self.Tx, self.Tm, self.dev
        dur, path, score = filled(d, torch.int32, B, Tx), filled(d, torch.float32, B, Tx, Tm), filled(d, torch.float32, B)
        xl, yl = i64(d, x_len), i64(d, self.y_len)             # (named: a temporary's memory is re-used by the next allocation)
        self.hip.check(self.lib.mtts_mas(self.lp.data_ptr(), None, None, xl.data_ptr(), yl.data_ptr(), B, 0, Tx, Tm,
                                         dur.data_ptr(), path.data_ptr(), score.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stream))
        return dur, path, score

    def status(self):
        return self.lib.mtts_mas_status(self.ws.data_ptr(), self.stream)


class Score(Mas):
    F = 2

    def __init__(self, dev):
        super().__init__(dev)
        B, F, Tx, Tm = self.B, self.F, self.Tx, self.Tm
        f32 = lambda *s: torch.from_numpy(self.rng.standard_normal(s).astype(np.float32)).to(dev)
        self.mu_x, self.logw, self.y = f32(B, F, Tx), f32(B, 1, Tx), f32(B, F, Tm)
        dur = [[yl, 0] if xl == 1 else [1, yl - 1] for xl, yl in zip(self.good, self.y_len)]      # valid: they sum to y_length
        self.dur = torch.tensor(dur, dtype=torch.int32, device=dev)
        self.ws = self.workspace(self.lib.mtts_score_workspace_bytes(B, Tx, Tm))

    def names(self, row, length):
        return f"mtts_score_prior_dur: utterance {row} has x_length = {length}, y_length = {self.y_len[row]} (need 1 <= x_length"

    def run(self, x_len):
        B, F, Tx, Tm, d = self.B, self.F, self.Tx, self.Tm, self.dev
        prior, dsum = filled(d, torch.float32, B), filled(d, torch.float32, B)
        frame, err = filled(d, torch.float32, B, Tm), filled(d, torch.float32, B, Tx)
        xl, yl = i64(d, x_len), i64(d, self.y_len)
        self.hip.check(self.lib.mtts_score_prior_dur(self.mu_x.data_ptr(), self.logw.data_ptr(), self.dur.data_ptr(), self.y.data_ptr(),
                                                     xl.data_ptr(), yl.data_ptr(), B, F, Tx, Tm, 1.0, 1.0,
                                                     prior.data_ptr(), dsum.data_ptr(), frame.data_ptr(), err.data_ptr(), self.ws.data_ptr(),
                                                     self.ws.numel(), self.stream))
        return prior, dsum, frame, err

    def status(self):
        return self.lib.mtts_score_status(self.ws.data_ptr(), self.stream)


class Rows(Entry):
    """The entries on rows of audio [B, ld]: lengths in [0, ld] are accepted, ld + 1 + row is refused."""
    ld = 8

    def __init__(self, dev):
        super().__init__(dev)
        self.audio = torch.from_numpy(self.rng.uniform(-1, 1, (self.B, self.ld)).astype(np.float32)).to(dev)
        self.good = [int(v) for v in self.rng.integers(0, self.ld + 1, self.B)]

    def bad(self, row):
        return self.ld + 1 + row


class Resample(Rows):
    ld = 64

    def __init__(self, dev):
        super().__init__(dev)
        self.rs = sub("resample").Resampler(48000, 24000)
        self.ld_out = (self.rs.out_length(self.ld) + 3) // 4 * 4
        self.ws = self.workspace(self.lib.mtts_resample_workspace_bytes(self.rs.ctx, self.B, self.ld))

    def names(self, row, length):
        return f"mtts_resample_forward: row {row} has length {length} "

    def run(self, lengths):
        out, out_len = filled(self.dev, torch.float32, self.B, self.ld_out), filled(self.dev, torch.int64, self.B)
        d_len = i64(self.dev, lengths)
        self.hip.check(self.lib.mtts_resample_forward(self.rs.ctx, self.audio.data_ptr(), self.ld, d_len.data_ptr(), self.B,
                                                      out.data_ptr(), self.ld_out, out_len.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                      self.stream))
        return out, out_len

    def status(self):
        return self.lib.mtts_resample_status(self.ws.data_ptr(), self.stream)


class Measure(Rows):
    RATE = 400                                   # a 10 ms window of 4 samples: a row of 8 is two windows

    def __init__(self, dev):
        super().__init__(dev)
        assert self.lib.mtts_silence_window(self.RATE) * 2 == self.ld
        self.ws = self.workspace(self.lib.mtts_silence_workspace_bytes(self.ld, self.B, self.RATE))

    def names(self, row, length):
        return f"mtts_silence_measure: row {row} has length {length} "

    def measure(self, lengths):
        out = filled(self.dev, torch.int64, self.B, 6)
        self.hip.check(self.lib.mtts_silence_measure(self.audio.data_ptr(), self.ld, lengths.data_ptr(), self.B, self.RATE, -20.0, -40.0,
                                                     out.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stream))
        return out

    def run(self, lengths):
        return (self.measure(i64(self.dev, lengths)),)

    def status(self):
        return self.lib.mtts_silence_status(self.ws.data_ptr(), self.stream)


class Normalize(Measure):
    def names(self, row, length):
        return f"mtts_silence_normalize: row {row} has length {length} "

    def run(self, lengths):
        d_len = i64(self.dev, lengths)
        bounds = self.measure(d_len)
        ld_out = self.ld + 4                     # one window of leading silence at most is added
        out, out_len = filled(self.dev, torch.float32, self.B, ld_out), filled(self.dev, torch.int64, self.B)
        changed = filled(self.dev, torch.int32, self.B)
        self.hip.check(self.lib.mtts_silence_normalize(self.audio.data_ptr(), self.ld, d_len.data_ptr(), bounds.data_ptr(), self.B, self.RATE, 4, -1,
                                                       out.data_ptr(), ld_out, out_len.data_ptr(), changed.data_ptr(), self.ws.data_ptr(),
                                                       self.ws.numel(), self.stream))
        return out, out_len, changed


class MelStats(Entry):
    F, T = 4, 4

    def __init__(self, dev):
        super().__init__(dev)
        self.mel = torch.from_numpy(self.rng.standard_normal((self.B, self.F, self.T)).astype(np.float32)).to(dev)
        self.good = [int(v) for v in self.rng.integers(0, self.T + 1, self.B)]
        self.ws = self.workspace(self.lib.mtts_mel_stats_workspace_bytes(self.B, self.T))

    def bad(self, row):
        return self.T + 1 + row

    def names(self, row, length):
        return f"mtts_mel_stats: row {row} has length {length} "

    def run(self, lengths):
        sums, frames = filled(self.dev, torch.float64, self.B, 2), filled(self.dev, torch.int64, self.B)
        flags = filled(self.dev, torch.int32, self.B)
        d_len = i64(self.dev, lengths)
        self.hip.check(self.lib.mtts_mel_stats(self.mel.data_ptr(), self.F, self.T, d_len.data_ptr(), self.B, sums.data_ptr(),
                                               frames.data_ptr(), flags.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stream))
        return sums, frames, flags

    def status(self):
        return self.lib.mtts_mel_stats_status(self.ws.data_ptr(), self.stream)


class VocosDecode(Entry):
    T = 4

    def __init__(self, dev):
        super().__init__(dev)
        sd = sub("synthetic").make_vocos_state_dict(seed=23, **{k: v for k, v in SMALL.items() if k != "hop"})
        self.model = sub("vocoder").Vocos(**SMALL)
        self.model.load_state_dict(sd, strict=True)
        self.model = self.model.to(dev).eval()
        self.model._ready()
        self.mel = (torch.from_numpy(self.rng.standard_normal((self.B, SMALL["n_mels"], self.T)).astype(np.float32)) * 2.0 - 4.0).to(dev)
        self.good = [int(v) for v in self.rng.integers(1, self.T + 1, self.B)]
        self.ws = self.workspace(self.lib.mtts_vocos_ragged_workspace_bytes(self.model._ctx, self.B, self.T))

    def bad(self, row):
        return self.T + 1 + row

    def names(self, row, length):
        return f"mtts_vocos_decode_ragged: lengths[{row}] = {length} is outside [1, T = {self.T}]"

    def run(self, lengths):
        audio = filled(self.dev, torch.float32, self.B, SMALL["hop"] * (self.T - 1))
        d_len = i64(self.dev, lengths)
        self.hip.check(self.lib.mtts_vocos_decode_ragged(self.model._ctx, self.mel.data_ptr(), d_len.data_ptr(), self.B, self.T,
                                                         audio.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.stream))
        return (audio,)

    def status(self):
        return self.lib.mtts_vocos_ragged_status(self.ws.data_ptr(), self.stream)


def bits(t):
    """Bit patterns, so that ``torch.equal`` also holds for a NaN that both calls produced."""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("entry", [Mas, Score, Resample, Measure, Normalize, MelStats, VocosDecode], ids=lambda e: e.__name__)
def test_first_refused_row_beyond_one_trip_of_the_scan(entry, dev):
    e = entry(dev)
    B = e.B
    clean = [t.cpu() for t in e.run(e.good)]
    rc, msg = e.verdict()
    assert rc == 0, msg
    # {1, B-1}: both in the scan's first trip, the smaller one wins.  {B-1} alone: found in the first trip by one thread, while row 0
    # is the only row of the last trip
    for refused in ((1, B - 1), (B - 1,)):
        lengths = list(e.good)
        for row in refused:
            lengths[row] = e.bad(row)
        outs = [t.cpu() for t in e.run(lengths)]
        rc, msg = e.verdict()
        first = refused[0]
        print(f"{entry.__name__} refused {refused}: rc {rc}, {msg!r}")
        assert rc == -1 and e.names(first, lengths[first]) in msg, msg
        accepted = [b for b in range(B) if b not in refused]
        for got, want in zip(outs, clean):
            assert torch.equal(bits(got[accepted]), bits(want[accepted]))
    again = [t.cpu() for t in e.run(e.good)]                   # a clean call after a refused one: the header is rewritten
    rc, msg = e.verdict()
    assert rc == 0, msg
    for got, want in zip(again, clean):
        assert torch.equal(bits(got), bits(want))

"""The Python half of the ragged-batch contract (``_hip.py``: ``Workspaces``, ``row_lengths``, ``aligned_rows``, ``size``,
``raise_refused``), driven without a device: the stream is a variable of the test, buffers live on "cpu" (and on "meta" as a second
device) and the device check is stubbed."""
import weakref
from types import SimpleNamespace

import pytest
import torch

from conftest import sub


@pytest.fixture
def stream():
    return SimpleNamespace(now=1)


@pytest.fixture
def hip(monkeypatch, stream):
    h = sub("_hip")
    monkeypatch.setattr(h, "stream_ptr", lambda: stream.now)
    monkeypatch.setattr(h, "on_device", lambda t: True)
    return h


# ---------------------------------------------------------------------------------------------- the workspace cache
def test_cache_grows_only_and_drops_the_buffer_it_replaces(hip):
    c = hip.Workspaces()
    a = c.get("k", 100, "cpu")
    assert a.dtype == torch.uint8 and a.numel() == 100 and c.bytes_held() == 100
    assert c.get("k", 40, "cpu") is a and c.get("k", 100, "cpu") is a and c.bytes_held() == 100
    gone = weakref.ref(a)
    del a
    b = c.get("k", 101, "cpu")
    assert b.numel() == 101 and gone() is None                 # neither the cache nor ``latest`` kept the old one
    assert c.bytes_held() == 101 and c.latest("k") is b


def test_cache_separates_kinds_streams_and_devices(hip, stream):
    c = hip.Workspaces()
    a = c.get("k", 8, "cpu")
    other_kind = c.get("j", 16, "cpu")
    stream.now = 2
    assert c.latest("k") is None
    other_stream = c.get("k", 32, "cpu")
    other_device = c.get("k", 64, "meta")
    assert len({id(a), id(other_kind), id(other_stream), id(other_device)}) == 4 and other_device.device.type == "meta"
    assert c.bytes_held() == 8 + 16 + 32 + 64
    assert c.get("k", 1, "cpu") is other_stream and c.get("k", 1, "meta") is other_device
    stream.now = 1
    assert c.get("k", 1, "cpu") is a and c.latest("j") is other_kind


def test_cache_note_overrides_latest_and_clear_empties(hip):
    c = hip.Workspaces()
    assert c.latest("k") is None
    a = c.get("k", 8, "cpu")
    mine = torch.empty(4, dtype=torch.uint8)
    c.note("k", mine)                                          # a captured graph's own buffer
    assert c.latest("k") is mine and c.bytes_held() == 8       # noted, not held
    assert c.get("k", 8, "cpu") is a and c.latest("k") is a    # the next cached call is the latest again
    c.note("k", mine)
    assert c.get("k", 9, "cpu").numel() == 9 and c.latest("k").numel() == 9
    c.clear()
    assert c.latest("k") is None and c.bytes_held() == 0
    assert c.get("k", 8, "cpu") is not a


def test_cache_refuses_a_negative_size_through_check(hip, monkeypatch):
    monkeypatch.setattr(hip, "check", lambda rc: (_ for _ in ()).throw(RuntimeError("mtts: boom")))
    with pytest.raises(RuntimeError, match="mtts: boom"):
        hip.Workspaces().get("k", -1, "cpu")


# ---------------------------------------------------------------------------------------------- lengths
def test_row_lengths(hip):
    d = hip.row_lengths(None, 3, 7, "cpu")
    assert d.dtype == torch.long and d.tolist() == [7, 7, 7]
    got = hip.row_lengths([1, 2, 3], 3, 7, "cpu")
    assert got.dtype == torch.long and got.tolist() == [1, 2, 3] and got.is_contiguous()
    assert hip.row_lengths(torch.tensor([4, 5], dtype=torch.int32), 2, 0, "cpu").tolist() == [4, 5]
    with pytest.raises(ValueError) as e:
        hip.row_lengths([1, 2], 3, 7, "cpu")
    assert str(e.value) == "lengths must have shape (3,), got (2,)"
    with pytest.raises(ValueError) as e:
        hip.row_lengths(torch.zeros(3, 1), 3, 7, "cpu", "mel_lengths")
    assert str(e.value) == "mel_lengths must have shape (3,), got (3, 1)"


# ---------------------------------------------------------------------------------------------- rows of aligned quanta
def test_aligned_rows_passes_an_aligned_batch_through(hip):
    x = torch.arange(16, dtype=torch.float32).reshape(2, 8)
    assert x.data_ptr() % 16 == 0
    rows, L = hip.aligned_rows(x, 4, "audio")
    assert L == 8 and rows.data_ptr() == x.data_ptr() and rows.shape == (2, 8)
    raw = torch.arange(32, dtype=torch.uint8).reshape(1, 32)
    rows, L = hip.aligned_rows(raw, 16, "data")
    assert L == 32 and rows.data_ptr() == raw.data_ptr()
    one = torch.arange(8, dtype=torch.float32)
    rows, L = hip.aligned_rows(one, 4, "audio")                # 1-D: one row, still no copy
    assert rows.shape == (1, 8) and rows.data_ptr() == one.data_ptr()


@pytest.mark.parametrize("L,quantum,dtype", [(1, 4, torch.float32), (3, 4, torch.float32), (4, 4, torch.float32), (5, 4, torch.float32),
                                             (15, 16, torch.uint8), (16, 16, torch.uint8), (17, 16, torch.uint8)])
def test_aligned_rows_pads_with_zeros_and_keeps_the_prefix(hip, L, quantum, dtype):
    x = (torch.arange(3 * L).reshape(3, L) % 200 + 1).to(dtype)
    rows, got = hip.aligned_rows(x, quantum, "audio" if quantum == 4 else "data")
    ld = (L + quantum - 1) // quantum * quantum
    assert got == L and rows.shape == (3, ld) and rows.dtype == dtype and rows.is_contiguous() and rows.data_ptr() % 16 == 0
    assert torch.equal(rows[:, :L], x) and not rows[:, L:].any()
    # a misaligned base or a strided view is copied even when L is a whole number of quanta
    wide = (torch.arange(3 * (ld + quantum)).reshape(3, ld + quantum) % 200 + 1).to(dtype)
    view = wide[:, 1:1 + ld]
    rows, got = hip.aligned_rows(view, quantum, "audio" if quantum == 4 else "data")
    assert got == ld and rows.data_ptr() != view.data_ptr() and rows.is_contiguous() and torch.equal(rows, view)


def test_aligned_rows_converts_samples_and_insists_on_bytes(hip):
    rows, _ = hip.aligned_rows(torch.ones(2, 4, dtype=torch.float64), 4, "audio")
    assert rows.dtype == torch.float32
    with pytest.raises(ValueError) as e:
        hip.aligned_rows(torch.ones(2, 16), 16, "data", "a uint8 [B, ld_bytes] tensor")
    assert str(e.value) == "data must be a uint8 [B, ld_bytes] tensor"


def test_aligned_rows_error_texts(hip, monkeypatch):
    with pytest.raises(ValueError) as e:
        hip.aligned_rows(torch.zeros(1, 2, 4), 4, "audio")
    assert str(e.value) == "audio must be [B, L]"
    with pytest.raises(ValueError) as e:
        hip.aligned_rows(torch.zeros(2, 0), 4, "audio")
    assert str(e.value) == "audio must have at least one row and one sample"
    with pytest.raises(ValueError) as e:
        hip.aligned_rows(torch.zeros(0, 16, dtype=torch.uint8), 16, "data")
    assert str(e.value) == "data must have at least one row and one byte"
    monkeypatch.setattr(hip, "on_device", lambda t: t.is_cuda)
    with pytest.raises(RuntimeError) as e:
        hip.aligned_rows(torch.zeros(1, 4), 4, "audio")
    assert str(e.value) == "matcha-tts-24k_amd: audio is not on a HIP device; there is no CPU path"


# ---------------------------------------------------------------------------------------------- size and the status reader
def test_size_passes_counts_through_and_raises_through_check(hip, monkeypatch):
    seen = []
    monkeypatch.setattr(hip, "check", lambda rc: seen.append(rc))
    assert hip.size(0) == 0 and hip.size(12345) == 12345 and seen == []
    hip.size(-1)
    assert seen == [-1]
    monkeypatch.setattr(hip, "check", lambda rc: (_ for _ in ()).throw(RuntimeError("mtts: the library's text")))
    with pytest.raises(RuntimeError, match="mtts: the library's text"):
        hip.size(-7)


def test_raise_refused_carries_the_library_text(hip, monkeypatch):
    text = "mtts_mas: utterance 1 has x_length = 0, y_length = 4 (need ...)"
    monkeypatch.setattr(hip, "load", lambda: SimpleNamespace(mtts_last_error=lambda: text.encode()))
    calls = []

    def status(*args):
        calls.append(args)
        return -1 if args[0] else 0

    hip.raise_refused(status, 0, 11)                           # a clean verdict: nothing raised, nothing read
    with pytest.raises(ValueError) as e:
        hip.raise_refused(status, 5, 11)
    assert str(e.value) == text and calls == [(0, 11), (5, 11)]
    with pytest.raises(ValueError) as e:
        hip.raise_refused(status, 5, 11, prefix="mtts: ")
    assert str(e.value) == "mtts: " + text

"""CPU checks of the estimator's launch-form decision (csrc/decoder.hip tblock_plan through mtts_tblock_plan; nothing runs on a GPU):
which of the tiled launches, the chain launch and its pair form a transformer block's row-local part takes, enumerated over every
width, switch setting and EVERY row count from 1 to 12000 -- each plan names an instantiated kernel shape, pair grids are resident,
the production plan is pinned, the chain's rows per workgroup are those of mtts_chain_plan, the pair form stays at the one shape it
was measured at, and the packer carries a pair stream exactly where the decision can take it."""
import ctypes as C
import dataclasses
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import sub

M_MAX = 12000
CHAIN_MIN_ROWS, PAIR_MIN_ROWS = 5761, 3000           # csrc/model.h Switches: the defaults
WIDTHS = {128: (128,), 256: (256, 192), 384: (384,)}  # width -> attention widths (heads * 64) of the estimators the suite builds
TILED, CHAIN, PAIR = 0, 1, 2
SWITCH_ENV = ("MTTS_CHAIN", "MTTS_CHAIN_CH", "MTTS_CHAIN_QB", "MTTS_CHAIN_PF", "MTTS_CHAIN_MIN_ROWS", "MTTS_CHAIN_PAIR", "MTTS_CHAIN_PAIR_MIN_ROWS")


@pytest.fixture(scope="module")
def hip():
    h = sub("_hip")
    h.build()
    h.load()
    return h


@pytest.fixture(scope="module")
def lib(hip):
    return hip.load()


@pytest.fixture(scope="module")
def chain_plan_qb(lib):
    """qb of mtts_chain_plan for every M of the enumeration, per hidden chunk (computed once, at the default MTTS_CHAIN_PF: that entry
    reads it per call)."""
    out = {}
    keep = os.environ.pop("MTTS_CHAIN_PF", None)
    try:
        for ch in (128, 256):
            qb, pf = C.c_int(0), C.c_int(0)
            col = np.zeros(M_MAX, dtype=np.int32)
            for M in range(1, M_MAX + 1):
                assert lib.mtts_chain_plan(M, ch, C.byref(qb), C.byref(pf)) == 0
                col[M - 1] = qb.value
            out[ch] = col
    finally:
        if keep is not None:
            os.environ["MTTS_CHAIN_PF"] = keep
    return out


def cells():
    """(C, inner, n_qkv, chain_ch switch, chain_qb, pair_on, (chain_min_rows, pair_min_rows))"""
    for width, inners in WIDTHS.items():
        for inner in inners:
            yield from itertools.product([width], [inner], [0, 3 * inner], [128, 256], [0, 32, 48, 64], [0, 1],
                                         [(CHAIN_MIN_ROWS, PAIR_MIN_ROWS), (0, PAIR_MIN_ROWS), (CHAIN_MIN_ROWS, 0)])


@pytest.fixture(scope="module")
def plans(hip):
    """Every plan of the enumeration: cell -> (ch, form, qb, grid, prefetch), arrays over M = 1 .. M_MAX."""
    out = {}
    for cell in cells():
        width, inner, n_qkv, chain_ch, chain_qb, pair_on, (cmin, pmin) = cell
        out[cell] = hip.tblock_plan(width, inner, n_qkv, 1, M_MAX, chain_ch=chain_ch, chain_qb=chain_qb, pair_on=pair_on, chain_min_rows=cmin,
                                    pair_min_rows=pmin)
    assert len(out) == 4 * 2 * 2 * 4 * 2 * 3
    return out


def test_entries_are_bound_and_the_environment_is_not_read(hip, lib, monkeypatch):
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert callable(hip.tblock_plan) and lib.mtts_chain_shape_exists.restype is C.c_int
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in hip.tblock_plan(384, 384, 1152, 1, M_MAX)]
    for k, v in zip(SWITCH_ENV, ("0", "128", "64", "0", "0", "0", "0")):
        monkeypatch.setenv(k, v)
    after = hip.tblock_plan(384, 384, 1152, 1, M_MAX)
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))
    ip = C.POINTER(C.c_int)
    one = [np.zeros(1, dtype=np.int32) for _ in range(5)]
    ptrs = [a.ctypes.data_as(ip) for a in one]
    for bad in ((384, 384, 0, 0, 1), (384, 384, 0, 1, 0), (384, 384, 0, 1, 1 << 24), (384, -32, 0, 1, 1)):
        assert lib.mtts_tblock_plan(*bad, 1, 256, 0, 16, CHAIN_MIN_ROWS, 1, PAIR_MIN_ROWS, *ptrs) == -1
        assert b"mtts_tblock_plan" in lib.mtts_last_error()
    assert lib.mtts_tblock_plan(384, 384, 0, 1, 1, 1, 192, 0, 16, CHAIN_MIN_ROWS, 1, PAIR_MIN_ROWS, *ptrs) == -1      # chunk 192
    assert lib.mtts_tblock_plan(384, 384, 0, 1, 1, 1, 256, 0, 16, CHAIN_MIN_ROWS, 1, PAIR_MIN_ROWS, None, *ptrs[1:]) == -1
    # a width or attention width the chain does not exist for: tiled at every M, not an error
    _, form, _, _, _ = hip.tblock_plan(192, 192, 576, 1, M_MAX, chain_min_rows=0, pair_min_rows=0)
    assert (form == TILED).all()
    _, form, _, _, _ = hip.tblock_plan(384, 384, 1152, 1, M_MAX, chain_on=0, chain_min_rows=0, pair_min_rows=0)
    assert (form == TILED).all()                                     # MTTS_CHAIN=0: nothing is packed


def test_shape_table_is_the_launchers(lib):
    """The instantiations of tblock_chain_kernel, as include/mtts.h states them for mtts_tblock_chain: 64- and 32-row workgroups with
    hidden chunk 128 at every width, 48- and 32-row ones with chunk 256 at width 384."""
    want = {(c, qb, 128) for c in (128, 256, 384) for qb in (64, 32)} | {(384, 48, 256), (384, 32, 256)}
    got = {(c, qb, ch) for c in (64, 128, 192, 256, 384, 512) for qb in (0, 16, 32, 48, 64, 96) for ch in (64, 128, 256, 512)
           if lib.mtts_chain_shape_exists(c, qb, ch)}
    assert got == want


def test_every_chain_or_pair_plan_names_an_instantiated_shape(lib, plans):
    n = 0
    for cell, (ch, form, qb, grid, pf) in plans.items():
        width, chain_ch = cell[0], cell[3]
        assert ch == (256 if width == 384 and chain_ch == 256 else 128), cell
        launched = form != TILED
        for q in np.unique(qb[launched]):
            assert lib.mtts_chain_shape_exists(width, int(q), ch) == 1, (cell, int(q), ch)
        assert set(np.unique(form)) <= {TILED, CHAIN, PAIR}
        assert not qb[~launched].any() and not grid[~launched].any() and not pf[~launched].any(), cell
        assert (grid[launched] > 0).all(), cell
        n += int(launched.sum())
    assert n > 0


def test_pair_grids_are_resident(plans):
    M = np.arange(1, M_MAX + 1)
    n = 0
    for cell, (ch, form, qb, grid, pf) in plans.items():
        pair = form == PAIR
        if not pair.any():
            continue
        n += int(pair.sum())
        tiles = -(-M[pair] // qb[pair])
        assert np.array_equal(grid[pair], 16 * (-(-tiles // 8))), cell
        assert (grid[pair] + pf[pair] <= 256).all(), cell
        assert np.isin(pf[pair], (0, 16)).all(), cell
    assert n > 0
    # no prefetch workgroups asked for: none planned, same grids
    _, form, qb, grid, pf = next(v for c, v in plans.items() if c[:6] == (384, 384, 1152, 256, 0, 1) and c[6] == (CHAIN_MIN_ROWS, PAIR_MIN_ROWS))
    _, form0, qb0, grid0, pf0 = sub("_hip").tblock_plan(384, 384, 1152, 1, M_MAX, chain_pf=0)
    assert np.array_equal(form0, form) and np.array_equal(grid0[form == PAIR], grid[form == PAIR]) and not pf0[form == PAIR].any()


def test_chain_grids_cover_the_rows(plans):
    M = np.arange(1, M_MAX + 1)
    for cell, (ch, form, qb, grid, pf) in plans.items():
        chain = form == CHAIN
        assert np.array_equal(grid[chain], -(-M[chain] // np.maximum(qb[chain], 1))), cell
        assert ((pf[chain] >= 0) & (pf[chain] <= 64)).all(), cell


@pytest.mark.parametrize("n_qkv", [0, 1152])
def test_production_plan_is_pinned(plans, chain_plan_qb, n_qkv):
    """Width 384, hidden chunk 256, default switches: tiled below 3000 rows, the pair form with 48-row tiles up to 5760 rows (120
    tiles: 240 + 16 workgroups), the chain launch from 5761 rows with mtts_chain_plan's rows per workgroup."""
    ch, form, qb, grid, pf = plans[(384, 384, n_qkv, 256, 0, 1, (CHAIN_MIN_ROWS, PAIR_MIN_ROWS))]
    M = np.arange(1, M_MAX + 1)
    assert ch == 256
    assert (form[M < 3000] == TILED).all()
    mid = (M >= 3000) & (M <= 5760)
    assert (form[mid] == PAIR).all() and (qb[mid] == 48).all() and (pf[mid] == 16).all()
    assert grid[M == 5760][0] == 240 and grid[M == 3000][0] == 128
    big = M >= 5761
    assert (form[big] == CHAIN).all() and np.array_equal(qb[big], chain_plan_qb[256][big])
    assert qb[M == 7680][0] == 32 and qb[M == 7681][0] == 48         # (tests/test_abi.py states the same edge for mtts_chain_plan)


def test_chain_qb_is_chain_plans(plans, chain_plan_qb):
    """chain_min_rows = 0: every row count takes the chain launch wherever a stream is packed, with mtts_chain_plan's rows per
    workgroup -- or MTTS_CHAIN_QB where it names 32 or the hidden chunk's tall shape (48 with chunk 256, 64 with chunk 128)."""
    n = 0
    for cell, (ch, form, qb, grid, pf) in plans.items():
        if cell[6][0] != 0:
            continue
        forced = cell[4]
        tall = 48 if ch == 256 else 64
        want = np.full(M_MAX, forced, dtype=np.int32) if forced in (32, tall) else chain_plan_qb[ch]
        assert (form == CHAIN).all(), cell
        assert np.array_equal(qb, want), cell
        n += 1
    assert n == 4 * 2 * 2 * 4 * 2


def test_pair_form_is_gated_to_width_384_chunk_256(plans):
    n_pair_cells = 0
    for cell, (ch, form, qb, grid, pf) in plans.items():
        width, pair_on, (cmin, pmin) = cell[0], cell[5], cell[6]
        if width != 384 or ch != 256 or not pair_on:
            assert not (form == PAIR).any(), cell
        elif cmin == 0:
            assert not (form == PAIR).any(), cell                    # the chain launch from the first row on
        else:
            M = np.arange(1, M_MAX + 1)
            assert np.array_equal(form == PAIR, (M >= pmin) & (M <= 5760)), cell
            assert (qb[form == PAIR] == 48).all()
            n_pair_cells += 1
        if cmin:                                                     # below both thresholds and beyond the residency bound: tiled
            M = np.arange(1, M_MAX + 1)
            assert (form[(M < cmin) & (form != PAIR)] == TILED).all(), cell
    assert n_pair_cells == 2 * 4 * 2                                 # n_qkv x chain_qb x two threshold sets


def make_context(hip, hp, synthetic):
    """A context with every tensor registered, never uploaded (tests/test_abi.py test_packing_sizes_without_gpu)."""
    h = hip.HipModel(hp)
    for k, v in synthetic.make_state_dict(hp).items():
        if k in ("mel_mean", "mel_std"):
            continue
        h._set(k, v)
        if k.endswith("ff.net.0.alpha"):
            h._set(k + "_exp", torch.exp(v))
        elif k.endswith("ff.net.0.beta"):
            h._set(k[:-4] + "inv_beta", 1.0 / (torch.exp(v) + 1e-9))
    cos, sin = hip.rope_tables(12)
    h._set("aux.rope_cos", cos)
    h._set("aux.rope_sin", sin)
    h._set("aux.time_freqs", hip.time_freqs(2 * hp.n_feats))
    return h


@pytest.mark.parametrize("channels,n_blocks,heads,chain_ch,pair_blocks", [((384, 384), 2, 6, "256", True), ((384, 384), 2, 6, "128", False),
                                                                          ((256, 256), 2, 3, "256", False), ((128, 128), 2, 2, "256", False)])
def test_packer_carries_a_pair_stream_only_where_the_plan_can_take_it(hip, lib, hparams, synthetic, monkeypatch, channels, n_blocks, heads,
                                                                      chain_ch, pair_blocks):
    """The weight image's size (mtts_weights_bytes) with and without MTTS_CHAIN_PAIR: the production estimator (width 384, hidden chunk
    256) grows by exactly its twelve blocks' pair streams; a (256, 256) or (128, 128) estimator and width 384 with MTTS_CHAIN_CH=128,
    whose blocks the plan never runs in the pair form, carry none."""
    hp = hparams.tiny(n_spks=2)
    hp = dataclasses.replace(hp, decoder=dataclasses.replace(hp.decoder, channels=channels, attention_head_dim=64, n_blocks=n_blocks,
                                                             num_mid_blocks=2, num_heads=heads))
    for k in SWITCH_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MTTS_CHAIN_CH", chain_ch)
    nbytes = {}
    for pair_on in ("1", "0"):
        monkeypatch.setenv("MTTS_CHAIN_PAIR", pair_on)
        h = make_context(hip, hp, synthetic)
        nbytes[pair_on] = lib.mtts_weights_bytes(h.ctx)
        assert nbytes[pair_on] > 0, lib.mtts_last_error()
    width, inner = channels[0], 64 * heads
    ch = 256 if width == 384 and chain_ch == "256" else 128
    streams = 0
    n_tblocks = (2 * len(channels) + 2) * n_blocks
    for n_qkv in (3 * inner, 0):                                     # per run of n_blocks: all but the last carry the next q|k|v
        per = n_tblocks // n_blocks * ((n_blocks - 1) if n_qkv else 1)
        can_pair = (hip.tblock_plan(width, inner, n_qkv, 1, M_MAX, chain_ch=int(chain_ch), pair_min_rows=0)[1] == PAIR).any()
        assert bool(can_pair) == pair_blocks
        if can_pair:
            streams += per * lib.mtts_chain_stream_frags_pair(width, inner, ch, n_qkv) * 2 * 8 * 1024
    assert (streams > 0) == pair_blocks
    assert nbytes["1"] - nbytes["0"] == streams, (nbytes, streams)

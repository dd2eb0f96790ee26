"""Build-time guard of the one-plane chain kernel's instruction streams (csrc/tblock_chain_h16.hip; CPU only, the gfx950 code
object of the in-tree build is disassembled).  Same hazards as tests/test_isa_guard.py guards for tblock_chain_kernel: the weight
ring is filled by inline-asm loads the compiler does not count, so every instantiation must keep its hands off a register whose
load is outstanding, must not spill or add loads inside the MFMA loops, and may wait only on the hand-written constants."""
import importlib.util
import re
from collections import Counter

import pytest

from conftest import ROOT
from test_isa_guard import disassemble, hot_loops, vm_waits


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return disassemble("tblock_chain_h16", tmp_path_factory)


def shapes(isa):
    out = []
    for name in isa:
        m = re.search(r"tblock_h16_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", name)
        if m:
            out.append((name, *(int(v) for v in m.groups())))
    return out


def test_instantiations_present_and_apart_from_the_two_plane_guard(isa):
    got = {(c, qb, ch, bf) for _, c, qb, ch, bf in shapes(isa)}
    for c, qb, ch in [(384, 32, 256), (384, 64, 256), (384, 96, 256), (384, 64, 128), (256, 32, 128), (256, 64, 128), (128, 32, 128), (128, 64, 128)]:
        assert (c, qb, ch, 0) in got and (c, qb, ch, 1) in got, (c, qb, ch)
    assert not any("tblock_chain_kernel" in n for n in isa)      # tests/test_isa_guard.py enumerates that substring


def test_h16_kernel_never_touches_a_register_with_its_load_outstanding(isa):
    spec = importlib.util.spec_from_file_location("isa_pending", ROOT / "tools" / "isa_pending.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    names = [s[0] for s in shapes(isa)]
    assert len(names) >= 16
    for name in names:
        bad = mod.pending_violations(isa[name])
        assert not bad, (name, [(hex(o), m, ops) for o, m, ops, _ in bad[:6]])


def test_h16_rings_are_not_spilled_waits_are_the_written_ones_and_one_mfma_per_mac(isa):
    for name, C, QB, CH, BF in shapes(isa):
        NT, NT1, MT, KG, KG2, SP = C // 128, CH // 128, QB // 16, C // 32, CH // 32, (QB + 63) // 64
        R = 4 * NT
        insns = isa[name]
        mf = [i for i, x in enumerate(insns) if x[1].startswith("v_mfma")]
        # no scratch traffic anywhere between the first and the last matrix instruction, and the right matrix instruction
        assert not any(x[1].startswith("scratch_") for x in insns[mf[0]:mf[-1]]), (name, "scratch traffic among the k-loops")
        kinds = {insns[i][1] for i in mf}
        assert kinds == {"v_mfma_f32_16x16x32_bf16" if BF else "v_mfma_f32_16x16x32_f16"}, (name, kinds)
        if C != 384:
            continue        # (the narrow widths of the test suite: the compiler unrolls some of their loops completely)
        hot = hot_loops(insns)
        assert len(hot) >= 3, (name, hot)                     # out-projection, hidden chunks, q|k|v passes
        allowed = {0, R - NT, R - NT1, 2 * NT + SP}           # 0: the drain that ends every k-loop
        seen_chunk = seen_qkv = False
        for a, b in hot:
            body = insns[a:b + 1]
            ops = Counter(x[1] for x in body)
            assert not any(k.startswith("scratch_") for k in ops), (name, "scratch traffic inside a k-loop")
            foreign = [k for k in ops if (k.startswith("global_load") and k != "global_load_dwordx4") or k.startswith("buffer_load")
                       or k.startswith("flat_load")]
            assert not foreign, (name, foreign)
            waits = vm_waits(body)
            assert set(waits) <= allowed, (name, dict(waits), allowed)
            n_mfma = sum(v for k, v in ops.items() if k.startswith("v_mfma"))
            n_load = ops["global_load_dwordx4"]
            if n_mfma == MT * (KG * NT1 + KG2 * NT) and ops.get("s_barrier", 0):      # one hidden chunk, one MFMA per MAC
                seen_chunk = True
                assert n_load == KG * NT1 + KG2 * NT, (name, n_load)
                assert waits[R - NT1] >= KG and waits[0] >= 2, (name, dict(waits))
                assert ops["s_barrier"] == 2
            elif n_mfma == MT * KG * NT and ops.get("global_store_dwordx2", 0):       # a q|k|v pass
                seen_qkv = True
                assert n_load == KG * NT, (name, n_load)
                assert waits[R - NT] >= KG and waits[0] >= 1, (name, dict(waits))
        assert seen_chunk and seen_qkv, name

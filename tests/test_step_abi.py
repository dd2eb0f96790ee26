"""CPU checks of the step-level entry: declared in include/mtts.h, exported, bound by _hip.py; the ABI version did not move; the
argument checks that need no device."""
import ctypes
import inspect

import pytest
import torch

from conftest import ROOT, sub


@pytest.fixture(scope="module")
def lib():
    hip = sub("_hip")
    hip.build()
    return hip.load()


def test_step_entries_are_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "mtts.h").read_text()
    # (declaration, export, arity and types: test_abi.py checks them for every entry of the header)
    assert lib.mtts_abi_version() == 2                               # entries were only added
    assert len(lib.mtts_cfm_step.argtypes) == 17
    # the entries existing tests bind keep their argument counts
    assert len(lib.mtts_conv_gn.argtypes) == 20 and len(lib.mtts_groupnorm_mish.argtypes) == 12
    assert len(lib.mtts_conv_gn_rows.argtypes) == 21 and len(lib.mtts_groupnorm_mish_rows.argtypes) == 14


def test_python_surface():
    hip, modules, bt = sub("_hip"), sub("modules"), sub("batcher")
    assert list(inspect.signature(hip.HipModel.cfm_step).parameters)[:10] == ["self", "z_pool", "mu_pool", "slots", "t0", "t1", "y_lengths",
                                                                               "y_max", "t_fold", "solver"]
    for name in ("step_pool", "step_prepare", "step_advance", "step_read", "step_rows"):
        assert callable(getattr(modules.CFM, name))
    assert callable(hip.conv_gn_rows) and callable(hip.groupnorm_mish_rows)
    assert bt.StepBatcher.submit.__doc__ == bt.FrameBudgetBatcher.submit.__doc__      # (the same contract)


def test_step_entry_checks_its_arguments_before_any_launch(lib, hparams):
    """No device is needed to be refused: a context without weights, then null arguments."""
    hip = sub("_hip")
    h = hip.HipModel(hparams.tiny())
    slots = (ctypes.c_int32 * 2)(0, 1)
    rc = lib.mtts_cfm_step(h.ctx, None, None, 2, 24, None, slots, None, None, None, 10, 0, 2, 12, None, 0, None)
    assert rc == -1 and b"weights not uploaded" in lib.mtts_last_error()
    assert lib.mtts_cfm_step(None, None, None, 2, 24, None, slots, None, None, None, 10, 0, 2, 12, None, 0, None) == -1
    with pytest.raises(ValueError, match="unsupported solver"):
        h.cfm_step(torch.zeros(1, 1, 1), torch.zeros(1, 1, 1), [0], [0.0], [1.0], [1], 1, 4, "heun")
    with pytest.raises(RuntimeError, match="HIP device"):
        h.cfm_step(torch.zeros(2, hparams.tiny().n_feats, 24), torch.zeros(2, hparams.tiny().n_feats, 24), [0], [0.0], [1.0], [1], 1, 4, "euler")

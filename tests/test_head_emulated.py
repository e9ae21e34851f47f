"""`not gpu` tier of the fused head-and-loss kernels (amx_px_ce_train, amx_px_dice_sums / amx_px_dice_train, amx_px_bce_sum /
amx_px_focal_train; csrc/head.hip, dice.hip): the kernel sources compiled for the CPU SIMT emulator (tests/emu) and called
through the C ABI, against the same formulas in fp64 torch, at geometries beyond one tile.  The `gpu` tier
(test_head_gpu.py) repeats the checks on the MI355X binary."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _head_checks as C  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_head_vs_fp64(name):
    C.check_case(name, "cpu")


@pytest.mark.parametrize("fn,why", C.REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(fn, why):
    C.check_refusal(fn, why, "cpu")


def test_scale_unless_one_multi():
    C.check_scale_unless_one_multi("cpu")

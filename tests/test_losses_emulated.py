"""`not gpu` tier of the dice / focal losses (select_loss('dice' | 'focal'), reference: atomai/losses_metrics/losses.py:13-89):
the kernel sources of csrc/dice.hip and head.hip compiled for the CPU SIMT emulator (tests/emu) and driven through the real
host code, against goldens of the reference.  The `gpu` tier (test_losses_gpu.py) repeats the checks on the MI355X binary."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _loss_checks as C  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", C.loss_case_names())
def test_loss_and_gradient_vs_reference(name):
    C.check_loss_level(name, "cpu")


def test_dice_with_more_classes_than_registers_hold():
    C.check_many_classes("cpu")


def test_dice_fused_with_the_head_equals_the_modular_path():
    C.check_fused_dice("cpu")


def test_focal_fused_with_the_head_equals_the_modular_path():
    C.check_fused_focal("cpu")


@pytest.mark.parametrize("name", list(C.NET_CASES))
def test_net_fwd_bwd_adam(name):
    C.check_net_case(name, "cpu")


@pytest.mark.parametrize("ncls,lossname", C.FIT_CASES)
def test_segmentor_fit_trajectory(ncls, lossname, tmp_path):
    C.check_fit_trajectory(ncls, lossname, tmp_path)


def test_dice_fit_is_bit_identical_when_repeated(tmp_path):
    C.check_fit_determinism(tmp_path)


def test_api():
    C.check_api("cpu")

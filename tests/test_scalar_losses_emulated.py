"""`not gpu` tier of the modular loss and metric kernels of csrc/head.hip (CrossEntropyLoss, BCEWithLogitsLoss, IoU): the
kernel sources compiled for the CPU SIMT emulator (tests/emu) and driven through the real host code, against fp64 torch
and a numpy restatement of the reference's IoU.  The `gpu` tier (test_scalar_losses_gpu.py) repeats every check on the
MI355X binary, where expf / logf / log1pf are the device's; no case is left to that tier alone (the 4096 * 256 + 5
element BCE case takes about three seconds here)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _scalar_loss_checks as C  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("shape", C.CE_SHAPES, ids=C.ce_case_ids())
def test_cross_entropy_vs_fp64(shape):
    C.check_ce_vs_fp64(shape, "cpu")


def test_cross_entropy_saturated_pixels_one_by_one():
    C.check_ce_saturated_pixels("cpu")


def test_cross_entropy_takes_views_and_rejects_wrong_targets():
    C.check_ce_wrapper("cpu")


def test_cross_entropy_abi_rejects_one_class_and_no_rows():
    C.check_ce_abi_rejects("cpu")


@pytest.mark.parametrize("shape", C.BCE_SHAPES, ids=C.bce_case_ids())
def test_bce_vs_fp64(shape):
    C.check_bce_vs_fp64(shape, "cpu")


def test_bce_fixed_saturating_vector():
    C.check_bce_fixed_vector("cpu")


def test_bce_bool_and_int64_targets():
    C.check_bce_target_dtypes("cpu")


def test_bce_second_grid_stride_pass_at_the_default_block_count():
    C.check_bce_second_pass("cpu")


@pytest.mark.parametrize("name", list(C.IOU_CASES))
def test_iou_histogram_is_exact(name):
    C.check_iou_hist(name, "cpu")


def test_iou_threshold_is_strict():
    C.check_iou_threshold_is_strict("cpu")

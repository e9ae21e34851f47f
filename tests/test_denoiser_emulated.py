"""`not gpu` tier for the DenoisingAutoencoder family: the kernel sources (the fused 1x1-head + MSE kernel of csrc/head.hip
and everything the net's tape launches) on the CPU SIMT emulator against float64 torch and the reference goldens.  The
`gpu` tier (test_denoiser_gpu.py) runs the same bodies on the MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _denoiser_checks as D  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", list(D.KERNEL_CASES))
def test_px_mse_train_vs_fp64(name):
    D.check_kernel_case(name, "cpu")


@pytest.mark.parametrize("why", D.REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(why):
    D.check_refusal(why, "cpu")


@pytest.mark.parametrize("last_filters,expect", [(16, "loss"), (12, "logits")])
def test_fused_node_equals_the_modular_path_beyond_one_tile(last_filters, expect):
    D.check_net_beyond_one_tile("cpu", last_filters, expect)


@pytest.mark.parametrize("name", sorted(D.NET_CASES))
def test_net_parity_vs_reference(name):
    D.check_net_case(name, "cpu")


def test_denoiser_api(tmp_path):
    D.check_api("cpu", tmp_path)


def test_two_fits_are_bit_identical(tmp_path):
    D.check_determinism("cpu", tmp_path)


def test_preprocess_denoiser_data():
    D.check_preprocess()


def test_indivisible_input_is_refused_up_front(tmp_path):
    D.check_refuses_indivisible_input("cpu", tmp_path)


def test_forward_hook_sees_its_child():
    D.check_forward_hooks("cpu")

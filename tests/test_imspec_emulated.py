"""`not gpu` tier for the ImSpec family (im2spec / spec2im): the kernel sources of csrc/conv1d.hip and csrc/signal.hip (and
of the 2-D blocks, BatchNorm passes and GEMM they work with) on the CPU SIMT emulator against the reference goldens and
float64 torch.  The `gpu` tier runs the same bodies on the MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _imspec_checks as I  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_net_parity_vs_reference(name):
    I.check_net_case(name, "cpu")


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_f64_statement_of_signal_ed_equals_reference(name):
    I.check_f64_statement_vs_golden(name)


@pytest.mark.parametrize("dims", [((16, 16), (64,)), ((64,), (16, 16))], ids=["im2spec", "spec2im"])
def test_default_architecture_inputs_clear_the_kink(dims):
    I.default_inputs_clear_the_kink(*dims)


@pytest.mark.parametrize("shape", I.KERNEL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv1d_kernels_vs_fp64(shape):
    I.check_conv1d_kernels("cpu", shape)


@pytest.mark.parametrize("dil", [1, 2, 4])
def test_conv1d_equals_conv2d_on_h1_view(dil):
    I.check_conv1d_vs_conv2d("cpu", dil)


def test_conv1d_refuses_only_what_it_cannot_do():
    I.check_conv1d_refusals("cpu")


def test_conv1d_layer_is_refused_before_any_launch():
    I.check_conv1d_node_refuses_up_front("cpu")


def test_pointwise_kernels_vs_fp64():
    I.check_pointwise_kernels("cpu")


def test_nearest_upsample_carries_the_affine_bit_exactly():
    I.check_upsample_carries_affine("cpu")


def test_mse_loss_kernel_and_deferral():
    I.check_mse_loss("cpu")


def test_two_fits_are_bit_identical(tmp_path):
    I.check_determinism("cpu", tmp_path)


def test_imspec_api(tmp_path):
    I.check_api("cpu", tmp_path)

"""`gpu` tier for the ImSpec family (im2spec / spec2im): the bodies of tests/_imspec_checks.py on the MI355X, plus the
default architecture against the float64 statement of SignalED that the `not gpu` tier pins to the reference."""
import pytest

import _imspec_checks as I

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_net_parity_vs_reference(name):
    I.check_net_case(name, "cuda")


@pytest.mark.parametrize("shape", I.KERNEL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv1d_kernels_vs_fp64(shape):
    I.check_conv1d_kernels("cuda", shape)


@pytest.mark.parametrize("dil", [1, 2, 4])
def test_conv1d_equals_conv2d_on_h1_view(dil):
    I.check_conv1d_vs_conv2d("cuda", dil)


def test_conv1d_refuses_only_what_it_cannot_do():
    I.check_conv1d_refusals("cuda")


def test_conv1d_layer_is_refused_before_any_launch():
    I.check_conv1d_node_refuses_up_front("cuda")


def test_pointwise_kernels_vs_fp64():
    I.check_pointwise_kernels("cuda")


def test_nearest_upsample_carries_the_affine_bit_exactly():
    I.check_upsample_carries_affine("cuda")


def test_mse_loss_kernel_and_deferral():
    I.check_mse_loss("cuda")


def test_two_fits_are_bit_identical(tmp_path):
    I.check_determinism("cuda", tmp_path)


def test_imspec_api(tmp_path):
    I.check_api("cuda", tmp_path)


@pytest.mark.parametrize("dims", [((16, 16), (64,)), ((64,), (16, 16))], ids=["im2spec", "spec2im"])
def test_default_architecture_vs_fp64(dims):
    I.check_default_architecture("cuda", *dims)

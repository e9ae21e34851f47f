"""`not gpu` tier of the pass kernels between the convolutions (csrc/spatial.hip, res.hip, resize.hip, pack.hip and the
BatchNorm part of bn.hip): the kernel sources compiled for the CPU SIMT emulator (tests/emu) and called through the C ABI,
against plain torch / numpy on the host, at ragged NHWC geometries with negative producer scales.  The `gpu` tier
(test_pass_gpu.py) repeats the checks on the MI355X binary and adds the second grid-stride trip of the capped launches."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _pass_checks as C  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()
    yield
    C.report()


@pytest.mark.parametrize("name", list(C.POOL_CASES))
def test_max_pool_fwd_bwd(name):
    C.check_pool_case(name, "cpu")


def test_max_pool_bwd_second_grid_stride_trip_with_bstats():
    C.check_pool_case("second_trip", "cpu", combos=[(True, True, True)])


def test_pool_backward_falls_back_to_bn_bwd_reduce_at_g5():
    C.check_pool_engine_fallback("cpu")


@pytest.mark.parametrize("G", C.WG1_GROUPS)
@pytest.mark.parametrize("shape", C.WG1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_bwd_with_first_layer_wgrad(shape, G):
    C.check_pool_wgrad1(shape, G, "cpu")


def test_pool_bwd_wgrad1_domain():
    C.check_pool_wgrad1_domain("cpu")


@pytest.mark.parametrize("name", list(C.UP_CASES))
def test_upsample_bwd(name):
    C.check_upsample_bwd(name, "cpu")


@pytest.mark.parametrize("name", list(C.RESIZE_CASES))
def test_resize_cat(name):
    C.check_resize_cat(name, "cpu")


@pytest.mark.parametrize("Cs", [8, 52])
@pytest.mark.parametrize("npix", [15, 1073])
def test_dilated_sum(npix, Cs):
    C.check_dilated_sum("cpu", npix, Cs)


@pytest.mark.parametrize("Cs", [4, 20, 256])
@pytest.mark.parametrize("npix", [1, 257, 1073])
def test_res_out_and_lrelu_bwd(npix, Cs):
    C.check_res_passes("cpu", npix, Cs)


def test_bn_eval_affine():
    C.check_bn_eval_affine("cpu")


@pytest.mark.parametrize("name", list(C.BN_CASES))
def test_bn_backward_chain(name):
    C.check_bn_chain(name, "cpu")


def test_rows_rule():
    C.check_rows_rule("cpu")


def test_layout_converters():
    C.check_layout("cpu")


def test_add_inplace():
    C.check_add_inplace("cpu")


def test_copy16():
    C.check_copy16("cpu")


@pytest.mark.parametrize("fn,why", C.REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(fn, why):
    C.check_refusal(fn, why, "cpu")


@pytest.mark.parametrize("model", list(C.TRAINED_NETS))
def test_training_step_with_trained_batchnorm_state(model):
    C.check_trained_bn_step(model, "cpu")

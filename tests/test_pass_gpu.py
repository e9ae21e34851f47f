"""`gpu` tier of the pass kernels between the convolutions: the checks of test_pass_emulated.py through the C ABI of
libatomai_amd.so on a real MI355X, plus one case per capped launch at the smallest size that needs a second grid-stride
trip."""
import pytest
import torch

import _pass_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "gpu tier needs an MI355X"
    from atomai_amd import _lib
    _lib.load()                                   # raises if the HIP extension is missing
    assert not _lib.is_test_backend()
    maps = open("/proc/self/maps").read()
    assert "libatomai_amd.so" in maps, "native library not mapped"
    hips = {l.split()[-1] for l in maps.splitlines() if "libamdhip64" in l}
    assert len(hips) == 1, f"more than one HIP runtime mapped: {hips}"
    yield
    C.report()


@pytest.mark.parametrize("name", list(C.POOL_CASES))
def test_max_pool_fwd_bwd(name):
    C.check_pool_case(name, "cuda")


def test_max_pool_bwd_second_grid_stride_trip_with_bstats():
    C.check_pool_case("second_trip", "cuda", combos=[(True, True, True)])


def test_pool_backward_falls_back_to_bn_bwd_reduce_at_g5():
    C.check_pool_engine_fallback("cuda")


@pytest.mark.parametrize("G", C.WG1_GROUPS)
@pytest.mark.parametrize("shape", C.WG1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_bwd_with_first_layer_wgrad(shape, G):
    C.check_pool_wgrad1(shape, G, "cuda")


def test_pool_bwd_wgrad1_domain():
    C.check_pool_wgrad1_domain("cuda")


@pytest.mark.parametrize("name", list(C.UP_CASES))
def test_upsample_bwd(name):
    C.check_upsample_bwd(name, "cuda")


@pytest.mark.parametrize("name", list(C.RESIZE_CASES))
def test_resize_cat(name):
    C.check_resize_cat(name, "cuda")


@pytest.mark.parametrize("Cs", [8, 52])
@pytest.mark.parametrize("npix", [15, 1073])
def test_dilated_sum(npix, Cs):
    C.check_dilated_sum("cuda", npix, Cs)


@pytest.mark.parametrize("Cs", [4, 20, 256])
@pytest.mark.parametrize("npix", [1, 257, 1073])
def test_res_out_and_lrelu_bwd(npix, Cs):
    C.check_res_passes("cuda", npix, Cs)


def test_bn_eval_affine():
    C.check_bn_eval_affine("cuda")


@pytest.mark.parametrize("name", list(C.BN_CASES))
def test_bn_backward_chain(name):
    C.check_bn_chain(name, "cuda")


def test_rows_rule():
    C.check_rows_rule("cuda")


def test_layout_converters():
    C.check_layout("cuda")


def test_add_inplace():
    C.check_add_inplace("cuda")


def test_copy16():
    C.check_copy16("cuda")


@pytest.mark.parametrize("fn,why", C.REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(fn, why):
    C.check_refusal(fn, why, "cuda")


@pytest.mark.parametrize("kernel", C.SECOND_TRIP)
def test_second_grid_stride_trip_of_a_capped_launch(kernel):
    C.check_second_trip(kernel, "cuda")


@pytest.mark.parametrize("model", list(C.TRAINED_NETS))
def test_training_step_with_trained_batchnorm_state(model):
    C.check_trained_bn_step(model, "cuda")

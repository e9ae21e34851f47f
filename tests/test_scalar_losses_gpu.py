"""`gpu` tier of the modular loss and metric kernels of csrc/head.hip: the checks of test_scalar_losses_emulated.py through
the C ABI of libatomai_amd.so on a real MI355X, where expf, logf and log1pf are the device's."""
import pytest
import torch

import _scalar_loss_checks as C

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


@pytest.mark.parametrize("shape", C.CE_SHAPES, ids=C.ce_case_ids())
def test_cross_entropy_vs_fp64(shape):
    C.check_ce_vs_fp64(shape, "cuda")


def test_cross_entropy_saturated_pixels_one_by_one():
    C.check_ce_saturated_pixels("cuda")


def test_cross_entropy_takes_views_and_rejects_wrong_targets():
    C.check_ce_wrapper("cuda")


def test_cross_entropy_abi_rejects_one_class_and_no_rows():
    C.check_ce_abi_rejects("cuda")


@pytest.mark.parametrize("shape", C.BCE_SHAPES, ids=C.bce_case_ids())
def test_bce_vs_fp64(shape):
    C.check_bce_vs_fp64(shape, "cuda")


def test_bce_fixed_saturating_vector():
    C.check_bce_fixed_vector("cuda")


def test_bce_bool_and_int64_targets():
    C.check_bce_target_dtypes("cuda")


def test_bce_second_grid_stride_pass_at_the_default_block_count():
    C.check_bce_second_pass("cuda")


@pytest.mark.parametrize("name", list(C.IOU_CASES))
def test_iou_histogram_is_exact(name):
    C.check_iou_hist(name, "cuda")


def test_iou_threshold_is_strict():
    C.check_iou_threshold_is_strict("cuda")

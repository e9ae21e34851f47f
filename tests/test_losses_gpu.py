"""`gpu` tier of the dice / focal losses: the checks of test_losses_emulated.py through the C ABI of libatomai_amd.so on a
real MI355X, plus full-size cases against the reference's formulas restated in fp64 torch on the host."""
import pytest
import torch

import _loss_checks as C

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


@pytest.mark.parametrize("name", C.loss_case_names())
def test_loss_and_gradient_vs_reference(name):
    C.check_loss_level(name, "cuda")


def test_dice_with_more_classes_than_registers_hold():
    C.check_many_classes("cuda")


def test_dice_fused_with_the_head_equals_the_modular_path():
    C.check_fused_dice("cuda")


def test_focal_fused_with_the_head_equals_the_modular_path():
    C.check_fused_focal("cuda")


@pytest.mark.parametrize("name", list(C.NET_CASES))
def test_net_fwd_bwd_adam(name):
    C.check_net_case(name, "cuda")


@pytest.mark.parametrize("ncls,lossname", C.FIT_CASES)
def test_segmentor_fit_trajectory(ncls, lossname, tmp_path):
    C.check_fit_trajectory(ncls, lossname, tmp_path)


def test_dice_fit_is_bit_identical_when_repeated(tmp_path):
    C.check_fit_determinism(tmp_path)


def test_api():
    C.check_api("cuda")


@pytest.mark.parametrize("K", [3, 1])
def test_full_size_vs_fp64_formulas(K):
    C.check_full_size("cuda", K)

"""`gpu` tier for the DenoisingAutoencoder family: the bodies of tests/_denoiser_checks.py through libatomai_amd.so on a
real MI355X."""
import pytest
import torch

import _denoiser_checks as D

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


@pytest.mark.parametrize("name", list(D.KERNEL_CASES))
def test_px_mse_train_vs_fp64(name):
    D.check_kernel_case(name, "cuda")


@pytest.mark.parametrize("why", D.REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(why):
    D.check_refusal(why, "cuda")


@pytest.mark.parametrize("last_filters,expect", [(16, "loss"), (12, "logits")])
def test_fused_node_equals_the_modular_path_beyond_one_tile(last_filters, expect):
    D.check_net_beyond_one_tile("cuda", last_filters, expect)


@pytest.mark.parametrize("name", sorted(D.NET_CASES))
def test_net_parity_vs_reference(name):
    D.check_net_case(name, "cuda")


def test_denoiser_api(tmp_path):
    D.check_api("cuda", tmp_path)


def test_two_fits_are_bit_identical(tmp_path):
    D.check_determinism("cuda", tmp_path)


def test_preprocess_denoiser_data():
    D.check_preprocess()


def test_indivisible_input_is_refused_up_front(tmp_path):
    D.check_refuses_indivisible_input("cuda", tmp_path)


def test_forward_hook_sees_its_child():
    D.check_forward_hooks("cuda")

"""`not gpu` tier for the peak-refinement kernels (CPU SIMT emulator) vs the reference golden."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _refine_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", K.CASES)
def test_parity_with_reference(name):
    K.check_parity(name, "cpu")


@pytest.mark.parametrize("name", ["d5", "d8_border", "half"])
def test_peak_refinement_entry_point(name):
    K.check_peak_refinement(name)


def test_locator_refine():
    K.check_locator("cpu")


def test_default_half_side():
    K.check_default_d("cpu")


def test_determinism():
    K.check_determinism("cpu")


def test_segmentor_predict_refine():
    K.check_end_to_end()


def test_edges():
    K.check_edges("cpu")

"""`gpu` tier for the peak-refinement kernels through libatomai_amd.so on the MI355X."""
import pytest

import _refine_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", K.CASES)
def test_parity_with_reference(name):
    K.check_parity(name, "cuda")


@pytest.mark.parametrize("name", ["d5", "d8_border", "half"])
def test_peak_refinement_entry_point(name):
    K.check_peak_refinement(name)


def test_locator_refine():
    K.check_locator("cuda")


def test_default_half_side():
    K.check_default_d("cuda")


def test_determinism():
    K.check_determinism("cuda")


def test_segmentor_predict_refine():
    K.check_end_to_end()


def test_edges():
    K.check_edges("cuda")

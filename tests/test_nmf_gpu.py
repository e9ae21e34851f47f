"""`gpu` tier for NMF on the device through libatomai_amd.so on the MI355X."""
import numpy as np
import pytest

import _nmf_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("trans", [0, 1], ids=["W", "Ht"])
@pytest.mark.parametrize("shape", K.HALF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_step_against_rule(shape, trans, dtype):
    K.check_half_step(shape, trans, dtype, "cuda")


@pytest.mark.parametrize("trans", [0, 1], ids=["W", "Ht"])
@pytest.mark.parametrize("shape,variant", K.HALF_VARIANTS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_half_step_zero_branches(shape, variant, trans):
    K.check_half_step(shape, trans, np.float64, "cuda", variant)


def test_splits_depend_on_shape_only():
    K.check_splits()


@pytest.mark.parametrize("name", list(K.FITS))
def test_fit_against_sklearn(name):
    K.check_fit(name, "cuda")


@pytest.mark.parametrize("name", list(K.FITS))
def test_fit_float32_input(name):
    K.check_fit(name, "cuda", np.float32)


def test_determinism():
    K.check_determinism("cuda")


@pytest.mark.parametrize("name", list(K.FFTS))
def test_fftwin_against_reference(name):
    K.check_fft(name)


def test_windows_in_place_equal_stack():
    K.check_in_place_equals_stack()


def test_analyze_image(tmp_path):
    K.check_analyze_image(tmp_path)


def test_two_windows_reduce_components(tmp_path):
    K.check_two_windows(tmp_path)


@pytest.mark.parametrize("name", K.STAT_CASES)
def test_imlocal_nmf_against_reference(name):
    K.check_imlocal(name)


def test_spectral_unmixer():
    K.check_unmixer()


def test_errors_and_warnings():
    K.check_errors("cuda")


def test_module_paths():
    K.check_module_paths()

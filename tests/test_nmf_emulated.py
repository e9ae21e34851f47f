"""`not gpu` tier for NMF on the device (CPU SIMT emulator): csrc/nmf.hip against the fp64 numpy rule and the scikit-learn
golden, csrc/fftwin.hip and the public functions and classes against the reference's recorded output."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _nmf_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("trans", [0, 1], ids=["W", "Ht"])
@pytest.mark.parametrize("shape", K.HALF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_step_against_rule(shape, trans, dtype):
    K.check_half_step(shape, trans, dtype, "cpu")


@pytest.mark.parametrize("trans", [0, 1], ids=["W", "Ht"])
@pytest.mark.parametrize("shape,variant", K.HALF_VARIANTS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_half_step_zero_branches(shape, variant, trans):
    K.check_half_step(shape, trans, np.float64, "cpu", variant)


def test_splits_depend_on_shape_only():
    K.check_splits()


@pytest.mark.parametrize("name", list(K.FITS))
def test_fit_against_sklearn(name):
    K.check_fit(name, "cpu")


@pytest.mark.parametrize("name", list(K.FITS))
def test_fit_float32_input(name):
    K.check_fit(name, "cpu", np.float32)


def test_determinism():
    K.check_determinism("cpu")


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
    K.check_errors("cpu")


def test_module_paths():
    K.check_module_paths()

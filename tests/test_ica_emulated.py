"""`not gpu` tier for FastICA on the device (CPU SIMT emulator): csrc/ica.hip against the fp64 numpy rule and the
scikit-learn golden, and the public functions and classes against the reference's recorded output."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _ica_checks as K  # noqa: E402

DEVICE = "cpu"


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("fun", K.FUN_NAMES)
@pytest.mark.parametrize("shape", K.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_against_rule(shape, fun):
    K.check_step(shape, fun, DEVICE)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", K.PROJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_projection_against_rule(shape, dtype):
    K.check_project(shape, dtype, DEVICE)


def test_grid_depends_on_shape_only():
    K.check_blocks()


@pytest.mark.parametrize("name", list(K.FITS))
def test_fit_against_sklearn(name):
    K.check_fit(name, DEVICE)


@pytest.mark.parametrize("name", list(K.FITS))
def test_fit_float32_input(name):
    K.check_fit(name, DEVICE, np.float32)


def test_determinism():
    K.check_determinism(DEVICE)


@pytest.mark.parametrize("name", K.STAT_CASES)
def test_imlocal_ica_against_reference(name):
    K.check_imlocal(name)


def test_ica_unmixer():
    K.check_unmixer()


def test_errors_and_warnings():
    K.check_errors(DEVICE)


def test_module_paths():
    K.check_module_paths()

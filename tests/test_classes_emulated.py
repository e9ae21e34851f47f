"""`not gpu` tier for the intensity-based classes (CPU SIMT emulator): csrc/intensity.hip against the numpy restatement and
the scikit-learn golden, update_classes against the reference's recorded tables."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _classes_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", K.cases())
def test_kth_gap_against_rule(name):
    K.check_gap(name, "cpu")


@pytest.mark.parametrize("name", K.cases())
def test_meanshift_seeds_against_rule(name):
    K.check_seeds(name, "cpu")


def test_lloyd_against_rule():
    K.check_lloyd("cpu")


def test_assign():
    K.check_assign("cpu")


@pytest.mark.parametrize("name", K.cases())
def test_bandwidth_and_mean_shift_against_golden(name):
    K.check_public(name, "cpu")


@pytest.mark.parametrize("name", K.km_cases())
def test_kmeans_against_golden(name):
    K.check_kmeans(name, "cpu")


def test_degenerate_inputs():
    K.check_degenerate("cpu")


def test_determinism():
    K.check_determinism("cpu")


def test_update_classes_against_reference():
    K.check_update_classes()


def test_errors():
    K.check_errors()


def test_package_level_update_classes():
    K.check_package_level()


def test_no_sklearn_behind_the_classes():
    K.check_no_sklearn()

"""`not gpu` tier for the density clustering of atom tables (CPU SIMT emulator): csrc/cluster.hip against the numpy rule
and the scikit-learn golden, cluster_coord against the reference's recorded output, ensemble_locate end to end."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _cluster_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


def test_tiny_tables():
    K.check_tiny("cpu")


@pytest.mark.parametrize("name", K.cases())
def test_dbscan_against_rule_and_golden(name):
    K.check_case(name, "cpu")


def test_segments_do_not_link():
    K.check_segments("cpu")


def test_grid_is_sized_by_rows():
    K.check_far_cells("cpu")


def test_determinism():
    K.check_determinism("cpu")


def test_validation():
    K.check_validation("cpu")


def test_cluster_coord_against_reference():
    K.check_cluster_coord()


def test_ensemble_locate():
    K.check_ensemble_locate()


def test_no_sklearn_on_the_analysis_path():
    K.check_no_sklearn()

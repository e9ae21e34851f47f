"""`gpu` tier for the density clustering of atom tables through libatomai_amd.so on the MI355X."""
import pytest

import _cluster_checks as K

pytestmark = pytest.mark.gpu


def test_tiny_tables():
    K.check_tiny("cuda")


@pytest.mark.parametrize("name", K.cases())
def test_dbscan_against_rule_and_golden(name):
    K.check_case(name, "cuda")


def test_segments_do_not_link():
    K.check_segments("cuda")


def test_grid_is_sized_by_rows():
    K.check_far_cells("cuda")


def test_determinism():
    K.check_determinism("cuda")


def test_validation():
    K.check_validation("cuda")


def test_cluster_coord_against_reference():
    K.check_cluster_coord()


def test_ensemble_locate():
    K.check_ensemble_locate()

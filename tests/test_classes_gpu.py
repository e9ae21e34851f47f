"""`gpu` tier for the intensity-based classes through libatomai_amd.so on the MI355X."""
import pytest

import _classes_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", K.cases())
def test_kth_gap_against_rule(name):
    K.check_gap(name, "cuda")


@pytest.mark.parametrize("name", K.cases())
def test_meanshift_seeds_against_rule(name):
    K.check_seeds(name, "cuda")


def test_lloyd_against_rule():
    K.check_lloyd("cuda")


def test_assign():
    K.check_assign("cuda")


@pytest.mark.parametrize("name", K.cases())
def test_bandwidth_and_mean_shift_against_golden(name):
    K.check_public(name, "cuda")


@pytest.mark.parametrize("name", K.km_cases())
def test_kmeans_against_golden(name):
    K.check_kmeans(name, "cuda")


def test_degenerate_inputs():
    K.check_degenerate("cuda")


def test_determinism():
    K.check_determinism("cuda")


def test_update_classes_against_reference():
    K.check_update_classes()


def test_errors():
    K.check_errors()


def test_package_level_update_classes():
    K.check_package_level()

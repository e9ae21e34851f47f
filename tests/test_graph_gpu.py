"""`gpu` tier for the graph analysis of atom tables through libatomai_amd.so on the MI355X."""
import pytest

import _graph_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", K.cases())
def test_case_against_rule_and_golden(name):
    K.check_case(name, "cuda")


def test_tiny_tables():
    K.check_tiny("cuda")


def test_dense_pile_is_searched_in_bounded_time():
    K.check_dense("cuda")


def test_frames_do_not_link():
    K.check_frames("cuda")


def test_pairs_at_the_cutoff():
    K.check_cutoff("cuda")


def test_determinism():
    K.check_determinism("cuda")


def test_validation():
    K.check_validation("cuda")


def test_no_host_libraries_on_the_computing_path(monkeypatch):
    K.check_no_host_libraries(monkeypatch)


def test_exports():
    K.check_exports()

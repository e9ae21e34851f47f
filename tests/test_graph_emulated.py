"""`not gpu` tier for the graph analysis of atom tables (CPU SIMT emulator): csrc/graph.hip and atomai_amd.utils.graphx
against the restatement of the rules and the golden recorded from the reference's graphx.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _graph_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", K.cases())
def test_case_against_rule_and_golden(name):
    K.check_case(name, "cpu")


def test_tiny_tables():
    K.check_tiny("cpu")


def test_dense_pile_is_searched_in_bounded_time():
    K.check_dense("cpu")


def test_frames_do_not_link():
    K.check_frames("cpu")


def test_pairs_at_the_cutoff():
    K.check_cutoff("cpu")


def test_determinism():
    K.check_determinism("cpu")


def test_validation():
    K.check_validation("cpu")


def test_no_host_libraries_on_the_computing_path(monkeypatch):
    K.check_no_host_libraries(monkeypatch)


def test_exports():
    K.check_exports()

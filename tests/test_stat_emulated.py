"""`not gpu` tier for atomai_amd.stat (CPU SIMT emulator): the EM pass kernels against fp64, imlocal against the golden."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _stat_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("shape", K.PASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pass_against_fp64(shape):
    K.check_pass(shape, "cpu")


def test_update_against_fp64():
    K.check_update("cpu")


def test_determinism():
    K.check_determinism("cpu")


def test_convergence_warning():
    K.check_no_convergence_warning("cpu")


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("cov", ["diag", "spherical"])
@pytest.mark.parametrize("name", K.CASES)
def test_gmm_partition(name, cov, seed):
    K.check_gmm(name, cov, seed)


@pytest.mark.parametrize("name", K.CASES)
def test_pca(name):
    K.check_pca(name)


def test_pca_gram_over_features():
    K.check_pca_wide("cpu")


def test_pca_gmm():
    K.check_pca_gmm()


def test_host_logic():
    K.check_host_logic()


def test_transition_matrix():
    K.check_transition_matrix()


def test_update_classes():
    K.check_update_classes()


def test_edges():
    K.check_edges("cpu")

"""`not gpu` tier for the nearest-neighbour functions of atomai_amd.utils (CPU SIMT emulator): csrc/knn.hip against fp64
brute force, the public functions against the golden."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _coords_checks as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("mode", ["self", "two"])
@pytest.mark.parametrize("k", K.KS)
@pytest.mark.parametrize("dim", [2, 3])
def test_knn_against_brute_force(dim, k, mode):
    K.check_knn(dim, k, mode, "cpu")


def test_knn_bound_and_ties():
    K.check_knn_bound_and_ties("cpu")


@pytest.mark.parametrize("dim", [2, 3])
def test_radius_against_brute_force(dim):
    K.check_radius(dim, "cpu")


@pytest.mark.parametrize("r", [1, 2, 3, 4, 7])
def test_window_mean_against_fp64(r):
    K.check_window_mean(r, "cpu")


@pytest.mark.parametrize("nn", [1, 2, 6, 15, 31])
def test_get_nn_distances(nn):
    K.check_get_nn_distances(nn)


def test_get_nn_distances_upper_bound():
    K.check_get_nn_distances_upper_bound()


def test_compare_coordinates():
    K.check_compare_coordinates()


def test_find_coord_clusters():
    K.check_find_coord_clusters()


@pytest.mark.parametrize("r", [2, 3, 4])
def test_get_intensities(r):
    K.check_get_intensities(r)


def test_determinism():
    K.check_determinism("cpu")


def test_edges():
    K.check_edges("cpu")

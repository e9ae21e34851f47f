"""`gpu` tier for the nearest-neighbour functions of atomai_amd.utils through libatomai_amd.so on the MI355X."""
import pytest

import _coords_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["self", "two"])
@pytest.mark.parametrize("k", K.KS)
@pytest.mark.parametrize("dim", [2, 3])
def test_knn_against_brute_force(dim, k, mode):
    K.check_knn(dim, k, mode, "cuda")


def test_knn_bound_and_ties():
    K.check_knn_bound_and_ties("cuda")


@pytest.mark.parametrize("dim", [2, 3])
def test_radius_against_brute_force(dim):
    K.check_radius(dim, "cuda")


@pytest.mark.parametrize("r", [1, 2, 3, 4, 7])
def test_window_mean_against_fp64(r):
    K.check_window_mean(r, "cuda")


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
    K.check_determinism("cuda")


def test_edges():
    K.check_edges("cuda")

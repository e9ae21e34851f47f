"""`gpu` tier for the training-set functions through libatomai_amd.so on the MI355X."""
import pytest

import _lattice_checks as K

pytestmark = pytest.mark.gpu


def test_make_atom_against_reference():
    K.check_make_atom()


@pytest.mark.parametrize("name", K.mask_cases())
def test_mask_against_reference(name):
    K.check_mask_case(name)


def test_class_column_is_not_modified():
    K.check_input_unchanged()


def test_owner_kernel_guards():
    K.check_owner_kernel("cuda")


def test_fill_float32_float64_and_background():
    K.check_fill_dtypes("cuda")


def test_bad_stamps_raise_before_launch():
    K.check_stamp_errors()


def test_custom_stamp_function_called_once_per_class():
    K.check_custom_called_once()


def test_as_tensor():
    K.check_as_tensor()


def test_crop_windows():
    K.check_crop("cuda")


@pytest.mark.parametrize("k", range(len(K.PATCH_SETTINGS)))
def test_extract_patches_against_sklearn(k):
    K.check_patches(k)


def test_extract_random_subimages_against_reference():
    K.check_random_subimages()


def test_no_sklearn_scipy_cv2_behind_the_training_sets():
    K.check_no_sklearn()

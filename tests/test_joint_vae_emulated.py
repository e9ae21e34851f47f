"""`not gpu` tier for the joint VAEs (jVAE / jrVAE): the kernel sources of csrc/joint.hip (and of the trunks, decoder and
ELBO kernels they feed) on the CPU SIMT emulator against the reference goldens.  The `gpu` tier runs the same bodies on the
MI355X."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import _joint_checks as J  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def emulator():
    if torch.cuda.is_available():
        pytest.skip("emulator tier is for GPU-less hosts")
    import emu_backend
    emu_backend.use_emulator()


@pytest.mark.parametrize("name", J.kernel_cases())
def test_joint_kernels_vs_reference(name):
    J.check_joint_kernels(name, "cpu")


@pytest.mark.parametrize("name", J.model_cases())
def test_joint_elbo_grads_adam(name):
    J.check_joint_case(name, "cpu")


def test_default_path_equals_step_by_step_path():
    J.check_default_path_equals_step_path("cpu")


def test_joint_api(tmp_path):
    J.check_api("cpu", tmp_path)


def test_c_abi_refuses_tables_beyond_the_limits():
    J.check_c_abi_limits("cpu")

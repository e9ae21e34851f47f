"""`gpu` tier for the joint VAEs (jVAE / jrVAE), through libatomai_amd.so on a real MI355X."""
import numpy as np
import pytest
import torch

import _joint_checks as J

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", J.kernel_cases())
def test_joint_kernels_vs_reference(name):
    J.check_joint_kernels(name, "cuda")


@pytest.mark.parametrize("name", J.model_cases())
def test_joint_elbo_grads_adam(name):
    J.check_joint_case(name, "cuda")


def test_default_path_equals_step_by_step_path():
    J.check_default_path_equals_step_path("cuda")


def test_joint_api(tmp_path):
    J.check_api("cuda", tmp_path)


def test_c_abi_refuses_tables_beyond_the_limits():
    J.check_c_abi_limits("cuda")


def test_jrvae_fit_loss_improves_and_is_deterministic(tmp_path):
    import atomai_amd as aoi
    X = np.random.RandomState(0).rand(256, 32, 32).astype(np.float32)
    hist = []
    for _ in range(2):
        m = aoi.models.jrVAE((32, 32), latent_dim=2, discrete_dim=[10], seed=0)
        torch.manual_seed(0)
        torch.cuda.manual_seed_all(0)
        m.fit(X, training_cycles=3, batch_size=64, filename=str(tmp_path / "m"))
        hist.append(list(m.loss_history["train_loss"]))
    assert hist[0] == hist[1]
    assert hist[0][-1] > hist[0][0]          # ELBO increases


def test_jrvae_full_shape_vs_oracle_on_device():
    J.check_full_shape_vs_oracle(128)

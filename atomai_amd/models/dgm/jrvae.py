"""jrVAE: rotationally (and translationally) invariant VAE with joint continuous and discrete latent variables
(reference: atomai/models/dgm/jrvae.py:23-233)."""
from typing import List

from .jvae import _JointVAE


class jrVAE(_JointVAE):
    """``jrVAE(in_dim, latent_dim=2, discrete_dim=[2], nb_classes=0, translation=True, seed=0, **kwargs)`` with the
    spatial decoder on the fused HIP kernels.  z = (angle, [dx, dy], content..., Gumbel-Softmax samples...)."""

    def __init__(self, in_dim: int = None, latent_dim: int = 2, discrete_dim: List[int] = [2], nb_classes: int = 0,
                 translation: bool = True, seed: int = 0, **kwargs) -> None:
        super().__init__(in_dim, latent_dim, discrete_dim, nb_classes, 3 if translation else 1, seed, kwargs)
        self.translation = translation

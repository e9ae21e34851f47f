"""jVAE: VAE with joint continuous and discrete (Gumbel-Softmax) latent variables (reference:
atomai/models/dgm/jvae.py:23-200).  ``_JointVAE`` holds what jVAE and jrVAE share."""
from copy import deepcopy as dc
from typing import List, Optional

import torch

from ..._joint import joint_latent
from ...losses_metrics import joint_rvae_loss, joint_vae_loss
from ...losses_metrics.vi_losses import _joint_elbo
from ...utils import set_train_rng
from .vae import BaseVAE


class _JointVAE(BaseVAE):
    """Forward pass and fit of the joint models.  Two paths, as rVAE has them:

    * default — neither ``reparameterize`` nor ``reparameterize_discrete`` (nor ``elbo_fn``) is overridden: the noise is
      drawn in the reference's order (one ``normal_()`` of (B, Z), then one ``uniform_()`` per head) and ONE kernel does
      the reparameterisation, the (phi, dx, dy) / content split, the Gumbel-Softmax sample of every head, the
      concatenation and the per-sample discrete KL (csrc/joint.hip);
    * step by step — the reference's dataflow through the (overridden) methods, ``torch.cat`` and ``kld_discrete``.
    Same noise -> same ELBO and gradients."""

    fused_latent = True          # class-level switch of the default path (measured: DESIGN.md, joint VAEs)

    def __init__(self, in_dim, latent_dim, discrete_dim, nb_classes, coord, seed, kwargs) -> None:
        if not isinstance(discrete_dim, list):
            raise ValueError("discrete_dim must be a list with the sizes of the discrete latent variables")
        super().__init__(in_dim, latent_dim, nb_classes, coord, discrete_dim, **kwargs)
        set_train_rng(seed)
        self.translation = coord == 3
        self.dx_prior = None
        self.phi_prior = None
        self.kdict_ = dc(kwargs)
        self.kdict_["num_iter"] = 0
        self.loss = "mse"

    def elbo_fn(self, x, x_reconstr, *args, **kwargs) -> torch.Tensor:
        fn = joint_rvae_loss if self.coord else joint_vae_loss
        return fn(self.loss, self.in_dim, x, x_reconstr, *args, **kwargs)

    def _default_sampling(self) -> bool:
        """True unless ``reparameterize`` / ``reparameterize_discrete`` / ``elbo_fn`` was overridden (subclass or instance
        attribute, as tests do to inject noise)."""
        from ...trainers import viBaseTrainer

        def stock(name):
            return (name not in self.__dict__
                    and getattr(getattr(type(self), name), "__func__", None) is getattr(viBaseTrainer, name).__func__)
        return (stock("reparameterize") and stock("reparameterize_discrete") and "elbo_fn" not in self.__dict__
                and hasattr(self.encoder_net, "forward_packed"))

    def _decode_train(self, theta, z):
        if self.coord:   # transform_coordinates(x_coord, phi, dx) is applied per pixel inside the decoder kernels
            return self.decoder_net.forward_grid(self.x_coord, theta, z)
        return self.decoder_net(z)

    def forward_compute_elbo(self, x: torch.Tensor, y: Optional[torch.Tensor] = None,
                             mode: str = "train") -> torch.Tensor:
        """Dataflow of jvae.py:98-134 / jrvae.py:105-152: encoder -> continuous and Gumbel-Softmax reparameterisation
        -> [rotate / translate the coordinate grid ->] decoder -> joint ELBO."""
        if y is not None:
            raise ValueError("the joint models learn their discrete classes: they take no labels (the decoder has no "
                             "inputs for a class one-hot once discrete_dim is given)")
        tau = self.kdict_.get("temperature", .67)
        x = x.to(self.device)
        with torch.set_grad_enabled(mode != "eval"):
            if self.fused_latent and self._default_sampling() and x.dtype == torch.float32:
                z_mean, z_logsd, alpha = self.encoder_net.forward_packed(x)
                if mode != "eval":
                    self.kdict_["num_iter"] += 1
                sizes = self.encoder_net.discrete_dim
                eps = z_mean.new(z_mean.size(0), z_mean.size(1)).normal_()
                us = [alpha.new(alpha.size(0), k).uniform_() for k in sizes]
                u = us[0] if len(us) == 1 else torch.cat(us, 1)
                theta, z, kl_disc = joint_latent(z_mean, z_logsd, eps, alpha, u, sizes, tau, self.coord,
                                                 float(self.dx_prior or 0.0))
                x_reconstr = self._decode_train(theta, z)
                return _joint_elbo(self.loss, self.in_dim, x, x_reconstr, z_mean, z_logsd, kl_disc.mean(), sizes,
                                   bool(self.coord), self.kdict_)
            latent_ = self.encoder_net(x)
            if mode != "eval":
                self.kdict_["num_iter"] += 1
            z_mean, z_logsd = latent_[:2]
            z_cont = self.reparameterize(z_mean, torch.exp(z_logsd))
            theta = None
            if self.coord:
                phi = z_cont[:, :1]
                if self.translation:
                    theta = torch.cat((phi, z_cont[:, 1:3] * self.dx_prior), 1)
                    z_cont = z_cont[:, 3:]
                else:
                    theta = torch.cat((phi, torch.zeros_like(z_cont[:, :1]).expand(-1, 2)), 1)
                    z_cont = z_cont[:, 1:]
            alphas = latent_[2:]
            z_disc = torch.cat([self.reparameterize_discrete(a, tau) for a in alphas], 1)
            z = torch.cat((z_cont, z_disc), dim=1)
            x_reconstr = self._decode_train(theta, z)
            return self.elbo_fn(x, x_reconstr, z_mean, z_logsd, alphas, **self.kdict_)

    def fit(self, X_train, y_train=None, X_test=None, y_test=None, loss: str = "mse", **kwargs) -> None:
        """Trains the model.  ``**kwargs``: ``temperature`` (Gumbel-Softmax relaxation, default 0.67), ``cont_capacity``
        / ``disc_capacity`` ([max_capacity, num_iters, gamma], default [5.0, 25000, 30]), for jrVAE ``translation_prior``
        and ``rotation_prior``, ``filename``, and the arguments of ``compile_trainer`` (``distributed`` among them)."""
        if y_train is not None or y_test is not None:
            raise ValueError("the joint models learn their discrete classes: fit() takes no labels")
        self._check_inputs(X_train, y_train, X_test, y_test)
        if self.coord:
            self.dx_prior = kwargs.get("translation_prior", 0.1)
            self.kdict_["phi_prior"] = kwargs.get("rotation_prior", 0.1)
        for k, v in kwargs.items():
            if k in ["cont_capacity", "disc_capacity", "temperature"]:
                self.kdict_[k] = v
        self.compile_trainer((X_train, y_train), (X_test, y_test), **kwargs)
        self.loss = loss
        if self.loss == "ce":                                 # decode() then applies a sigmoid ("prediction" stage)
            self.sigmoid_out = True
            self.metadict["sigmoid_out"] = True
        if kwargs.get("recording", False):
            raise NotImplementedError("manifold recording (matplotlib/torchvision tooling) is out of scope")
        self._fit_loop()


class jVAE(_JointVAE):
    """``jVAE(in_dim, latent_dim=2, discrete_dim=[2], nb_classes=0, seed=0, **kwargs)``: z = [content | samples]."""

    def __init__(self, in_dim: int = None, latent_dim: int = 2, discrete_dim: List[int] = [2], nb_classes: int = 0,
                 seed: int = 0, **kwargs) -> None:
        super().__init__(in_dim, latent_dim, discrete_dim, nb_classes, 0, seed, kwargs)

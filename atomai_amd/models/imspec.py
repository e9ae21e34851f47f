"""ImSpec: sklearn-like user API for image -> spectrum and spectrum -> image models
(reference: atomai/models/imspec.py:9-170)."""
from typing import Optional, Tuple, Type, Union

import numpy as np
import torch

from ..predictors import ImSpecPredictor
from ..trainers import ImSpecTrainer
from ..transforms import imspec_augmentor


class ImSpec(ImSpecTrainer):
    """``ImSpec(in_dim, out_dim, latent_dim, **kwargs).fit(...).predict(...)``: ``in_dim`` / ``out_dim`` are
    (height, width) for images and (length,) for spectra, one of each; keyword arguments as ImSpecTrainer.

    >>> model = aoi.models.ImSpec((16, 16), (64,), latent_dim=10)
    >>> model.fit(imgs_train, spectra_train, imgs_test, spectra_test, full_epoch=True, training_cycles=120, swa=True)
    >>> prediction = model.predict(imgs_test, norm=False)
    """

    def __init__(self, in_dim: Tuple[int], out_dim: Tuple[int], latent_dim: int = 2, **kwargs) -> None:
        super().__init__(in_dim, out_dim, latent_dim, **kwargs)
        self.latent_dim = latent_dim

    def fit(self, X_train: Union[np.ndarray, torch.Tensor], y_train: Union[np.ndarray, torch.Tensor],
            X_test: Optional[Union[np.ndarray, torch.Tensor]] = None,
            y_test: Optional[Union[np.ndarray, torch.Tensor]] = None, loss: str = 'mse',
            optimizer: Optional[Type[torch.optim.Optimizer]] = None, training_cycles: int = 1000, batch_size: int = 64,
            compute_accuracy: bool = False, full_epoch: bool = False, swa: bool = False,
            perturb_weights: bool = False, **kwargs):
        """Compiles the trainer and trains (imspec.py:63-145).  The on-the-fly augmentation keywords (gauss_noise,
        jitter, poisson_noise, contrast, salt_and_pepper, blur, background, custom_transform) raise
        NotImplementedError; ``distributed=True`` is not offered for this family."""
        if kwargs.get("distributed"):
            raise NotImplementedError("distributed=True is not offered for the ImSpec family")
        self.augment_fn = imspec_augmentor(self.in_dim, self.out_dim, **kwargs)       # refuses before any work is done
        self.compile_trainer((X_train, y_train, X_test, y_test), loss, optimizer, training_cycles, batch_size,
                             compute_accuracy, full_epoch, swa, perturb_weights, **kwargs)
        _ = self.run()

    def predict(self, data: np.ndarray, **kwargs) -> np.ndarray:
        """Applies the (trained) model to new data; ``num_batches`` (10), ``norm`` (True), ``verbose`` (True)
        (imspec.py:147-163)."""
        use_gpu = self.device == 'cuda'
        return ImSpecPredictor(self.net, self.out_dim, use_gpu, **kwargs).run(data, **kwargs)

    def load_weights(self, filepath: str) -> None:
        self.net.load_state_dict(torch.load(filepath, map_location=self.device))

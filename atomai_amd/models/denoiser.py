"""DenoisingAutoencoder: sklearn-like user API for cleaning images with a convolutional autoencoder trained on
noisy / clean pairs (reference: atomai/models/denoiser.py:20-270)."""
import warnings
from typing import Optional, Tuple, Type, Union

import numpy as np
import torch

from ..nets import DenoiserNet
from ..predictors import BasePredictor
from ..trainers import BaseTrainer
from ..utils import preprocess_denoiser_data, set_train_rng


class DenoisingAutoencoder(BaseTrainer):
    """``DenoisingAutoencoder(encoder_filters, decoder_filters, encoder_layers, decoder_layers, use_batch_norm,
    upsampling_mode, seed=1).fit(noisy, clean, ...).predict(noisy_new)``.  The net is nets.DenoiserNet (one HIP tape);
    training is BaseTrainer's loop with the one-pass MSE head (engine.PxLossNode) and the fused Adam.

    >>> model = aoi.models.DenoisingAutoencoder()
    >>> model.fit(noisy_images, clean_images, noisy_test, clean_test, training_cycles=500, swa=True)
    >>> cleaned = model.predict(new_noisy_images)
    """

    def __init__(self, encoder_filters: list = [8, 16, 32, 64], decoder_filters: list = [64, 32, 16, 8],
                 encoder_layers: list = [1, 2, 2, 2], decoder_layers: list = [2, 2, 2, 1],
                 use_batch_norm: bool = False, upsampling_mode: str = 'nearest', **kwargs) -> None:
        super().__init__()
        set_train_rng(kwargs.get("seed", 1))
        self.encoder_filters, self.decoder_filters = encoder_filters, decoder_filters
        self.encoder_layers, self.decoder_layers = encoder_layers, decoder_layers
        self.use_batch_norm, self.upsampling_mode = use_batch_norm, upsampling_mode
        self.net = DenoiserNet(encoder_filters, decoder_filters, encoder_layers, decoder_layers, use_batch_norm,
                               upsampling_mode)
        self.net.to(self.device)
        if self.device == 'cpu':
            warnings.warn("No GPU found: the MI355X kernels cannot run (there is no CPU fallback)", UserWarning)
        self.meta_state_dict = {
            "model_type": "denoising_autoencoder",
            "encoder_filters": encoder_filters,
            "decoder_filters": decoder_filters,
            "encoder_layers": encoder_layers,
            "decoder_layers": decoder_layers,
            "use_batch_norm": use_batch_norm,
            "upsampling_mode": upsampling_mode,
            "weights": self.net.state_dict(),
        }

    def fit(self, X_train: Union[np.ndarray, torch.Tensor], y_train: Union[np.ndarray, torch.Tensor],
            X_test: Optional[Union[np.ndarray, torch.Tensor]] = None,
            y_test: Optional[Union[np.ndarray, torch.Tensor]] = None, loss: str = 'mse',
            optimizer: Optional[Type[torch.optim.Optimizer]] = None, training_cycles: int = 500, batch_size: int = 32,
            compute_accuracy: bool = False, full_epoch: bool = False, swa: bool = True,
            perturb_weights: bool = False, **kwargs):
        """Noisy inputs and clean targets -> compile_trainer -> run (denoiser.py:132-186).  Without a test set 15 % of
        the data (``test_size``, ``seed``) is split off.  ``distributed=True`` is not offered for this family."""
        if kwargs.get("distributed"):
            raise NotImplementedError("distributed=True is not offered for the denoising autoencoder")
        if X_test is None or y_test is None:
            from sklearn.model_selection import train_test_split
            X_train, X_test, y_train, y_test = train_test_split(
                X_train, y_train, test_size=kwargs.get("test_size", .15), shuffle=True,
                random_state=kwargs.get("seed", 1))
        X_train, y_train, X_test, y_test = preprocess_denoiser_data(X_train, y_train, X_test, y_test)
        self.net._check_input(X_train[:1])                       # refuses before any work is done
        self.compile_trainer((X_train, y_train, X_test, y_test), loss=loss, optimizer=optimizer,
                             training_cycles=training_cycles, batch_size=batch_size, compute_accuracy=compute_accuracy,
                             full_epoch=full_epoch, swa=swa, perturb_weights=perturb_weights, **kwargs)
        self.run()
        self.meta_state_dict["weights"] = self.net.state_dict()

    def predict(self, data: Union[np.ndarray, torch.Tensor], **kwargs) -> np.ndarray:
        """Denoised images as a squeezed numpy array; a 2-D array is one image, a 3-D array a stack without the channel
        axis (denoiser.py:188-213).  ``num_batches`` as BasePredictor.predict."""
        predictor = BasePredictor(self.net, self.device == 'cuda', **kwargs)
        if isinstance(data, np.ndarray):
            if data.ndim == 2:
                data = data[None, None, ...]
            elif data.ndim == 3:
                data = data[:, None, ...]
        prediction = predictor.predict(data, **kwargs)
        return prediction.detach().cpu().numpy().squeeze()

    def load_weights(self, filepath: str) -> None:
        weight_dict = torch.load(filepath, map_location=self.device, weights_only=False)
        self.net.load_state_dict(weight_dict["weights"] if "weights" in weight_dict else weight_dict)


def init_denoising_autoencoder(**kwargs) -> Tuple[Type[torch.nn.Module], dict]:
    """(net, meta_state_dict) of a DenoisingAutoencoder built from ``kwargs``."""
    model = DenoisingAutoencoder(**kwargs)
    return model.net, model.meta_state_dict


def denoise_images(noisy_images: np.ndarray, clean_images: np.ndarray, test_noisy: Optional[np.ndarray] = None,
                   test_clean: Optional[np.ndarray] = None, training_cycles: int = 500,
                   **kwargs) -> Tuple[DenoisingAutoencoder, Optional[np.ndarray]]:
    """Trains a DenoisingAutoencoder and denoises ``test_noisy`` (None without it); ``kwargs`` go to the constructor AND
    to ``fit``, as in the reference (denoiser.py:238-270)."""
    model = DenoisingAutoencoder(**kwargs)
    model.fit(noisy_images, clean_images, test_noisy, test_clean, training_cycles=training_cycles, **kwargs)
    predictions = model.predict(test_noisy) if test_noisy is not None else None
    return model, predictions

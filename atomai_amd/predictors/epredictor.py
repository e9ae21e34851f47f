"""Prediction with an ensemble of trained weights (reference: atomai/predictors/epredictor.py:21-330).

``EnsemblePredictor(skeleton, ensemble, nb_classes=...).predict(data)`` -> (mean, variance) over the members, and
``ensemble_locate`` -> per-frame mean / variance of every detected coordinate.  Image-to-image (segmentation) models
only; every member's forward runs on the HIP engine (probabilities from the fused softmax / sigmoid head).
"""
from typing import Dict, Tuple, Type, Union

import numpy as np
import torch

from ..nets.fcnn import _HipNet, predict_proba
from ..utils import cluster_coord as _cluster_coord
from ..utils import cluster_coord_frames, get_downsample_factor, torch_format_image
from .locator import Locator
from .predictor import BasePredictor


class EnsemblePredictor(BasePredictor):
    def __init__(self, skeleton: Type[torch.nn.Module], ensemble: Dict[int, Dict[str, torch.Tensor]],
                 data_type: str = "image", output_type: str = "image", nb_classes: int = None,
                 in_dim: Tuple[int] = None, out_dim: Tuple[int] = None, **kwargs: Union[str, Tuple[int]]) -> None:
        super().__init__()
        if output_type not in ["image", "spectra"]:
            raise TypeError("Supported output types are 'image' and 'spectra'")
        if data_type != "image" or output_type != "image":
            raise NotImplementedError("ensembles of ImSpec models (spectra in or out) are outside the MI355X hot path of "
                                      "this build (single models: aoi.models.ImSpec / predictors.ImSpecPredictor)")
        self.device = "cpu"
        if kwargs.get("use_gpu", True) and torch.cuda.is_available():
            self.device = kwargs.get("device") or "cuda"
        self.model = skeleton
        self.ensemble = ensemble
        self.data_type, self.output_type = data_type, output_type
        self.nb_classes = nb_classes
        self.in_dim, self.out_dim = in_dim, out_dim
        self.downsample_factor = None
        self.logits = kwargs.get("logits", True)
        self.output_shape = kwargs.get("output_shape")
        verbose = kwargs.get("verbose", 1)
        self.everbose = bool(verbose)
        self.verbose = verbose > 1

    def _set_output_shape(self, data) -> None:
        ch = self.nb_classes if self.nb_classes else 1
        self.output_shape = (len(data), ch, *data.shape[2:])

    def preprocess(self, data: np.ndarray, norm: bool = True) -> torch.Tensor:
        if data.ndim == 2:
            data = data[np.newaxis, ...]
        return torch_format_image(data, norm)

    def _member_probabilities(self, data: torch.Tensor) -> torch.Tensor:
        """Channel-first probabilities of the currently loaded member."""
        nclasses = self.nb_classes or 0
        if isinstance(self.model, _HipNet) and self.logits and nclasses >= 1:
            self.model.eval()
            return predict_proba(self.model, data.to(self.device)).permute(0, 3, 1, 2)
        prob = self.forward_(data)
        if self.logits:
            if nclasses > 1:
                prob = torch.softmax(prob, dim=1)
            elif self.nb_classes == 1:
                prob = torch.sigmoid(prob)
        elif nclasses > 1:
            prob = torch.exp(prob)
        return prob

    def ensemble_forward(self, data: torch.Tensor, out_shape: Tuple[int], num_batches: int = 1) -> np.ndarray:
        """ALL predictions (n_models x n_samples x ...), float64 as in the reference."""
        epred = np.zeros((len(self.ensemble), *out_shape))
        for i, m in enumerate(self.ensemble.values()):
            self.model.load_state_dict(m)
            self._model2device()
            if num_batches > 1:
                bs = max(1, len(data) // num_batches)
                for s in range(0, len(data), bs):
                    epred[i, s:s + bs] = self._member_probabilities(data[s:s + bs]).cpu().numpy()
            else:
                epred[i] = self._member_probabilities(data).cpu().numpy()
        return epred

    def ensemble_forward_(self, data: torch.Tensor, out_shape: Tuple[int]) -> Tuple[np.ndarray]:
        epred = self.ensemble_forward(data, out_shape)
        return np.mean(epred, axis=0), np.var(epred, axis=0)

    def ensemble_batch_predict(self, data, num_batches: int = 10) -> Tuple[np.ndarray]:
        batch_size = len(data) // num_batches
        if batch_size < 1:
            num_batches = batch_size = 1
        mean, var = np.zeros(self.output_shape), np.zeros(self.output_shape)
        i = 0
        for i in range(num_batches):
            if self.everbose:
                print("\rBatch {}/{}".format(i + 1, num_batches), end="")
            sl = slice(i * batch_size, (i + 1) * batch_size)
            mean[sl], var[sl] = self.ensemble_forward_(data[sl], (batch_size, *self.output_shape[1:]))
        rest = data[(i + 1) * batch_size:]
        if len(rest) > 0:
            mean[(i + 1) * batch_size:], var[(i + 1) * batch_size:] = self.ensemble_forward_(
                rest, (len(rest), *self.output_shape[1:]))
        return mean, var

    def predict(self, data: np.ndarray, num_batches: int = 10, format_out: str = "channel_last",
                norm: bool = True) -> Tuple[np.ndarray]:
        if format_out not in ["channel_first", "channel_last"]:
            raise ValueError("Specify channel_last or channel_first output format")
        data = self.preprocess(data, norm)
        if not self.output_shape:
            self._set_output_shape(data)
        if self.downsample_factor is None:
            self._model2device()                 # the mock forward below runs HIP kernels: the net must be on the GPU
            self.downsample_factor = get_downsample_factor(self.model)
        mean, var = self.ensemble_batch_predict(data, num_batches)
        if format_out == "channel_last":
            tr = (0, *(np.arange(mean.ndim - 2) + 2), 1)
            return mean.transpose(tr), var.transpose(tr)
        return mean, var


def cluster_coord(coord_class_dict, eps: float, min_samples: int = 10) -> Tuple[np.ndarray]:
    """DBSCAN clustering of coordinates collapsed over the members (atomai/utils/coords.py:304-347), on the device:
    ``atomai_amd.utils.cluster_coord``."""
    return _cluster_coord(coord_class_dict, eps, min_samples)


def ensemble_locate(nn_output_ensemble: np.ndarray, **kwargs) -> Tuple[Dict, Dict]:
    """Mean and variance of every detected coordinate over the members' predictions (5D input:
    members x frames x H x W x C); epredictor.py:297-330.  The Locator runs over the whole members x frames stack and
    the members' centres of all frames are clustered in one segmented pass, every frame a segment."""
    eps = kwargs.get("eps", 0.5)
    thresh = kwargs.get("threshold", 0.5)
    nn_output_ensemble = np.asarray(nn_output_ensemble)
    if nn_output_ensemble.ndim != 5:
        raise ValueError("expected a 5D array: members x frames x H x W x C")
    M, F = nn_output_ensemble.shape[:2]
    tables = Locator(thresh).run(nn_output_ensemble.reshape(M * F, *nn_output_ensemble.shape[2:]))
    means, variances = cluster_coord_frames([[tables[m * F + i] for m in range(M)] for i in range(F)], eps)
    return dict(enumerate(means)), dict(enumerate(variances))

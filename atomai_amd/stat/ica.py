"""FastICA on the device (csrc/ica.hip) at the reference's entry points: ICA of the sub-image stack of an ``imlocal``
instance (atomai/stat/multivar.py: imlocal.ica, imlocal.imblock_ica) and of a hyperspectral cube
(atomai/stat/unmixer.py: SpectralUnmixer(method='ica')).  The methods of ``imlocal`` and ``SpectralUnmixer('ica')``
themselves still raise; these functions take the instance as their first argument:

    >>> imstack = aoi.stat.imlocal(nn_output, coordinates, window_size=32, coord_class=1)
    >>> components, X_vec_t, com_frames = aoi.stat.ica.imlocal_ica(imstack, n_components=4)
    >>> spectra, maps = aoi.stat.ica.ICAUnmixer(n_components=3).fit(cube)

The arithmetic is fp64 on the values of the stack whatever its dtype: a float32 stack gives what scikit-learn gives on its
float64 copy, not what scikit-learn's float32 arithmetic gives.
"""
from typing import Tuple

import numpy as np

from ._ica import fit_ica  # noqa: F401  (re-exported)
from .multivar import imlocal
from .nmf import _stack_matrix


def imlocal_ica(stack: imlocal, n_components: int, random_state: int = 1,
                plot_results: bool = False) -> Tuple[np.ndarray]:
    """ICA independent sources of the stack of sub-images (scikit-learn's FastICA defaults: 'parallel', 'logcosh',
    whiten='unit-variance', 200 iterations, tol 1e-4).

    Returns (4D array of the computed and reshaped sources, 2D array of the stack transformed by the model, 2D array
    with the centre coordinates and the frame number of every sub-image), all float64."""
    res = fit_ica(_stack_matrix(stack), n_components, random_state=random_state)
    components = res["components"].cpu().numpy().reshape(-1, stack.d1, stack.d2, stack.d3)
    X_vec_t = res["sources"].cpu().numpy()
    com_frames = np.concatenate((stack.imgstack_com, stack.imgstack_frames[:, None]), axis=-1).astype(np.float64)
    if plot_results:
        stack.plot_decomposition_results(components, X_vec_t, plot_loading_maps=False)
    return components, X_vec_t, com_frames


def imblock_ica(stack: imlocal, n_components: int, random_state: int = 1, plot_results: bool = False,
                **kwargs: int) -> Tuple[np.ndarray]:
    """ICA sources and their loading maps, for finding domains in a single image: (sources, transformed stack,
    coordinates of every sub-image).  ``marker_size`` sets the marker size of the loading maps."""
    components, X_vec_t, com_frames = imlocal_ica(stack, n_components, random_state)
    centres = com_frames[:, :2]
    if plot_results:
        if len(stack.network_output) != 1:
            raise ValueError("loading maps need a single mother image: network_output must be (1, h, w, c), got "
                             f"{tuple(stack.network_output.shape)}")
        stack.plot_decomposition_results(components, X_vec_t, stack.network_output.shape[1:3], centres,
                                         **{k: v for k, v in kwargs.items() if k == "marker_size" and v is not None})
    return components, X_vec_t, centres


class ICAUnmixer:
    """Decomposes an (h, w, e) hyperspectral cube into ``n_components`` independent spectra and their abundance maps, as
    the reference's ``SpectralUnmixer('ica', n_components, normalize, max_iter=...)`` does.

    Args:
        n_components: number of components (at most 32)
        normalize: L1-normalise every spectrum before the decomposition; the abundances are scaled back
        max_iter: iterations of the fixed point (200)
        random_state: seed of the initial unmixing matrix; None draws from numpy's global state, as the reference does
            (``np.random.seed(s)`` before ``fit`` reproduces it)
    """
    method = "ica"

    def __init__(self, n_components: int = 4, normalize: bool = False, max_iter: int = 200, random_state=None):
        self.n_components = n_components
        self.normalize = normalize
        self.max_iter = max_iter
        self.random_state = random_state
        self.components_ = None
        self.abundance_maps_ = None
        self.image_shape_ = None
        self.n_iter_ = None

    def fit(self, hspy_data: np.ndarray):
        """Fits the model to the cube and returns (components (k, e), abundance maps (h, w, k))."""
        hspy_data = np.asarray(hspy_data)
        if hspy_data.ndim != 3:
            raise ValueError("Input data must be a 3D hyperspectral cube (h, w, e).")
        self.image_shape_ = hspy_data.shape[:2]
        h, w, e = hspy_data.shape
        spectra = hspy_data.reshape((h * w, e))
        to_fit = spectra
        if self.normalize:
            l1_norms = np.sum(spectra, axis=1, keepdims=True)
            l1_norms[l1_norms == 0] = 1
            to_fit = spectra / l1_norms
        res = fit_ica(to_fit, self.n_components, whiten="unit-variance", max_iter=self.max_iter,
                      random_state=self.random_state)
        self.n_iter_ = res["n_iter"]
        self.components_ = res["components"].cpu().numpy()
        abundances = res["sources"].cpu().numpy()
        if self.normalize:
            abundances = abundances * l1_norms
        self.abundance_maps_ = abundances.reshape((h, w, abundances.shape[1]))
        return self.components_, self.abundance_maps_

    def plot_results(self, x_axis_vals=None, x_axis_units=None, **kwargs):
        from .unmixer import SpectralUnmixer
        SpectralUnmixer.plot_results(self, x_axis_vals, x_axis_units, **kwargs)

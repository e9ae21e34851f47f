"""NMF of the sub-image stack of an ``imlocal`` instance (atomai/stat/multivar.py: imlocal.nmf, imlocal.imblock_nmf), on
the device.  The methods of the class itself still raise; these functions take the instance as their first argument:

    >>> imstack = aoi.stat.imlocal(nn_output, coordinates, window_size=32, coord_class=1)
    >>> components, X_vec_t, com_frames = aoi.stat.nmf.imlocal_nmf(imstack, n_components=4)
"""
from typing import Tuple

import numpy as np

from ._nmf import fit_nmf  # noqa: F401  (re-exported)
from .multivar import imlocal


def _stack_matrix(stack: imlocal) -> np.ndarray:
    X = stack.imgstack.reshape(stack.d0, stack.d1 * stack.d2 * stack.d3)
    return X if X.dtype in (np.float32, np.float64) else X.astype(np.float64)


def imlocal_nmf(stack: imlocal, n_components: int, random_state: int = 1, plot_results: bool = False,
                **kwargs: int) -> Tuple[np.ndarray]:
    """NMF source separation of the stack of sub-images, with scikit-learn's default initialisation.

    Returns (4D array of the computed and reshaped sources, 2D array of the stack transformed by the model, 2D array
    with the centre coordinates and the frame number of every sub-image), all float64.  ``max_iterations``: default 1000."""
    res = fit_nmf(_stack_matrix(stack), n_components, init=None, random_state=random_state,
                  max_iter=kwargs.get("max_iterations", 1000))
    components = res["H"].cpu().numpy().reshape(n_components, stack.d1, stack.d2, stack.d3)
    X_vec_t = res["W"].cpu().numpy()
    com_frames = np.concatenate((stack.imgstack_com, stack.imgstack_frames[:, None]), axis=-1).astype(np.float64)
    if plot_results:
        stack.plot_decomposition_results(components, X_vec_t, plot_loading_maps=False)
    return components, X_vec_t, com_frames


def imblock_nmf(stack: imlocal, n_components: int, random_state: int = 1, plot_results: bool = False,
                **kwargs: int) -> Tuple[np.ndarray]:
    """NMF sources and their loading maps, for finding domains in a single image: (sources, transformed stack,
    coordinates of every sub-image).  ``marker_size`` sets the marker size of the loading maps."""
    components, X_vec_t, com_frames = imlocal_nmf(stack, n_components, random_state,
                                                  **{k: v for k, v in kwargs.items() if k == "max_iterations"})
    centres = com_frames[:, :2]
    if plot_results:
        if len(stack.network_output) != 1:
            raise ValueError("loading maps need a single mother image: network_output must be (1, h, w, c), got "
                             f"{tuple(stack.network_output.shape)}")
        stack.plot_decomposition_results(components, X_vec_t, stack.network_output.shape[1:3], centres,
                                         **{k: v for k, v in kwargs.items() if k == "marker_size" and v is not None})
    return components, X_vec_t, centres

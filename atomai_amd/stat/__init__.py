"""Statistical analysis of local image descriptors (atomai.stat): GMM and PCA of atom sub-images on the device; NMF in the
submodules ``nmf`` (imlocal_nmf, imblock_nmf, fit_nmf), ``fft_nmf`` (SlidingFFTNMF) and ``unmixer`` (SpectralUnmixer);
FastICA in the submodule ``ica`` (imlocal_ica, imblock_ica, ICAUnmixer, fit_ica); intensity-based classes in the submodule
``intensity`` (update_classes with 'threshold' / 'kmeans' / 'meanshift', estimate_bandwidth, mean_shift, kmeans)."""
from . import fft_nmf, ica, intensity, nmf, unmixer  # noqa: F401
from .multivar import (SlidingFFTNMF, SpectralUnmixer, calculate_transition_matrix, imlocal, sum_transitions,
                       update_classes)

__all__ = ["imlocal", "calculate_transition_matrix", "sum_transitions", "update_classes", "SlidingFFTNMF",
           "SpectralUnmixer"]

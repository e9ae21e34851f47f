"""Statistical analysis of local image descriptors (atomai.stat): GMM and PCA of atom sub-images on the device."""
from .multivar import (SlidingFFTNMF, SpectralUnmixer, calculate_transition_matrix, imlocal, sum_transitions,
                       update_classes)

__all__ = ["imlocal", "calculate_transition_matrix", "sum_transitions", "update_classes", "SlidingFFTNMF",
           "SpectralUnmixer"]

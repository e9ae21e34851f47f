"""Statistical analysis of local image descriptors (atomai/stat/multivar.py): ``imlocal`` cuts sub-images around the
located atoms and runs a Gaussian mixture model or a principal component analysis on the flattened stack.

The stack is extracted on the host, exact in the input's dtype (``utils.extract_subimages``); its float32 copy is uploaded
once, on the first ``gmm`` / ``pca`` call, and kept.  The mixture runs on the device (csrc/stat.hip through ``_gmm.py``);
PCA is a Gram matrix on the fp32-MFMA GEMM plus ``torch.linalg.eigh`` in fp64.  No scipy or scikit-learn dependency.
"""
import copy
from typing import Dict, List, Tuple, Union

import numpy as np
import torch

from ..nets._linear import _gemm
from ..utils import extract_subimages
from . import _gmm

_ICA_ELSEWHERE = ("{} still raises here; the working code is {}: FastICA (parallel, fixed point) runs on the device "
                  "(csrc/ica.hip).")
_NMF_ELSEWHERE = ("{} still raises here; the working code is {}: NMF by coordinate descent runs on the device "
                  "(csrc/nmf.hip).")


def _pyplot():
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise ImportError("plot_results=True needs matplotlib, which does not import here; "
                          "call with plot_results=False") from e
    return plt


def _panel(img: np.ndarray) -> dict:
    """imshow arguments for one (h, w, c) image: RGB for three channels, a diverging map of the channel sum otherwise."""
    if img.shape[-1] == 3:
        return dict(X=np.clip(img, 0, 1))
    return dict(X=img.sum(-1), cmap="seismic")


def _show_images(images, titles, suptitle=None):
    """A near-square grid of small images, one panel each."""
    plt = _pyplot()
    n = len(images)
    ncols = max(1, int(np.ceil(np.sqrt(n))))
    nrows = -(-n // ncols)
    fig, axes = plt.subplots(nrows, ncols, figsize=(3 * ncols, 3.3 * nrows), squeeze=False)
    for ax in axes.ravel():
        ax.set_axis_off()
    for ax, img, title in zip(axes.ravel(), images, titles):
        ax.imshow(interpolation="gaussian", **_panel(img))
        ax.set_title(title, fontsize=10)
    if suptitle:
        fig.suptitle(suptitle)
    fig.tight_layout()
    plt.show()


def _show_scree(ratios, title):
    plt = _pyplot()
    fig, ax = plt.subplots(figsize=(5, 4))
    ax.plot(np.arange(1, len(ratios) + 1), ratios, marker="o")
    ax.set_xlim(0.5, min(len(ratios), 50) + 0.5)
    ax.set_xlabel("principal component")
    ax.set_ylabel("explained variance ratio")
    ax.set_title(title)
    fig.tight_layout()
    plt.show()


def _device():
    from .. import _lib as L
    return torch.device("cpu") if L.is_test_backend() and not torch.cuda.is_available() else torch.device("cuda")


def _pca_device(X: torch.Tensor, n_components: int = None, ratios_only: bool = False):
    """PCA of the (N, D) float32 device tensor ``X``: returns (components (n, D), projections (N, n), explained variance
    ratio (n,)) as float64 numpy arrays, n = min(N, D) when ``n_components`` is None; ``ratios_only`` stops after the
    eigenvalues and returns (None, None, ratio).  The Gram matrix of the centred
    stack is D x D when D <= N, else N x N; sign convention of sklearn's svd_flip(u_based_decision=False): the
    largest-magnitude entry of every component is positive."""
    N, D = X.shape
    full = min(N, D)
    n = full if n_components is None else int(n_components)
    if not 1 <= n <= full:
        raise ValueError(f"n_components={n_components} must be between 1 and min(n_samples, n_features)={full}")
    mean = _gmm.column_mean(X)
    Xc = (X - mean.to(torch.float32)).contiguous()
    if D <= N:                                       # G[i][j] = sum_n Xc[n][i] Xc[n][j]
        G = _gemm(Xc, 1, D, Xc, D, 1, D, D, N)
    else:                                            # G[a][b] = sum_d Xc[a][d] Xc[b][d]
        G = _gemm(Xc, D, 1, Xc, 1, D, N, N, D)
    G = G.to(torch.float64)
    lam, vec = torch.linalg.eigh((G + G.T) * 0.5)
    lam = lam.flip(0).clamp_(min=0.0)[:full]         # descending
    vec = vec.flip(1)[:, :n].contiguous()
    ratio = (lam / lam.sum())[:n]
    if ratios_only:
        return None, None, ratio.cpu().numpy()
    if D <= N:
        comp = vec.T.contiguous()                    # (n, D)
    else:                                            # right singular vectors from the left ones: V^T = S^-1 U^T Xc
        U32 = vec.to(torch.float32).contiguous()
        comp = _gemm(U32, 1, n, Xc, D, 1, n, D, N).to(torch.float64)
        comp = comp / torch.linalg.norm(comp, dim=1, keepdim=True).clamp_(min=torch.finfo(torch.float64).tiny)
    idx = comp.abs().argmax(1, keepdim=True)
    comp = comp * torch.sign(comp.gather(1, idx))
    C32 = comp.to(torch.float32).contiguous()
    proj = _gemm(Xc, D, 1, C32, 1, D, N, n, D)       # projection: one more GEMM
    return comp.cpu().numpy(), proj.to(torch.float64).cpu().numpy(), ratio.cpu().numpy()


class imlocal:
    """Extraction and statistical analysis of local image descriptors (atomai/stat/multivar.py:23-755).

    Args:
        network_output: 4D numpy array (images, height, width, channels), e.g. the output of ``Segmentor.predict``
        coord_class_dict_all: the Locator's dictionary of (N, 3) arrays (row, col, class)
        window_size: side of the square sub-images
        coord_class: class of the atoms around which the sub-images are cropped

    Example:

        >>> nn_output, coordinates = model.predict(expdata)
        >>> imstack = aoi.stat.imlocal(nn_output, coordinates, window_size=32, coord_class=1)
        >>> components_img, classes_list, com_frames = imstack.gmm(n_components=10)
        >>> trans = imstack.transition_matrix(n_components=10, rmax=10)
    """

    def __init__(self, network_output: np.ndarray, coord_class_dict_all: Dict[int, np.ndarray],
                 window_size: int = None, coord_class: int = 0) -> None:
        self.network_output = network_output
        self.nb_classes = network_output.shape[-1]
        self.coord_all = coord_class_dict_all
        self.coord_class = float(coord_class)
        self.r = window_size
        self.imgstack, self.imgstack_com, self.imgstack_frames = self.extract_subimages_()
        if isinstance(self.imgstack, list):
            raise ValueError(f"no sub-image of class {coord_class} with window_size={window_size} lies inside its "
                             "frame: nothing to analyse")
        self.d0, self.d1, self.d2, self.d3 = self.imgstack.shape
        self._stack_dev = None

    def extract_subimages_(self) -> Tuple[np.ndarray]:
        return extract_subimages(self.network_output, self.coord_all, self.r, self.coord_class)

    def _device_stack(self) -> torch.Tensor:
        """The (d0, d1*d2*d3) float32 device copy of the stack: uploaded once and kept."""
        if self._stack_dev is None:
            flat = np.ascontiguousarray(self.imgstack.reshape(self.d0, -1), dtype=np.float32)
            self._stack_dev = torch.from_numpy(flat).to(_device())
        return self._stack_dev

    # ------------------------------------------------------------------------------------------------ mixture model
    def gmm(self, n_components: int, covariance: str = 'diag', random_state: int = 1,
            plot_results: bool = False) -> Tuple[np.ndarray, List, np.ndarray]:
        """Gaussian mixture model of the stack, on the device ('diag' or 'spherical'; 'full' and 'tied' raise).

        Returns (4D array of class-averaged images, list of the 4D image stacks of every class, 2D array with the xy
        coordinates, the 1-based class and the frame number of every sub-image) as the reference does.  The component
        NUMBERING depends on the initialisation (k-means++ draws from ``numpy.random.default_rng(random_state)``) and is
        not the reference's; the partition is the same wherever the classes are well separated."""
        if covariance in ("full", "tied"):
            raise NotImplementedError(f"covariance '{covariance}' is not implemented on the device; "
                                      "choose 'diag' or 'spherical'")
        if covariance not in _gmm.COVARIANCES:
            raise ValueError(f"unknown covariance '{covariance}'")
        _gmm._check_k(n_components)
        labels = _gmm.fit_gmm(self._device_stack(), n_components, covariance, random_state)["labels"].cpu().numpy()
        members = [self.imgstack[labels == k] for k in range(int(labels.max()) + 1)]    # up to the last class in use
        averages = np.stack([m.mean(axis=0, dtype=np.float64) for m in members])         # on the host, in fp64
        if plot_results:
            _show_images(averages, [f"class {k + 1}: {len(m)} sub-images" for k, m in enumerate(members)],
                         "GMM class averages")
        table = np.column_stack((self.imgstack_com, labels + 1, self.imgstack_frames)).astype(np.float64)
        return averages, members, table

    # ------------------------------------------------------------------------------------------------ PCA
    def _pca_of(self, imgs: np.ndarray, n_components, ratios_only=False):
        if imgs is self.imgstack:
            X = self._device_stack()
        else:
            X = torch.from_numpy(np.ascontiguousarray(imgs.reshape(imgs.shape[0], -1), dtype=np.float32)).to(_device())
        return _pca_device(X, n_components, ratios_only)

    def _window_shape(self, n):
        return (n, self.d1, self.d2, self.d3)

    def pca(self, n_components: int, random_state: int = 1, plot_results: bool = False) -> Tuple[np.ndarray]:
        """PCA eigenvectors of the stack: (4D array of the reshaped principal axes, 2D projection of the flattened
        sub-images on them, 2D array with the coordinates and frame number of every sub-image).  ``random_state`` is
        accepted for the reference's signature; the full decomposition is deterministic."""
        axes, scores, _ = self._pca_of(self.imgstack, n_components)
        axes = axes.reshape(self._window_shape(n_components))
        if plot_results:
            self.plot_decomposition_results(axes, scores, plot_loading_maps=False)
        return axes, scores, np.column_stack((self.imgstack_com, self.imgstack_frames)).astype(np.float64)

    def pca_gmm(self, n_components_gmm: int, n_components_pca: Union[int, List[int]], plot_results: bool = False,
                covariance_type: str = 'diag', random_state: int = 1) -> Tuple[np.ndarray, List]:
        """PCA of every GMM class: (GMM class averages, list of 4D PCA components, list of PCA-transformed data, 2D array
        of coordinates, GMM labels and frame numbers).  ``n_components_pca``: an int, or one int per GMM class."""
        averages, members, table = self.gmm(n_components_gmm, covariance_type, random_state, plot_results)
        if isinstance(n_components_pca, (int, np.integer)):
            n_components_pca = [int(n_components_pca)] * len(members)
        axes_all, scores_all = [], []
        for k, (imgs, n) in enumerate(zip(members, n_components_pca)):
            axes, scores, _ = self._pca_of(imgs, n)
            axes_all.append(axes.reshape(self._window_shape(n)))
            scores_all.append(scores)
            if plot_results:
                _show_images(axes_all[-1], [f"axis {i + 1}" for i in range(n)], f"PCA of GMM class {k + 1}")
        return averages, axes_all, scores_all, table

    def pca_scree_plot(self, plot_results: bool = True) -> np.ndarray:
        """PCA 'scree plot': explained variance ratio of all min(n_samples, n_features) components."""
        ratios = self._pca_of(self.imgstack, None, ratios_only=True)[2]
        if plot_results:
            _show_scree(ratios, "whole stack")
        return ratios

    def pca_gmm_scree_plot(self, n_components_gmm: int, covariance_type: str = 'diag', random_state: int = 1,
                           plot_results: bool = True) -> List[np.ndarray]:
        """PCA scree plot of every GMM class."""
        members = self.gmm(n_components_gmm, covariance_type, random_state, plot_results)[1]
        ratios_all = [self._pca_of(imgs, None, ratios_only=True)[2] for imgs in members]
        if plot_results:
            for k, ratios in enumerate(ratios_all):
                _show_scree(ratios, f"GMM class {k + 1}")
        return ratios_all

    def imblock_pca(self, n_components: int, random_state: int = 1, plot_results: bool = False,
                    **kwargs: int) -> Tuple[np.ndarray]:
        """PCA eigenvectors and their loading maps, for finding domains in a single image: (components, projections,
        coordinates of every sub-image).  ``marker_size`` sets the marker size of the loading maps."""
        axes, scores, table = self.pca(n_components, random_state)
        centres = table[:, :2]
        if plot_results:
            if len(self.network_output) != 1:
                raise ValueError("loading maps need a single mother image: network_output must be (1, h, w, c), got "
                                 f"{tuple(self.network_output.shape)}")
            self.plot_decomposition_results(axes, scores, self.network_output.shape[1:3], centres,
                                            **{k: v for k, v in kwargs.items() if k == "marker_size" and v is not None})
        return axes, scores, centres

    # ------------------------------------------------------------------------------------------------ not offered
    def ica(self, *args, **kwargs):
        raise NotImplementedError(_ICA_ELSEWHERE.format("imlocal.ica", "atomai_amd.stat.ica.imlocal_ica(stack, ...)"))

    def nmf(self, *args, **kwargs):
        raise NotImplementedError(_NMF_ELSEWHERE.format("imlocal.nmf", "atomai_amd.stat.nmf.imlocal_nmf(stack, ...)"))

    def imblock_ica(self, *args, **kwargs):
        raise NotImplementedError(_ICA_ELSEWHERE.format("imlocal.imblock_ica",
                                                        "atomai_amd.stat.ica.imblock_ica(stack, ...)"))

    def imblock_nmf(self, *args, **kwargs):
        raise NotImplementedError(_NMF_ELSEWHERE.format("imlocal.imblock_nmf",
                                                        "atomai_amd.stat.nmf.imblock_nmf(stack, ...)"))

    # ------------------------------------------------------------------------------------------------ plots
    @classmethod
    def plot_decomposition_results(cls, components: np.ndarray, X_vec_t: np.ndarray, image_hw: Tuple = None,
                                   xy_centers: np.ndarray = None, plot_loading_maps: bool = True,
                                   **kwargs: int) -> None:
        """One column per component: the component as an image (for several channels: the sum of all but the last, the
        background) and, with ``plot_loading_maps``, below it the projections ``X_vec_t[:, i]`` drawn at the window
        centres ``xy_centers`` (row, col) of a mother image of ``image_hw`` pixels.  ``marker_size``: default 32."""
        plt = _pyplot()
        n = len(components)
        shown = components[..., :-1] if components.shape[-1] > 1 else components
        nrows = 2 if plot_loading_maps else 1
        fig, axes = plt.subplots(nrows, n, figsize=(3 * n, 3.3 * nrows), squeeze=False)
        for i in range(n):
            axes[0, i].imshow(shown[i].sum(-1), cmap="seismic", interpolation="gaussian")
            axes[0, i].set_title(f"component {i + 1}", fontsize=10)
            axes[0, i].set_axis_off()
        if plot_loading_maps:
            if image_hw is None or xy_centers is None:
                raise ValueError("loading maps need image_hw and xy_centers")
            rows, cols = np.asarray(xy_centers)[:, 0], np.asarray(xy_centers)[:, 1]
            for i in range(n):
                ax = axes[1, i]
                ax.scatter(cols, rows, c=X_vec_t[:, i], s=kwargs.get("marker_size", 32), marker="s", cmap="seismic")
                ax.set(xlim=(0, image_hw[1]), ylim=(image_hw[0], 0), aspect="equal")
                ax.set_title(f"loading map {i + 1}", fontsize=10)
                ax.set_axis_off()
        fig.tight_layout()
        plt.show()

    # ------------------------------------------------------------------------------------------------ trajectories
    @classmethod
    def get_trajectory(cls, coord_class_dict: Dict[int, np.ndarray], start_coord: np.ndarray,
                       rmax: int) -> Tuple[np.ndarray]:
        """Trajectory of a single defect / atom through the frames: in every frame the nearest neighbour (brute force)
        of the previous position, if it lies within ``rmax``.  Returns (coordinates of the trajectory, its frames)."""
        flow = np.empty((0, 3))
        frames = []
        c0 = np.asarray(start_coord, dtype=np.float64)
        for k, c in coord_class_dict.items():
            if len(c) == 0:
                continue
            diff = np.asarray(c[:, :2], dtype=np.float64) - c0
            d2 = np.einsum("ij,ij->i", diff, diff)
            index = int(np.argmin(d2))                               # first of equally near points
            if np.sqrt(d2[index]) < rmax:
                flow = np.append(flow, [c[index]], axis=0)
                frames.append(k)
                c0 = np.asarray(c[index][:2], dtype=np.float64)
        return flow, np.array(frames)

    def get_all_trajectories(self, min_length: int = 0, run_gmm: bool = False, rmax: int = 10,
                             **kwargs: Union[int, str]) -> Dict:
        """One trajectory per sub-image of the first frame that has any, each followed through the later frames by
        ``get_trajectory``; trajectories of ``min_length`` points or fewer are dropped.  The third column of a trajectory
        is the GMM class (``run_gmm`` with ``n_components`` = 5, ``covariance`` = 'diag', ``random_state`` = 1 unless
        given) or 0.  Returns {"trajectories": [...], "frames": [...]} plus "gmm_components" when ``run_gmm``."""
        result = {}
        labels = np.zeros(self.d0)
        if run_gmm:
            averages, _, table = self.gmm(kwargs.get("n_components", 5), kwargs.get("covariance", "diag"),
                                          kwargs.get("random_state", 1))
            labels = table[:, 2]
        per_frame = {}
        for f in np.unique(self.imgstack_frames):                    # (the stack is ordered by frame)
            here = self.imgstack_frames == f
            per_frame[f] = np.column_stack((self.imgstack_com[here], labels[here]))
        first = next(iter(per_frame.values()))
        tracks = [self.get_trajectory(per_frame, start, rmax) for start in first[:, :2]]
        tracks = [(points, frames) for points, frames in tracks if len(points) > min_length]
        result["trajectories"] = [points for points, _ in tracks]
        result["frames"] = [frames for _, frames in tracks]
        if run_gmm:
            result["gmm_components"] = averages
        return result

    @classmethod
    def renumerate_classes(cls, classes: np.ndarray) -> np.ndarray:
        """Replaces every class by its rank among the classes that occur (0 for the smallest), as int64."""
        return np.unique(np.asarray(classes), return_inverse=True)[1].reshape(-1).astype(np.int64)

    def transition_matrix(self, n_components: int, covariance: str = 'diag', random_state: int = 1, rmax: int = 10,
                          min_length: int = 0, sum_all_transitions: bool = False) -> Dict:
        """GMM classes, trajectories from the first frame, and the Markov transition matrix of every trajectory over
        the classes it visits: {"trajectories", "frames", "gmm_components", "transitions"} and, with
        ``sum_all_transitions``, "all_transitions" (``sum_transitions`` over ``n_components`` classes)."""
        result = self.get_all_trajectories(min_length, run_gmm=True, rmax=rmax, n_components=n_components,
                                           covariance=covariance, random_state=random_state)
        result["transitions"] = [calculate_transition_matrix(self.renumerate_classes(points[:, -1]))
                                 for points in result["trajectories"]]
        if sum_all_transitions:
            result["all_transitions"] = sum_transitions(result, n_components)
        return result


def calculate_transition_matrix(trace: Union[List, np.ndarray]) -> np.ndarray:
    """Markov transition matrix of a sequence of states 0 .. n-1: entry (i, j) is the share of the steps out of state i
    that lead to state j; the row of a state that is never left stays zero."""
    trace = np.asarray(trace).astype(np.int64).reshape(-1)
    n = int(trace.max()) + 1
    counts = np.zeros((n, n))
    np.add.at(counts, (trace[:-1], trace[1:]), 1.0)
    left = counts.sum(axis=1, keepdims=True)
    return np.divide(counts, left, out=counts, where=left > 0)


def sum_transitions(trans_dict: Dict, msize: int, plot_results: bool = False, **kwargs: int) -> np.ndarray:
    """Adds the transition matrices of the individual trajectories (``trans_dict["transitions"]``, each over the
    1-based classes its trajectory in ``trans_dict["trajectories"]`` visits) into one (msize, msize) matrix and
    normalises its rows."""
    if plot_results:
        raise NotImplementedError("sum_transitions(plot_results=True) is not implemented: plot the returned matrix")
    total = np.zeros((msize, msize))
    for points, matrix in zip(trans_dict["trajectories"], trans_dict["transitions"]):
        visited = np.unique(points[:, -1]).astype(np.int64) - 1
        total[np.ix_(visited, visited)] += matrix
    return total / total.sum(axis=1, keepdims=True)


def _as_frames(images: np.ndarray) -> np.ndarray:
    """(h, w), (n, h, w) or (h, w, c) with c < 10, or (n, h, w, c)  ->  (n, h, w, c)."""
    images = np.asarray(images)
    if images.ndim == 2:
        return images[None, :, :, None]
    if images.ndim == 3:
        return images[None] if images.shape[-1] < 10 else images[..., None]    # a last axis under 10 is channels
    return images


def update_classes(coordinates: Union[Dict[int, np.ndarray], np.ndarray], nn_input: np.ndarray,
                   method: str = 'threshold', **kwargs: float) -> Dict[int, np.ndarray]:
    """New classes for the located atoms.  ``method='gmm_local'``: from a GMM of the image patches around them, with
    ``n_components``, ``window_size`` and optionally ``coord_class`` (default 0: only atoms of that class are kept and
    re-classified, 0-based; atoms whose window leaves the image are dropped).  ``method='threshold'`` (``thresh``,
    the reference's default) and ``method='meanshift'`` (``quantile``): from the mean intensity in the window of side
    ``window_size`` (default 3) around every atom, through ``stat.intensity.update_classes`` (csrc/intensity.hip).
    ``coordinates``: the Locator's dictionary, or one frame's table together with that frame as ``nn_input``.  Returns a
    new dictionary.  ``method='kmeans'`` still raises here; it runs as
    ``atomai_amd.stat.intensity.update_classes(..., method='kmeans')``."""
    if method == "kmeans":
        raise NotImplementedError("update_classes(method='kmeans') still raises here; the working code is "
                                  "atomai_amd.stat.intensity.update_classes(..., method='kmeans'): k-means of the "
                                  "intensities runs on the device (csrc/intensity.hip).")
    if method != "gmm_local":
        from . import intensity
        return intensity.update_classes(coordinates, nn_input, method, **kwargs)
    n_components, window_size = kwargs.get("n_components"), kwargs.get("window_size")
    if n_components is None or window_size is None:
        raise AttributeError("method='gmm_local' needs n_components and window_size")
    tables = {0: coordinates} if isinstance(coordinates, np.ndarray) else coordinates
    stack = imlocal(_as_frames(nn_input), copy.deepcopy(tables), window_size, kwargs.get("coord_class", 0))
    table = stack.gmm(n_components, plot_results=kwargs.get("plot_results", False))[2]
    updated = {}
    for key in tables:
        rows = table[table[:, 3] == float(key), :3].copy()
        rows[:, 2] -= 1
        updated[key] = rows
    return updated


class SlidingFFTNMF:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(_NMF_ELSEWHERE.format("atomai_amd.stat.SlidingFFTNMF",
                                                        "atomai_amd.stat.fft_nmf.SlidingFFTNMF"))


class SpectralUnmixer:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(_NMF_ELSEWHERE.format("atomai_amd.stat.SpectralUnmixer",
                                                        "atomai_amd.stat.unmixer.SpectralUnmixer (method='nmf')"))

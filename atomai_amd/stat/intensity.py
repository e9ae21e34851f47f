"""Intensity-based classes of located atoms on the device (csrc/intensity.hip): the reference's ``update_classes``
(atomai/stat/multivar.py:816-916) with ``method`` 'threshold', 'kmeans' and 'meanshift', and the one-dimensional
clustering behind it.  ``aoi.stat.update_classes`` runs 'threshold', 'meanshift' and 'gmm_local' and still raises for
'kmeans'; this module runs all four:

    >>> coordinates = aoi.stat.intensity.update_classes(coordinates, nn_input, method='kmeans', n_components=2)
    >>> fit = aoi.stat.intensity.mean_shift(intensities, quantile=.25)          # centres, labels, n_iter, bandwidth

The arithmetic is fp64 on the values given: a float32 column gives what scikit-learn gives on its float64 copy.  In one
dimension the neighbours of a value are a contiguous range of the sorted column, so ``estimate_bandwidth`` is a sort and
one binary search per row, not the k-neighbours query with k = n / 4 that scikit-learn runs for every row.

Departures from scikit-learn.  ``kmeans`` is seeded by this package's greedy k-means++ (as ``imlocal.gmm`` is), so the
NUMBERING of its clusters is this package's, not scikit-learn's; a cluster that a Lloyd round leaves empty keeps its
centre, where scikit-learn moves it to the row farthest from its centre.  ``mean_shift`` has no ``cluster_all=False`` and
``estimate_bandwidth`` no ``n_samples``.
"""
import copy
import warnings
from typing import Dict, Union

import numpy as np
import torch

from ..utils import get_intensities
from . import _gmm
from . import _intensity as _I
from . import multivar

_METHODS = "Choose between 'threshold', 'kmeans', 'meanshift' and 'gmm_local' methods"


def _finite_column(x, what):
    x = _I.column(x)
    if x.shape[0] < 1:
        raise ValueError(f"{what} needs at least one intensity")
    bad = torch.nonzero(~torch.isfinite(x))
    if len(bad):
        raise ValueError(f"{what} needs finite intensities: row {int(bad[0])} is {float(x[int(bad[0])])}")
    return x


def _bandwidth(xs, quantile):
    if not 0.0 < float(quantile) <= 1.0:
        raise ValueError(f"quantile must be in (0, 1], got {quantile}")
    K = max(int(xs.shape[0] * quantile), 1)
    return float(_I.kth_gap(xs, K)[1])                       # the one read-back


def estimate_bandwidth(x, quantile: float = 0.25) -> float:
    """``sklearn.cluster.estimate_bandwidth(x[:, None], quantile=quantile)`` of a column of intensities: the mean
    distance of a value to its K-th nearest value (itself included), K = max(int(n * quantile), 1).  A device sort, one
    launch and one scalar read back."""
    return _bandwidth(torch.sort(_finite_column(x, "estimate_bandwidth"))[0], quantile)


def _unique_centres(centre, count, bw):
    """scikit-learn's post-processing on the host (the list is short): centres of seeds that found members (of seeds that
    end on the identical centre the last one's count is kept, as scikit-learn's dictionary does), by (count, centre)
    descending; going down, a centre still kept removes every later one within bw of it."""
    found = {}
    for c, m in zip(centre.tolist(), count.tolist()):
        if m > 0:
            found[c] = m                                       # (seeds in scikit-learn's order: a later one overwrites)
    if not found:
        raise ValueError(f"No point was within bandwidth={bw:f} of any seed. Try a different seeding strategy or "
                         "increase the bandwidth.")
    c = np.array([v for v, _ in sorted(found.items(), key=lambda t: (t[1], t[0]), reverse=True)])
    keep = np.ones(len(c), dtype=bool)
    for i in range(len(c)):
        if keep[i]:
            keep[np.abs(c - c[i]) <= bw] = False
            keep[i] = True
    return c[keep]


def mean_shift(x, bandwidth: float = None, quantile: float = 0.25, max_iter: int = 300) -> dict:
    """``sklearn.cluster.MeanShift(bandwidth, bin_seeding=True, max_iter=max_iter).fit(x[:, None])`` of a column of
    intensities, with ``bandwidth = estimate_bandwidth(x, quantile)`` when none is given.  Returns a dict: ``centres``
    (C,) float64 and ``labels`` (n,) int64 on the device, ``n_iter`` (the most iterations any seed ran) and
    ``bandwidth``.  Seeds are the occupied bins of width ``bandwidth``; every seed is one workgroup of one launch."""
    x = _finite_column(x, "mean_shift")
    xs = torch.sort(x)[0]
    bw = _bandwidth(xs, quantile) if bandwidth is None else float(bandwidth)
    if bw == 0.0:
        raise ValueError("the bandwidth is 0: at least a `quantile` share of the intensities are identical, so the "
                         "distance to the K-th nearest value is 0 for every row; pass a bandwidth or a larger quantile")
    if not 0.0 < bw < float("inf"):
        raise ValueError(f"bandwidth must be positive and finite, got {bw}")
    if int(max_iter) < 0:
        raise ValueError(f"max_iter must not be negative, got {max_iter}")
    binned, row = torch.sort(torch.round(x / bw), stable=True)          # (round half to even, as numpy.round)
    bins, rows = torch.unique_consecutive(binned, return_counts=True)
    if bins.shape[0] == x.shape[0]:
        warnings.warn(f"Binning data failed with provided bin_size={bw:f}, using data points as seeds.", UserWarning)
        seeds = x
    else:                                                     # scikit-learn's order: by the first row of every bin
        first = row[torch.cumsum(rows, 0) - rows]            # (the sort is stable: a bin's first entry is its first row)
        seeds = (bins[torch.argsort(first)].to(torch.float32).to(torch.float64) * bw).contiguous()
    centre, count, iters = _I.meanshift(xs, seeds, bw, max_iter)
    centres = torch.from_numpy(_unique_centres(centre.cpu(), count.cpu(), bw)).to(x.device)
    return {"centres": centres, "labels": _I.assign(x, centres), "n_iter": int(iters.max()), "bandwidth": bw}


def kmeans(x, n_components: int, random_state: int = 42, tol: float = 1e-4, max_iter: int = 300) -> dict:
    """k-means of a column of intensities: Lloyd's algorithm in fp64 in one launch, with scikit-learn's stopping rules
    (``tol`` scaled by the variance of the column).  Returns a dict: ``centres`` (k,) float64 and ``labels`` (n,) int64
    (the nearest final centre) on the device, and ``n_iter``.

    The starting centres come from this package's greedy k-means++ on the float32 copy of the column with
    ``numpy.random.default_rng(random_state)``: the partition agrees with ``sklearn.cluster.KMeans`` wherever the
    optimum is unambiguous, but the cluster NUMBERING follows this package's seeding, not scikit-learn's (as for
    ``imlocal.gmm``).  At most 32 clusters.  A cluster left empty keeps its centre; scikit-learn relocates it."""
    x = _finite_column(x, "kmeans")
    k = int(n_components)
    _gmm._check_k(k)
    if x.shape[0] < k:
        raise ValueError(f"n_samples={x.shape[0]} should be >= n_clusters={k}.")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")
    start = _gmm._seed(x.to(torch.float32)[:, None].contiguous(), k, np.random.default_rng(random_state))
    scaled = float(x.var(unbiased=False)) * float(tol)
    centres, n_iter = _I.lloyd(torch.sort(x)[0], start.view(k).to(torch.float64).contiguous(), scaled, max_iter)
    return {"centres": centres, "labels": _I.assign(x, centres), "n_iter": int(n_iter)}


def _histogram(values, thresh):
    """The distribution of the window intensities with the threshold marked on it."""
    plt = multivar._pyplot()
    finite = values[np.isfinite(values)]
    fig, ax = plt.subplots(figsize=(6, 4))
    ax.hist(finite, bins=min(50, max(10, int(np.sqrt(max(len(finite), 1))))), color="0.6")
    ax.axvline(thresh, linestyle="--", color="tab:red", label=f"thresh = {thresh:g}")
    ax.set_xlabel("mean window intensity")
    ax.set_ylabel("atoms")
    ax.legend(loc="best")
    fig.tight_layout()
    plt.show()


def update_classes(coordinates: Union[Dict[int, np.ndarray], np.ndarray], nn_input: np.ndarray,
                   method: str = 'threshold', **kwargs: float) -> Dict[int, np.ndarray]:
    """New classes for the located atoms from the mean image intensity around each of them (``utils.get_intensities``,
    window side ``window_size``, default 3), or from a GMM of the image patches ('gmm_local').

    Args:
        coordinates: the Locator's dictionary, or one frame's table together with that frame as ``nn_input``
        nn_input: the image(s) the network saw: (h, w), (n, h, w) or (n, h, w, 1)
        method: 'threshold' (``thresh``: class 1.0 where intensity >= thresh, else 0.0; ``plot_results=True`` draws the
            histogram with the threshold), 'kmeans' (``n_components``), 'meanshift' (``quantile``, default .25) or
            'gmm_local' (``n_components``, ``window_size``, ``coord_class``: ``aoi.stat.update_classes``)

    Returns a deep copy of the dictionary with the last column of every table overwritten.  'kmeans' and 'meanshift' fit
    the intensities of all frames together.  An atom whose window starts above or left of the image has intensity NaN:
    'threshold' leaves NaN as its class, as the reference does; 'kmeans' and 'meanshift' raise ValueError, as
    scikit-learn's input validation does.  (The reference tests ``>= thresh`` after zeroing the values below it, so for
    ``thresh <= 0`` it returns class 1 everywhere; here the test is made on the intensities.)"""
    if method == "gmm_local":
        return multivar.update_classes(coordinates, nn_input, method, **kwargs)
    if method not in ("threshold", "kmeans", "meanshift"):
        raise NotImplementedError(_METHODS)
    tables = copy.deepcopy({0: coordinates} if isinstance(coordinates, np.ndarray) else coordinates)
    keys = list(tables.keys())
    r = kwargs.get("window_size", 3)
    intensities = get_intensities(tables, multivar._as_frames(nn_input), r)
    every = np.concatenate(intensities) if intensities else np.empty(0)
    if method == "threshold":
        thresh = kwargs.get("thresh")
        if thresh is None:
            raise AttributeError("Specify intensity threshold value ('thresh'), e.g. thresh=.5")
        classes = np.where(np.isnan(every), np.nan, (every >= thresh).astype(np.float64))
        if kwargs.get("plot_results", False):
            _histogram(every, thresh)
    else:
        if method == "kmeans" and kwargs.get("n_components") is None:
            raise AttributeError("Specify number of components ('n_components')")
        for key, values in zip(keys, intensities):
            bad = np.nonzero(np.isnan(values))[0]
            if len(bad):
                raise ValueError(f"the intensity of atom {int(bad[0])} of frame {key} is NaN (its window of side {r} "
                                 f"starts outside the image): method='{method}' needs finite intensities")
        if method == "kmeans":
            fit = kmeans(every, kwargs["n_components"], random_state=42)
        else:
            fit = mean_shift(every, quantile=kwargs.get("quantile", .25))
        classes = fit["labels"].cpu().numpy()
    start = 0
    for key, values in zip(keys, intensities):
        tables[key][:, -1] = classes[start:start + len(values)]
        start += len(values)
    return tables

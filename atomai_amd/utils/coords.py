"""Coordinate grids for the rVAE spatial decoder (reference: atomai/utils/coords.py:37-83), the Gaussian peak
refinement of atom positions (coords.py:152-231) and the nearest-neighbour analysis of atom tables (coords.py:86-149,
234-301, 350-400, 475-537) on the kernels of csrc/knn.hip."""
import warnings
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch


def grid2xy(X1: torch.Tensor, X2: torch.Tensor) -> torch.Tensor:
    """(M, N) grids -> (M*N, 2) xy pairs."""
    return torch.stack((X1.reshape(-1), X2.reshape(-1)), 1)


def imcoordgrid(im_dim: Tuple) -> torch.Tensor:
    """x in linspace(-1, 1, H) along rows, y in linspace(1, -1, W) along columns, 'ij' meshgrid."""
    xx = torch.linspace(-1, 1, im_dim[0])
    yy = torch.linspace(1, -1, im_dim[1])
    x0, x1 = torch.meshgrid(xx, yy, indexing="ij")
    return grid2xy(x0, x1)


def transform_coordinates(coord: Union[np.ndarray, torch.Tensor], phi: torch.Tensor,
                          coord_dx: Union[np.ndarray, torch.Tensor, int] = 0) -> torch.Tensor:
    """Batched rotation by phi (coord @ [[cos, sin], [-sin, cos]]) followed by translation.  B x n x 2
    elementwise math (17 MB at bs 512, 64x64): torch ops, differentiable."""
    if isinstance(coord, np.ndarray):
        coord = torch.from_numpy(coord).float()
    if isinstance(coord_dx, np.ndarray):
        coord_dx = torch.from_numpy(coord_dx).float()
    c, s = torch.cos(phi)[:, None], torch.sin(phi)[:, None]
    x, y = coord[..., 0], coord[..., 1]
    return torch.stack((x * c - y * s, x * s + y * c), -1) + coord_dx


def gaussian_2d(xy: Tuple[np.ndarray], amp: float, xo: float, yo: float, sigma_x: float, sigma_y: float,
                theta: float, offset: float) -> np.ndarray:
    """``offset + amp * exp(-q)`` on the grids ``xy = (x, y)``, raveled, with the quadratic form
    ``q = qa dx^2 + 2 qb dx dy + qc dy^2`` of a Gaussian of widths ``sigma_x``, ``sigma_y`` rotated by ``theta``
    about ``(xo, yo)`` — the model ``amx_peak_refine`` fits (``ref_quad`` in csrc/refine.hip), for callers that want
    to evaluate it on the host (reference signature: coords.py:152-154)."""
    dx, dy = np.asarray(xy[0]) - xo, np.asarray(xy[1]) - yo
    ct, st = np.cos(theta), np.sin(theta)
    hx, hy = 0.5 / sigma_x ** 2, 0.5 / sigma_y ** 2            # half inverse variances
    qa = ct * ct * hx + st * st * hy
    qb = 0.5 * np.sin(2 * theta) * (hy - hx)
    qc = st * st * hx + ct * ct * hy
    return np.ravel(offset + amp * np.exp(-(qa * dx * dx + 2 * qb * dx * dy + qc * dy * dy)))


def peak_refinement(imgdata: np.ndarray, coordinates: np.ndarray, d: Optional[int] = None) -> np.ndarray:
    """Refines atomic positions by fitting a 2-D Gaussian to the 2d x 2d patch around each of them
    (coords.py:179-231), all atoms of the frame in one launch of ``amx_peak_refine``.

    ``imgdata`` is a single 2-D frame; it is converted to float32 on the way to the device (the fit itself runs in
    float64).  ``coordinates`` is an (N, >=3) table [row, col, class, ...]; the result is (N, 3) float64.  Without
    ``d`` the half-side is a quarter of the mean nearest-neighbour distance, with the reference's warning; that needs
    at least 3 atoms.  ``d`` outside 2 .. 32 raises ValueError.  An empty table is returned as an empty (0, 3) table
    (the reference crashes there)."""
    from .. import _lib as L
    from ..predictors.locator import check_d, refine_device, warn_default_d
    imgdata, coordinates = np.asarray(imgdata), np.asarray(coordinates)
    if imgdata.ndim != 2:
        raise ValueError("peak_refinement takes a single 2D frame")
    if coordinates.ndim != 2 or coordinates.shape[1] < 3:
        raise ValueError("expected an (N, >=3) table of coordinates")
    check_d(d)
    warn_default_d(d)
    n = len(coordinates)
    cls = coordinates[:, 2:3].astype(np.float64)
    if n == 0:
        return np.empty((0, 3), dtype=np.float64)
    device = "cuda" if torch.cuda.is_available() and not L.is_test_backend() else "cpu"
    frames = torch.from_numpy(np.ascontiguousarray(imgdata[None], dtype=np.float32)).to(device)
    xy = torch.from_numpy(np.ascontiguousarray(coordinates[:, :2], dtype=np.float64)).to(device)
    meta = torch.zeros((n, 2), dtype=torch.int32, device=device)
    out = refine_device(frames, xy, meta, d)
    return np.concatenate((out.cpu().numpy(), cls), axis=-1)


# ------------------------------------------------------------------------------------------ nearest-neighbour analysis
def _device():
    from .. import _lib as L
    return "cuda" if torch.cuda.is_available() and not L.is_test_backend() else "cpu"


def _to_device(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_device())


def _tables(coordinates) -> List[np.ndarray]:
    """The frames' tables in dictionary order; a single array is one frame."""
    if isinstance(coordinates, np.ndarray):
        coordinates = {0: coordinates}
    tables = [np.asarray(t) for t in coordinates.values()]
    for t in tables:
        if t.ndim != 2 or t.shape[1] < 2:
            raise ValueError("expected (N, >=2) tables of coordinates [row, col, class, ...]")
    return tables


def _nn_tables(tables: List[np.ndarray], nn: int, upper_bound: Optional[float]):
    """get_nn_distances_ for every table, all of them through ONE launch of ``amx_knn``: the tables are concatenated
    into one flat table and every frame is a segment."""
    from . import _knn
    k = int(nn) + 1
    if int(nn) != nn or not 2 <= k <= _knn.K_MAX:
        raise ValueError(f"nn + 1 = {nn + 1} neighbours per atom (the atom itself is one) must lie between 2 and "
                         f"{_knn.K_MAX}, the limit of the device kernel")
    bound = np.inf if upper_bound is None else float(upper_bound)
    offs = np.concatenate(([0], np.cumsum([len(t) for t in tables]))).astype(np.int64)
    if offs[-1] > 0:
        flat = _to_device(np.concatenate([t[:, :2] for t in tables], axis=0))
        dist, idx = (a.cpu().numpy() for a in _knn.knn(flat, flat, k, bound, offs, offs))
    else:
        dist, idx = np.empty((0, k)), np.empty((0, k), dtype=np.int64)
    distances, pairs = [], []
    for t, lo, hi in zip(tables, offs[:-1], offs[1:]):
        d, ix = dist[lo:hi], idx[lo:hi] - lo
        keep = ~np.isinf(d).any(axis=1)                 # a row with any missing neighbour is dropped
        distances.append(d[keep, 1:])
        pairs.append(t[ix[keep]])
    return distances, pairs


def get_nn_distances_(coordinates: np.ndarray, nn: int = 2,
                      upper_bound: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Distances of every atom of one frame to its ``nn`` nearest neighbours (coords.py:86-113): an (atoms' x nn) array
    of distances and the (atoms' x (nn+1) x columns) coordinates of the atom and its neighbours.  ``upper_bound`` is
    cKDTree's ``distance_upper_bound`` (only ``distance < upper_bound`` counts); atoms with fewer than ``nn`` such
    neighbours are dropped, so a table with fewer than ``nn + 1`` atoms gives empty arrays.  ``nn + 1 <= 32``."""
    d, p = _nn_tables(_tables(np.asarray(coordinates)), nn, upper_bound)
    return d[0], p[0]


def get_nn_distances(coordinates: Union[Dict[int, np.ndarray], np.ndarray], nn: int = 2,
                     upper_bound: Optional[float] = None) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """``get_nn_distances_`` for a dictionary of frames (coords.py:116-149), all frames in one launch.  Returns the two
    lists in dictionary order."""
    return _nn_tables(_tables(coordinates), nn, upper_bound)


def _pyplot():
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise ImportError("plot_results=True needs matplotlib, which does not import here; "
                          "call with plot_results=False") from e
    return plt


def _plot_bonds(distances, pairs, distance_ideal, frame, **kwargs):
    """One figure per frame: every atom-neighbour bond as a line coloured by its deviation from ``distance_ideal``."""
    from matplotlib.collections import LineCollection
    plt = _pyplot()
    fig, ax = plt.subplots(figsize=(8, 8))
    if len(distances):
        centre = np.repeat(pairs[:, :1, :2], pairs.shape[1] - 1, axis=1)
        seg = np.stack((centre, pairs[:, 1:, :2]), axis=2).reshape(-1, 2, 2)[..., ::-1]      # (x, y) = (col, row)
        lines = LineCollection(seg, cmap="bwr", linewidths=1.5)
        lines.set_array(distances.reshape(-1) - distance_ideal)
        ax.add_collection(lines)
        fig.colorbar(lines, ax=ax, label="bond length - ideal (px)")
        ax.scatter(pairs[:, 0, 1], pairs[:, 0, 0], s=4, c="k")
    if kwargs.get("h") is not None and kwargs.get("w") is not None:
        ax.set_xlim(0, kwargs["w"])
        ax.set_ylim(kwargs["h"], 0)
    else:
        ax.autoscale()
        ax.invert_yaxis()
    ax.set_aspect("equal")
    ax.set_title(f"frame {frame}")
    if kwargs.get("savedir") is not None:
        import os
        fig.savefig(os.path.join(kwargs["savedir"], f"frame_{frame}.png"))
    plt.show()


def map_bonds(coordinates: Dict[int, np.ndarray], nn: int = 2, upper_bound: Optional[float] = None,
              distance_ideal: Optional[float] = None, plot_results: bool = True, **kwargs) -> np.ndarray:
    """Nearest-neighbour bond lengths of every frame (coords.py:475-515), concatenated; with ``plot_results`` one bond
    map per frame, coloured by the deviation from ``distance_ideal`` (default: the mean).  Keywords ``h``, ``w`` (frame
    size) and ``savedir``."""
    distances, pairs = get_nn_distances(coordinates, nn, upper_bound)
    out = np.concatenate(distances)
    if plot_results:
        if distance_ideal is None:
            distance_ideal = np.mean(out)
        for i, (d, p) in enumerate(zip(distances, pairs)):
            _plot_bonds(d, p, distance_ideal, i, **kwargs)
    return out


def compare_coordinates(coordinates1: np.ndarray, coordinates2: np.ndarray, d_max: float, plot_results: bool = False,
                        **kwargs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Matches every row of ``coordinates1`` (predicted) to its nearest row of ``coordinates2`` (true) and keeps the
    pairs with ``distance < d_max`` (coords.py:266-301).  As in the reference the distance is taken over ALL columns
    of the tables (the class column takes part), so both need the same 2 or 3 columns.  Returns the matched rows of
    both tables and their distances.  For plotting pass the image as ``expdata`` (and ``fsize``)."""
    from . import _knn
    c1, c2 = np.asarray(coordinates1, dtype=np.float64), np.asarray(coordinates2, dtype=np.float64)
    if c1.ndim != 2 or c2.ndim != 2 or c1.shape[1] != c2.shape[1]:
        raise ValueError("expected two (N, dim) tables with the same number of columns")
    if c2.shape[1] not in _knn.DIMS:
        raise ValueError(f"the device neighbour search handles dim 2 or 3, got {c2.shape[1]} columns")
    if len(c1) and len(c2):
        dist, idx = (a.cpu().numpy()[:, 0] for a in _knn.knn(_to_device(c2), _to_device(c1), 1))
    else:
        dist, idx = np.full(len(c1), np.inf), np.full(len(c1), -1, dtype=np.int64)
    keep = dist < d_max
    m1, m2, delta_r = c1[keep], c2[idx[keep]], dist[keep]
    if plot_results:
        expdata = kwargs.get("expdata")
        if expdata is None:
            raise AssertionError("For plotting, provide 2D image via 'expdata' keyword")
        plt = _pyplot()
        fsize = kwargs.get("fsize", 20)
        plt.figure(figsize=(int(fsize * 1.25), fsize))
        plt.imshow(expdata, cmap="gray")
        im = plt.scatter(m1[:, 1], m1[:, 0], c=delta_r, cmap="jet", s=5)
        plt.colorbar(im).set_label("Position deviation (px)")
        plt.show()
    return m1, m2, delta_r


def find_coord_clusters(coord_class_dict_1, coord_class_dict_2, rmax: float):
    """For every atom of ``coord_class_dict_1[0]`` collects the atoms of ALL frames of ``coord_class_dict_2`` (keys
    0 .. len - 1, or a list) whose (row, col) lies within ``distance < rmax`` (coords.py:350-400).  Returns the
    clusters' means and standard deviations over (row, col), (n, 2) each, and the list of clusters, every one a table
    ordered by distance.  An atom without a neighbour gives an empty cluster and NaN."""
    from . import _knn
    frames = [np.asarray(coord_class_dict_2[k], dtype=np.float64) for k in range(len(coord_class_dict_2))]
    every = np.concatenate(frames, axis=0) if frames else np.empty((0, 3))
    c0 = np.asarray(coord_class_dict_1[0], dtype=np.float64)[:, :2]
    if len(c0):
        count, idx, _ = (a.cpu().numpy() for a in _knn.radius(_to_device(every[:, :2]), _to_device(c0), float(rmax)))
    else:
        count, idx = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    clusters = [every[ix] for ix in np.split(idx, np.cumsum(count)[:-1])] if len(c0) else []
    nan = np.full(2, np.nan)
    means = [c[:, :2].mean(axis=0) if len(c) else nan for c in clusters]
    stds = [c[:, :2].std(axis=0) if len(c) else nan for c in clusters]
    return np.array(means).reshape(-1, 2), np.array(stds).reshape(-1, 2), clusters


def _cluster_segments(tables: List[np.ndarray], eps: float, min_samples: int, members: bool = True):
    """DBSCAN of every table of ``tables`` on its own, all of them through ONE segmented pass of csrc/cluster.hip.
    Returns one (clusters, mean, var) per table as ``cluster_coord`` does; ``clusters`` is None unless ``members``."""
    from . import _cluster
    tables = [np.asarray(t, dtype=np.float64) for t in tables]
    for t in tables:
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("expected (N, 3) tables of coordinates [row, col, class]")
    sizes = np.array([len(t) for t in tables], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    flat = np.concatenate(tables, axis=0) if len(tables) else np.empty((0, 3))
    pts = _to_device(flat[:, :2])
    r = _cluster._run(pts, eps, min_samples, offs)
    kseg, count, mean, var, rows, moff = _cluster.cluster_stats(pts, r["labels"], r["rank"], r["seg"])
    count, mean, var = count.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
    if members:
        rows, moff = rows.cpu().numpy(), moff.cpu().numpy()
    placed = np.concatenate(([0], np.cumsum(count)))
    out = []
    for s in range(len(tables)):
        k0, k1 = int(kseg[s]), int(kseg[s + 1])
        # the reference takes np.unique(labels)[1:], which assumes the first label is DBSCAN's noise label -1: a table
        # without noise loses its cluster 0 instead (kept on purpose)
        if placed[k1] - placed[k0] == sizes[s]:
            k0 = min(k0 + 1, k1)
        clusters = [flat[rows[moff[k]:moff[k + 1]]] for k in range(k0, k1)] if members else None
        # (the reference's np.array of an empty list has shape (0,))
        none = np.array([])
        out.append((clusters, mean[k0:k1].copy() if k1 > k0 else none, var[k0:k1].copy() if k1 > k0 else none.copy()))
    return out


def cluster_coord(coord_class_dict: Union[Dict[int, np.ndarray], List[np.ndarray]], eps: float,
                  min_samples: int = 10) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Collapses the (N, 3) tables of a stack (keys 0 .. len - 1, or a list) onto the xy plane and clusters them with
    DBSCAN (coords.py:304-347; ``sklearn.cluster.DBSCAN(eps, min_samples)`` there, csrc/cluster.hip here, with the same
    labels).  Returns the member rows of every cluster (an object array of (m, 3) tables, rows in stack order), the
    clusters' means and their population variances over (row, col).  As in the reference the first of the sorted labels
    is skipped: the noise, or cluster 0 when there is no noise."""
    frames = [np.asarray(coord_class_dict[k], dtype=np.float64) for k in range(len(coord_class_dict))]
    every = np.concatenate(frames, axis=0) if frames else np.empty((0, 3))
    clusters, mean, var = _cluster_segments([every], eps, min_samples)[0]
    return np.array(clusters, dtype=object), mean, var


def cluster_coord_frames(stacks, eps: float, min_samples: int = 10) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """``cluster_coord`` for many stacks at once: ``stacks[i]`` is a dictionary or list of (N, 3) tables (the members'
    detections of frame i, say).  Every stack is one segment of a single pass.  Returns the list of the stacks' cluster
    means and the list of their variances."""
    every = []
    for st in stacks:
        frames = [np.asarray(st[k], dtype=np.float64) for k in range(len(st))]
        every.append(np.concatenate(frames, axis=0) if frames else np.empty((0, 3)))
    res = _cluster_segments(every, eps, min_samples, members=False)
    return [m for _, m, _ in res], [v for _, _, v in res]


def _frame2d(img) -> np.ndarray:
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[-1] == 1:
        img = img[..., 0]
    if img.ndim != 2:
        raise ValueError(f"expected a 2-D frame or (H, W, 1), got shape {img.shape}")
    return img


def _intensities(tables, frames, r):
    """Mean window intensity for every atom of every table, one launch of ``amx_window_mean`` for all of them."""
    from . import _knn
    if int(r) != r or int(r) < 1:
        raise ValueError(f"the window side r must be a positive integer, got {r}")
    tables = [np.asarray(t, dtype=np.float64) for t in tables]
    tables = [t if t.size else np.empty((0, 2)) for t in tables]
    if any(t.ndim != 2 or t.shape[1] < 2 for t in tables):
        raise ValueError("expected (N, >=2) tables of coordinates [row, col, ...]")
    frames = [_frame2d(f) for f in frames]
    counts = [len(t) for t in tables]
    if sum(counts) == 0:
        return [np.empty(0) for _ in tables]
    if len({f.shape for f in frames}) != 1:
        raise ValueError("all frames must have the same shape")
    meta = np.zeros((sum(counts), 2), dtype=np.int32)
    meta[:, 0] = np.repeat(np.arange(len(tables)), counts)
    xy = np.concatenate([t[:, :2] for t in tables], axis=0)
    out = _knn.window_mean(_to_device(np.stack(frames), np.float32), _to_device(xy), _to_device(meta, np.int32), int(r))
    return np.split(out.cpu().numpy(), np.cumsum(counts)[:-1])


def get_intensities_(coordinates: np.ndarray, img: np.ndarray, r: int = 3) -> np.ndarray:
    """Mean intensity of ``img`` (2-D, or (H, W, 1)) in the window of side ``r`` around every rounded atom position
    (coords.py:234-252), as float64 means of the float32 frame.  Odd ``r``: [c - r//2, c + r//2 + 1); even ``r``:
    [c - r//2, c + r//2).  numpy's slicing rules: a window cut by the high edge averages what is left, one that starts
    below 0 is an empty slice, NaN."""
    return _intensities([coordinates], [img], r)[0]


def get_intensities(coordinates_all: Dict[int, np.ndarray], nn_input, r: int = 3) -> List[np.ndarray]:
    """``get_intensities_`` for every frame of the dictionary (coords.py:255-263), frame ``k`` of ``nn_input`` for key
    ``k``, all atoms of all frames in one launch."""
    keys = list(coordinates_all.keys())
    return _intensities([coordinates_all[k] for k in keys], [nn_input[k] for k in keys], r)


def remove_edge_coord(coordinates: np.ndarray, dim: Tuple[int, int], dist_edge: int) -> np.ndarray:
    """Drops the rows closer than ``dist_edge`` to the frame's edges, with the reference's comparison as written
    (coords.py:518-537): column 0 against ``w`` and column 1 against ``h`` of ``dim = (h, w)``."""
    coordinates = np.asarray(coordinates)
    h, w = dim
    c0, c1 = coordinates[:, 0], coordinates[:, 1]
    edge = (c0 > w - dist_edge) | (c0 < dist_edge) | (c1 > h - dist_edge) | (c1 < dist_edge)
    return coordinates[~edge]

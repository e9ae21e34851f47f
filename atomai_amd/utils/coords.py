"""Coordinate grids for the rVAE spatial decoder (reference: atomai/utils/coords.py:37-83) and the Gaussian peak
refinement of atom positions (coords.py:152-231)."""
import warnings
from typing import Optional, Tuple, Union

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

"""Ground-truth masks for Segmentor training from labelled atom positions (reference: atomai/utils/imgen.py), rasterised
on the device (csrc/lattice.hip):

    >>> masks = aoi.utils.create_multiclass_lattice_mask(frames, coordinates)      # (n, h, w, classes + 1) float64
    >>> X, y = aoi.utils.extract_patches(frames, masks, patch_size=256, num_patches=128)

The reference makes one ``MakeAtom`` and one slice assignment per atom per frame on the host.  Here the stamp of every
distinct class is made ONCE on the host, all frames of a call become one flat atom table, and two launches (who owns a
pixel, then the values) write every mask.  The result equals the reference's bit for bit, overlaps included: the stamp
is a square that is assigned whole, zeros too, so where two stamps of a channel overlap the LATER row of the table wins.

Departures from the reference, all on inputs it handles badly:
  * a user-supplied ``create_mask_func`` is called once per distinct class value of the call, not once per atom: a
    function that returns something different on each call is not supported;
  * a stamp that leaves the frame on any side raises ``ValueError`` naming the frame and the row (the reference raises
    numpy's broadcast error, and silently wraps a stamp that lies wholly at negative indices);
  * ``create_multiclass_lattice_mask_`` does not add 1 to the caller's class column in place;
  * stamps are squares of odd side up to 63 (an even side fails in the reference as well).
"""
from typing import Callable, Dict, List, Tuple, Union

import numpy as np
import torch

from . import _lattice as _T


class MakeAtom:
    """Image of an atom as a rotated 2-D Gaussian on an ``sc`` x ``sc`` grid (an even ``sc`` is raised to the next odd
    number) and the matching circular mask of diameter ``r_mask``: g = offset + intensity * exp(-(a dx^2 + 2 b dx dy +
    c dy^2)) with a = cos^2(theta) / 2 sx^2 + sin^2(theta) / 2 sy^2, b = -sin(2 theta) / 4 sx^2 + sin(2 theta) / 4 sy^2,
    c = sin^2(theta) / 2 sx^2 + cos^2(theta) / 2 sy^2, centre sc / 2 and sx = sy = sc / 4 on ``linspace(0, sc, sc)``."""

    def __init__(self, sc: int = 5, r_mask: int = 3, intensity: int = 1, theta: int = 0, offset: int = 0):
        sc = sc + 1 if sc % 2 == 0 else sc
        axis = np.linspace(0, sc, sc)
        self.x, self.y = np.meshgrid(axis, axis)
        self.xo = self.yo = sc / 2
        self.sigma_x = self.sigma_y = sc / 4
        self.intensity, self.theta, self.offset, self.r_mask = intensity, theta, offset, r_mask

    def atom2dgaussian(self) -> np.ndarray:
        t, sx2, sy2 = self.theta, self.sigma_x ** 2, self.sigma_y ** 2
        a = (np.cos(t) ** 2) / (2 * sx2) + (np.sin(t) ** 2) / (2 * sy2)
        b = -(np.sin(2 * t)) / (4 * sx2) + (np.sin(2 * t)) / (4 * sy2)
        c = (np.sin(t) ** 2) / (2 * sx2) + (np.cos(t) ** 2) / (2 * sy2)
        dx, dy = self.x - self.xo, self.y - self.yo
        return self.offset + self.intensity * np.exp(-(a * (dx ** 2) + 2 * b * dx * dy + c * (dy ** 2)))

    def circularmask(self, image: np.ndarray, radius: int) -> np.ndarray:
        """Zeroes ``image`` (in place) outside the disc of ``radius`` around the grid centre, measured from pixel
        index + 0.5."""
        rows, cols = np.ogrid[:self.x.shape[0], :self.x.shape[1]]
        outside = np.sqrt((rows - self.xo + 0.5) ** 2 + (cols - self.yo + 0.5) ** 2) > radius
        image[outside] = 0
        return image

    def gen_atom_mask(self) -> Tuple[np.ndarray]:
        """(atom, mask): the Gaussian and the disc of diameter ``r_mask`` cut to its bounding box, 1 inside."""
        atom = self.atom2dgaussian()
        mask = self.circularmask(atom.copy(), self.r_mask / 2)
        rows, cols = np.where(mask > 0)
        if len(rows) == 0:
            raise ValueError("gen_atom_mask: no pixel of the atom is positive inside the mask radius")
        mask = mask[rows.min():rows.max() + 1, cols.min():cols.max() + 1]
        mask[mask > 0] = 1
        return atom, mask


def create_atom_mask_pair(sc: int = 5, r_mask: int = 5, intensity: int = 1):
    """(atom, mask) of ``MakeAtom(sc, r_mask, intensity)``."""
    return MakeAtom(sc, r_mask, intensity).gen_atom_mask()


def _stamp(func, *call):
    """The mask of ``func(*call)`` as a float64 square of odd side; ValueError otherwise (before anything is launched)."""
    mask = np.asarray(func(*call)[1], dtype=np.float64)
    top = _T.max_side()
    if mask.ndim != 2 or mask.shape[0] != mask.shape[1]:
        raise ValueError(f"the atom mask must be a square 2-D array, got shape {mask.shape}")
    if mask.shape[0] % 2 == 0 or mask.shape[0] > top:
        raise ValueError(f"the atom mask must have an odd side of at most {top}, got {mask.shape[0]}")
    return np.ascontiguousarray(mask)


def _rasterise(F, H, W, xy, meta, stamps, nch, dtype, rows_of):
    """The flat table through amx_lattice_owner and amx_lattice_fill.  ``xy`` (N, 2) float64, ``meta`` (N, 3) int32,
    ``stamps`` a list of squares, ``nch`` the frames' channel counts (None: one channel, no background), ``rows_of``
    maps a flat row to (frame, row in its table) for the error.  Returns the device tensor (F, H, W, C [+ 1])."""
    dev = _T.device()
    C = 1 if nch is None else max(1, int(max(nch)))
    sside = np.array([s.shape[0] for s in stamps], dtype=np.int32)
    soff = np.concatenate(([0], np.cumsum(sside.astype(np.int64) ** 2)))
    flat = np.concatenate([s.ravel() for s in stamps]) if stamps else np.zeros(0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    xy_d, meta_d = up(xy.reshape(-1, 2), np.float64), up(meta.reshape(-1, 3), np.int32)
    sside_d, soff_d, flat_d = up(sside, np.int32), up(soff[:-1], np.int64), up(flat, np.float64)
    own, bad = _T.owner(xy_d, meta_d, sside_d, F, H, W, C)
    first = int(bad)                                                       # the one scalar read back per call
    if first != _T.INT_MAX:
        f, r = rows_of(first)
        x, y = xy[first]
        m = int(sside[meta[first, 2]])
        raise ValueError(f"atom {r} of frame {f} at ({x}, {y}): its {m} x {m} mask does not lie inside the {H} x {W} "
                         "frame (or the coordinate is not finite)")
    return _T.fill(own, xy_d, meta_d, sside_d, soff_d, flat_d, None if nch is None else up(nch, np.int32), dtype)


def create_lattice_mask(lattice: np.ndarray, xy_atoms: np.ndarray,
                        *args: Callable[[int, int], Tuple[np.ndarray, np.ndarray]], **kwargs: int) -> np.ndarray:
    """Ground truth of one frame whose atoms are all of one class (imgen.py:82-131); fractional positions are rounded
    half to even.

    Args:
        lattice: the 2-D experimental image; only its shape and dtype are used.
        xy_atoms: (N, 2) atom positions (row, column).
        *args: optionally a function (scale, rmask) -> (atom, mask); it is called ONCE per call of this function
            (the reference: once per atom), and its mask values reach the output unchanged.
        **scale (7), **rmask (5): size of the simulated atom and of its mask.
        **as_tensor (False): keep the result on the device as a torch tensor (float32 for a float32 lattice, else
            float64) instead of returning a numpy array of ``lattice.dtype``.
    """
    func = args[0] if len(args) == 1 else create_atom_mask_pair
    lattice = np.asarray(lattice)
    if lattice.ndim != 2:
        raise ValueError(f"create_lattice_mask takes a 2-D image, got shape {lattice.shape}")
    xy = np.asarray(xy_atoms, dtype=np.float64)
    xy = xy.reshape(0, 2) if xy.size == 0 else xy
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"xy_atoms must be an (N, 2) array, got shape {xy.shape}")
    stamp = _stamp(func, kwargs.get("scale", 7), kwargs.get("rmask", 5))
    H, W = lattice.shape
    out = _rasterise(1, H, W, xy, np.zeros((len(xy), 3), dtype=np.int32), [stamp], None,
                     torch.float32 if lattice.dtype == np.float32 else torch.float64, lambda i: (0, i))[0, :, :, 0]
    if kwargs.get("as_tensor", False):
        return out
    return out.cpu().numpy().astype(lattice.dtype, copy=False)


def _multiclass(H, W, tables, args, kwargs):
    """Masks of all frames from one flat table: (device tensor (F, H, W, C + 1), channel count of every frame)."""
    func = args[0] if len(args) == 1 else create_atom_mask_pair
    scale, rmask = kwargs.get("scale", 7), kwargs.get("rmask", 7)
    xy, cls, frame, nch = [], [], [], []
    for f, table in enumerate(tables):
        table = np.asarray(table)
        if table.ndim != 2 or table.shape[1] < 3:
            raise ValueError(f"the coordinates of frame {f} must be an (N, 3) array, got shape {table.shape}")
        z = table[:, -1]
        if 0 in np.unique(z):
            z = z + 1                                                       # (a copy: the caller's array is not modified)
        nch.append(len(np.unique(z)))
        xy.append(table[:, :2].astype(np.float64))
        cls.append(z)
        frame.append(np.full(len(table), f, dtype=np.int32))
    values = np.unique(np.concatenate(cls)) if cls and sum(map(len, cls)) else np.zeros(0)
    stamps = [_stamp(func, scale, rmask, z) for z in values]               # once per distinct class value of the call
    meta = np.zeros((sum(map(len, cls)), 3), dtype=np.int32)
    if len(meta):
        meta[:, 0] = np.concatenate(frame)
        meta[:, 1] = np.concatenate([np.searchsorted(np.unique(z), z) for z in cls])
        meta[:, 2] = np.searchsorted(values, np.concatenate(cls))
    xy = np.concatenate(xy) if xy else np.zeros((0, 2))
    starts = np.concatenate(([0], np.cumsum([len(z) for z in cls])))

    def rows_of(i):
        f = int(np.searchsorted(starts, i, side="right")) - 1
        return f, i - int(starts[f])

    f32 = kwargs.get("as_tensor", False) and kwargs.get("dtype") in (np.float32, torch.float32)
    dtype = torch.float32 if f32 else torch.float64
    return _rasterise(len(tables), H, W, xy, meta, stamps, np.array(nch, dtype=np.int32), dtype, rows_of), nch


def create_multiclass_lattice_mask_(lattice: np.ndarray, xyz_atoms: np.ndarray,
                                    *args: Callable[[int, int, int], Tuple[np.ndarray, np.ndarray]],
                                    **kwargs: int) -> np.ndarray:
    """Ground truth of one frame with several atom classes (imgen.py:178-229): one channel per distinct value of the
    last column of ``xyz_atoms`` in ascending order (the values need not be contiguous), plus the background channel
    max(0, 1 - sum of the class channels); float64, shape (h, w, classes + 1).  An empty table gives the background alone.

    When the class column contains 0 the reference adds 1 to the caller's array IN PLACE before it makes the masks; here
    the shift is applied to a copy (the mask function is still called with the shifted value) and ``xyz_atoms`` is left
    as it was.  The returned mask is the same.

    ``*args``: optionally a function (scale, rmask, intensity) -> (atom, mask), called once per distinct class value.
    ``**scale`` (7), ``**rmask`` (7); ``**as_tensor`` (False) keeps the result on the device (``dtype=np.float32``
    is allowed there).  As in the reference, negative mask values are clamped to 0 after the background is formed."""
    H, W = np.shape(lattice)[:2]
    out, nch = _multiclass(H, W, [xyz_atoms], args, kwargs)
    out = out[0, :, :, :nch[0] + 1]
    return out.contiguous() if kwargs.get("as_tensor", False) else out.cpu().numpy()


def create_multiclass_lattice_mask(imgdata: np.ndarray, coord_class_dict: Union[Dict[int, np.ndarray], np.ndarray],
                                   *args: Callable[[int, int, int], Tuple[np.ndarray, np.ndarray]],
                                   **kwargs: int) -> Union[List[np.ndarray], np.ndarray]:
    """Ground truth of a stack of frames (or one 2-D frame) from the Locator-style dictionary {frame: (N, 3) array of
    row, column, class} (or one (N, 3) array for a single frame) (imgen.py:134-175).  All frames go through ONE flat
    table and one pair of launches.  Returns one (n, h, w, classes + 1) float64 array when every frame has the same
    number of classes, else a list of (h, w, classes_i + 1) arrays, as the reference does.  Arguments and keywords as
    for ``create_multiclass_lattice_mask_``; with ``as_tensor=True`` the array / the list's members are device tensors."""
    shape = tuple(imgdata.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if isinstance(coord_class_dict, np.ndarray):
        coord_class_dict = {0: coord_class_dict}
    F, H, W = shape[:3]
    out, nch = _multiclass(H, W, [coord_class_dict[i] for i in range(F)], args, kwargs)
    host = (lambda t: t.contiguous()) if kwargs.get("as_tensor", False) else (lambda t: t.cpu().numpy())
    if len(set(nch)) <= 1:
        return host(out[..., :nch[0] + 1])
    return [host(out[f, :, :, :n + 1]) for f, n in enumerate(nch)]

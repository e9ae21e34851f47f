"""Locator: class-probability maps -> blob centres on the device
(reference: atomai/predictors/predictor.py:531-639; cv_thresh utils/img.py:554-564; find_com
utils/coords.py:21-34).

Same constructor / ``run`` contract and the same result — ``{frame: (n, 3) float64 [row, col, class]}`` with the
reference's ordering — but threshold, 4-connected labelling, centres of mass and the border filter run as HIP
kernels over whole chunks of frames (``amx_locate_label`` / ``amx_locate_emit``) instead of a per-frame
cv2 + scipy.ndimage loop on the host.  ``refine=True`` (utils/coords.py:179-231: one scipy curve_fit per atom)
runs as ``amx_peak_refine`` on the same device-resident table before it is copied back.
"""
import warnings
from typing import Dict, Union

import numpy as np
import torch

from .. import _lib as L


def _locate_tensors(prob: torch.Tensor, threshold: float, dist_edge: int):
    """``amx_locate_label`` + ``amx_locate_emit`` on a chunk: the flat atom table as device tensors, coords (n, 2)
    float64 [row, col] and meta (n, 2) int32 [frame, class], rows sorted by frame."""
    if prob.ndim != 4 or prob.dtype != torch.float32:
        raise ValueError("expected (B, H, W, C) float32 probabilities")
    prob = prob.contiguous()
    B, H, W, C = prob.shape
    nch = max(C - 1, 1)                         # 1-channel output: background = 1 - p is appended by the reference
    lib = L.load()
    nbytes = lib.amx_locate_workspace_bytes(B, H, W, nch)
    if nbytes < 0:
        raise L.AmxError("chunk too large for int32 labels: pass fewer frames per call")
    dev = prob.device
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    sp = L.stream_ptr(prob)
    L.call("amx_locate_label", L.ptr(prob), B, H, W, C, nch, float(threshold), int(dist_edge), L.ptr(work),
           L.ptr(count), sp)
    n = int(count.item())                       # one 4-byte read-back per chunk sizes the ragged output
    coords = torch.empty((n, 2), dtype=torch.float64, device=dev)
    meta = torch.empty((n, 2), dtype=torch.int32, device=dev)
    if n:
        L.call("amx_locate_emit", L.ptr(work), B, H, W, nch, int(dist_edge), L.ptr(coords), L.ptr(meta), n, sp)
    return coords, meta


def _tables(coords: np.ndarray, meta: np.ndarray, B: int) -> Dict[int, np.ndarray]:
    table = np.concatenate((coords, meta[:, 1:2].astype(np.float64)), axis=1)
    bounds = np.searchsorted(meta[:, 0], np.arange(B + 1))      # rows are sorted by frame
    return {i: table[bounds[i]:bounds[i + 1]] for i in range(B)}


def locate_device(prob: torch.Tensor, threshold: float, dist_edge: int, frames: torch.Tensor = None,
                  d=None, first_frame: int = 0) -> Dict[int, np.ndarray]:
    """Centres for a chunk of NHWC probabilities already resident on the device (or, under the test
    backend, on the host).  Returns {local frame index: (n, 3)}.  With ``frames`` — the chunk's (B, H, W) float32
    input images on the same device — the centres are refined (``refine_device``) before they leave the device."""
    coords, meta = _locate_tensors(prob, threshold, dist_edge)
    if frames is not None:
        coords = refine_device(frames, coords, meta, d, first_frame)
    return _tables(coords.cpu().numpy(), meta.cpu().numpy(), prob.shape[0])


MAX_D = 32          # amx_peak_refine: a wave's patch of (2 d)^2 fp32 pixels lives in LDS


def check_d(d) -> None:
    """The half-side must leave more pixels than the 7 parameters (the reference fails with TypeError at d = 1 and
    IndexError at d = 0) and fit the kernel's LDS patch."""
    if d is None:
        return
    for v in np.atleast_1d(d):
        if int(v) != v or not 2 <= int(v) <= MAX_D:
            raise ValueError(f"peak refinement needs an integer half-side 2 <= d <= {MAX_D}, got {v}")


def warn_default_d(d, stacklevel: int = 3) -> None:
    """The reference's warning about a missing half-side (coords.py:200-204), once per call of an entry point."""
    if d is None:
        warnings.warn("The d-value for bounding box not found. Defaulting to 1/4 of mean atomic distance.",
                      stacklevel=stacklevel)


def refine_device(frames: torch.Tensor, coords: torch.Tensor, meta: torch.Tensor, d=None, first_frame: int = 0,
                  return_status: bool = False):
    """Gaussian peak refinement (``amx_peak_refine``) of a flat atom table that is resident on the device of its
    (B, H, W) float32 ``frames``.  ``d``: one half-side for all frames, one per frame, or None for the reference's
    default int(mean nearest-neighbour distance * 0.25) per frame (``amx_nn2_quarter_mean``).  Returns the refined
    (n, 2) float64 device tensor (and the per-atom int32 status)."""
    if frames.ndim != 3 or frames.dtype != torch.float32:
        raise ValueError("expected (B, H, W) float32 frames")
    check_d(d)
    frames = frames.contiguous()
    B, H, W = frames.shape
    n = len(coords)
    dev = frames.device
    out = torch.empty_like(coords)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:                                  # (the reference crashes on a frame without atoms)
        return (out, status) if return_status else out
    sp = L.stream_ptr(frames)
    if d is None:
        per_frame = np.bincount(meta[:, 0].cpu().numpy(), minlength=B)
        for f in np.nonzero((per_frame > 0) & (per_frame < 3))[0]:
            raise ValueError(f"frame {first_frame + int(f)} has {per_frame[f]} atom(s): the default d needs the two "
                             f"nearest neighbours of every atom, pass d explicitly")
        dt = torch.empty(B, dtype=torch.int32, device=dev)
        L.call("amx_nn2_quarter_mean", L.ptr(coords), L.ptr(meta), n, B, L.ptr(dt), sp)
        dh = dt.cpu().numpy()
        for f in np.nonzero(per_frame > 0)[0]:
            if not 2 <= dh[f] <= MAX_D:
                raise ValueError(f"frame {first_frame + int(f)}: the default d = {dh[f]} (a quarter of the mean "
                                 f"nearest-neighbour distance) is outside 2 <= d <= {MAX_D}, pass d explicitly")
        dmax = int(dh[per_frame > 0].max())
    else:
        dh = np.array(np.broadcast_to(np.asarray(d, dtype=np.int32), (B,)))
        dt = torch.from_numpy(dh).to(dev)
        dmax = int(dh.max())
    L.call("amx_peak_refine", L.ptr(frames), B, H, W, L.ptr(coords), L.ptr(meta), L.ptr(dt), dmax, n, L.ptr(out),
           L.ptr(status), sp)
    return (out, status) if return_status else out


class Locator:
    """``Locator(threshold=0.5, dist_edge=5, dim_order='channel_last', **kwargs).run(nn_output)``."""

    def __init__(self, threshold: float = 0.5, dist_edge: int = 5, dim_order: str = "channel_last",
                 **kwargs: Union[bool, float]) -> None:
        self.dim_order = dim_order
        self.threshold = threshold
        self.dist_edge = dist_edge
        self.refine = kwargs.get("refine")
        self.d = kwargs.get("d")
        self.device = kwargs.get("device", "cuda" if torch.cuda.is_available() else "cpu")
        self.chunk_bytes = int(kwargs.get("chunk_bytes", 1 << 30))

    def preprocess(self, nn_output: np.ndarray) -> np.ndarray:
        """Channel-last view of the network output.  (The reference also appends a background channel to
        1-channel data, only to skip it again in ``run``; the kernels take the channel count instead.)"""
        if self.dim_order == "channel_first":
            nn_output = np.transpose(nn_output, (0, 2, 3, 1))
        elif self.dim_order != "channel_last":
            raise NotImplementedError('For dim_order, use "channel_first"', 'or "channel_last" (e.g. tensorflow)')
        return nn_output

    def run(self, nn_output: np.ndarray, *args: np.ndarray) -> Dict[int, np.ndarray]:
        """With ``refine=True`` pass the input images (N, H, W, 1) as the second argument (predictor.py:609-619):
        every chunk's centres are refined on the device, against its frames converted to float32."""
        imgdata = None
        if self.refine:
            if len(args) == 0:
                raise AssertionError("Pass input image(s) for coordinates refinement")
            check_d(self.d)
            warn_default_d(self.d)
            imgdata = np.asarray(args[0])
            if imgdata.ndim != 4 or imgdata.shape[-1] != 1:
                raise ValueError("expected (N, H, W, 1) input images")
        nn_output = self.preprocess(np.asarray(nn_output))
        if nn_output.ndim != 4:
            raise ValueError("expected a 4D network output")
        n = len(nn_output)
        if imgdata is not None and imgdata.shape[:3] != nn_output.shape[:3]:
            raise ValueError("input images and network output differ in shape")
        per_frame = int(np.prod(nn_output.shape[1:])) * 4 * 8   # probabilities + labelling workspace
        chunk = max(1, min(n, self.chunk_bytes // max(per_frame, 1)))
        out = {}
        for s in range(0, n, chunk):
            x = torch.from_numpy(np.ascontiguousarray(nn_output[s:s + chunk], dtype=np.float32)).to(self.device)
            frames = None
            if imgdata is not None:
                frames = torch.from_numpy(np.ascontiguousarray(imgdata[s:s + chunk, ..., 0], dtype=np.float32))
                frames = frames.to(self.device)
            for i, v in locate_device(x, self.threshold, self.dist_edge, frames, self.d, s).items():
                out[s + i] = v
        return out

    def rem_edge_coord(self, coordinates: np.ndarray, h: int, w: int) -> np.ndarray:
        """Host version of the border filter (predictor.py:621-639), kept for API compatibility."""
        c = np.asarray(coordinates)
        drop = (c[:, 0] > h - self.dist_edge) | (c[:, 0] < self.dist_edge) | \
               (c[:, 1] > w - self.dist_edge) | (c[:, 1] < self.dist_edge)
        return c[~drop]

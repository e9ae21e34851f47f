"""Atom stamps rasterised into masks and windows gathered on the device (csrc/lattice.hip): thin wrappers over the C ABI.

Tables, stamps and frames are device tensors here; ``crop_host`` is the one helper that takes and returns numpy arrays
(one upload, one launch, one download)."""
import numpy as np
import torch

from .. import _lib as L

INT_MAX = 2 ** 31 - 1


def device():
    return torch.device("cpu") if L.is_test_backend() and not torch.cuda.is_available() else torch.device("cuda")


def max_side():
    """The largest stamp side the kernels take (odd)."""
    return int(L.load().amx_lattice_max_side())


def owner(xy, meta, sside, F, H, W, C):
    """(owner (F, H, W, C) int32, bad () int32) of the flat table ``xy`` (N, 2) float64 / ``meta`` (N, 3) int32 =
    (frame, channel, stamp id) with stamp sides ``sside`` (K,) int32: owner = -(i + 1) of the latest row i whose square
    covers the pixel, 0 where none; bad = the first refused row, INT_MAX if none.  Nothing is read back."""
    dev = xy.device
    own = torch.zeros((F, H, W, C), dtype=torch.int32, device=dev)
    bad = torch.full((), INT_MAX, dtype=torch.int32, device=dev)
    L.call("amx_lattice_owner", L.ptr(xy), L.ptr(meta), xy.shape[0], L.ptr(sside), sside.shape[0], F, H, W, C,
           L.ptr(own), L.ptr(bad), L.stream_ptr(own))
    return own, bad


def fill(own, xy, meta, sside, soff, stamps, nch=None, dtype=torch.float64):
    """(F, H, W, C) masks of ``dtype`` (float32 / float64) from the owner array; with ``nch`` (F,) int32, the frames'
    channel counts, (F, H, W, C + 1): the background 1 - sum at channel nch[f], zeros above it, negative values clamped."""
    F, H, W, C = own.shape
    background = nch is not None
    out = torch.empty((F, H, W, C + int(background)), dtype=dtype, device=own.device)
    L.call("amx_lattice_fill", L.ptr(own), L.ptr(xy), L.ptr(meta), xy.shape[0], L.ptr(sside), L.ptr(soff), sside.shape[0],
           L.ptr(stamps), stamps.shape[0], L.ptr(nch) if background else L.ptr(None), F, H, W, C, int(background),
           L.ptr(out), int(dtype == torch.float64), L.stream_ptr(own))
    return out


_BITS = {4: torch.int32, 8: torch.int64}


def crop(src, win, ph, pw, dst=None):
    """(dst (P, ph, pw, C), flag (P,) int32): the windows ``win`` (P, 3) int32 = (frame, first row, first column) of
    ``src`` (F, H, W, C) float32 / float64 / int32 / int64, copied bit for bit.  flag: -1 window not inside its frame
    (dst untouched), 1 a NaN in a floating-point window, else 0.  ``dst`` may be given (it is written in place)."""
    F, H, W, C = src.shape
    P = win.shape[0]
    esize = src.element_size()
    if src.dtype not in (torch.float32, torch.float64, torch.int32, torch.int64):
        raise TypeError(f"crop takes float32, float64, int32 or int64 elements, not {src.dtype}")
    if dst is None:
        dst = torch.empty((P, ph, pw, C), dtype=src.dtype, device=src.device)
    assert dst.shape == (P, ph, pw, C) and dst.dtype == src.dtype
    flag = torch.empty(P, dtype=torch.int32, device=src.device)
    L.call("amx_crop_windows", L.ptr(src), esize, int(src.is_floating_point()), F, H, W, C, L.ptr(win), P, int(ph),
           int(pw), L.ptr(dst), L.ptr(flag), L.stream_ptr(src))
    return dst, flag


def crop_host(frames, win, ph, pw):
    """numpy in, numpy out: the windows of ``frames`` (F, H, W, C) of any numeric dtype.  Elements of 4 or 8 bytes go to
    the device as they are (unsigned and other types as their bits); narrower ones are widened exactly (bool and
    integers to int32, float16 to float32) and narrowed again afterwards.  Returns (windows of frames.dtype, flag)."""
    frames = np.ascontiguousarray(frames)
    dt = frames.dtype
    if dt.kind not in "biuf":
        raise TypeError(f"windows of dtype {dt} cannot be gathered (numeric arrays only)")
    if dt.itemsize in (4, 8):
        wide = frames if dt.kind == "f" or dt in (np.int32, np.int64) else frames.view(f"i{dt.itemsize}")
    elif dt.itemsize < 4:
        wide = frames.astype(np.float32 if dt.kind == "f" else np.int32)
    else:
        raise TypeError(f"windows of dtype {dt} cannot be gathered (elements of at most 8 bytes)")
    dev = device()
    src = torch.from_numpy(wide).to(dev)
    dst, flag = crop(src, torch.from_numpy(np.ascontiguousarray(win, dtype=np.int32)).to(dev), ph, pw)
    out = dst.cpu().numpy()
    out = out.view(dt) if out.dtype.itemsize == dt.itemsize else out.astype(dt)
    return out, flag.cpu().numpy()

"""Image helpers on the predict path and between Segmentor predictions and VAE training stacks
(reference: atomai/utils/img.py:112-180, 298-350, 502-551)."""
from typing import Dict, Tuple, Union

import numpy as np


def img_resize(image_data: np.ndarray, rs: Tuple[int], round_: bool = False) -> np.ndarray:
    """Resizes an (n, h, w) stack to ``rs`` (reference: atomai/utils/img.py:20-68, ``img_resize`` + ``cv_resize``) on the
    device: ``amx_aug_resample`` carries OpenCV's INTER_CUBIC and enlarging INTER_AREA arithmetic (restated, UNPINNED
    against cv2 itself — absent from this image; oracle/aug_oracle.py:img_resize is the checker).  Reference quirks kept:
    ``rs`` is swapped when its entries differ (img.py:36-37); a stack that already has the target shape is copied; per
    image INTER_AREA is chosen when the height is below the target's second entry, INTER_CUBIC otherwise (img.py:63-64);
    float64 result.  True area averaging (INTER_AREA with both axes shrunk: non-square targets only) is not provided.
    Precision: the stack is resampled in fp32 on the device whatever its dtype (cv2 keeps CV_64F data in double), so a
    float64 input agrees with a double-precision evaluation of the same arithmetic to ~1e-6 of the data range — a
    TOLERANCE, not bit-level parity (tests/test_oracle_aug_resize.py states it); there is no cv2 in this image to
    generate a golden from."""
    import torch
    from .. import _lib as L
    rs = tuple(int(v) for v in rs)
    if rs[0] != rs[1]:
        rs = (rs[1], rs[0])
    image_data = np.asarray(image_data)
    if image_data.shape[1:3] == rs:
        return image_data.copy()
    n, h, w = image_data.shape
    area = h < rs[1]
    if area and h >= rs[0] and w >= rs[1]:
        raise NotImplementedError("img_resize: cv2.INTER_AREA with both axes shrunk (true area averaging) is not on the "
                                  "device path; it is only reached for non-square targets")
    if torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    elif L.is_test_backend():
        dev = torch.device("cpu")
    else:
        raise L.AmxError("img_resize runs on the MI355X (amx_aug_resample); there is no CPU fallback")
    out = np.empty((n, rs[0], rs[1]), dtype=np.float64)
    per = max(1, (256 << 20) // (4 * max(h * w, rs[0] * rs[1])))            # frames per upload (<= 256 MB each way)
    for i0 in range(0, n, per):
        x = torch.from_numpy(np.ascontiguousarray(image_data[i0:i0 + per], dtype=np.float32)).to(dev)
        m = x.shape[0]
        y = torch.empty((m, rs[0], rs[1]), dtype=torch.float32, device=dev)
        win = torch.tensor([[0, 0, h, w]] * m, dtype=torch.int32, device=dev)
        L.call("amx_aug_resample", L.ptr(x), L.ptr(y), L.ptr(win), m, h, w, rs[0], rs[1], 2 if area else 1, 0,
               int(bool(round_)), L.stream_ptr(x))
        out[i0:i0 + m] = y.cpu().numpy()
    return out


def img_pad(image_data: np.ndarray, pooling: int) -> np.ndarray:
    """Zero-pads (bottom/right) an (n, h, w) stack until h and w are divisible by ``pooling``.
    Same result as the reference's row-by-row np.concatenate loop (float64 output), in one allocation."""
    pooling = int(pooling)
    n, h, w = image_data.shape
    H = -(-h // pooling) * pooling
    W = -(-w // pooling) * pooling
    if H == h and W == w:
        return image_data
    out = np.zeros((n, H, W), dtype=np.result_type(image_data.dtype, np.float64))
    out[:, :h, :w] = image_data
    return out


def get_imgstack(imgdata: np.ndarray, coord: np.ndarray, r: int) -> Tuple[np.ndarray]:
    """Square windows of side ``r`` around the given (row, col) centres of ONE image (h, w, c); centres whose window
    sticks out of the image or contains NaN are dropped (img.py:138-180).  Vectorised: one fancy-indexing gather
    instead of a Python loop over the centres."""
    coord = np.asarray(coord)
    if len(coord) == 0:
        return None, None
    r = int(r)
    centres = np.around(coord[:, :2]).astype(np.int64)
    lo = centres - r // 2
    hi = lo + r                                      # odd r: [c - r//2, c + r//2]; even r: [c - r//2, c + r//2 - 1]
    h, w = imgdata.shape[:2]
    ok = (lo[:, 0] >= 0) & (lo[:, 1] >= 0) & (hi[:, 0] <= h) & (hi[:, 1] <= w)
    if not ok.any():
        return None, None
    rows = lo[ok, 0][:, None] + np.arange(r)[None, :]
    cols = lo[ok, 1][:, None] + np.arange(r)[None, :]
    stack = imgdata[rows[:, :, None], cols[:, None, :]]
    kept = coord[ok]
    finite = ~np.isnan(stack.reshape(len(stack), -1)).any(axis=1)
    if not finite.any():
        return None, None
    return stack[finite], kept[finite]


def extract_subimages(imgdata: np.ndarray, coordinates: Union[Dict[int, np.ndarray], np.ndarray],
                      window_size: int, coord_class: int = 0) -> Tuple[np.ndarray]:
    """Sub-images centred on the detected objects of one class, for every frame (img.py:298-350): returns
    (stack, centres, frame numbers) — the usual bridge from ``Segmentor.predict`` output to ``rVAE.fit`` input."""
    single = isinstance(coordinates, np.ndarray)
    per_frame = [np.column_stack((coordinates, np.zeros(len(coordinates))))] if single else list(coordinates.values())
    frames = np.asarray(imgdata)
    if frames.ndim == 2:
        frames = frames[None, :, :, None]
    parts = []                                          # (windows, centres, frame index) of every frame that yields any
    for frame_no, (frame, table) in enumerate(zip(frames, per_frame)):
        table = np.asarray(table)
        wanted = table[table[:, 2] == coord_class, :2]
        windows, centres = get_imgstack(frame, wanted, window_size)
        if windows is not None:
            parts.append((windows, centres, np.full(len(centres), frame_no, dtype=int)))
    if not parts:
        return [], [], []                               # the reference's return value when nothing survives
    return tuple(np.concatenate(col, axis=0) for col in zip(*parts))


def crop_borders(imgdata: np.ndarray, thresh: float = 0) -> np.ndarray:
    """Drops the border rows / columns of an (h, w, c) array whose values are all <= thresh (img.py:502-519)."""
    def crop(img):
        mask = img > thresh
        return img[np.ix_(mask.any(1), mask.any(0))]
    return np.array([crop(imgdata[..., i]) for i in range(imgdata.shape[-1])]).transpose(1, 2, 0)


def get_coord_grid(imgdata: np.ndarray, step: int, return_dict: bool = True):
    """Square grid of coordinates for every image of a stack, in the Locator's output format (img.py:522-551)."""
    if np.ndim(imgdata) == 2:
        imgdata = np.expand_dims(imgdata, axis=0)
    ii, jj = np.meshgrid(np.arange(0, imgdata.shape[1], step), np.arange(0, imgdata.shape[2], step), indexing="ij")
    coord = np.stack((ii.ravel(), jj.ravel()), axis=1)
    if return_dict:
        coord = np.concatenate((coord, np.zeros((coord.shape[0], 1))), axis=-1)
        return {i: coord for i in range(imgdata.shape[0])}
    return np.concatenate([coord for _ in range(imgdata.shape[0])], axis=0)


# ---- training patches and random sub-images (img.py:183-296, 353-389): the offsets are drawn on the host exactly as the
# reference / scikit-learn draw them, the windows of ALL frames are gathered by one amx_crop_windows launch per array.
def _windows(frames: np.ndarray, frame_idx, rows, cols, ph: int, pw: int):
    """(windows (P, ph, pw, C) of frames.dtype, flag (P,)) of the (F, H, W, C) stack; flag as amx_crop_windows."""
    from . import _lattice
    win = np.stack((np.asarray(frame_idx), np.asarray(rows), np.asarray(cols)), axis=1).astype(np.int32)
    return _lattice.crop_host(frames, win.reshape(-1, 3), ph, pw)


def _patch_offsets(h: int, w: int, patch_size, num_patches, random_state):
    """Top-left corners of scikit-learn's ``extract_patches_2d(max_patches=num_patches, random_state=...)``: random WITH
    replacement, all rows drawn before all columns."""
    import numbers
    ph, pw = (patch_size, patch_size) if isinstance(patch_size, numbers.Integral) else patch_size
    ph, pw = int(ph), int(pw)
    if ph > h:
        raise ValueError("Height of the patch should be less than the height of the image.")
    if pw > w:
        raise ValueError("Width of the patch should be less than the width of the image.")
    if not isinstance(num_patches, numbers.Integral) or num_patches < 1:
        raise ValueError(f"num_patches must be a positive integer, got {num_patches!r}")
    every = (h - ph + 1) * (w - pw + 1)
    m = min(int(num_patches), every)
    rng = np.random.RandomState(random_state)
    i = rng.randint(h - ph + 1, size=m)
    j = rng.randint(w - pw + 1, size=m)
    return ph, pw, i, j


def _as_stack(a: np.ndarray) -> np.ndarray:
    """(F, H, W) or (F, H, W, C) -> (F, H, W, C)."""
    a = np.asarray(a)
    if a.ndim not in (3, 4):
        raise ValueError(f"expected a stack (n, h, w) or (n, h, w, c), got shape {a.shape}")
    return a[..., None] if a.ndim == 3 else a


def _drop_unit_channel(p: np.ndarray) -> np.ndarray:
    return p[..., 0] if p.shape[-1] == 1 else p                # scikit-learn drops a colour axis of length 1


def extract_patches(images: np.ndarray, masks: np.ndarray, patch_size: int, num_patches: int,
                    **kwargs: int) -> Tuple[np.ndarray]:
    """``num_patches`` random patches of every image-mask pair of two stacks (or of one 2-D pair), concatenated over the
    frames (img.py:369-389).  The offsets follow scikit-learn's ``extract_patches_2d``: m = min(num_patches, number of
    distinct patches) corners drawn WITH replacement from ``np.random.RandomState(random_state)`` (``**random_state``,
    default 0), rows first, then columns; image and mask share them, and — the reference's behaviour — so does every
    frame.  ``patch_size`` is an int or a (height, width) pair; a trailing channel axis of length 1 is dropped; the
    dtypes are kept; a patch larger than the frame raises ``ValueError``.  scikit-learn is not imported."""
    images, masks = np.asarray(images), np.asarray(masks)
    images = images[None] if images.ndim == 2 else images
    masks = masks[None] if masks.ndim == 2 else masks
    n = min(len(images), len(masks))
    images, masks = _as_stack(images[:n]), _as_stack(masks[:n])
    if images.shape[1:3] != masks.shape[1:3]:
        raise ValueError(f"images {images.shape[1:3]} and masks {masks.shape[1:3]} differ in size")
    ph, pw, i, j = _patch_offsets(images.shape[1], images.shape[2], patch_size, num_patches, kwargs.get("random_state", 0))
    frame_idx, rows, cols = np.repeat(np.arange(n), len(i)), np.tile(i, n), np.tile(j, n)
    return tuple(_drop_unit_channel(_windows(a, frame_idx, rows, cols, ph, pw)[0]) for a in (images, masks))


def extract_patches_(lattice_im: np.ndarray, lattice_mask: np.ndarray, patch_size: int, num_patches: int,
                     **kwargs: int) -> Tuple[np.ndarray]:
    """Patches of ONE image (h, w[, c]) and its mask at shared random offsets (img.py:353-366); see ``extract_patches``."""
    lattice_im, lattice_mask = np.asarray(lattice_im), np.asarray(lattice_mask)
    if lattice_im.ndim not in (2, 3) or lattice_mask.ndim not in (2, 3):
        raise ValueError("extract_patches_ takes one image (h, w) or (h, w, c) and its mask")
    return extract_patches(lattice_im[None], lattice_mask[None], patch_size, num_patches, **kwargs)


def _centred(frames: np.ndarray, frame_idx, centres: np.ndarray, r: int):
    """``get_imgstack`` for centres in several frames at once: windows [c - r//2, c - r//2 + r) around the centres
    rounded half to even; (windows, keep) with keep False where the window leaves the frame or holds a NaN."""
    lo = np.around(np.asarray(centres, dtype=np.float64)[:, :2]).astype(np.int64) - r // 2
    lo = np.clip(lo, -2 ** 30, 2 ** 30)                        # (far-off centres stay outside, without int32 overflow)
    stack, flag = _windows(frames, frame_idx, lo[:, 0], lo[:, 1], r, r)
    return stack, flag == 0


def _single(img: np.ndarray) -> np.ndarray:
    img = np.asarray(img)
    if img.ndim not in (2, 3):
        raise ValueError(f"expected one image (h, w) or (h, w, c), got shape {img.shape}")
    return img[None, ..., None] if img.ndim == 2 else img[None]


def _kept(img: np.ndarray, com_xy: np.ndarray, window_size: int):
    """What ``get_imgstack(img, com_xy, window_size)`` returns, with the gather on the device."""
    if len(com_xy) == 0:
        return None, None
    stack, keep = _centred(_single(img), np.zeros(len(com_xy), dtype=np.int64), com_xy, int(window_size))
    if not keep.any():
        return None, None
    stack = stack[keep]
    return (stack[..., 0] if np.ndim(img) == 2 else stack), com_xy[keep]


def _draw_pixels(h: int, w: int, window_size: int, num_images: int) -> np.ndarray:
    """The reference's draws: scalar np.random.randint calls on numpy's GLOBAL state, row then column, repeats rejected."""
    lo = window_size // 2 + 1
    if num_images > max(h - 2 * lo, 0) * max(w - 2 * lo, 0):
        raise ValueError("Number of images cannot be greater than the number of pixels they can be centred on")
    seen, out = set(), []
    while len(out) < num_images:
        x = np.random.randint(lo, h - window_size // 2 - 1)
        y = np.random.randint(lo, w - window_size // 2 - 1)
        if (x, y) not in seen:
            seen.add((x, y))
            out.append((x, y))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def _draw_rows(n_rows: int, num_images: int) -> list:
    if num_images > n_rows:
        raise ValueError("Number of images cannot be greater than the available coordinates")
    seen, out = set(), []
    while len(out) < num_images:
        i = np.random.randint(n_rows)
        if i not in seen:
            seen.add(i)
            out.append(i)
    return out


def imcrop_randpx(img: np.ndarray, window_size: int, num_images: int, random_state: int = 0) -> Tuple[np.ndarray]:
    """``num_images`` windows of side ``window_size`` centred on distinct random pixels of one image (img.py:183-211):
    (windows, centres).  The draws come from numpy's global state (``np.random.seed`` reproduces the reference);
    ``random_state`` is unused, as in the reference."""
    h, w = np.shape(img)[:2]
    return _kept(img, _draw_pixels(h, w, int(window_size), int(num_images)), window_size)


def imcrop_randcoord(img: np.ndarray, coord: np.ndarray, window_size: int, num_images: int,
                     random_state: int = 0) -> Tuple[np.ndarray]:
    """``num_images`` windows centred on distinct random rows of ``coord`` (img.py:214-236): (windows, centres); a window
    that leaves the image or holds a NaN is dropped.  Draws as for ``imcrop_randpx``."""
    coord = np.asarray(coord)
    com_xy = np.array([coord[i].tolist() for i in _draw_rows(len(coord), int(num_images))])
    return _kept(img, com_xy, window_size)


def extract_random_subimages(imgdata: np.ndarray, window_size: int, num_images: int,
                             coordinates: Dict[int, np.ndarray] = None, **kwargs: int) -> Tuple[np.ndarray]:
    """``num_images`` random sub-images of every frame of a stack (n, h, w[, c]), centred on atoms of one class
    (``coordinates`` = the Locator's dictionary, ``**coord_class``, default 0; rows nearer than window_size // 2 + 1 to
    an edge are removed first) or on random pixels (img.py:239-295).  Returns float64 (windows (n * num_images, ws, ws,
    c), centres, frame numbers).  The draws are the reference's, frame by frame from numpy's global state; the windows of
    all frames are gathered by one launch.  A window dropped for a NaN, which makes the reference's block assignment
    fail, raises ``ValueError``; so does ``num_images`` above the available coordinates."""
    from .coords import remove_edge_coord
    imgdata = np.asarray(imgdata)
    if imgdata.ndim < 4:
        imgdata = imgdata[..., None]
    window_size, num_images = int(window_size), int(num_images)
    n, h, w = imgdata.shape[:3]
    centres = []
    for i in range(n):
        if coordinates is None:
            centres.append(_draw_pixels(h, w, window_size, num_images).astype(np.float64))
        else:
            coord = np.asarray(coordinates[i])
            coord = coord[coord[:, -1] == kwargs.get("coord_class", 0)][:, :2]
            coord = remove_edge_coord(coord, imgdata.shape[1:3], window_size // 2 + 1)
            centres.append(np.array([coord[r].tolist() for r in _draw_rows(len(coord), num_images)],
                                    dtype=np.float64).reshape(-1, 2))
    com_all = np.concatenate(centres, axis=0) if centres else np.zeros((0, 2))
    frames_all = np.repeat(np.arange(n), num_images).astype(np.float64)
    stack, keep = _centred(imgdata, frames_all.astype(np.int64), com_all, window_size)
    if not keep.all():
        bad = int(np.argmin(keep))
        raise ValueError(f"the window around {tuple(com_all[bad])} of frame {int(frames_all[bad])} holds a NaN or leaves "
                         "the frame; the reference fails here as well (its block assignment needs every window)")
    return stack.astype(np.float64), com_all, frames_all

"""numpy -> tensor plumbing for Segmentor and ImSpec training / prediction
(reference: atomai/utils/preproc.py:18-135, 138-362, 365-441, 798-854)."""
import warnings

import numpy as np
import torch


def num_classes_from_labels(labels: np.ndarray) -> int:
    """Number of classes from the label values: must be 0..K-1; two values mean ONE class (binary)."""
    uval = np.unique(labels)
    if min(uval) != 0:
        raise AssertionError("Labels should start from 0")
    if np.any(np.diff(uval) != 1):
        raise AssertionError("Mask values should be in range between 0 and total number of classes "
                             "with an increment of 1")
    k = len(uval)
    return k - 1 if k == 2 else k


def check_image_dims(X_train, y_train, X_test, y_test, num_classes: int):
    """Adds the channel axis to 3-D image stacks, and to 3-D masks in the single-class case."""
    def chan(a, what):
        if a.ndim == 3:
            warnings.warn(f'Adding a channel dimension of 1 to {what}', UserWarning)
            return a[:, None]
        return a
    X_train, X_test = chan(X_train, "training images"), chan(X_test, "test images")
    if num_classes == 1:
        y_train, y_test = chan(y_train, "training labels"), chan(y_test, "test labels")
    return X_train, y_train, X_test, y_test


def check_signal_dims(X_train, y_train, X_test, y_test):
    """ImSpec data: adds the channel axis of 1 to image stacks passed as (n, h, w) and spectra passed as (n, l).  Which
    side holds the images is read off the ranks: the features have more axes than the targets (im2spec) or fewer
    (spec2im); with equal ranks nothing is touched (atomai/utils/preproc.py:77-135)."""
    def chan(a, bare_ndim, what):
        if a.ndim == bare_ndim:
            warnings.warn(f'Adding a channel dimension of 1 to {what}', UserWarning)
            return a[:, None]
        return a
    if X_train.ndim == y_train.ndim:
        return X_train, y_train, X_test, y_test
    # as in the reference both messages name the features "images" and the targets "spectra"
    x_bare, y_bare = (3, 2) if X_train.ndim > y_train.ndim else (2, 3)
    X_train, X_test = chan(X_train, x_bare, "training images"), chan(X_test, x_bare, "test images")
    y_train, y_test = chan(y_train, y_bare, "training spectra"), chan(y_test, y_bare, "test spectra")
    out = (X_train, y_train, X_test, y_test)
    # (the reference compares the train / test shapes in its spec2im branch only; kept, so that the same calls raise)
    if X_train.ndim < y_train.ndim and (out[0].shape[1:] != out[2].shape[1:] or out[1].shape[1:] != out[3].shape[1:]):
        raise ValueError("The image/spectra dimensions must be the same for training and test data")
    return out


def get_array_memsize(X_arr, precision: str = "single") -> float:
    """Bytes the array takes once cast to single (or double) precision."""
    if X_arr is None:
        return 0
    if precision not in ("single", "double"):
        raise NotImplementedError("Specify 'single' or 'double' precision type")
    n = X_arr.numel() if isinstance(X_arr, torch.Tensor) else X_arr.size
    return n * (4 if precision == "single" else 8)


def _data_device(store_on_cpu: bool) -> str:
    return 'cuda' if torch.cuda.is_available() and not store_on_cpu else 'cpu'


def array2list_(x, batch_size: int, store_on_cpu: bool = False):
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise TypeError("Provide data as numpy array or torch tensor")
    if isinstance(x, torch.Tensor):
        x = x.to(_data_device(store_on_cpu))
    n_batches = x.shape[0] // batch_size
    split = np.split if isinstance(x, np.ndarray) else torch.chunk
    return split(x[:n_batches * batch_size], n_batches)


def array2list(X_train, y_train, X_test, y_test, batch_size: int, memory_alloc: float = 4):
    """Lists of whole mini-batches (remainder dropped); device-resident if the set is < memory_alloc GB."""
    data = [X_train, y_train, X_test, y_test]
    on_cpu = sum(get_array_memsize(x) for x in data) / 1e9 > memory_alloc
    return tuple(array2list_(x, batch_size, on_cpu) for x in data)


def preprocess_training_image_data_(images_all, labels_all, images_test_all, labels_test_all):
    data = (images_all, labels_all, images_test_all, labels_test_all)
    all_np = all(isinstance(i, np.ndarray) for i in data)
    all_t = all(isinstance(i, torch.Tensor) for i in data)
    if not all_np and not all_t:
        raise TypeError("Provide training and test data in the form of numpy arrays or torch tensors")
    num_classes = num_classes_from_labels(labels_all if all_np else labels_all.cpu().numpy())
    X, y, Xt, yt = check_image_dims(*data, num_classes)
    if all_np:
        X, y, Xt, yt = (torch.from_numpy(np.ascontiguousarray(a)) for a in (X, y, Xt, yt))
    X, Xt = X.float(), Xt.float()
    y, yt = (y.long(), yt.long()) if num_classes > 1 else (y.float(), yt.float())
    return X, y, Xt, yt, num_classes


def preprocess_training_image_data(images_all, labels_all, images_test_all, labels_test_all,
                                   batch_size: int, memory_alloc: float = 4):
    *tensors, num_classes = preprocess_training_image_data_(
        images_all, labels_all, images_test_all, labels_test_all)
    return (*array2list(*tensors, batch_size, memory_alloc), num_classes)


def init_dataloaders(X_train, y_train, X_test, y_test, batch_size: int, memory_alloc: float = 4):
    on_cpu = sum(get_array_memsize(x) for x in (X_train, y_train, X_test, y_test)) / 1e9 > memory_alloc
    dev = _data_device(on_cpu)
    tr = torch.utils.data.TensorDataset(X_train.to(dev), y_train.to(dev))
    te = torch.utils.data.TensorDataset(X_test.to(dev), y_test.to(dev))
    return (torch.utils.data.DataLoader(tr, batch_size=batch_size, shuffle=True, drop_last=True),
            torch.utils.data.DataLoader(te, batch_size=batch_size, drop_last=True))


def init_fcnn_dataloaders(X_train, y_train, X_test, y_test, batch_size: int, num_classes=None,
                          memory_alloc: float = 4):
    *tensors, num_classes = preprocess_training_image_data_(X_train, y_train, X_test, y_test)
    return (*init_dataloaders(*tensors, batch_size, memory_alloc), num_classes)


def preprocess_training_imspec_data_(X_train, y_train, X_test, y_test):
    """float32 tensors with a channel axis + ((input dims), (output dims)) (atomai/utils/preproc.py:281-313)."""
    data = (X_train, y_train, X_test, y_test)
    all_np = all(isinstance(i, np.ndarray) for i in data)
    all_t = all(isinstance(i, torch.Tensor) for i in data)
    if not all_np and not all_t:
        raise TypeError("Provide training and test data in the form of numpy arrays or torch tensors")
    X, y, Xt, yt = check_signal_dims(*data)
    dims = (tuple(X.shape[2:]), tuple(y.shape[2:]))
    if all_np:
        X, y, Xt, yt = (torch.from_numpy(np.ascontiguousarray(a)) for a in (X, y, Xt, yt))
    return X.float(), y.float(), Xt.float(), yt.float(), dims


def preprocess_training_imspec_data(X_train, y_train, X_test, y_test, batch_size: int, memory_alloc: float = 4):
    """Lists of whole mini-batches for the im2spec / spec2im trainers + the data's (in_dim, out_dim)
    (atomai/utils/preproc.py:316-362)."""
    *tensors, dims = preprocess_training_imspec_data_(X_train, y_train, X_test, y_test)
    return (*array2list(*tensors, batch_size, memory_alloc), dims)


def init_imspec_dataloaders(X_train, y_train, X_test, y_test, batch_size: int, memory_alloc: float = 4):
    """(train loader, test loader, (in_dim, out_dim)) (atomai/utils/preproc.py:424-441)."""
    *tensors, dims = preprocess_training_imspec_data_(X_train, y_train, X_test, y_test)
    return (*init_dataloaders(*tensors, batch_size, memory_alloc), dims)


def preprocess_denoiser_data(X_train, y_train, X_test, y_test):
    """Noisy / clean image pairs for the denoising autoencoder as float32 tensors (n, 1, h, w)
    (atomai/utils/preproc.py:698-758): numpy arrays or torch tensors, all of one kind; a stack without the channel axis
    gains one, with a warning; a noisy stack and its clean stack must agree in shape."""
    data = (X_train, y_train, X_test, y_test)
    all_np = all(isinstance(i, np.ndarray) for i in data)
    all_t = all(isinstance(i, torch.Tensor) for i in data)
    if not all_np and not all_t:
        raise TypeError("Provide training and test data in the form of numpy arrays or torch tensors")
    out = []
    for a, what in zip(data, ("noisy training", "clean training", "noisy test", "clean test")):
        if a.ndim == 3:
            warnings.warn(f"Adding channel dimension of 1 to {what} images", UserWarning)
            a = a[:, None]
        out.append((torch.from_numpy(a) if all_np else a).float())
    if out[0].shape != out[1].shape:
        raise ValueError("Noisy and clean training images must have the same shape")
    if out[2].shape != out[3].shape:
        raise ValueError("Noisy and clean test images must have the same shape")
    return tuple(out)


def torch_format_spectra(spectra: np.ndarray, norm: bool = False) -> torch.Tensor:
    """(n, l) -> float32 (n, 1, l); optional global min-max normalisation over the WHOLE stack
    (atomai/utils/preproc.py:828-854)."""
    if spectra.ndim not in (2, 3):
        raise AssertionError("Provide spectrum(s) as 2D (n, length) or 3D (n, 1, length) tensor")
    if spectra.ndim == 2:
        spectra = spectra[:, None]
    elif spectra.shape[1] != 1:
        raise AssertionError("3D spectra tensor must have (n, 1, length) dimensions")
    if norm:
        spectra = (spectra - spectra.min()) / np.ptp(spectra)
    return torch.from_numpy(np.ascontiguousarray(spectra)).float()


def torch_format_image(image_data: np.ndarray, norm: bool = True) -> torch.Tensor:
    """(n,h,w) -> float32 (n,1,h,w); global min-max normalisation over the WHOLE stack."""
    if image_data.ndim not in (3, 4):
        raise AssertionError("Provide image(s) as 3D (n, h, w) or 4D (n, 1, h, w) tensor")
    if image_data.ndim == 3:
        image_data = image_data[:, None]
    if norm:
        image_data = (image_data - image_data.min()) / np.ptp(image_data)
    return torch.from_numpy(np.ascontiguousarray(image_data)).float()


def to_onehot(idx: torch.Tensor, n: int) -> torch.Tensor:
    """One-hot encoding of integer labels (reference: atomai/utils/preproc.py:915-928; the reference allocates on
    'cuda' whenever CUDA exists, here the result lives on the labels' own device)."""
    if torch.max(idx).item() >= n:
        raise AssertionError("Labelling must start from 0 and "
                             "maximum label value must be less than total number of classes")
    if idx.dim() == 1:
        idx = idx.unsqueeze(1)
    onehot = torch.zeros(idx.size(0), int(n), device=idx.device)
    onehot.scatter_(1, idx.long(), 1)
    return onehot

"""Sliding-window FFT with NMF unmixing (atomai/stat/fft_nmf.py), on the device: csrc/fftwin.hip evaluates the cropped
spectrum of every window, csrc/nmf.hip factorises the feature matrix.  No scipy, scikit-learn or skimage dependency."""
import numpy as np

from . import _nmf


class SlidingFFTNMF:
    """Sliding window FFT whose output is unmixed by NMF.

    Args:
        window_size_x, window_size_y: window dimensions; None: from the image size (a power of two between 32 and 128)
        window_step_x, window_step_y: step of the sliding windows; None: window_size // 4
        interpolation_factor: factor of the linear interpolation of the cropped spectrum (applied if > 1)
        zoom_factor: the central 1 / zoom_factor of the shifted spectrum is kept
        hamming_filter: multiply every window by a Hamming table first (square windows only)
        components: number of NMF components

    Windows of up to 128 x 128 pixels are supported.
    """

    def __init__(self, window_size_x=None, window_size_y=None, window_step_x=None, window_step_y=None,
                 interpolation_factor=2, zoom_factor=2, hamming_filter=True, components=4):
        self._user_window_size_x = window_size_x
        self._user_window_size_y = window_size_y
        self._user_window_step_x = window_step_x
        self._user_window_step_y = window_step_y
        self.interpol_factor = interpolation_factor
        self.zoom_factor = zoom_factor
        self.hamming_filter = hamming_filter
        self.components = components
        self.hamming_window = None

    def _calculate_window_params(self, image_shape):
        """Window and step sizes from the image dimensions (the user's values where given), and the Hamming table."""
        height, width = image_shape[:2]
        if self._user_window_size_x is None:
            self.window_size_x = 2 ** int(np.log2(max(32, min(128, height // 8))))
        else:
            self.window_size_x = self._user_window_size_x
        if self._user_window_size_y is None:
            self.window_size_y = 2 ** int(np.log2(max(32, min(128, width // 8))))
        else:
            self.window_size_y = self._user_window_size_y
        self.window_step_x = (max(1, self.window_size_x // 4) if self._user_window_step_x is None
                              else self._user_window_step_x)
        self.window_step_y = (max(1, self.window_size_y // 4) if self._user_window_step_y is None
                              else self._user_window_step_y)
        if self.window_size_x > height:
            self.window_size_x = min(64, height)
            self.window_step_x = max(1, self.window_size_x // 4)
        if self.window_size_y > width:
            self.window_size_y = min(64, width)
            self.window_step_y = max(1, self.window_size_y // 4)
        if max(self.window_size_x, self.window_size_y) > _nmf.FFT_WINDOW_MAX:
            raise ValueError(f"windows above {_nmf.FFT_WINDOW_MAX} x {_nmf.FFT_WINDOW_MAX} pixels are not supported on "
                             f"the device, got {self.window_size_x} x {self.window_size_y}")
        if self.hamming_filter:
            if self.window_size_x != self.window_size_y:
                raise ValueError("hamming_filter=True needs a square window (the reference's table is "
                                 f"sqrt(h h^T)), got {self.window_size_x} x {self.window_size_y}")
            bw2d = np.outer(np.hamming(self.window_size_x), np.ones(self.window_size_y))
            self.hamming_window = np.sqrt(bw2d * bw2d.T)
        else:
            self.hamming_window = None

    def _normalised(self, image):
        """Grey, float64, scaled to 0 .. 1; sets the window parameters, the window grid and the position vectors."""
        image = np.asarray(image)
        if image.ndim > 2:
            if image.shape[2] >= 3:                             # Rec. 709 luma of the first three channels
                rgb = image[:, :, :3].astype(np.float64)
                image = 0.2125 * rgb[..., 0] + 0.7154 * rgb[..., 1] + 0.0721 * rgb[..., 2]
            else:
                image = np.mean(image, axis=2)
        self._calculate_window_params(image.shape)
        image = image.astype(float)
        if np.max(image) > 0:
            image = (image - np.min(image)) / (np.max(image) - np.min(image))
        if image.shape[0] < self.window_size_x or image.shape[1] < self.window_size_y:
            raise ValueError(f"Image dimensions {image.shape} are smaller than window size "
                             f"({self.window_size_x}, {self.window_size_y})")
        n0 = (image.shape[0] - self.window_size_x) // self.window_step_x + 1
        n1 = (image.shape[1] - self.window_size_y) // self.window_step_y + 1
        self.windows_shape = (n0, n1)
        xx, yy = np.meshgrid(np.arange(0, n1 * self.window_step_y, self.window_step_y),
                             np.arange(0, n0 * self.window_step_x, self.window_step_x))
        self.pos_vec = np.column_stack((yy.flatten(), xx.flatten()))
        return np.ascontiguousarray(image)

    def make_windows(self, image):
        """The (n, window_size_x, window_size_y) stack of the sliding windows of the normalised image (host numpy)."""
        image = self._normalised(image)
        size = (self.window_size_x, self.window_size_y)
        windows = np.lib.stride_tricks.sliding_window_view(image, size)[::self.window_step_x, ::self.window_step_y]
        return windows.reshape(-1, size[0], size[1])

    def _features(self, data, grid=None):
        feats, self.fft_size = _nmf.fft_features(
            data, (self.window_size_x, self.window_size_y), grid, (self.window_step_x, self.window_step_y),
            self.hamming_window if self.hamming_filter else None, self.zoom_factor, self.interpol_factor)
        return feats

    def process_fft(self, windows):
        """Log-magnitude spectrum of every window of the (n, wx, wy) stack: Hamming table, fft2, fftshift, abs, log1p,
        centre crop, linear interpolation.  Returns an (n, fx, fy) float64 array."""
        windows = np.asarray(windows)
        if not hasattr(self, "window_size_x"):
            raise AttributeError("call make_windows (or analyze_image) first: the window sizes are not set")
        feats = self._features(windows)
        return feats.cpu().numpy().reshape(windows.shape[0], *self.fft_size)

    def run_nmf(self, fft_results):
        """NMF of the (n, fx, fy) spectra (array or the device feature matrix): (components (k, fx, fy), abundances
        (windows down, windows across, k))."""
        flat = fft_results if hasattr(fft_results, "is_cuda") else np.asarray(fft_results)
        flat = flat.reshape(flat.shape[0], -1)
        if flat.shape[0] < self.components:
            self.components = min(flat.shape[0], 3)
        if not hasattr(flat, "is_cuda"):
            flat = np.maximum(0, flat)
            if np.all(flat == 0) or not np.isfinite(flat).all():
                raise ValueError("Invalid data for NMF: contains zeros, NaNs or Infs")
        res = _nmf.fit_nmf(flat, self.components, init="random", random_state=42, max_iter=1000, tol=1e-4)
        components = res["H"].cpu().numpy().reshape(self.components, self.fft_size[0], self.fft_size[1])
        abundances = res["W"].cpu().numpy().reshape(self.windows_shape[0], self.windows_shape[1], self.components)
        return components, abundances

    def analyze_image(self, image_input, output_path=None):
        """The whole pipeline for an image array: returns (components (k, fx, fy), abundances (k, windows down, windows
        across)) and saves both as ``{output_path}_components.npy`` / ``_abundances.npy`` (default "array_analysis").
        The windows are read in place from the normalised image; the window stack is never built."""
        if isinstance(image_input, str):
            raise NotImplementedError("reading an image file is not implemented (there is no image reader here): "
                                      "pass the image as a numpy array")
        if not isinstance(image_input, np.ndarray):
            raise TypeError("image_input must be a numpy array")
        self.image_path = "numpy_array_input"
        if output_path is None:
            output_path = "array_analysis"
        image = self._normalised(image_input.copy())
        feats = self._features(image, self.windows_shape)
        components, abundances = self.run_nmf(feats)
        abundances = abundances.transpose(-1, 0, 1)
        np.save(f"{output_path}_components.npy", components)
        np.save(f"{output_path}_abundances.npy", abundances)
        return components, abundances

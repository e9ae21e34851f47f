from .dgm import VAE, BaseVAE, jrVAE, jVAE, rVAE
from .dklgp import dklGPR
from .denoiser import DenoisingAutoencoder, denoise_images, init_denoising_autoencoder
from .imspec import ImSpec
from .segmentor import Segmentor
from .loaders import (load_ensemble, load_denoising_autoencoder, load_imspec_model, load_model, load_pretrained_model,  # noqa: E402
                      load_seg_model, load_vae_model)

__all__ = ["Segmentor", "ImSpec", "DenoisingAutoencoder", "denoise_images", "init_denoising_autoencoder", "BaseVAE", "VAE", "rVAE", "jVAE", "jrVAE", "dklGPR", "load_model", "load_ensemble", "load_pretrained_model",
           "load_seg_model", "load_imspec_model", "load_denoising_autoencoder", "load_vae_model"]

"""Checkpoint loaders (reference: atomai/models/loaders.py:25-195, 236-292).

The ``*_metadict_final.tar`` files written by the trainers (trainers/trainer.py ``save_model`` here,
atomai/trainers/trainer.py:344-358 and atomai/trainers/vitrainer.py:361-377 in the reference) are plain
``torch.save`` pickles of {architecture kwargs, weights, optimizer}.  Both directions interchange: a file
written by the reference loads here onto the HIP modules (same state-dict keys / shapes), and files written
here hold only torch types (the fused optimizer is stored as its ``torch.optim.Adam`` equivalent).

"denoising_autoencoder" checkpoints rebuild a DenoisingAutoencoder (load_denoising_autoencoder; a file without the
"use_batch_norm" entry is rebuilt WITH BatchNorm, as the reference's loader does).  Model families outside SURVEY.md
section 8 (reg / cls: torchvision backbones) raise, and so do ImSpec and denoiser ensembles.
"""
import warnings
from copy import deepcopy as dc
from typing import Dict, Tuple, Type, Union

import torch

from ..utils import average_weights
from .denoiser import DenoisingAutoencoder
from .dgm import VAE, BaseVAE, jrVAE, jVAE, rVAE
from .imspec import ImSpec
from .segmentor import Segmentor

_OUT_OF_SCOPE = ("reg", "cls")


def _read(filepath: str) -> Dict:
    device = "cuda" if torch.cuda.is_available() else "cpu"
    return torch.load(filepath, map_location=device, weights_only=False)


def load_model(filepath: str) -> Union[Segmentor, BaseVAE, Dict[str, torch.Tensor]]:
    """Rebuilds a trained model (evaluation state) from a meta-state dictionary file."""
    loaded = _read(filepath)
    if "model_type" not in loaded:
        warnings.warn("Returning model's state dictionary. You will need to load it into your model's "
                      "skeleton by yourself", UserWarning)
        return loaded["weights"]
    model_type = loaded.pop("model_type")
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", category=UserWarning)
        if model_type == "seg":
            return load_seg_model(loaded)
        if model_type == "vae":
            return load_vae_model(loaded)
        if model_type == "imspec":
            return load_imspec_model(loaded)
        if model_type == "denoising_autoencoder":
            return load_denoising_autoencoder(loaded)
    if model_type in _OUT_OF_SCOPE:
        raise NotImplementedError(f"model type '{model_type}' is outside the MI355X hot path of this build")
    raise ValueError("The model type {} cannot be loaded".format(model_type))


def load_seg_model(meta_dict: Dict) -> Type[Segmentor]:
    """Segmentor from {model, nb_classes, weights, [optimizer], **architecture kwargs}."""
    name = meta_dict.pop("model")
    nb_classes = meta_dict.pop("nb_classes")
    weights = meta_dict.pop("weights")
    model = Segmentor(name, nb_classes, **meta_dict)
    model.net.load_state_dict(weights)
    if "optimizer" in meta_dict:
        model.optimizer = meta_dict.pop("optimizer")
    model.net.eval()
    return model


def load_imspec_model(meta_dict: Dict) -> Type[ImSpec]:
    """ImSpec from {in_dim, out_dim, latent_dim, weights, [optimizer], **architecture kwargs}, written here or by the
    reference.  Deviation: the reference's loader drops its own "batchnorm" entry (atomai/models/loaders.py), so a model
    trained with batch_norm=False is rebuilt WITH BatchNorm there and its weights fail to load; here the entry is mapped
    to the ``batch_norm`` argument."""
    in_dim = meta_dict.pop("in_dim")
    out_dim = meta_dict.pop("out_dim")
    latent_dim = meta_dict.pop("latent_dim")
    weights = meta_dict.pop("weights")
    if "batchnorm" in meta_dict:
        meta_dict["batch_norm"] = meta_dict.pop("batchnorm")
    optimizer = meta_dict.pop("optimizer", None)
    model = ImSpec(in_dim, out_dim, latent_dim, **meta_dict)
    model.net.load_state_dict(weights)
    if optimizer is not None:
        model.optimizer = optimizer
    model.net.eval()
    return model


def load_denoising_autoencoder(meta_dict: Dict) -> Type[DenoisingAutoencoder]:
    """DenoisingAutoencoder from {encoder_filters, decoder_filters, encoder_layers, decoder_layers, use_batch_norm,
    upsampling_mode, weights, [optimizer]}, written here or by the reference; absent entries take the reference loader's
    defaults (atomai/models/loaders.py:212-217: ``use_batch_norm`` True, unlike the constructor's False)."""
    arch = dict(encoder_filters=meta_dict.pop("encoder_filters", [8, 16, 32, 64]),
                decoder_filters=meta_dict.pop("decoder_filters", [64, 32, 16, 8]),
                encoder_layers=meta_dict.pop("encoder_layers", [1, 2, 2, 2]),
                decoder_layers=meta_dict.pop("decoder_layers", [2, 2, 2, 1]),
                use_batch_norm=meta_dict.pop("use_batch_norm", True),
                upsampling_mode=meta_dict.pop("upsampling_mode", "nearest"))
    weights = meta_dict.pop("weights")
    optimizer = meta_dict.pop("optimizer", None)
    model = DenoisingAutoencoder(**arch, **meta_dict)
    model.net.load_state_dict(weights)
    if optimizer is not None:
        model.optimizer = optimizer
    model.net.eval()
    return model


def load_vae_model(meta_dict: Dict) -> Type[BaseVAE]:
    """VAE / rVAE / jVAE / jrVAE from {in_dim, latent_dim, coord, encoder, decoder, optimizer, **kwargs}."""
    in_dim = meta_dict.pop("in_dim")
    latent_dim = meta_dict.pop("latent_dim")
    enc_w, dec_w = meta_dict.pop("encoder"), meta_dict.pop("decoder")
    coord = meta_dict.pop("coord")
    optimizer = meta_dict.pop("optimizer")
    joint = bool(meta_dict.get("discrete_dim"))
    if coord:
        m = (jrVAE if joint else rVAE)(in_dim, latent_dim, translation=(coord == 3), **meta_dict)
    else:
        m = (jVAE if joint else VAE)(in_dim, latent_dim, **meta_dict)
    if joint:                                                # the capacity schedule resumes where training stopped
        m.kdict_["num_iter"] = meta_dict.get("num_iter", 0)
    m.encoder_net.load_state_dict(enc_w)
    m.encoder_net.eval()
    m.decoder_net.load_state_dict(dec_w)
    m.decoder_net.eval()
    m.optim = optimizer
    return m


def load_ensemble(filepath: str) -> Tuple[Type[torch.nn.Module], Dict[int, Dict[str, torch.Tensor]]]:
    """Single model with the ensemble-averaged weights + the dictionary of all members' weights."""
    loaded = _read(filepath)
    if "model_type" not in loaded:
        warnings.warn("Returning dictionary with ensemble weights. You will need to load them into your "
                      "model's skeleton by yourself")
        return None, dc(loaded["weights"])
    model_type = loaded.pop("model_type")
    ensemble_weights = dc(loaded["weights"])
    loaded["weights"] = average_weights(loaded["weights"])
    if model_type == "seg":
        smodel = load_seg_model(loaded)
    elif model_type == "imspec":
        raise NotImplementedError("ImSpec ensembles are outside the MI355X hot path of this build "
                                  "(single ImSpec models load with load_model)")
    elif model_type == "denoising_autoencoder":
        raise NotImplementedError("denoiser ensembles are outside the MI355X hot path of this build "
                                  "(single DenoisingAutoencoder models load with load_model)")
    elif model_type in _OUT_OF_SCOPE:
        raise NotImplementedError(f"model type '{model_type}' is outside the MI355X hot path of this build")
    else:
        raise ValueError("The model type {} cannot be loaded".format(model_type))
    return smodel.net, ensemble_weights


def load_pretrained_model(model_name: str):
    """'G_MD' / 'BFO' pretrained Segmentors.  The reference downloads them (loaders.py:274-292); this build
    runs without network access, so the ``.tar`` must already be in the working directory."""
    import os
    fname = {"BFO": "./bfo.tar", "G_MD": "./G_MD.tar"}.get(model_name)
    if fname is None:
        raise ValueError("Available pretrained models are 'G_MD' and 'BFO'")
    if not os.path.exists(fname):
        raise FileNotFoundError(f"{fname} not found: download it from the reference's 'pretrained' folder")
    return load_model(fname)

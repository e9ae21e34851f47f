from .blocks import ConvBlock, DilatedBlock, ResBlock, ResModule, UpsampleBlock
from .ed import SignalDecoder, SignalED, SignalEncoder, init_imspec_model, convDecoderNet, convEncoderNet, coord_latent, fcDecoderNet, fcEncoderNet, init_VAE_nets, jconvEncoderNet, jfcEncoderNet, rDecoderNet
from .fcnn import ResHedNet, SegResNet, Unet, dilnet, init_fcnn_model
from .denoiser import DenoiserNet
from .gp import GPRegressionModel, convFeatureExtractor, fcFeatureExtractor

__all__ = ["ConvBlock", "UpsampleBlock", "DilatedBlock", "ResBlock", "ResModule", "Unet", "dilnet", "SegResNet", "ResHedNet",
           "init_fcnn_model", "DenoiserNet",
           "fcEncoderNet", "convEncoderNet", "jfcEncoderNet", "jconvEncoderNet", "convDecoderNet", "fcDecoderNet", "rDecoderNet", "coord_latent", "init_VAE_nets",
           "SignalEncoder", "SignalDecoder", "SignalED", "init_imspec_model",
           "fcFeatureExtractor", "convFeatureExtractor", "GPRegressionModel"]

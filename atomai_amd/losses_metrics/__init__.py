from .losses import BCEWithLogitsLoss, CrossEntropyLoss, MSELoss, dice_loss, focal_loss, select_loss
from .metrics import IoU
from .vi_losses import (elbo_terms, infocapacity, joint_rvae_loss, joint_vae_loss, kld_discrete, rvae_loss,
                        vae_loss)

__all__ = ["select_loss", "CrossEntropyLoss", "BCEWithLogitsLoss", "MSELoss", "dice_loss", "focal_loss", "vae_loss", "rvae_loss", "infocapacity",
           "joint_vae_loss", "joint_rvae_loss", "kld_discrete", "elbo_terms", "IoU"]

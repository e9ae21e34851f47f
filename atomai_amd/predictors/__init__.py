from .epredictor import EnsemblePredictor, ensemble_locate
from .locator import Locator
from .predictor import BasePredictor, ImSpecPredictor, SegPredictor

__all__ = ["BasePredictor", "SegPredictor", "ImSpecPredictor", "Locator", "EnsemblePredictor", "ensemble_locate"]

from .etrainer import BaseEnsembleTrainer, EnsembleTrainer
from .gptrainer import dklGPTrainer
from .trainer import BaseTrainer, ImSpecTrainer, SegTrainer
from .vitrainer import viBaseTrainer

__all__ = ["BaseTrainer", "SegTrainer", "ImSpecTrainer", "viBaseTrainer", "dklGPTrainer", "BaseEnsembleTrainer", "EnsembleTrainer"]

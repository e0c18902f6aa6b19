from .AT import Attention
from .KD import DistillKL
from .NST import NSTLoss

__all__ = ["Attention", "DistillKL", "NSTLoss"]

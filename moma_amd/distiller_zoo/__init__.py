from .AT import Attention
from .KD import DistillKL

__all__ = ["Attention", "DistillKL"]

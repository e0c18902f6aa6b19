from .AT import Attention
from .CC import Correlation, LinearEmbed
from .FitNet import ConvReg, HintLoss
from .KD import DistillKL
from .NST import NSTLoss
from .PKT import PKT
from .RKD import RKDLoss
from .SemCKD import MLPEmbed, Proj, SelfA, SemCKDLoss
from .SP import Similarity
from .SRRL import SRRL
from .VID import VIDLoss

__all__ = ["Attention", "ConvReg", "Correlation", "DistillKL", "HintLoss", "LinearEmbed", "MLPEmbed", "NSTLoss", "PKT", "Proj", "RKDLoss",
           "SRRL", "SelfA", "SemCKDLoss", "Similarity", "VIDLoss"]

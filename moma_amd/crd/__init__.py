"""Contrastive Representation Distillation (`--distill crd`): the reference's crd/ package names (ContrastMemory, AliasMethod,
CRDLoss, ContrastLoss, Embed, Normalize) over the gather-contrast kernels of libmoma_hip.so (csrc/crd.hip)."""
from .criterion import CRDLoss, ContrastLoss, Embed, Normalize  # noqa: F401
from .memory import AliasMethod, ContrastMemory  # noqa: F401

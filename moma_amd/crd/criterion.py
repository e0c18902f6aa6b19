"""CRD loss (reference crd/criterion.py): two embedding heads, the memory banks, and the contrastive loss of both sides."""
import torch
from torch import nn

from .memory import ContrastMemory

eps = 1e-7


class CRDLoss(nn.Module):
    """opt.s_dim / opt.t_dim: feature widths of student / teacher; opt.feat_dim: width of the embedding; opt.nce_k negatives per
    positive; opt.nce_t temperature; opt.nce_m momentum of the banks; opt.n_data samples in the training set (rows of the banks).
    opt.moma_fused (default True): one fused gather pass for loss and gradient; False: the reference sequence -- materialised
    scores -> ContrastLoss -- on the same kernels' materialised form."""

    def __init__(self, opt):
        super().__init__()
        self.embed_s = Embed(opt.s_dim, opt.feat_dim)
        self.embed_t = Embed(opt.t_dim, opt.feat_dim)
        self.contrast = ContrastMemory(opt.feat_dim, opt.n_data, opt.nce_k, opt.nce_t, opt.nce_m)
        self.criterion_t = ContrastLoss(opt.n_data)
        self.criterion_s = ContrastLoss(opt.n_data)
        self.fused = bool(getattr(opt, "moma_fused", True))

    def forward(self, f_s, f_t, idx, contrast_idx=None):
        """f_s [B, s_dim], f_t [B, t_dim], idx [B] sample indices, contrast_idx [B, nce_k + 1] (column 0 = idx) or None"""
        f_s = self.embed_s(f_s).float()
        f_t = self.embed_t(f_t).float()
        if self.fused:
            return self.contrast.forward_fused(f_s, f_t, idx, contrast_idx)
        out_s, out_t = self.contrast(f_s, f_t, idx, contrast_idx)
        return self.criterion_s(out_s) + self.criterion_t(out_t)


class ContrastLoss(nn.Module):
    """the noise-contrastive loss of one side over materialised scores x [B, K+1, 1], column 0 the positive"""

    def __init__(self, n_data):
        super().__init__()
        self.n_data = n_data

    def forward(self, x):
        B, m = x.shape[0], x.size(1) - 1
        c = m / float(self.n_data)
        pos, neg = x.select(1, 0), x.narrow(1, 1, m)
        log_d1 = torch.log(pos / (pos + (c + eps)))
        log_d0 = torch.log(c / (neg + (c + eps)))
        return -(log_d1.sum(0) + log_d0.reshape(-1, 1).sum(0)) / B


class Embed(nn.Module):
    """linear projection + L2 normalisation"""

    def __init__(self, dim_in=1024, dim_out=128):
        super().__init__()
        self.linear = nn.Linear(dim_in, dim_out)
        self.l2norm = Normalize(2)

    def forward(self, x):
        return self.l2norm(self.linear(x.view(x.shape[0], -1)))


class Normalize(nn.Module):
    def __init__(self, power=2):
        super().__init__()
        self.power = power

    def forward(self, x):
        return x / x.pow(self.power).sum(1, keepdim=True).pow(1. / self.power)

"""Attention Transfer (Zagoruyko & Komodakis, "Paying More Attention to Attention", ICLR 2017) -- the criterion of
`--distill attention` (reference distiller_zoo/AT.py; loop branch helper/loops_moma.py:287-292).

Per feature pair: spatial attention map a = mean_c f^p, flattened and L2-normalised per image; loss = mean((ah_s - ah_t)^2); when the
heights differ the larger map is average-pooled to (h, h), h the smaller height.  For p = 2 on GPU tensors in float32 / bfloat16 the
pair runs on the fused kernels of csrc/attention.hip (ops.attention_loss: one read of each map forward, one read + one write of the
student's map backward, NCHW or channels_last as they come).  CPU tensors, float16 storage and p != 2 take the same formula in stock
torch ops.  The formula needs [B, C, H, W] maps: token lists (the ViT backbones) are refused."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


class Attention(nn.Module):
    def __init__(self, p=2):
        super().__init__()
        self.p = p

    def forward(self, g_s, g_t):
        """lists of feature maps -> list of per-pair losses (as many as the shorter list)"""
        return [self.at_loss(f_s, f_t) for f_s, f_t in zip(g_s, g_t)]

    def at_loss(self, f_s, f_t):
        if f_s.dim() != 4 or f_t.dim() != 4:
            raise ValueError("Attention transfer compares [B, C, H, W] feature maps; got {} and {} (the token lists of a ViT backbone "
                             "have no spatial attention map in this formula)".format(tuple(f_s.shape), tuple(f_t.shape)))
        if (self.p == 2 and f_s.is_cuda and f_t.is_cuda and f_s.dtype in _KERNEL_DTYPES and f_t.dtype in _KERNEL_DTYPES):
            return ops.attention_loss(f_s, f_t)
        return self.composite(f_s, f_t)

    def composite(self, f_s, f_t):
        """the same formula in stock torch ops, evaluated in float32 (or wider when the maps are)"""
        hs, ht = f_s.shape[2], f_t.shape[2]
        if hs != ht:
            h = min(hs, ht)
            if hs > ht:
                f_s = F.adaptive_avg_pool2d(f_s, (h, h))
            else:
                f_t = F.adaptive_avg_pool2d(f_t, (h, h))
        a_s, a_t = self.at(f_s), self.at(f_t)
        return (a_s - a_t).square().mean()

    def at(self, f):
        """[B, C, H, W] -> [B, H W]: channel mean of f^p, L2-normalised per image"""
        if f.dtype in (torch.float16, torch.bfloat16):
            f = f.float()
        return F.normalize(f.pow(self.p).mean(dim=1).flatten(1), dim=1, eps=1e-12)

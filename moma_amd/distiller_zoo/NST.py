"""Neuron Selectivity Transfer (Huang & Wang, "Like What You Like: Knowledge Distill via Neuron Selectivity Transfer", 2017) -- the
criterion of `--distill nst` (reference distiller_zoo/NST.py; loop branch helper/loops_moma.py:150-154).

Per feature pair: both maps on a common grid (the larger one average-pooled to (h, h), h the smaller height), every channel
flattened over the pixels and L2-normalised; loss = mean (x_i . x_j)^2 - 2 mean (x_i . y_j)^2 over the student-student and
student-teacher channel pairs of every image (the polynomial-kernel MMD without its teacher-teacher term, which carries no
gradient: the reference's `full_loss = False`).  On GPU tensors in float32 / bfloat16 with at most 256 channels per side the pair
runs on the fused kernels of csrc/nst.hip (ops.nst_loss: one read of each map forward and backward, a [B, Cs, Cs + Ct] Gram as the
only temporary, NCHW or channels_last as they come).  CPU tensors, float16 storage, wider maps and a teacher map that wants a
gradient take the same formula in stock torch ops, written with bmm (the reference's broadcast product is a [B, Ct, Cs, H W]
temporary) and evaluated in float64.  The formula needs [B, C, H, W] maps: token lists (the ViT backbones) are refused."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


class NSTLoss(nn.Module):
    def forward(self, g_s, g_t):
        """lists of feature maps -> list of per-pair losses (as many as the shorter list)"""
        return [self.nst_loss(f_s, f_t) for f_s, f_t in zip(g_s, g_t)]

    def nst_loss(self, f_s, f_t):
        if f_s.dim() != 4 or f_t.dim() != 4:
            raise ValueError("Neuron selectivity transfer compares [B, C, H, W] feature maps; got {} and {} (the token lists of a ViT "
                             "backbone have no channel-by-pixel activation pattern in this formula)".format(tuple(f_s.shape), tuple(f_t.shape)))
        if (f_s.is_cuda and f_t.is_cuda and f_s.dtype in _KERNEL_DTYPES and f_t.dtype in _KERNEL_DTYPES
                and max(f_s.shape[1], f_t.shape[1]) <= _lib.NST_MAX_C and not (f_t.requires_grad and torch.is_grad_enabled())):
            return ops.nst_loss(f_s, f_t)
        return self.composite(f_s, f_t)

    def composite(self, f_s, f_t, dtype=torch.float64):
        """the same formula in stock torch ops, evaluated in `dtype` and returned in float32 (float64 maps: in float64).  float64
        unless told otherwise: where the channels resemble each other (maps far from zero mean) the gradient is what is left of a
        sum ten times its size, and the fp32 chains of a BLAS bmm lose twice what the reference's pairwise sums do"""
        hs, ht = f_s.shape[2], f_t.shape[2]
        if hs > ht:
            f_s = F.adaptive_avg_pool2d(f_s, (ht, ht))
        elif hs < ht:
            f_t = F.adaptive_avg_pool2d(f_t, (hs, hs))
        x, y = self.rows(f_s, dtype), self.rows(f_t, dtype)
        loss = torch.bmm(x, x.transpose(1, 2)).square().mean() - 2 * torch.bmm(x, y.transpose(1, 2)).square().mean()
        return loss if f_s.dtype == torch.float64 else loss.float()

    @staticmethod
    def rows(f, dtype=torch.float64):
        """[B, C, H, W] -> [B, C, H W] in `dtype` (never narrower than float32), every row L2-normalised"""
        if f.dtype != torch.float64:
            f = f.to(dtype if dtype in (torch.float32, torch.float64) else torch.float32)
        return F.normalize(f.flatten(2), dim=2, eps=1e-12)

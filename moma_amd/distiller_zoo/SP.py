"""Similarity-Preserving Knowledge Distillation (Tung & Mori, ICCV 2019) -- the criterion of `--distill similarity` (reference
distiller_zoo/SP.py; loop branch helper/loops_moma.py:140-144, on feat[-2] of both networks).

Per feature pair, with X = f_s flattened to [B, Ks] and Y = f_t to [B, Kt]: G = X X^T (B x B), H = G with every row divided by
max(its L2 norm, 1e-12), likewise for the teacher; loss = mean_ij (H^t_ij - H^s_ij)^2.  On GPU tensors in float32 / bfloat16 with
B <= 1024 the pair runs on the fused kernels of csrc/sp.hip (ops.sp_loss: one split-K Gram launch per side on the matrix cores,
everything behind it in double, one [B,B].[B,K] product for the gradient), reading the maps in STORAGE ORDER -- the Gram matrix does
not depend on the order of the columns, so contiguous and channels_last maps are taken as they are, without a flattened copy.  CPU
tensors, float16 storage, larger batches, maps that are not dense and a teacher that wants a gradient take the same formulas in stock
torch ops, evaluated in float64 (`composite`, which flattens with reshape: the reference's `.view(bsz, -1)` raises on a channels_last
map).

`forward` returns a list of 0-dim float32 scalars, one per pair, as Attention does here.  The reference returns tensors of shape
[1]: an artefact of its `.view(-1, 1).sum(0)`; the loop sums the list either way."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


class Similarity(nn.Module):
    def forward(self, g_s, g_t):
        """lists of feature maps -> list of per-pair losses (as many as the shorter list)"""
        return [self.similarity_loss(f_s, f_t) for f_s, f_t in zip(g_s, g_t)]

    def similarity_loss(self, f_s, f_t):
        if f_s.dim() < 2 or f_t.dim() < 2 or f_s.shape[0] != f_t.shape[0] or f_s.shape[0] < 1:
            raise ValueError("similarity preservation compares the samples of ONE batch; got {} and {}"
                             .format(tuple(f_s.shape), tuple(f_t.shape)))
        if (f_s.is_cuda and f_t.is_cuda and f_s.dtype in _KERNEL_DTYPES and f_t.dtype in _KERNEL_DTYPES
                and f_s.shape[0] <= _lib.SP_MAX_B and f_s.numel() and f_t.numel() and ops.sp_dense(f_s) and ops.sp_dense(f_t)
                and not (f_t.requires_grad and torch.is_grad_enabled())):
            return ops.sp_loss(f_s, f_t)
        return self.composite(f_s, f_t)

    def composite(self, f_s, f_t, dtype=torch.float64):
        """the same formulas in stock torch ops, evaluated in `dtype` and returned in float32 (float64 inputs: in float64)"""
        d = (self.normalised_gram(f_t, dtype) - self.normalised_gram(f_s, dtype)).square().mean()
        return d if f_s.dtype == torch.float64 else d.float()

    @staticmethod
    def normalised_gram(f, dtype=torch.float64):
        """[B, ...] -> H [B, B]: the Gram matrix of the flattened samples, every row divided by max(its L2 norm, 1e-12)"""
        x = f.reshape(f.shape[0], -1)
        if x.dtype != torch.float64:
            x = x.to(dtype)
        return F.normalize(x @ x.t(), dim=1, eps=1e-12)

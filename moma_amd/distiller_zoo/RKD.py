"""Relational Knowledge Distillation (Park et al., "Relational Knowledge Distillation", CVPR 2019) -- the criterion of `--distill rkd`
(reference distiller_zoo/RKD.py; loop branch helper/loops_moma.py:155-158, on feat[-1] of both networks).

loss = w_d * smooth_l1(d_s / mean(d_s), d_t / mean(d_t)) over the pairwise distances of the batch + w_a * smooth_l1 of the cosines of
the angles (x_b - x_a, x_c - x_a) over all triples.  Both are functions of the B x B matrix of squared distances S alone: by the law
of cosines (x_b - x_a).(x_c - x_a) = (S_ab + S_ac - S_bc) / 2, so the reference's [B, B, D] difference tensor, its normalised copy
and their bmm never exist.  On GPU tensors in float32 / bfloat16 with 2 <= B <= 1024 the pair runs on the fused kernels of
csrc/rkd.hip (ops.rkd_loss: S of both sides from the differences in double, one O(B^3) pass over scalars, one [B,B].[B,D] product for
the gradient).  CPU tensors, float16 storage, larger batches and a teacher that wants a gradient take the same formulas in stock
torch ops, evaluated in float64 with [B, B, B] temporaries at most and torch autograd over S.

One deliberate deviation: a pair of exactly equal student rows contributes value 0 and gradient 0 to the angle term.  The
reference's autograd divides by F.normalize's clamp 1e-12 there and hands those rows gradients of 1e10."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)
_EPS = 1e-12


class RKDLoss(nn.Module):
    def __init__(self, w_d=25, w_a=50):
        super().__init__()
        self.w_d, self.w_a = w_d, w_a

    def forward(self, f_s, f_t):
        if f_s.shape[0] != f_t.shape[0] or f_s.shape[0] < 2:
            raise ValueError("relational distillation compares the relations inside ONE batch of at least two samples; got {} and {}"
                             .format(tuple(f_s.shape), tuple(f_t.shape)))
        if (f_s.is_cuda and f_t.is_cuda and f_s.dtype in _KERNEL_DTYPES and f_t.dtype in _KERNEL_DTYPES
                and f_s.shape[0] <= _lib.RKD_MAX_B and not (f_t.requires_grad and torch.is_grad_enabled())):
            return ops.rkd_loss(f_s.contiguous(), f_t.contiguous(), self.w_d, self.w_a)
        return self.composite(f_s, f_t)

    def composite(self, f_s, f_t, dtype=torch.float64):
        """the same formulas in stock torch ops, evaluated in `dtype` and returned in float32 (float64 inputs: in float64)"""
        S_s, S_t = self.sqdist(f_s, dtype), self.sqdist(f_t, dtype)
        loss = self.w_d * F.smooth_l1_loss(self.distances(S_s), self.distances(S_t)) \
            + self.w_a * F.smooth_l1_loss(self.angles(S_s), self.angles(S_t))
        return loss if f_s.dtype == torch.float64 else loss.float()

    @staticmethod
    def sqdist(f, dtype=torch.float64, chunk=1 << 24):
        """[B, ...] -> S [B, B], S_ij = sum_k (x_ik - x_jk)^2 summed from the differences, a block of rows at a time"""
        x = f.reshape(f.shape[0], -1)
        if x.dtype != torch.float64:
            x = x.to(dtype if dtype in (torch.float32, torch.float64) else torch.float32)
        B, D = x.shape
        step = max(1, chunk // max(1, B * D))
        return torch.cat([(x[i:i + step, None, :] - x[None, :, :]).square().sum(-1) for i in range(0, B, step)])

    @staticmethod
    def distances(S):
        """d / mean of its off-diagonal entries, d = sqrt(max(S, 1e-12)) off the diagonal and 0 on it"""
        B = S.shape[0]
        d = S.clamp(min=_EPS).sqrt() * (1 - torch.eye(B, dtype=S.dtype, device=S.device))
        return d / (d.sum() / (B * (B - 1)))

    @staticmethod
    def angles(S):
        """A[a, b, c] = (S_ab + S_ac - S_bc) / (2 n_ab n_ac), n = max(sqrt(S), 1e-12); 0 (value and gradient) where S_ab or S_ac is 0"""
        pos = S > 0
        r = torch.where(pos, 1.0 / torch.where(pos, S, torch.ones_like(S)).sqrt().clamp(min=_EPS), torch.zeros_like(S))
        return (S[:, :, None] + S[:, None, :] - S[None, :, :]) * 0.5 * r[:, :, None] * r[:, None, :]

"""Probabilistic Knowledge Transfer (Passalis & Tefas, "Learning Deep Representations with Probabilistic Knowledge Transfer",
ECCV 2018) -- the criterion of `--distill pkt` (reference distiller_zoo/PKT.py; loop branch helper/loops_moma.py:159-162, on feat[-1]
of both networks).

Per side, with F = the features flattened to [B, D] and eps = 1e-7: G = F F^T, n_i = sqrt(G_ii), C_ij = G_ij / ((n_i + eps)(n_j + eps))
(the cosines), K = (C + 1) / 2, P = K with every row divided by its sum (student: P, teacher: T);
loss = mean_ij T_ij log((T_ij + eps) / (P_ij + eps)).  Everything is a function of the two raw B x B Gram matrices, so no normalised
copy of either side is made.  On GPU tensors in float32 / bfloat16 with B <= 1024 the pair runs on the fused kernels of csrc/pkt.hip
(ops.pkt_loss: one Gram launch per side on the f64 matrix cores, two launches for everything behind them in double, one
[B,B].[B,D] product for the gradient).  CPU tensors, float16 storage, larger batches and a teacher that wants a gradient take the
same formulas in stock torch ops, evaluated in float64 (`composite`).

One deliberate deviation: an all-zero student row gets the finite gradient of x / (|x| + eps) at 0 (norm held constant there).  The
reference's autograd returns NaN for that row -- sqrt's backward at 0 is 0 * inf.  A zero teacher row is no special case:
its cosines are 0."""
import torch
import torch.nn as nn

from .. import _lib, ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)
_EPS = 1e-7


class PKT(nn.Module):
    def forward(self, f_s, f_t):
        if f_s.dim() < 2 or f_t.dim() < 2 or f_s.shape[0] != f_t.shape[0] or f_s.shape[0] < 1:
            raise ValueError("probabilistic knowledge transfer compares the samples of ONE batch; got {} and {}"
                             .format(tuple(f_s.shape), tuple(f_t.shape)))
        if (f_s.is_cuda and f_t.is_cuda and f_s.dtype in _KERNEL_DTYPES and f_t.dtype in _KERNEL_DTYPES
                and f_s.shape[0] <= _lib.PKT_MAX_B and f_s.numel() and f_t.numel()
                and not (f_t.requires_grad and torch.is_grad_enabled())):
            return ops.pkt_loss(f_s.contiguous(), f_t.contiguous())
        return self.composite(f_s, f_t)

    def composite(self, f_s, f_t, dtype=torch.float64):
        """the same formulas in stock torch ops, evaluated in `dtype` and returned in float32 (float64 inputs: in float64)"""
        P, T = self.probabilities(f_s, dtype), self.probabilities(f_t, dtype)
        loss = (T * torch.log((T + _EPS) / (P + _EPS))).mean()
        return loss if f_s.dtype == torch.float64 else loss.float()

    @staticmethod
    def probabilities(f, dtype=torch.float64):
        """[B, ...] -> P [B, B]: (cosine + 1) / 2 of every pair of flattened samples, every row divided by its sum.  The norm of an
        all-zero row is the constant 0 (no sqrt at 0 on autograd's path): that row's gradient is finite"""
        x = f.reshape(f.shape[0], -1)
        if x.dtype != torch.float64:
            x = x.to(dtype)
        sq = x.square().sum(1, keepdim=True)
        pos = sq > 0
        n = torch.where(pos, torch.where(pos, sq, torch.ones_like(sq)).sqrt(), torch.zeros_like(sq))
        z = x / (n + _EPS)
        K = (z @ z.t() + 1.0) / 2.0
        return K / K.sum(1, keepdim=True)

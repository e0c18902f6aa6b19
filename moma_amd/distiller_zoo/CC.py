"""Correlation Congruence (Peng et al., "Correlation Congruence for Knowledge Distillation", ICCV 2019) -- the criterion of
`--distill correlation` (reference distiller_zoo/CC.py Correlation behind two models/util.py LinearEmbed heads; built in
train_student_comparison.py:388-395, loop branch helper/loops_moma.py:168-171; scripts/run_comparison.sh launches it with
`--distill correlation -c 1 -d 1 -b 0.02`).

`LinearEmbed` takes a backbone's last feature to `--feat_dim` outputs with one nn.Linear (attribute `linear`, state-dict keys
`linear.weight`, `linear.bias`); one head per side, BOTH trained -- the teacher's too.  `Correlation.forward(f_s, f_t)` is the
reference's: with delta = |f_s - f_t| the mean over the B - 1 pairs of neighbouring rows of sum_k delta[i, k] delta[i + 1, k].

`Correlation.loss(embed_s, embed_t, f_s, f_t)` is what the training loop calls: both heads and the criterion as one value.  GPU tensors in
float32 / bfloat16 with B >= 2, a teacher feature that records no gradient and a shape ops.cc_native admits run on the kernels of
csrc/cc.hip (ops.cc_embed_neighbour: three launches forward, one backward).  CPU tensors, float16 or float64 storage, a teacher
feature that records a gradient, B < 2 (the reference's NaN: a mean over no pair) and shapes the table turns away take `composite`: the
same formula in stock torch ops, evaluated in float64.

Deviations from the reference (Correlation Congruence):
  * under autocast the kernels read the heads' float32 master weights, where stock ops would cast them to bfloat16 first;
  * the difference of the two embeddings is rounded once to float32, not once per side."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


class LinearEmbed(nn.Module):
    """Linear Embedding"""

    def __init__(self, dim_in=1024, dim_out=128):
        super(LinearEmbed, self).__init__()
        self.linear = nn.Linear(dim_in, dim_out)

    def forward(self, x):
        x = x.view(x.shape[0], -1)
        x = self.linear(x)
        return x


class Correlation(nn.Module):
    """Correlation Congruence for Knowledge Distillation, ICCV 2019"""

    def __init__(self):
        super(Correlation, self).__init__()

    def forward(self, f_s, f_t):
        delta = torch.abs(f_s - f_t)
        loss = torch.mean((delta[:-1] * delta[1:]).sum(1))
        return loss

    @staticmethod
    def takes_kernels(embed_s, embed_t, x_s, x_t):
        """whether this step (x_s, x_t: each side's feature as [B, C]) runs on csrc/cc.hip"""
        ls, lt = embed_s.linear, embed_t.linear
        return (x_s.is_cuda and x_t.is_cuda and x_s.dtype in _KERNEL_DTYPES and x_t.dtype in _KERNEL_DTYPES
                and x_s.dim() == 2 and x_t.dim() == 2 and x_s.shape[0] == x_t.shape[0] and x_s.shape[0] >= 2
                and ls.bias is not None and lt.bias is not None
                and all(p.is_cuda and p.dtype == torch.float32 for p in (ls.weight, ls.bias, lt.weight, lt.bias))
                and ls.weight.shape[1] == x_s.shape[1] and lt.weight.shape[1] == x_t.shape[1] and ls.weight.shape[0] == lt.weight.shape[0]
                and not (torch.is_grad_enabled() and x_t.requires_grad)
                and ops.cc_native(x_s.shape[0], x_s.shape[1], x_t.shape[1], ls.weight.shape[0], dtype=x_s.dtype))

    def loss(self, embed_s, embed_t, f_s, f_t):
        """forward(embed_s(f_s), embed_t(f_t)) -> scalar float32"""
        x_s, x_t = f_s.reshape(f_s.shape[0], -1), f_t.reshape(f_t.shape[0], -1)
        if self.takes_kernels(embed_s, embed_t, x_s, x_t):
            ls, lt = embed_s.linear, embed_t.linear
            return ops.cc_embed_neighbour(x_s.contiguous(), x_t.contiguous(), ls.weight.contiguous(), ls.bias, lt.weight.contiguous(),
                                          lt.bias)
        return self.composite(embed_s, embed_t, x_s, x_t)

    def composite(self, embed_s, embed_t, x_s, x_t, dtype=torch.float64):
        """both heads and the criterion on x_s [B, Cs], x_t [B, Ct] in stock torch ops, evaluated in `dtype` and returned in float32
        (float64 inputs: in float64); B < 2 gives the reference's NaN"""
        ls, lt = embed_s.linear, embed_t.linear
        with torch.autocast(x_s.device.type, enabled=False):
            def head(lin, x):
                return F.linear(x.to(dtype), lin.weight.to(dtype), lin.bias.to(dtype) if lin.bias is not None else None)
            loss = self.forward(head(ls, x_s), head(lt, x_t))
        return loss if x_s.dtype == torch.float64 else loss.float()

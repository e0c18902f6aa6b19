"""Variational Information Distillation (Ahn et al., "Variational Information Distillation for Knowledge Transfer", CVPR 2019) -- the
criterion of `--distill vid` (reference distiller_zoo/VID.py; built in train_student_comparison.py:304-311, loop branch
helper/loops_moma.py:145-149).

One VIDLoss per feature pair, and the first comparison criterion here with trained state: a bias-free regressor conv1x1 -> ReLU ->
conv1x1 -> ReLU -> conv1x1 that maps the student's map to the mean of a Gaussian over the teacher's, and a per-channel `log_scale`
whose softplus (+ eps) is its variance; loss = 0.5 mean((mean - target)^2 / var + log var).  Both maps are first put on a common
grid as the reference does (the side with the larger height average-pooled to (h, h), h the smaller height, the input BEFORE the
regressor).  Parameter names (`regressor.0/2/4.weight`, `log_scale`), construction order (so the RNG draws) and the initial
`log_scale` are the reference's.

The three convolutions are backbones.efficientnet.SamePadConv2d (an nn.Conv2d with nn.Conv2d's initialisation): under bf16 autocast
on the GPU their forward and input gradient run on the streaming kernel of csrc/pwstream.hip wherever ops.pwconv_fwd_native admits
the shape, as stock conv2d everywhere else; the ReLUs are stock.  The likelihood itself runs on the kernels of csrc/vid.hip
(ops.vid_nll: two reads forward, two reads and one write backward, no activation-sized temporary) for GPU tensors in float32 /
bfloat16 that are dense in NCHW or channels_last, with a target that wants no gradient.  CPU tensors, float16 or float64 storage, odd
strides and a target that records a gradient take `composite`: the same formula in stock torch ops, evaluated in float64.  For
log_scale above about 88 the reference's fp32 exp overflows; both paths here evaluate the softplus in float64 and stay finite.  The
formula needs [B, C, H, W] maps: token lists (the ViT backbones) are refused."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..backbones.efficientnet import SamePadConv2d

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


def _dense(f):
    return f.is_contiguous() or f.is_contiguous(memory_format=torch.channels_last)


class VIDLoss(nn.Module):
    def __init__(self, num_input_channels, num_mid_channel, num_target_channels, init_pred_var=5.0, eps=1e-5):
        super().__init__()

        def conv1x1(cin, cout):
            return SamePadConv2d(cin, cout, 1, bias=False)

        self.regressor = nn.Sequential(
            conv1x1(num_input_channels, num_mid_channel),
            nn.ReLU(),
            conv1x1(num_mid_channel, num_mid_channel),
            nn.ReLU(),
            conv1x1(num_mid_channel, num_target_channels),
        )
        self.log_scale = nn.Parameter(np.log(np.exp(init_pred_var - eps) - 1.0) * torch.ones(num_target_channels))
        self.eps = eps

    def forward(self, input, target):
        if input.dim() != 4 or target.dim() != 4:
            raise ValueError("Variational information distillation compares [B, C, H, W] feature maps; got {} and {} (the token lists "
                             "of a ViT backbone have no per-channel pixel likelihood in this formula)".format(
                                 tuple(input.shape), tuple(target.shape)))
        s_h, t_h = input.shape[2], target.shape[2]
        if s_h > t_h:
            input = F.adaptive_avg_pool2d(input, (t_h, t_h))
        elif s_h < t_h:
            target = F.adaptive_avg_pool2d(target, (s_h, s_h))
        pred_mean = self.regressor(input)
        if self.takes_kernels(pred_mean, target):
            # a target in the other memory format than the regressor's output (channels_last backbones in front of the streaming
            # convolution, which writes NCHW) is copied into that format once: the kernels would read it element by element
            fmt = torch.contiguous_format if pred_mean.is_contiguous() else torch.channels_last
            if not target.is_contiguous(memory_format=fmt):
                target = target.contiguous(memory_format=fmt)
            return ops.vid_nll(pred_mean, target, self.log_scale, self.eps)
        return self.composite(pred_mean, target)

    def takes_kernels(self, pred_mean, target):
        """whether the likelihood of this pair runs on csrc/vid.hip"""
        return (pred_mean.is_cuda and target.is_cuda and pred_mean.dtype in _KERNEL_DTYPES and target.dtype in _KERNEL_DTYPES
                and self.log_scale.is_cuda and self.log_scale.dtype == torch.float32
                and _dense(pred_mean) and _dense(target) and pred_mean.shape == target.shape
                and not (target.requires_grad and torch.is_grad_enabled()))

    def composite(self, pred_mean, target, dtype=torch.float64):
        """the likelihood in stock torch ops, evaluated in `dtype` and returned in float32 (float64 maps: in float64)"""
        m, t, ls = pred_mean.to(dtype), target.to(dtype), self.log_scale.to(dtype)
        var = (F.softplus(ls, threshold=700.0) + self.eps).view(1, -1, 1, 1)
        loss = (0.5 * ((m - t) ** 2 / var + torch.log(var))).mean()
        return loss if pred_mean.dtype == torch.float64 else loss.float()

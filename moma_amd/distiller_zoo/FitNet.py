"""FitNets hint (Romero et al., "FitNets: Hints for Thin Deep Nets", ICLR 2015) -- the criterion of `--distill hint` (reference
distiller_zoo/FitNet.py and models/util.py ConvReg; built in train_student_moma.py:288-292, loop branch helper/loops_moma.py:284-286).

HintLoss is the mean squared error of two feature maps.  ConvReg is the trained regressor in front of it: a convolution that takes
the student's map `feat_s[hint_layer]` to the teacher's channels and grid, BatchNorm2d, ReLU.  The four shape branches, the attribute
names (`conv`, `bn`, `relu`), the state-dict keys and the construction order (so the RNG draws) are the reference's, and so is
`forward(x, t) -> (f_s, f_t)` in stock ops.

`ConvReg.loss(x, t)` is what the training loop calls: HintLoss(*forward(x, t)) as one value.  In training mode on GPU tensors in
float32 / bfloat16 the convolution runs WITHOUT its bias and everything behind it -- batch statistics, running statistics, ReLU, the
squared error and the whole backward -- on the kernels of csrc/hint.hip (ops.hint_bn_relu_mse: three reads of the convolution's
output, two of the teacher's map, one write of the gradient, nothing map-sized kept between forward and backward).  In training mode
a per-channel constant in front of a BatchNorm changes running_mean and nothing else, so the bias is handed to the kernels for that
update only and its gradient is exact zeros (the reference's autograd returns rounding noise there).  Where both maps share a grid
the convolution is 1 x 1: a backbones.efficientnet.SamePadConv2d that owns the bias but can be called without it, so that under bf16
autocast it reaches the streaming kernel of csrc/pwstream.hip wherever ops.pwconv_fwd_native admits the layer.
CPU tensors, float16 or float64 storage, eval mode, momentum=None, odd strides and a target that records a gradient take
`composite`: the same formula in stock torch ops, evaluated in float64.  Both routes advance `bn.num_batches_tracked`.
The formula needs [B, C, H, W] maps: token lists (the ViT backbones) are refused."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..backbones.efficientnet import SamePadConv2d

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


def _dense(f):
    return f.is_contiguous() or f.is_contiguous(memory_format=torch.channels_last)


def _refuse_tokens(a, b):
    if a.dim() != 4 or b.dim() != 4:
        raise ValueError("The FitNets hint compares [B, C, H, W] feature maps; got {} and {} (the token lists of a ViT backbone have "
                         "no grid for the regressor's convolution)".format(tuple(a.shape), tuple(b.shape)))


class HintLoss(nn.Module):
    """Fitnets: hints for thin deep nets, ICLR 2015"""

    def __init__(self):
        super().__init__()
        self.crit = nn.MSELoss()

    def forward(self, f_s, f_t):
        _refuse_tokens(f_s, f_t)
        return self.crit(f_s, f_t)


class _PointwiseConv(SamePadConv2d):
    """the 1 x 1 convolution of ConvReg: nn.Conv2d's parameters and initialisation, callable without its bias"""

    def forward(self, x, with_bias=True):
        if with_bias or self.bias is None:
            return super().forward(x)
        bias = self._parameters["bias"]
        self._parameters["bias"] = None               # (what a bias-free layer holds there: the streaming kernel takes such layers)
        try:
            return super().forward(x)
        finally:
            self._parameters["bias"] = bias


class ConvReg(nn.Module):
    """Convolutional regression for FitNet (feature-map layer)"""

    def __init__(self, s_shape, t_shape):
        super().__init__()
        if len(s_shape) != 4 or len(t_shape) != 4:
            raise ValueError("The FitNets hint compares [B, C, H, W] feature maps; got shapes {} and {} (the token lists of a ViT "
                             "backbone have no grid for the regressor's convolution)".format(tuple(s_shape), tuple(t_shape)))
        _, s_C, s_H, s_W = s_shape
        _, t_C, t_H, t_W = t_shape
        self.s_H = s_H
        self.t_H = t_H
        if s_H == 2 * t_H:
            self.conv = nn.Conv2d(s_C, t_C, kernel_size=3, stride=2, padding=1)
        elif s_H * 2 == t_H:
            self.conv = nn.ConvTranspose2d(s_C, t_C, kernel_size=4, stride=2, padding=1)
        elif s_H >= t_H:
            if s_H == t_H and s_W == t_W:
                self.conv = _PointwiseConv(s_C, t_C, 1)
            else:
                self.conv = nn.Conv2d(s_C, t_C, kernel_size=(1 + s_H - t_H, 1 + s_W - t_W))
        else:
            self.conv = nn.Conv2d(s_C, t_C, kernel_size=3, padding=1, stride=1)
        self.bn = nn.BatchNorm2d(t_C)
        self.relu = nn.ReLU(inplace=True)

    def _pools_teacher(self):
        return not (self.s_H == 2 * self.t_H or self.s_H * 2 == self.t_H or self.s_H >= self.t_H)

    def forward(self, x, t):
        _refuse_tokens(x, t)
        x = self.conv(x)
        if self._pools_teacher():
            t = F.adaptive_avg_pool2d(t, (self.s_H, self.s_H))
        return self.relu(self.bn(x)), t

    def _conv_without_bias(self, x):
        c = self.conv
        if isinstance(c, _PointwiseConv):
            return c(x, with_bias=False)
        if isinstance(c, nn.ConvTranspose2d):
            return F.conv_transpose2d(x, c.weight, None, c.stride, c.padding, c.output_padding, c.groups, c.dilation)
        return F.conv2d(x, c.weight, None, c.stride, c.padding, c.dilation, c.groups)

    def takes_kernels(self, x, t):
        """whether the tail of this pair (x: the convolution's output) runs on csrc/hint.hip"""
        bn = self.bn
        return (self.training and bn.momentum is not None and bn.affine and bn.track_running_stats
                and x.is_cuda and t.is_cuda and x.dtype in _KERNEL_DTYPES and t.dtype in _KERNEL_DTYPES
                and bn.weight.is_cuda and bn.weight.dtype == torch.float32 and x.dim() == 4 and x.shape == t.shape
                and x.shape[0] * x.shape[2] * x.shape[3] >= 2 and _dense(x) and _dense(t)
                and not (t.requires_grad and torch.is_grad_enabled())
                and ops.hint_native(x.shape[0], x.shape[1], x.shape[2] * x.shape[3], dtype=x.dtype,
                                    channels_last=not x.is_contiguous()))

    def loss(self, x, t):
        """HintLoss(*self.forward(x, t)) -> scalar float32"""
        _refuse_tokens(x, t)
        if self._pools_teacher():
            t = F.adaptive_avg_pool2d(t, (self.s_H, self.s_H))
        if self.training and x.is_cuda and t.is_cuda and self.bn.momentum is not None:
            y = self._conv_without_bias(x)
            if self.takes_kernels(y, t):
                # a target in the other memory format than the convolution's output (channels_last backbones in front of the
                # streaming convolution, which writes NCHW) is copied into that format once: the kernels would read it element by element
                fmt = torch.contiguous_format if y.is_contiguous() else torch.channels_last
                if not t.is_contiguous(memory_format=fmt):
                    t = t.contiguous(memory_format=fmt)
                bn = self.bn
                out = ops.hint_bn_relu_mse(y, t, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                           conv_bias=self.conv.bias)
                bn.num_batches_tracked.add_(1)
                return out
            if self.conv.bias is not None:
                y = y + self.conv.bias.to(y.dtype).view(1, -1, 1, 1)
        else:
            y = self.conv(x)
        return self.composite(y, t)

    def composite(self, y, t, dtype=torch.float64):
        """BatchNorm -> ReLU -> mean squared error behind the convolution's output y (bias included) in stock torch ops, evaluated in
        `dtype` and returned in float32 (float64 maps: in float64); the running statistics advance as nn.BatchNorm2d's do"""
        bn = self.bn
        with torch.autocast(y.device.type, enabled=False):
            yd, td = y.to(dtype), t.to(dtype)
            use_batch = self.training or not bn.track_running_stats
            if use_batch and bn.track_running_stats:
                bn.num_batches_tracked.add_(1)
            momentum = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            rm = rv = None
            if bn.track_running_stats:
                rm, rv = bn.running_mean.to(dtype), bn.running_var.to(dtype)
            w = bn.weight.to(dtype) if bn.affine else None
            b = bn.bias.to(dtype) if bn.affine else None
            out = F.batch_norm(yd, rm, rv, w, b, use_batch, momentum if use_batch else 0.0, bn.eps)
            if use_batch and bn.track_running_stats and rm is not bn.running_mean:      # (float64 buffers were updated in place)
                with torch.no_grad():
                    bn.running_mean.copy_(rm)
                    bn.running_var.copy_(rv)
            loss = F.mse_loss(F.relu(out), td)
        return loss if y.dtype == torch.float64 else loss.float()

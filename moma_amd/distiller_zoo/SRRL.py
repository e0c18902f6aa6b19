"""SRRL (Yang et al., "Knowledge Distillation via Softmax Regression Representation Learning", ICLR 2021) -- the connector of
`--distill srrl` (reference models/util.py SRRL; built in train_student_moma.py:365-371, loop branch helper/loops_moma.py:180-182 /
:340-342 with criterion_kd = nn.MSELoss()).

The connector takes the student's pooled feature `feat_s[-1]` to the teacher's width: a bias-free 1 x 1 convolution, BatchNorm2d, ReLU.
The KD term is the mean squared error of its output against `feat_t[-1]` plus the mean squared error of the TEACHER'S classifier applied
to that output against the teacher's logits.  The attribute name (`transfer`, a Sequential), the state-dict keys
(`transfer.0.weight`, `transfer.1.*`) and the construction order (so the RNG draws) are the reference's, and so is
`forward(feat_s, cls_t) -> (trans_feat_s, pred_feat_s)` in stock ops.

`SRRL.loss(feat_s, feat_t, logit_t, cls_t)` is what the training loop calls: both errors as one value.  In training mode on GPU
tensors in float32 / bfloat16, with a classifier that reduces to one affine map (an nn.Linear, or an nn.Sequential of inactive
Dropouts and one nn.Linear: EfficientNet's `classifier_` with the teacher in eval), the convolution runs as F.linear on the weight's
[t_n, s_n] view (at H W = 1 it is a plain GEMM and stays on the library) and everything behind it -- batch statistics, running
statistics, ReLU, the classifier's product, both squared errors and the whole backward -- on the kernels of csrc/srrl.hip
(ops.srrl_bn_relu_dual_mse).  CPU tensors, float16 or float64 storage, eval mode, momentum=None, an active Dropout, any other
classifier module and shapes ops.srrl_native turns away take `composite`: the same formula in stock torch ops, evaluated in float64.
Both routes advance `num_batches_tracked`.

Deviations from the reference (SRRL):
  * every feat[-1] of shape [B, C], [B, C, 1, 1] or any [B, C, 1, ...] is taken as [B, C], on both sides, in `forward` and in `loss`.
    The reference's moma loop hands the [B, C, 1, 1] feature of its shipped backbones to SRRL.forward, which unsqueezes it twice and
    raises in conv2d on a 6-D tensor; its comparison loop squeezes first.
  * the classifier is constant: its weight and bias are read in float32 and get no gradient (the reference accumulates one on the
    teacher that no optimizer ever reads)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


def _rows(f, name):
    """[B, C], [B, C, 1, 1] or any [B, C, 1, ...] -> [B, C]"""
    if f.dim() < 2 or any(d != 1 for d in f.shape[2:]):
        raise ValueError("SRRL works on pooled features [B, C] or [B, C, 1, ...]; got {} {}".format(name, tuple(f.shape)))
    return f.reshape(f.shape[0], f.shape[1])


def affine_classifier(cls_t):
    """-> the nn.Linear a classifier reduces to (an nn.Linear, or an nn.Sequential of inactive Dropouts and ONE nn.Linear), else None"""
    if isinstance(cls_t, nn.Linear):
        return cls_t
    if isinstance(cls_t, nn.Sequential):
        lin = None
        for m in cls_t:
            if isinstance(m, nn.Dropout) and (not m.training or m.p == 0):
                continue
            if isinstance(m, nn.Linear) and lin is None:
                lin = m
                continue
            return None
        return lin
    return None


class SRRL(nn.Module):
    """ICLR-2021: Knowledge Distillation via Softmax Regression Representation Learning"""

    def __init__(self, *, s_n, t_n):
        super().__init__()

        def conv1x1(in_channels, out_channels, stride=1):
            return nn.Conv2d(in_channels, out_channels, kernel_size=1, padding=0, stride=stride, bias=False)

        setattr(self, "transfer", nn.Sequential(
            conv1x1(s_n, t_n),
            nn.BatchNorm2d(t_n),
            nn.ReLU(inplace=True),
        ))

    def forward(self, feat_s, cls_t):
        feat_s = _rows(feat_s, "feat_s").unsqueeze(-1).unsqueeze(-1)
        temp_feat = self.transfer(feat_s)
        trans_feat_s = temp_feat.view(temp_feat.size(0), -1)
        pred_feat_s = cls_t(trans_feat_s)
        return trans_feat_s, pred_feat_s

    def takes_kernels(self, x, t, logit_t, cls_t):
        """whether the tail of this step (x: the convolution's output [B, t_n]) runs on csrc/srrl.hip"""
        bn = self.transfer[1]
        lin = affine_classifier(cls_t)
        return (self.training and bn.training and bn.momentum is not None and bn.affine and bn.track_running_stats
                and lin is not None and x.is_cuda and t.is_cuda and logit_t.is_cuda
                and x.dtype in _KERNEL_DTYPES and t.dtype in _KERNEL_DTYPES and logit_t.dtype in _KERNEL_DTYPES + (torch.float16,)
                and bn.weight.is_cuda and bn.weight.dtype == torch.float32
                and lin.weight.is_cuda and lin.weight.dtype == torch.float32
                and x.dim() == 2 and x.shape == t.shape and x.shape[0] >= 2
                and lin.weight.shape[1] == x.shape[1] and tuple(logit_t.shape) == (x.shape[0], lin.weight.shape[0])
                and not (torch.is_grad_enabled() and (t.requires_grad or logit_t.requires_grad))
                and ops.srrl_native(x.shape[0], x.shape[1], lin.weight.shape[0], dtype=x.dtype))

    def loss(self, feat_s, feat_t, logit_t, cls_t):
        """MSE(trans_feat_s, feat_t) + MSE(pred_feat_s, logit_t) of forward(feat_s, cls_t) -> scalar float32"""
        f_s, f_t = _rows(feat_s, "feat_s"), _rows(feat_t, "feat_t")
        conv, bn = self.transfer[0], self.transfer[1]
        x = F.linear(f_s, conv.weight.view(conv.weight.shape[0], conv.weight.shape[1]))     # (the 1 x 1 convolution at H W = 1)
        if self.takes_kernels(x, f_t, logit_t, cls_t):
            lin = affine_classifier(cls_t)
            bias = lin.bias.detach() if lin.bias is not None else None
            out = ops.srrl_bn_relu_dual_mse(x.contiguous(), f_t.contiguous(), lin.weight.detach().contiguous(), bias,
                                            logit_t.float().contiguous(), bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                            bn.momentum, bn.eps)
            bn.num_batches_tracked.add_(1)
            return out
        return self.composite(x, f_t, logit_t, cls_t)

    def composite(self, x, t, logit_t, cls_t, dtype=torch.float64):
        """BatchNorm -> ReLU -> mean squared error against t, plus the classifier -> mean squared error against logit_t, behind the
        convolution's output x [B, t_n], in stock torch ops, evaluated in `dtype` and returned in float32 (float64 inputs: in
        float64); the running statistics advance as nn.BatchNorm2d's do.  A classifier that reduces to one affine map is applied in
        `dtype` from its detached weights; any other module is called as it is, in its own dtype."""
        bn = self.transfer[1]
        with torch.autocast(x.device.type, enabled=False):
            xd, td, ld = x.to(dtype), t.to(dtype), logit_t.to(dtype)
            use_batch = (self.training and bn.training) or not bn.track_running_stats
            if use_batch and bn.track_running_stats:
                bn.num_batches_tracked.add_(1)
            momentum = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            rm = rv = None
            if bn.track_running_stats:
                rm, rv = bn.running_mean.to(dtype), bn.running_var.to(dtype)
            w = bn.weight.to(dtype) if bn.affine else None
            b = bn.bias.to(dtype) if bn.affine else None
            out = F.batch_norm(xd, rm, rv, w, b, use_batch, momentum if use_batch else 0.0, bn.eps)
            if use_batch and bn.track_running_stats and rm is not bn.running_mean:      # (float64 buffers were updated in place)
                with torch.no_grad():
                    bn.running_mean.copy_(rm)
                    bn.running_var.copy_(rv)
            y = F.relu(out)
            lin = affine_classifier(cls_t)
            if lin is not None:
                pred = F.linear(y, lin.weight.detach().to(dtype), lin.bias.detach().to(dtype) if lin.bias is not None else None)
            else:
                p0 = next(cls_t.parameters(), None)
                pred = cls_t(y.to(p0.dtype if p0 is not None else torch.float32)).to(dtype)
            loss = F.mse_loss(y, td) + F.mse_loss(pred, ld)
        return loss if x.dtype == torch.float64 else loss.float()

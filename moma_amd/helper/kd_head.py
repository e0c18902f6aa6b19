"""The student's head of every `--distill` step: nn.CrossEntropyLoss, DistillKL(T) (distiller_zoo/KD.py) and the top-1 of
helper.util.accuracy (reference helper/loops_moma.py:278-279 and the accuracy call behind them) as ONE module.

`StudentHead(T)(logit_s, logit_t, labels)` -> (loss_cls, loss_div, acc), scalar float32 each:

    loss_cls = nn.CrossEntropyLoss()(logit_s, labels)
    loss_div = DistillKL(T)(logit_s, logit_t)
    acc      = accuracy(logit_s, labels, topk=(1,))[0].squeeze(0)

GPU tensors with int64 labels and dtypes and a shape `ops.kd_head_native` holds run on csrc/kdhead.hip (two launches forward, one
backward, whatever the two loss weights are); the CPU, float16 / float64 and whatever is turned away take `composite`: the same
formulas in stock ops, evaluated in float64 and returned in float32.  Both follow one rule for labels: -100 is ignored as
nn.CrossEntropyLoss ignores it (no loss, left out of the mean, no gradient, never a hit); any other label outside [0, n_cls) is never
used as an index -- it makes loss_cls NaN and leaves its row without cross-entropy gradient (stock torch answers it with a device-side
assert: a deliberate deviation, the CE head's).  The KL term does not look at labels, and acc divides by the batch size.  The
teacher's logits get no gradient from the kernels; the composite gives them what autograd gives."""
import torch
import torch.nn as nn

from .. import ops

IGNORE_INDEX = -100


class StudentHead(nn.Module):
    def __init__(self, T):
        super().__init__()
        T = float(T)
        if not (0.0 < T < float("inf")):
            raise ValueError(f"StudentHead: the temperature must be finite and > 0, got {T}")
        self.T = T

    @staticmethod
    def native(logit_s, logit_t, labels):
        return (torch.is_tensor(logit_s) and logit_s.is_cuda and logit_s.dim() == 2 and torch.is_tensor(logit_t) and logit_t.is_cuda
                and logit_t.shape == logit_s.shape and torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int64
                and labels.dim() == 1 and not (logit_t.requires_grad and torch.is_grad_enabled())
                and ops.kd_head_native(logit_s.shape[0], logit_s.shape[1], logit_s.dtype, logit_t.dtype))

    def forward(self, logit_s, logit_t, labels):
        if self.native(logit_s, logit_t, labels):
            return ops.kd_head(logit_s if logit_s.is_contiguous() else logit_s.contiguous(),
                               logit_t if logit_t.is_contiguous() else logit_t.contiguous(), labels.contiguous(), self.T)
        return self.composite(logit_s, logit_t, labels, self.T)

    @staticmethod
    def composite(logit_s, logit_t, labels, T, full=False):
        """the kernels' formulas in stock ops: float64 arithmetic, float32 results, no host read.  full=True: the float64 values too
        -> ((loss_cls, loss_div, acc), dict(loss_cls, loss_div, acc, lse, lseS, lseT, pred) in float64)"""
        zs, zt = logit_s.double(), logit_t.double()
        B, K = zs.shape
        labels = labels.long()
        valid = (labels >= 0) & (labels < K)
        bad = ~valid & (labels != IGNORE_INDEX)
        ys = torch.where(valid, labels, torch.zeros_like(labels))
        m, pred = zs.max(dim=1)                                  # (a tie's index is torch's choice; the kernels take the lowest)
        ds0 = zs - m[:, None]
        lse = m + torch.log(torch.exp(ds0).sum(dim=1))
        rows = torch.where(valid, lse - zs.gather(1, ys[:, None])[:, 0], torch.zeros_like(lse))
        total, n = rows.sum(), valid.sum()
        # (n = 0: 0 / 0 = NaN, as torch; a bad label ADDS a NaN, so the other rows keep their gradient as they do on the kernels)
        loss_cls = total / n + torch.where(bad.any(), torch.full_like(total, float("nan")), torch.zeros_like(total))
        # the divergence on the rows' shifted values: W / (1 + ST) + (log S_s - log S_t); a term with e_t = 0 counts 0
        ds = ds0 / T
        dt = (zt - zt.max(dim=1, keepdim=True)[0]) / T
        et = torch.exp(dt)
        ls, lt = torch.log(torch.exp(ds).sum(dim=1)), torch.log(et.sum(dim=1))
        w = torch.where(et != 0, et * (dt - ds), torch.zeros_like(et)).sum(dim=1)
        kl = w / et.sum(dim=1) + (ls - lt)
        loss_div = kl.sum() * (T * T / B)
        with torch.no_grad():
            acc = (valid & (pred == labels)).sum().double() * (100.0 / B)
        res = (loss_cls.float(), loss_div.float(), acc.float())
        if full:
            return res, {"loss_cls": loss_cls, "loss_div": loss_div, "acc": acc, "lse": lse, "lseS": m / T + ls,
                         "lseT": zt.max(dim=1)[0] / T + lt, "pred": pred}
        return res

"""The classification head of the teacher trainer: nn.CrossEntropyLoss, the top-1 count of helper.util.accuracy and the confusion
matrix of the reference's validation (helper/loops_moma.py:40-45, :407-425 there) as ONE module.

`CrossEntropyHead()(output, labels)` is drop-in for `nn.CrossEntropyLoss()(output, labels)`.  With `meter=True` it also owns two
device buffers, `stats` [4] float64 (sum of the valid rows' losses, top-1 hits, valid rows, rows with a bad label) and `conf`
[n_cls, n_cls] int64 (row = label, column = prediction), which every call adds to; `read()` is the only call that touches the host, so
a training loop that reads once per print never waits for the device in between (the reference's loop calls `.item()` twice a step).

GPU tensors with int64 labels and a dtype and shape `ops.ce_native` holds (bfloat16 within the kernels' caps; float32 is turned away by
the microbenchmark, see there) run on csrc/ce.hip (two launches forward, one backward); the CPU, float16 / float64 and whatever is
turned away take `composite`: the same formulas in stock ops, evaluated in float64
and returned in float32, with the same meter updates.  Both follow one rule for labels: -100 is ignored as nn.CrossEntropyLoss
ignores it (no loss, left out of the mean, no gradient, never a hit, nothing in the matrix); any other label outside [0, n_cls) is
never used as an index -- it makes the loss NaN, leaves its row without gradient and is counted in stats[3].  Stock torch answers
such a label with a device-side assert that takes the process down: a deliberate deviation."""
import torch
import torch.nn as nn

from .. import ops

IGNORE_INDEX = -100


class CrossEntropyHead(nn.Module):
    def __init__(self, n_cls=None, meter=False):
        super().__init__()
        self.meter = bool(meter)
        if self.meter:
            if n_cls is None or int(n_cls) < 1:
                raise ValueError("CrossEntropyHead(meter=True) needs n_cls, the side of the confusion matrix")
            self.n_cls = int(n_cls)
            self.register_buffer("stats", torch.zeros(4, dtype=torch.float64), persistent=False)
            self.register_buffer("conf", torch.zeros(self.n_cls, self.n_cls, dtype=torch.int64), persistent=False)
        else:
            self.stats = self.conf = None

    def reset(self):
        if self.meter:
            self.stats.zero_()
            self.conf.zero_()

    def read(self):
        """-> (top-1 accuracy in percent of the valid rows, mean loss over them, confusion matrix as a numpy array): the one host read"""
        if not self.meter:
            raise RuntimeError("CrossEntropyHead.read(): built without meter=True")
        s = self.stats.tolist()
        n = max(s[2], 1.0)
        return 100.0 * s[1] / n, s[0] / n, self.conf.cpu().numpy()

    @staticmethod
    def native(output, labels):
        return (torch.is_tensor(output) and output.is_cuda and output.dim() == 2 and output.dtype in (torch.float32, torch.bfloat16)
                and torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int64 and labels.dim() == 1
                and ops.ce_native(output.shape[0], output.shape[1], output.dtype))

    def forward(self, output, labels):
        if self.meter and output.shape[-1] != self.n_cls:
            raise ValueError(f"CrossEntropyHead: {output.shape[-1]} logits per row for a meter of {self.n_cls} classes")
        if self.native(output, labels):
            return ops.ce_head(output if output.is_contiguous() else output.contiguous(), labels.contiguous(), self.stats, self.conf)
        return self.composite(output, labels, self.stats, self.conf)

    @staticmethod
    def composite(output, labels, stats=None, conf=None):
        """the kernels' formulas in stock ops: float64 arithmetic, float32 result, the same meter updates, no host read"""
        z = output.double()
        K = z.shape[1]
        labels = labels.long()
        valid = (labels >= 0) & (labels < K)
        bad = ~valid & (labels != IGNORE_INDEX)
        ys = torch.where(valid, labels, torch.zeros_like(labels))
        m, pred = z.max(dim=1)                                    # (the fixture's maxima are unique; a tie's index is torch's choice)
        lse = m + torch.log(torch.exp(z - m[:, None]).sum(dim=1))
        rows = torch.where(valid, lse - z.gather(1, ys[:, None])[:, 0], torch.zeros_like(lse))
        total, n = rows.sum(), valid.sum()
        # (n = 0: 0 / 0 = NaN, as torch; a bad label ADDS a NaN, so the other rows keep their gradient as they do on the kernels)
        loss = total / n + torch.where(bad.any(), torch.full_like(total, float("nan")), torch.zeros_like(total))
        with torch.no_grad():
            if stats is not None:
                hits = (valid & (pred == labels)).sum()
                stats += torch.stack([total.detach(), hits.double(), n.double(), bad.sum().double()]).to(stats.device)
            if conf is not None:
                # (index_add_ and not bincount, which reads its output's size back from the device; rows that are not valid add 0)
                conf.view(-1).index_add_(0, (ys * K + pred).to(conf.device), valid.long().to(conf.device))
        return loss.float()


"""The two sample-indexed memory banks of CRD (reference crd/memory.py) on the HIP gather kernels.

Same constructor, buffers (`params`, `memory_v1`, `memory_v2`: checkpoints carry over) and `forward` signature as the
reference.  What differs, all performance-only:
  * `forward` returns the materialised scores through moma_crd_scores (one gather launch for both sides) and `forward_fused`
    the loss itself through moma_crd_fused: no [B, K+1, d] copy of the gathered rows exists in either;
  * the normalisation constants Z live in `params[2:4]` ON THE DEVICE and are written there by the kernels; the reference reads
    `params` back five times per step (crd/memory.py:24-29).  Here K, T and the momentum are host attributes, and whether Z
    still has to be set is decided by ONE read of `params` at the first forward after construction or load_state_dict;
  * indices are data: an entry outside [0, n_data) contributes nothing and raises a device flag that `check_indices()` reads
    (call it where the host synchronises anyway: end of an epoch, tests), where the reference would fault inside index_select.
"""
import math

import numpy as np
import torch
from torch import nn

from .. import ops


class AliasMethod(object):
    """Walker / Vose alias tables for draws from a discrete distribution: built once on the host, `draw` runs on the device the
    tables were moved to (reference crd/memory.py:82-139)."""

    def __init__(self, probs):
        p = np.asarray(probs.detach().cpu().numpy() if isinstance(probs, torch.Tensor) else probs, dtype=np.float64)
        n = p.shape[0]
        if p.sum() > 1:
            p = p / p.sum()
        q = p * n
        alias = np.zeros(n, dtype=np.int64)
        small = [i for i in range(n) if q[i] < 1.0] if (q < 1.0).any() else []
        large = [i for i in range(n) if q[i] >= 1.0] if small else []
        while small and large:
            s, g = small.pop(), large.pop()
            alias[s] = g
            q[g] = (q[g] - 1.0) + q[s]
            (small if q[g] < 1.0 else large).append(g)
        for i in small + large:
            q[i] = 1.0
        if not small and not large and not (p * n < 1.0).any():
            q[:] = 1.0                                         # (uniform weights: every column is its own outcome)
        self.prob = torch.from_numpy(q.astype(np.float32))
        self.alias = torch.from_numpy(alias)

    def to(self, device):
        self.prob = self.prob.to(device)
        self.alias = self.alias.to(device)
        return self

    def cuda(self):
        return self.to("cuda")

    def draw(self, N, generator=None):
        """N draws (int64, on the tables' device)"""
        n = self.alias.shape[0]
        col = torch.randint(0, n, (N,), device=self.prob.device, generator=generator)
        keep = torch.rand(N, device=self.prob.device, generator=generator) < self.prob[col]
        return torch.where(keep, col, self.alias[col])


class ContrastMemory(nn.Module):
    """memory buffer that supplies a large amount of negative samples (reference crd/memory.py:6-79)"""

    def __init__(self, inputSize, outputSize, K, T=0.07, momentum=0.5):
        super().__init__()
        self.nLem = outputSize
        self.K = int(K)
        self.multinomial = AliasMethod(torch.ones(self.nLem))
        self.register_buffer("params", torch.tensor([K, T, -1, -1, momentum]))
        stdv = 1. / math.sqrt(inputSize / 3)
        self.register_buffer("memory_v1", torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))
        self.register_buffer("memory_v2", torch.rand(outputSize, inputSize).mul_(2 * stdv).add_(-stdv))
        self.register_buffer("bad_index", torch.zeros(1, dtype=torch.int32), persistent=False)
        self._host = None            # (K, T, momentum, set_z) as read from `params`; None = read them at the next forward

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.multinomial.to(self.params.device)
        return out

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self._host = None

    def _state(self):
        """(K, T, momentum, set_z): one host read of `params` after construction / load_state_dict, none afterwards"""
        if self._host is None:
            p = self.params.tolist()
            # (the reference sets each Z that is still negative; both are set by the same first forward, so one switch serves)
            self._host = [int(p[0]), p[1], p[4], p[2] < 0 or p[3] < 0]
        return self._host

    def _indices(self, y, idx, batch):
        if idx is None:
            idx = self.multinomial.draw(batch * (self.K + 1)).view(batch, -1)
            idx.select(1, 0).copy_(y.data)
        return idx.contiguous()

    def check_indices(self):
        """raise if any index handed to the kernels since the last check was not a row of the banks (one host read)"""
        if int(self.bad_index.item()) != 0:
            self.bad_index.zero_()
            raise IndexError(f"ContrastMemory: an index outside [0, {self.nLem}) was met (it was skipped, not dereferenced)")

    def forward(self, v1, v2, y, idx=None):
        """-> (out_v1, out_v2), [B, K+1, 1]: the reference's materialised scores; ends with the bank update"""
        K, T, momentum, set_z = self._state()
        idx = self._indices(y, idx, v1.size(0))
        out_v1, out_v2 = ops.crd_scores(v1, v2, self.memory_v1, self.memory_v2, idx, T, self.nLem, self.params[2:4], set_z,
                                        bad=self.bad_index, update_y=y)
        self._host[3] = False
        ops.crd_update_(self.memory_v1, self.memory_v2, v1.detach().contiguous(), v2.detach().contiguous(), y.contiguous(),
                        momentum, bad=self.bad_index)
        return out_v1.unsqueeze(2), out_v2.unsqueeze(2)

    def forward_fused(self, v1, v2, y, idx=None):
        """-> loss (scalar): ContrastLoss of both sides, summed, with its gradient from the same gather pass; ends with the
        bank update"""
        K, T, momentum, set_z = self._state()
        idx = self._indices(y, idx, v1.size(0))
        loss = ops.crd_fused(v1, v2, self.memory_v1, self.memory_v2, idx, T, self.nLem, self.params[2:4], set_z,
                             bad=self.bad_index)
        self._host[3] = False
        ops.crd_update_(self.memory_v1, self.memory_v2, v1.detach().contiguous(), v2.detach().contiguous(), y.contiguous(),
                        momentum, bad=self.bad_index)
        return loss.sum()

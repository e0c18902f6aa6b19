#!/usr/bin/env python3
"""CRD criterion on one GPU: the fused gather-contrast path against the materialised path and against the reference's op chain
in stock PyTorch (index_select -> bmm -> exp -> div -> ContrastLoss, autograd backward, index_copy_ update) -- the baseline: the
feature has no parent-commit time.

    python scripts/bench_crd.py [--out profiles/crd_bench.txt] [--iters 20] [--warmup 5]

Shapes: (B 64, d 512, nce_k 16384) and (B 64, d 128, nce_k 16384), each with n_data 15303 (banks of 31 / 8 MB: cache-resident, NOT
an HBM measurement) and 1281167 (banks in HBM, 2.6 GB each at d 512).  Timed with HIP events on the current stream after warm-up,
median over the iterations; each iteration uses another of 4 pre-drawn index matrices.
  (a) CRDLoss.forward + backward, fused path        (b) the same, materialised path        (c) the stock op chain, same heads
  (k) the moma_crd_fused call alone (gather pass + combine): gathered GB/s = 2 B K1 d 4 / time, quoted against the 8 TB/s HBM
      figure for the HBM-resident banks only."""
import argparse
import os
import sys
import types

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moma_amd import ops  # noqa: E402
from moma_amd.crd import CRDLoss, ContrastLoss  # noqa: E402

HBM_GBS = 8000.0
S_DIM = T_DIM = 256


class StockCRD(nn.Module):
    """the reference's sequence of stock ops over the same heads and banks as a CRDLoss (Z fixed, as after its first step)"""

    def __init__(self, crd: CRDLoss, n_data, T, momentum, Z):
        super().__init__()
        self.crd, self.T, self.m, self.Z, self.loss = crd, T, momentum, Z, ContrastLoss(n_data)

    def forward(self, f_s, f_t, y, idx):
        v1, v2 = self.crd.embed_s(f_s), self.crd.embed_t(f_t)
        mem = self.crd.contrast
        B, d = v1.shape
        w1 = torch.index_select(mem.memory_v1, 0, idx.view(-1)).detach().view(B, -1, d)
        out_v2 = torch.exp(torch.bmm(w1, v2.view(B, d, 1)) / self.T) / self.Z[1]
        w2 = torch.index_select(mem.memory_v2, 0, idx.view(-1)).detach().view(B, -1, d)
        out_v1 = torch.exp(torch.bmm(w2, v1.view(B, d, 1)) / self.T) / self.Z[0]
        with torch.no_grad():
            for bank, v in ((mem.memory_v1, v1), (mem.memory_v2, v2)):
                r = torch.index_select(bank, 0, y) * self.m + v * (1 - self.m)
                bank.index_copy_(0, y, r / r.pow(2).sum(1, keepdim=True).sqrt())
        return self.loss(out_v1) + self.loss(out_v2)


def timed(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = ["# CRD criterion, forward + backward + bank update, ms (median [min .. max] over %d iterations after %d warm-up), %s"
             % (a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# B  d  nce_k  n_data  banks | (a) fused | (b) materialised | (c) stock op chain | (c)/(a) | (k) moma_crd_fused alone | gathered GB/s"]
    for (B, d, K) in ((64, 512, 16384), (64, 128, 16384)):
        for n_data in (15303, 1281167):
            torch.manual_seed(0)
            opt = types.SimpleNamespace(s_dim=S_DIM, t_dim=T_DIM, feat_dim=d, nce_k=K, nce_t=0.07, nce_m=0.5, n_data=n_data)
            res = {}
            idxs = [torch.randint(0, n_data, (B, K + 1), device=dev) for _ in range(4)]
            ys = [torch.randperm(n_data, device=dev)[:B] for _ in range(4)]
            for i in range(4):
                idxs[i][:, 0] = ys[i]
            f_s, f_t = torch.randn(B, S_DIM, device=dev), torch.randn(B, T_DIM, device=dev)
            for name in ("a", "b", "c"):
                opt.moma_fused = name != "b"
                crd = CRDLoss(opt).to(dev)
                with torch.no_grad():                                    # one step to set Z
                    crd(f_s, f_t, ys[0], idxs[0])
                mod = crd if name != "c" else StockCRD(crd, n_data, 0.07, 0.5, crd.contrast.params[2:4].clone())

                def step(i, mod=mod, crd=crd):
                    crd.zero_grad(set_to_none=True)
                    mod(f_s, f_t, ys[i % 4], idxs[i % 4]).sum().backward()
                res[name] = timed(step, a.iters, a.warmup)
                if name == "a":
                    mem = crd.contrast
                    v1 = torch.nn.functional.normalize(torch.randn(B, d, device=dev)).requires_grad_(True)
                    v2 = torch.nn.functional.normalize(torch.randn(B, d, device=dev)).requires_grad_(True)

                    def kern(i):
                        ops.crd_fused(v1, v2, mem.memory_v1, mem.memory_v2, idxs[i % 4], 0.07, n_data, mem.params[2:4], False,
                                      mem.bad_index)
                    res["k"] = timed(kern, a.iters, a.warmup)
                    mem.check_indices()
                del crd, mod
                torch.cuda.empty_cache()
            gbs = 2.0 * B * (K + 1) * d * 4 / (res["k"][0] * 1e-3) / 1e9
            where = "HBM" if n_data * d * 4 * 2 > (256 << 20) else "cache-resident (not an HBM measurement)"
            f = lambda r: "%.3f [%.3f .. %.3f]" % r                                        # noqa: E731
            lines.append("%d %d %d %d %s | %s | %s | %s | %.2fx | %s | %.0f%s" % (
                B, d, K, n_data, where, f(res["a"]), f(res["b"]), f(res["c"]), res["c"][0] / res["a"][0], f(res["k"]), gbs,
                " (%.0f%% of %.0f GB/s HBM)" % (100 * gbs / HBM_GBS, HBM_GBS) if where == "HBM" else ""))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()

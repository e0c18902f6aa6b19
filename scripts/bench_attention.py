#!/usr/bin/env python3
"""Attention Transfer criterion on one GPU: the fused path (ops.attention_loss: at_map x 2 -> at_pair, at_bwd) against the same
formula in stock PyTorch ops with autograd (Attention.composite) -- the baseline: the feature has no parent-commit time.

    python scripts/bench_attention.py [--out profiles/attention_bench.txt] [--iters 50] [--warmup 10]

Shapes: the four feature pairs of EfficientNet-B0 at 224 px that `feat[1:-1]` holds, student = teacher architecture:
[B,24,56,56], [B,40,28,28], [B,112,14,14], [B,1280,7,7], for B in {64, 256}, as fp32 NCHW and as bf16 channels_last (what
`--amp bf16 --channels_last` hands over).  Per shape and for the sum of the four: criterion forward + backward (gradient to the
student only, the teacher's map detached), timed with HIP events around the whole call after warm-up, median [min .. max]; fused
and stock alternate inside one process.  GB/s = algorithmic bytes / median time, the algorithmic bytes being 3 passes over the
student's map (read forward, read + write backward) and 1 over the teacher's; the times are whole calls (launch gaps of the 5
launches included), not kernel times, so the rate is a lower bound of what the kernels reach."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moma_amd import ops  # noqa: E402
from moma_amd.distiller_zoo import Attention  # noqa: E402

SHAPES = [(24, 56), (40, 28), (112, 14), (1280, 7)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    crit = Attention()
    lines = ["# Attention Transfer criterion, forward + backward, us per call (median [min .. max] over %d iterations after %d "
             "warm-up, fused and stock alternating), %s" % (a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# config  B  C  HxW | MB algorithmic (3 student + 1 teacher passes) | fused us | fused GB/s | stock torch us | stock/fused"]
    f = lambda r: "%.1f [%.1f .. %.1f]" % tuple(1e3 * v for v in r)                # noqa: E731
    for name, dtype, mf in (("fp32-NCHW", torch.float32, torch.contiguous_format), ("bf16-channels_last", torch.bfloat16, torch.channels_last)):
        for B in (64, 256):
            torch.manual_seed(0)
            pairs = []
            for C, H in SHAPES:
                s = torch.randn(B, C, H, H, device=dev).to(dtype).contiguous(memory_format=mf).requires_grad_(True)
                t = torch.randn(B, C, H, H, device=dev).to(dtype).contiguous(memory_format=mf)
                pairs.append((s, t))

            def run(fn, ps):
                def step():
                    for s, _t in ps:
                        s.grad = None
                    sum(fn(s, t) for s, t in ps).backward()
                return step
            total = {"bytes": 0}
            rows = [(("%d %dx%d" % (C, H, H)), [p]) for (C, H), p in zip(SHAPES, pairs)] + [("all four pairs (the KD term)", pairs)]
            for label, ps in rows:
                nbytes = sum(4 * s.numel() * s.element_size() for s, _t in ps)
                fused = timed(run(ops.attention_loss, ps), a.iters, a.warmup)
                stock = timed(run(crit.composite, ps), a.iters, a.warmup)
                fused2 = timed(run(ops.attention_loss, ps), a.iters, a.warmup)
                if fused2[0] < fused[0]:
                    fused = fused2
                lines.append("%s %d %s | %.1f | %s | %.0f | %s | %.2fx" % (
                    name, B, label, nbytes / 1e6, f(fused), nbytes / (fused[0] * 1e-3) / 1e9, f(stock), stock[0] / fused[0]))
                print(lines[-1], flush=True)
            del pairs
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

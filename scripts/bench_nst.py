#!/usr/bin/env python3
"""Neuron Selectivity Transfer criterion on one GPU: the fused path (ops.nst_loss: nst_gram + nst_loss, nst_bwd) against the same
formula in stock PyTorch ops with autograd (NSTLoss.composite in float32: F.normalize + bmm) -- the baseline: the feature has no
parent-commit time, and the reference's own broadcast form does not fit these shapes (a [B, C, C, H W] temporary).

    python scripts/bench_nst.py [--out profiles/nst_bench.txt] [--iters 30] [--warmup 5]

Shapes: the three feature pairs of EfficientNet-B0 at 224 px that `feat[1:-2]` holds, student = teacher architecture:
[B,24,56,56], [B,40,28,28], [B,112,14,14], for B in {64, 256}, as fp32 NCHW and as bf16 channels_last (what `--amp bf16
--channels_last` hands over).  Per shape and for the sum of the three: criterion forward + backward (gradient to the student only,
the teacher's map detached), timed with HIP events around the whole call after warm-up, median [min .. max]; fused and stock
alternate inside one process (stock, fused, stock, fused: both medians of either side are printed, the better one of EACH side makes
the ratio).  Forward alone is timed too (under no_grad), so the two kernels can be told apart: backward = whole call - forward.
Per row: GFLOP of the two matrix products (2 B Cs (Cs + Ct) P each way), the algorithmic bytes (forward: one read of both maps + G
written; backward: one read of both maps + G read + dF written), the bytes nst_gram REQUESTS (every one of its ceil(Cs / 32)
row-block workgroups of an image stages both maps whole: 1 / 2 / 4 reads at 24 / 40 / 112 channels; whether the repeats are served
by L2 / MALL is not measured here), and the fractions of the 157.3 TF f32 matrix rate and of 8 TB/s HBM (algorithmic bytes) that
the times amount to -- host-timed calls, launch gaps and allocations included, so lower bounds of what the kernels reach."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moma_amd import ops  # noqa: E402
from moma_amd.distiller_zoo import NSTLoss  # noqa: E402

SHAPES = [(24, 56), (40, 28), (112, 14)]
PEAK_TF, PEAK_TBS = 157.3, 8.0


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    crit = NSTLoss()
    lines = ["# NST criterion, us per call (median [min .. max] over %d iterations after %d warm-up, fused and stock alternating), %s"
             % (a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# config  B  C  HxW | GFLOP each way | MB fwd (requested by nst_gram) / bwd | fused fwd+bwd us, 1st and 2nd run | "
             "fused fwd us | stock torch fwd+bwd us, 1st and 2nd run | stock/fused (better median of each) | fwd: %% of %.1f TF, %% of %.0f TB/s | bwd: %% of TF, %% of TB/s" % (PEAK_TF, PEAK_TBS)]
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

            def fwd(fn, ps):
                def step():
                    with torch.no_grad():
                        sum(fn(s, t) for s, t in ps)
                return step
            rows = [(("%d %dx%d" % (C, H, H)), [p]) for (C, H), p in zip(SHAPES, pairs)] + [("all three pairs (the KD term)", pairs)]
            for label, ps in rows:
                flop = sum(2.0 * B * s.shape[1] * (s.shape[1] + t.shape[1]) * s.shape[2] * s.shape[3] for s, t in ps)
                gbytes = sum(4.0 * B * s.shape[1] * (s.shape[1] + t.shape[1]) for s, t in ps)
                maps = sum((s.numel() + t.numel()) * s.element_size() for s, t in ps)
                b_fwd = maps + gbytes
                b_req = gbytes + sum(-(-s.shape[1] // 32) * (s.numel() + t.numel()) * s.element_size() for s, t in ps)
                b_bwd = maps + gbytes + sum(s.numel() * s.element_size() for s, _t in ps)
                run_stock, run_fused = run(lambda s, t: crit.composite(s, t, torch.float32), ps), run(ops.nst_loss, ps)
                stock1 = timed(run_stock, a.iters, a.warmup)
                fused1 = timed(run_fused, a.iters, a.warmup)
                stock2 = timed(run_stock, a.iters, a.warmup)
                fused2 = timed(run_fused, a.iters, a.warmup)
                stock, fused = min(stock1, stock2), min(fused1, fused2)
                ffwd = timed(fwd(ops.nst_loss, ps), a.iters, a.warmup)
                t_f, t_b = ffwd[0] * 1e-3, max(fused[0] - ffwd[0], 1e-6) * 1e-3
                lines.append("%s %d %s | %.2f | %.1f (%.1f) / %.1f | %s, %s | %s | %s, %s | %.2fx | %.1f%% %.1f%% | %.1f%% %.1f%%" % (
                    name, B, label, flop / 1e9, b_fwd / 1e6, b_req / 1e6, b_bwd / 1e6, f(fused1), f(fused2), f(ffwd), f(stock1), f(stock2),
                    stock[0] / fused[0],
                    100 * flop / t_f / (PEAK_TF * 1e12), 100 * b_fwd / t_f / (PEAK_TBS * 1e12),
                    100 * flop / t_b / (PEAK_TF * 1e12), 100 * b_bwd / t_b / (PEAK_TBS * 1e12)))
                print(lines[-1], flush=True)
            del pairs
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The tail of the FitNets hint on one GPU -- everything behind the regressor's convolution: training-mode BatchNorm, ReLU, mean
squared error, forward + backward -- as the fused pair (ops.hint_bn_relu_mse: moma_hint_fwd forward, moma_hint_bwd backward) against
the stock form (F.batch_norm -> relu -> mse_loss with autograd in the storage's dtype, what ConvReg.forward + HintLoss run).

    python scripts/bench_hint.py [--out profiles/hint_layer_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--batch 256] [--dtypes fp32,bf16]

Shapes: the five maps feat[hint_layer], hint_layer = 0 .. 4, of EfficientNet-B0 at the benchmark's image size and batch (256 images
of 224 pixels): 16 x 112 x 112, 24 x 56 x 56, 40 x 28 x 28, 112 x 14 x 14 and 1280 x 7 x 7, in fp32 and bf16 storage, NCHW and
channels_last (both sides alike).  Gradients go to x, gamma and beta, the target is detached, the running statistics are updated.
Timed with HIP events around the whole forward + backward after warm-up.  The routes alternate inside one process, `rounds` times
over (stock, fused, stock, ...); a route's figure is the median of its round medians, its spread their min .. max.  Verdict per row,
the project's standing one: the fused route `holds` when its median is at most the stock form's plus the stock form's own spread
(max - min of its round medians), `LOSES` otherwise -- such a row belongs to the composite in ops.hint_native.
Algorithmic bytes of the fused pair: x three times, t twice, dx once = 6 B C P e (e = bytes per element); the fraction of the HBM
rate is those bytes over the fused route's time, against 8 TB/s.  The two C-ABI calls are then timed one by one on preallocated
buffers (events around ONE call: the launches are inside, so these are upper bounds of the kernels' times)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0
MAPS = [(16, 112, 112), (24, 56, 56), (40, 28, 28), (112, 14, 14), (1280, 7, 7)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
LAYOUTS = {"NCHW": torch.contiguous_format, "channels_last": torch.channels_last}
EPS, MOM = 1e-5, 0.1


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
    return 1e3 * ts[len(ts) // 2]


def inputs(B, C, H, W, dtype, mf, dev):
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device=dev).to(dtype).contiguous(memory_format=mf).requires_grad_(True)
    t = torch.relu(torch.randn(B, C, H, W, device=dev)).to(dtype).contiguous(memory_format=mf)
    return x, t


def abi_times(x, t, gamma, beta, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _map_side, _ptr, _stream
    lib = _lib.load()
    x, ga, be, dev = x.detach(), gamma.detach(), beta.detach(), x.device
    B, C, H, W = x.shape
    lay_x, lay_t = (_map_side(f, nm, "hint_bn_relu_mse", "ConvReg") for f, nm in ((x, "x"), (t, "target")))
    codes = (_DT_CODES[x.dtype], lay_x, _DT_CODES[t.dtype], lay_t)
    n = lib.moma_hint_workspace_bytes(B, C, H * W, *codes)
    ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
    mean, invstd = (torch.empty(C, device=dev, dtype=torch.float64) for _ in range(2))
    sums = torch.empty(2 * C, device=dev, dtype=torch.float64)
    rm, rv, dga, dbe = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    loss, g = torch.empty((), device=dev), torch.ones((), device=dev)
    dx = torch.empty_like(x)
    calls = {
        "fwd": lambda: _lib.check(lib.moma_hint_fwd(_ptr(x), _ptr(t), _ptr(ga), _ptr(be), None, _ptr(rm), _ptr(rv), MOM, EPS, B, C, H * W,
                                                    *codes, _ptr(ws), n, _ptr(mean), _ptr(invstd), _ptr(sums), _ptr(loss), _stream()), "fwd"),
        "bwd": lambda: _lib.check(lib.moma_hint_bwd(_ptr(x), _ptr(t), _ptr(ga), _ptr(be), _ptr(mean), _ptr(invstd), _ptr(sums), _ptr(g),
                                                    _ptr(dx), _ptr(dga), _ptr(dbe), B, C, H * W, *codes, _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup) for k, fn in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtypes", default="fp32,bf16", help="storage types in the order they are timed")
    a = ap.parse_args()
    from moma_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_hint: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    B = a.batch
    lines = ["# hint tail (BatchNorm -> ReLU -> MSE), us per forward + backward (median [min .. max] of %d round medians, %d iterations "
             "after %d warm-up each, the routes alternating), B = %d, %s" % (a.rounds, a.iters, a.warmup, B, torch.cuda.get_device_name(0)),
             "# dtype layout C H W | fused | stock ops | stock/fused | verdict (fused <= stock + the stock form's spread) | algorithmic MB "
             "(6 B C P e) | fused: fraction of %.0f TB/s | one C-ABI call each, us (launches included): fwd [fraction of the HBM rate at "
             "3 B C P e] bwd [.. at 3 B C P e]" % PEAK_TBS]
    losers = []
    for name in a.dtypes.split(","):
        dtype = DTYPES[name]
        for lay, mf in LAYOUTS.items():
            for C, H, W in MAPS:
                gamma = torch.linspace(0.5, 1.5, C, device=dev).requires_grad_(True)
                beta = torch.linspace(-0.3, 0.3, C, device=dev).requires_grad_(True)
                rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
                x, t = inputs(B, C, H, W, dtype, mf, dev)

                def stock():
                    x.grad = gamma.grad = beta.grad = None
                    F.mse_loss(F.relu(F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS)), t).backward()

                def fused():
                    x.grad = gamma.grad = beta.grad = None
                    ops.hint_bn_relu_mse(x, t, gamma, beta, rm, rv, MOM, EPS).backward()

                routes = {"stock": stock, "fused": fused}
                got = {k: [] for k in routes}
                for _ in range(a.rounds):
                    for k, fn in routes.items():
                        got[k].append(timed(fn, a.iters, a.warmup))
                k = abi_times(x, t, gamma, beta, a.iters, a.warmup)
                unit = B * C * H * W * x.element_size()
                frac = lambda us, nbytes: nbytes / (us * 1e-6) / (PEAK_TBS * 1e12)   # noqa: E731
                holds = med(got["fused"]) <= med(got["stock"]) + (max(got["stock"]) - min(got["stock"]))
                if not holds:
                    losers.append("%s %s %d x %d x %d" % (name, lay, C, H, W))
                lines.append("%s %s %d %d %d | %s | %s | %.2fx | %s | %.1f | %.3f | fwd %.1f [%.3f]  bwd %.1f [%.3f]" % (
                    name, lay, C, H, W, f(got["fused"]), f(got["stock"]), med(got["stock"]) / med(got["fused"]),
                    "holds" if holds else "LOSES", 6 * unit / 1e6, frac(med(got["fused"]), 6 * unit), k["fwd"], frac(k["fwd"], 3 * unit),
                    k["bwd"], frac(k["bwd"], 3 * unit)))
                print(lines[-1], flush=True)
                del x, t, routes, stock, fused
                torch.cuda.empty_cache()
    lines.append("# rows where the fused pair is slower than the stock form by more than the stock form's spread: %s" % (", ".join(losers) or "none"))
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

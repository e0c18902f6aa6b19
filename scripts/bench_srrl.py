#!/usr/bin/env python3
"""The tail of SRRL on one GPU -- everything behind the connector's convolution: training-mode BatchNorm, ReLU, the mean squared error
against the teacher's feature, the teacher's classifier and the mean squared error against the teacher's logits, forward + backward --
as the fused pair (ops.srrl_bn_relu_dual_mse: moma_srrl_fwd forward, moma_srrl_bwd backward) against the stock form
(F.batch_norm -> relu -> mse_loss, F.linear -> mse_loss with autograd in the storage's dtype, what SRRL.forward + nn.MSELoss run).

    python scripts/bench_srrl.py [--out profiles/srrl_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--batch 256] [--dtypes fp32,bf16]

Shapes: B = 256 (the benchmark's batch), (t_n, n_cls) in (1280, 4), (1280, 8), (1280, 1000), (256, 100), (2048, 1000), (768, 1000), in
fp32 and bf16 storage (x and the teacher's feature alike; the classifier and the logits stay fp32 in the fused route and take the
storage's dtype in the stock one, as autocast would leave them).  Gradients go to x, gamma and beta; the target, the logits and the
classifier are constant; the running statistics are updated.
Timed with HIP events around the whole forward + backward after warm-up.  The routes alternate inside one process, `rounds` times
over (stock, fused, stock, ...); a route's figure is the median of its round medians, its spread their min .. max.  Verdict per row,
the project's standing one: the fused route `holds` when its median is at most the stock form's plus the stock form's own spread
(max - min of its round medians), `LOSES` otherwise -- such a row belongs to the composite in ops.srrl_native.
The two C-ABI calls are then timed one by one on preallocated buffers (events around ONE call: the launches are inside, so these are
upper bounds of the kernels' times).  Launches per step: fused 5 forward + 1 backward; the stock form's are counted with the profiler
(kernels of one forward + backward)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1280, 4), (1280, 8), (1280, 1000), (256, 100), (2048, 1000), (768, 1000)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
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


def abi_times(x, t, W, b, l, gamma, beta, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    x, ga, be, dev = x.detach(), gamma.detach(), beta.detach(), x.device
    B, C = x.shape
    K = W.shape[0]
    codes = (_DT_CODES[x.dtype], _DT_CODES[t.dtype])
    n = lib.moma_srrl_workspace_bytes(B, C, K)
    ws = torch.empty((n + 7) // 8, device=dev, dtype=torch.float64)
    sums = torch.empty(2 * C, device=dev, dtype=torch.float64)
    dxu = torch.empty(B * C, device=dev)
    rm, rv, dga, dbe = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    loss, g = torch.empty((), device=dev), torch.ones((), device=dev)
    dx = torch.empty_like(x)
    calls = {
        "fwd": lambda: _lib.check(lib.moma_srrl_fwd(_ptr(x), _ptr(t), _ptr(W), _ptr(b), _ptr(l), _ptr(ga), _ptr(be), _ptr(rm), _ptr(rv), MOM,
                                                    EPS, B, C, K, *codes, _ptr(ws), n, _ptr(sums), _ptr(dxu), _ptr(loss), None, None,
                                                    _stream()), "fwd"),
        "bwd": lambda: _lib.check(lib.moma_srrl_bwd(_ptr(dxu), _ptr(sums), _ptr(g), _ptr(dx), _ptr(dga), _ptr(dbe), B, C, codes[0],
                                                    _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup) for k, fn in calls.items()}


def count_kernels(fn):
    """kernels (memory copies and memsets included) of one call of fn, by torch's profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtypes", default="fp32,bf16", help="storage types in the order they are timed")
    ap.add_argument("--count_launches", action="store_true", help="count the kernels of one forward + backward of each route")
    a = ap.parse_args()
    from moma_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_srrl: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    B = a.batch
    lines = ["# srrl tail (BatchNorm -> ReLU -> MSE, classifier -> MSE), us per forward + backward (median [min .. max] of %d round "
             "medians, %d iterations after %d warm-up each, the routes alternating), B = %d, %s"
             % (a.rounds, a.iters, a.warmup, B, torch.cuda.get_device_name(0)),
             "# dtype t_n n_cls | fused | stock ops | stock/fused | verdict (fused <= stock + the stock form's spread) | one C-ABI call "
             "each, us (launches included): fwd bwd | kernels per forward + backward: fused, stock"]
    losers = []
    for name in a.dtypes.split(","):
        dtype = DTYPES[name]
        for C, K in SHAPES:
            torch.manual_seed(0)
            gamma = torch.linspace(0.5, 1.5, C, device=dev).requires_grad_(True)
            beta = torch.linspace(-0.3, 0.3, C, device=dev).requires_grad_(True)
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            x = torch.randn(B, C, device=dev).to(dtype).requires_grad_(True)
            t = torch.relu(torch.randn(B, C, device=dev)).to(dtype)
            W = (torch.rand(K, C, device=dev) * 2 - 1) / C ** 0.5
            b = (torch.rand(K, device=dev) * 2 - 1) / C ** 0.5
            l = torch.randn(B, K, device=dev)
            Ws, bs, ls = W.to(dtype), b.to(dtype), l.to(dtype)

            def stock():
                x.grad = gamma.grad = beta.grad = None
                y = F.relu(F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS))
                (F.mse_loss(y, t) + F.mse_loss(F.linear(y, Ws, bs), ls)).backward()

            def fused():
                x.grad = gamma.grad = beta.grad = None
                ops.srrl_bn_relu_dual_mse(x, t, W, b, l, gamma, beta, rm, rv, MOM, EPS).backward()

            routes = {"stock": stock, "fused": fused}
            got = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    got[k].append(timed(fn, a.iters, a.warmup))
            k = abi_times(x, t, W, b, l, gamma, beta, a.iters, a.warmup)
            nk = "%d, %d" % (count_kernels(fused), count_kernels(stock)) if a.count_launches else "-"
            holds = med(got["fused"]) <= med(got["stock"]) + (max(got["stock"]) - min(got["stock"]))
            if not holds:
                losers.append("%s %d x %d" % (name, C, K))
            lines.append("%s %d %d | %s | %s | %.2fx | %s | fwd %.1f  bwd %.1f | %s" % (
                name, C, K, f(got["fused"]), f(got["stock"]), med(got["stock"]) / med(got["fused"]), "holds" if holds else "LOSES",
                k["fwd"], k["bwd"], nk))
            print(lines[-1], flush=True)
            del x, t, routes, stock, fused
    lines.append("# rows where the fused pair is slower than the stock form by more than the stock form's spread: %s" % (", ".join(losers) or "none"))
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

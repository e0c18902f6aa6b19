#!/usr/bin/env python3
"""Correlation Congruence on one GPU -- both LinearEmbed heads, |f_s - f_t|, the product of neighbouring rows, forward + backward -- as
the fused pair (ops.cc_embed_neighbour: moma_cc_fwd forward, moma_cc_bwd backward) against the stock form (two F.linear, the
subtraction, abs, two slices, the product, both reductions, with autograd in the storage's dtype: what LinearEmbed.forward and
Correlation.forward run).

    python scripts/bench_cc.py [--out profiles/cc_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--batches 64,256] [--dtypes fp32,bf16]

Shapes: B in (64, 256), feat[-1] of width 256, 768, 1280, 2048 on both sides, --feat_dim 128 and 512, in two series: fp32 and bf16
storage (x_s and x_t alike; the heads stay fp32 in the fused route and take the storage's dtype in the stock one, as autocast would
leave them -- as leaves, so the stock form is spared autocast's casts).  Gradients go to x_s and to both heads' weights and biases; x_t is
constant.
Timed with HIP events around the whole forward + backward after warm-up.  The routes alternate inside one process, `rounds` times
over (stock, fused, stock, ...); a route's figure is the median of its round medians, its spread their min .. max.  Verdict per row,
the project's standing one: the fused route `holds` when its median is at most the stock form's plus the stock form's own spread
(max - min of its round medians), `LOSES` otherwise -- such a shape class belongs to the composite in ops.cc_native.
The two C-ABI calls are then timed one by one on preallocated buffers (events around ONE call: the launches are inside, so these are
upper bounds of the kernels' times).  Launches per step: fused 3 forward + 1 backward; the stock form's are counted with the profiler
(kernels of one forward + backward)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = [256, 768, 1280, 2048]
FEAT_DIMS = [128, 512]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


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


def abi_times(x_s, x_t, W_s, b_s, W_t, b_t, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    x_s, dev = x_s.detach(), x_s.device
    B, Cs = x_s.shape
    Ct, D = x_t.shape[1], W_s.shape[0]
    codes = (_DT_CODES[x_s.dtype], _DT_CODES[x_t.dtype])
    n = lib.moma_cc_workspace_bytes(B, Cs, Ct, D)
    ws = torch.empty((n + 7) // 8, device=dev, dtype=torch.float64)
    gu = torch.empty(B, D, device=dev)
    loss, g = torch.empty((), device=dev), torch.ones((), device=dev)
    dx, dws, dbs, dwt, dbt = (torch.empty_like(v) for v in (x_s, W_s, b_s, W_t, b_t))
    calls = {
        "fwd": lambda: _lib.check(lib.moma_cc_fwd(_ptr(x_s), _ptr(x_t), _ptr(W_s), _ptr(b_s), _ptr(W_t), _ptr(b_t), B, Cs, Ct, D, *codes,
                                                  _ptr(ws), n, _ptr(gu), _ptr(loss), None, _stream()), "fwd"),
        "bwd": lambda: _lib.check(lib.moma_cc_bwd(_ptr(gu), _ptr(x_s), _ptr(x_t), _ptr(W_s), _ptr(g), _ptr(dx), _ptr(dws), _ptr(dbs),
                                                  _ptr(dwt), _ptr(dbt), B, Cs, Ct, D, *codes, _stream()), "bwd"),
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
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--dtypes", default="fp32,bf16", help="the series: storage types in the order they are timed")
    ap.add_argument("--count_launches", action="store_true", help="count the kernels of one forward + backward of each route")
    a = ap.parse_args()
    from moma_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_cc: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    lines = ["# correlation congruence (two LinearEmbed heads -> |f_s - f_t| -> neighbouring-row product), us per forward + backward "
             "(median [min .. max] of %d round medians, %d iterations after %d warm-up each, the routes alternating), %s"
             % (a.rounds, a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# dtype B width feat_dim | fused | stock ops | stock/fused | verdict (fused <= stock + the stock form's spread) | one C-ABI "
             "call each, us (launches included): fwd bwd | kernels per forward + backward: fused, stock"]
    losers = []
    for name in a.dtypes.split(","):
        dtype = DTYPES[name]
        for B in (int(v) for v in a.batches.split(",")):
            for Cw in WIDTHS:
                for D in FEAT_DIMS:
                    torch.manual_seed(0)
                    x_s = torch.randn(B, Cw, device=dev).to(dtype).requires_grad_(True)
                    x_t = torch.randn(B, Cw, device=dev).to(dtype)
                    mk = lambda *s: ((torch.rand(*s, device=dev) * 2 - 1) / Cw ** 0.5).requires_grad_(True)     # noqa: E731
                    W_s, b_s, W_t, b_t = mk(D, Cw), mk(D), mk(D, Cw), mk(D)
                    stock_p = [p.detach().to(dtype).requires_grad_(True) for p in (W_s, b_s, W_t, b_t)]

                    def stock():
                        x_s.grad = None
                        for p in stock_p:
                            p.grad = None
                        delta = torch.abs(F.linear(x_s, stock_p[0], stock_p[1]) - F.linear(x_t, stock_p[2], stock_p[3]))
                        torch.mean((delta[:-1] * delta[1:]).sum(1)).backward()

                    def fused():
                        x_s.grad = W_s.grad = b_s.grad = W_t.grad = b_t.grad = None
                        ops.cc_embed_neighbour(x_s, x_t, W_s, b_s, W_t, b_t).backward()

                    routes = {"stock": stock, "fused": fused}
                    got = {k: [] for k in routes}
                    for _ in range(a.rounds):
                        for k, fn in routes.items():
                            got[k].append(timed(fn, a.iters, a.warmup))
                    k = abi_times(x_s, x_t, W_s.detach(), b_s.detach(), W_t.detach(), b_t.detach(), a.iters, a.warmup)
                    nk = "%d, %d" % (count_kernels(fused), count_kernels(stock)) if a.count_launches else "-"
                    holds = med(got["fused"]) <= med(got["stock"]) + (max(got["stock"]) - min(got["stock"]))
                    if not holds:
                        losers.append("%s B %d width %d feat_dim %d" % (name, B, Cw, D))
                    lines.append("%s %d %d %d | %s | %s | %.2fx | %s | fwd %.1f  bwd %.1f | %s" % (
                        name, B, Cw, D, f(got["fused"]), f(got["stock"]), med(got["stock"]) / med(got["fused"]),
                        "holds" if holds else "LOSES", k["fwd"], k["bwd"], nk))
                    print(lines[-1], flush=True)
                    del x_s, x_t, routes, stock, fused
    lines.append("# rows where the fused pair is slower than the stock form by more than the stock form's spread: %s" % (", ".join(losers) or "none"))
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

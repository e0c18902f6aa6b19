#!/usr/bin/env python3
"""Probabilistic Knowledge Transfer criterion on one GPU: the fused path (ops.pkt_loss: pkt_gram_pair, pkt_terms = pkt_rows + pkt_m,
pkt_bwd -- three launches forward, one backward) against two routes in stock PyTorch ops with autograd:
  (a) the criterion's composite (PKT.composite as the criterion runs it: float64);
  (b) the published form of the loss typed out in stock ops as published, in float32: rows / (norm + eps), mm with the transpose,
      (. + 1) / 2, rows / row sums, mean of T log((T + eps) / (P + eps)).

    python scripts/bench_pkt.py [--out profiles/pkt_bench.txt] [--iters 20] [--warmup 3] [--rounds 3]
    python scripts/bench_pkt.py --fused-only [--only B dtype]     # the fused route alone: the program of a kernel trace

Shapes: B in {64, 256}, Ds = Dt = 1280 (EfficientNet-B0's feat[-1] against itself), fp32 and bf16 storage.  Criterion forward +
backward (gradient to the student only, the teacher's feature detached), timed with HIP events around the whole call after
warm-up.  The three routes alternate, `rounds` times over; per route the median [min .. max] of its round medians.  Verdict per
row: fused <= stock + the stock route's own spread between its round medians (max - min).  The C-ABI calls are then timed one by
one on preallocated buffers (events around ONE call: the launch is inside, so these are upper bounds of the kernels' times); the
sum of the op's three calls is the launch-bound share of the fused time."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [(64, 1280, 1280), (256, 1280, 1280)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
EPS = 1e-7


def timed(fn, iters, warmup):
    """median ms of `iters` calls after `warmup`"""
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
    return ts[len(ts) // 2]


def inputs(B, Ds, Dt, dtype, dev):
    torch.manual_seed(0)
    s = torch.relu(torch.randn(B, Ds, device=dev)).to(dtype).requires_grad_(True)       # (feat[-1] is post-ReLU / post-pool)
    return s, torch.relu(torch.randn(B, Dt, device=dev)).to(dtype)


def published(f_s, f_t, eps=EPS):
    """the published form in stock float32 ops"""
    def prob(f):
        x = f.float().view(f.shape[0], -1)
        x = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)
        k = (torch.mm(x, x.t()) + 1.0) / 2.0
        return k / torch.sum(k, dim=1, keepdim=True)
    p, t = prob(f_s), prob(f_t)
    return torch.mean(t * torch.log((t + eps) / (p + eps)))


def step_of(fn, s, t):
    def step():
        s.grad = None
        fn(s, t).backward()
    return step


def abi_times(B, Ds, Dt, dtype, dev, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    s, t = inputs(B, Ds, Dt, dtype, dev)
    s = s.detach()
    G = torch.empty(2, B, B, device=dev, dtype=torch.float64)
    M = torch.empty(B, B, device=dev, dtype=torch.float64)
    n = lib.moma_pkt_workspace_bytes(B)
    ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
    loss, g = torch.empty((), device=dev), torch.ones((), device=dev)
    dF = torch.empty_like(s)
    code = _DT_CODES[dtype]
    calls = {
        "gram_pair": lambda: _lib.check(lib.moma_pkt_gram_pair(_ptr(s), Ds, code, _ptr(t), Dt, code, B, _ptr(G[0]), _ptr(G[1]), _stream()),
                                        "gram_pair"),
        "gram_one_side": lambda: _lib.check(lib.moma_pkt_gram(_ptr(s), B, Ds, code, _ptr(G[0]), _stream()), "gram"),
        "terms": lambda: _lib.check(lib.moma_pkt_terms(_ptr(G[0]), _ptr(G[1]), B, _ptr(ws), n, _ptr(M), _ptr(loss), _stream()), "terms"),
        "bwd": lambda: _lib.check(lib.moma_pkt_bwd(_ptr(s), _ptr(M), _ptr(g), _ptr(dF), B, Ds, code, _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup) * 1e3 for k, fn in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--only", nargs=2, default=None, metavar=("B", "dtype"), help="with --fused-only: that shape alone")
    a = ap.parse_args()
    from moma_amd import ops
    from moma_amd.distiller_zoo import PKT
    dev = torch.device("cuda", 0)
    crit = PKT()
    if a.fused_only:
        for name, dtype in DTYPES.items():
            for B, Ds, Dt in CONFIGS:
                if a.only and (str(B), name) != tuple(a.only):
                    continue
                s, t = inputs(B, Ds, Dt, dtype, dev)
                print(name, B, "%.1f us" % (1e3 * timed(step_of(ops.pkt_loss, s, t), a.iters, a.warmup)), flush=True)
        return
    f = lambda r: "%.1f [%.1f .. %.1f]" % (1e3 * sorted(r)[len(r) // 2], 1e3 * min(r), 1e3 * max(r))          # noqa: E731
    med = lambda r: sorted(r)[len(r) // 2]                                                                     # noqa: E731
    lines = ["# PKT criterion, us per forward + backward (median [min .. max] of %d round medians, %d iterations after %d warm-up each, "
             "the routes alternating), %s" % (a.rounds, a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# dtype B Ds Dt | fused | (b) stock fp32 | (b)/fused | verdict (fused <= stock + stock's spread) | (a) composite float64 | "
             "(a)/fused | fused forward only | one C-ABI call each, us (launch included): gram_pair (both sides, what the op calls), "
             "gram of one side for comparison, terms, bwd | sum of the op's three calls"]
    worst = 0.0
    for name, dtype in DTYPES.items():
        for B, Ds, Dt in CONFIGS:
            s, t = inputs(B, Ds, Dt, dtype, dev)
            routes = {"fused": step_of(ops.pkt_loss, s, t), "comp": step_of(crit.composite, s, t), "stock": step_of(published, s, t)}
            r = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    r[k].append(timed(fn, a.iters, a.warmup))

            def fwd():
                with torch.no_grad():
                    ops.pkt_loss(s, t)
            ffwd = timed(fwd, a.iters, a.warmup)
            k = abi_times(B, Ds, Dt, dtype, dev, a.iters, a.warmup)
            fused, stock, comp = med(r["fused"]), med(r["stock"]), med(r["comp"])
            ok = fused <= stock + (max(r["stock"]) - min(r["stock"]))
            worst = max(worst, fused / stock)
            lines.append("%s %d %d %d | %s | %s | %.2fx | %s | %s | %.2fx | %.1f | %s | %.1f" % (
                name, B, Ds, Dt, f(r["fused"]), f(r["stock"]), stock / fused, "ok" if ok else "SLOWER", f(r["comp"]), comp / fused,
                1e3 * ffwd, "  ".join("%s %.1f" % (c, k[c]) for c in k), sum(v for c, v in k.items() if c != "gram_one_side")))
            print(lines[-1], flush=True)
            del s, t
            torch.cuda.empty_cache()
    lines.append("# worst fused / stock over the rows: %.2f" % worst)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The teacher trainer's classification head on one GPU -- cross-entropy, top-1 and (in validation) the confusion matrix -- as the
fused head (helper.ce_head.CrossEntropyHead with its device meter: moma_ce_fwd, moma_ce_bwd) against the stock chain, in two series:

    train       forward + backward.  stock: F.cross_entropy + helper.util.accuracy (topk, eq, sum, mul) + loss.backward(), what the
                reference's train_vanilla runs per step, its two values left on the device.  fused: head(z, y).backward().
    validation  no-grad forward.  stock: F.cross_entropy + helper.util.accuracy + argmax + bincount into a [K * K] matrix and three
                running sums, what helper.loops_moma.validate_distill runs per batch.  fused: head(z, y).

    python scripts/bench_ce.py [--out profiles/ce_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--count_launches]

Shapes: B in (64, 256) x K in (4, 9, 100, 1000), fp32 and bf16 logits (the stock chain gets `.float()` logits for bf16, as the loops
hand them to nn.CrossEntropyLoss; that cast and its backward are part of its time).
Timed with HIP events around the whole call after warm-up.  The routes alternate inside one process, `rounds` times over (stock,
fused, stock, ...); a route's figure is the median of its round medians, its spread their min .. max.  Verdict per row, the project's
standing one: the row `holds` when in BOTH series the fused median is at most the stock chain's plus the stock chain's own spread
(max - min of its round medians), `LOSES` otherwise -- such a shape class belongs to the composite in ops.ce_native.
The two C-ABI calls are then timed one by one on preallocated buffers (events around ONE call: the launches are inside, so these are
upper bounds of the kernels' times).  Launches per call: fused 2 forward + 1 backward; both routes' kernels are counted with torch's
profiler (--count_launches)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = [64, 256]
CLASSES = [4, 9, 100, 1000]
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


def abi_times(z, y, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    z, dev = z.detach(), z.device
    B, K = z.shape
    code = _DT_CODES[z.dtype]
    n = lib.moma_ce_workspace_bytes(B, K)
    ws = torch.empty((n + 7) // 8, device=dev, dtype=torch.float64)
    lse, inv_n = torch.empty(B, device=dev, dtype=torch.float64), torch.empty(1, device=dev, dtype=torch.float64)
    stats, conf = torch.zeros(4, device=dev, dtype=torch.float64), torch.zeros(K, K, device=dev, dtype=torch.int64)
    loss, g, dz = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(z)
    calls = {
        "fwd": lambda: _lib.check(lib.moma_ce_fwd(_ptr(z), _ptr(y), B, K, code, _ptr(ws), ws.numel() * 8, _ptr(loss), _ptr(lse), _ptr(inv_n),
                                                  None, _ptr(stats), _ptr(conf), _stream()), "fwd"),
        "bwd": lambda: _lib.check(lib.moma_ce_bwd(_ptr(z), _ptr(y), _ptr(lse), _ptr(inv_n), _ptr(g), _ptr(dz), B, K, code, _stream()), "bwd"),
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
    ap.add_argument("--count_launches", action="store_true", help="count the kernels of one call of each route in each series")
    a = ap.parse_args()
    from moma_amd.helper.ce_head import CrossEntropyHead
    from moma_amd.helper.util import accuracy
    if not torch.cuda.is_available():
        raise SystemExit("bench_ce: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    lines = ["# classification head (cross-entropy + top-1; validation: + confusion matrix), us per call (median [min .. max] of %d round "
             "medians, %d iterations after %d warm-up each, the routes alternating), %s" % (a.rounds, a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# dtype B K | train (forward + backward): fused | stock | stock/fused || validation (no-grad forward): fused | stock | "
             "stock/fused || verdict (fused <= stock + the stock chain's spread, both series) | one C-ABI call each, us (launches "
             "included): fwd bwd | kernels per call: train fused, stock; validation fused, stock"]
    losers = []
    for name, dtype in DTYPES.items():
        for B in BATCHES:
            for K in CLASSES:
                torch.manual_seed(0)
                z = torch.randn(B, K, device=dev).to(dtype).requires_grad_(True)
                y = torch.randint(0, K, (B,), device=dev)
                head = CrossEntropyHead(K, meter=True).to(dev)
                head.native = lambda output, labels: True            # the kernels whatever ops.ce_native says: this run is what fills it
                conf = torch.zeros(K * K, dtype=torch.int64, device=dev)
                sums = torch.zeros(4, dtype=torch.float64, device=dev)
                keep = []

                def stock_train():
                    z.grad = None
                    out = z.float()
                    loss = F.cross_entropy(out, y)
                    keep[:] = [loss.detach(), accuracy(out, y, topk=(1,))[0]]
                    loss.backward()

                def fused_train():
                    z.grad = None
                    head(z, y).backward()

                def stock_val():
                    with torch.no_grad():
                        out = z.float()
                        keep[:] = [accuracy(out, y, topk=(1,))[0]]
                        pred = out.argmax(dim=1)
                        sums[0] += (pred == y).sum() * 100.0
                        sums[1] += F.cross_entropy(out, y).double() * B
                        sums[2] += B
                        conf.add_(torch.bincount(y * K + pred, minlength=K * K))

                def fused_val():
                    with torch.no_grad():
                        head(z, y)

                series = {"train": {"stock": stock_train, "fused": fused_train}, "val": {"stock": stock_val, "fused": fused_val}}
                got = {s: {k: [] for k in r} for s, r in series.items()}
                for _ in range(a.rounds):
                    for s, routes in series.items():
                        for k, fn in routes.items():
                            got[s][k].append(timed(fn, a.iters, a.warmup))
                k = abi_times(z, y, a.iters, a.warmup)
                nk = "-"
                if a.count_launches:
                    nk = "%d, %d; %d, %d" % tuple(count_kernels(series[s][r]) for s in ("train", "val") for r in ("fused", "stock"))
                holds = all(med(g["fused"]) <= med(g["stock"]) + (max(g["stock"]) - min(g["stock"])) for g in got.values())
                if not holds:
                    losers.append("%s B %d K %d" % (name, B, K))
                t, v = got["train"], got["val"]
                lines.append("%s %d %d | %s | %s | %.2fx || %s | %s | %.2fx || %s | fwd %.1f  bwd %.1f | %s" % (
                    name, B, K, f(t["fused"]), f(t["stock"]), med(t["stock"]) / med(t["fused"]), f(v["fused"]), f(v["stock"]),
                    med(v["stock"]) / med(v["fused"]), "holds" if holds else "LOSES", k["fwd"], k["bwd"], nk))
                print(lines[-1], flush=True)
    lines.append("# rows where the fused head is slower than the stock chain by more than the stock chain's spread in either series: %s"
                 % (", ".join(losers) or "none"))
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

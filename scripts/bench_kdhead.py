#!/usr/bin/env python3
"""The student's head of every `--distill` step on one GPU -- cross-entropy, the KD divergence at temperature T and the top-1 -- as the
fused head (helper.kd_head.StudentHead: moma_kdhead_fwd, moma_kdhead_bwd) against the stock chain it replaces, forward + backward:

    stock   logit_s.float(), nn.CrossEntropyLoss, DistillKL(T), helper.util.accuracy, (cls loss_cls + div loss_div).backward() -- what
            MomaStep.losses_and_query and backward_part run per step for the head, the accuracy left on the device.
    fused   StudentHead(T)(logit_s, logit_t, labels), the same weighted sum, .backward().

    python scripts/bench_kdhead.py [--out profiles/kdhead_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--count_launches]

Shapes: B in (64, 256) x K in (4, 9, 100, 1000), fp32 and bf16 student logits, the teacher's logits in fp32 (MomaStep.teacher_side hands
them over as float32); T = 4, both weights 1.
Timed with HIP events around the whole call after warm-up.  The routes alternate inside one process, `rounds` times over (stock,
fused, stock, ...); a route's figure is the median of its round medians, its spread their min .. max.  Verdict per row, the project's
standing one: the row `holds` when the fused median is at most the stock chain's plus the stock chain's own spread (max - min of its
round medians), `LOSES` otherwise -- such a shape class belongs to the composite in ops.kd_head_native.
The two C-ABI calls are then timed one by one on preallocated buffers (events around ONE call: the launches are inside, so these are
upper bounds of the kernels' times).  Launches per call: fused 2 forward + 1 backward; both routes' kernels are counted with torch's
profiler (--count_launches)."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.bench_ce import BATCHES, CLASSES, DTYPES, count_kernels, timed  # noqa: E402

T = 4.0


def abi_times(zs, zt, y, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    zs, dev = zs.detach(), zs.device
    B, K = zs.shape
    codes = (_DT_CODES[zs.dtype], _DT_CODES[zt.dtype])
    n = lib.moma_kdhead_workspace_bytes(B, K)
    ws = torch.empty((n + 7) // 8, device=dev, dtype=torch.float64)
    saved, out = torch.empty(3 * B + 1, device=dev, dtype=torch.float64), torch.empty(3, device=dev)
    g, dz = torch.ones((), device=dev), torch.empty_like(zs)
    calls = {
        "fwd": lambda: _lib.check(lib.moma_kdhead_fwd(_ptr(zs), _ptr(zt), _ptr(y), B, K, *codes, T, _ptr(ws), ws.numel() * 8, _ptr(out),
                                                      _ptr(saved), _stream()), "fwd"),
        "bwd": lambda: _lib.check(lib.moma_kdhead_bwd(_ptr(zs), _ptr(zt), _ptr(y), _ptr(saved), _ptr(g), _ptr(g), _ptr(dz), B, K, *codes, T,
                                                      _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup) for k, fn in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--count_launches", action="store_true", help="count the kernels of one call of each route")
    a = ap.parse_args()
    from moma_amd.distiller_zoo import DistillKL
    from moma_amd.helper.kd_head import StudentHead
    from moma_amd.helper.util import accuracy
    if not torch.cuda.is_available():
        raise SystemExit("bench_kdhead: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    lines = ["# student head (cross-entropy + KD divergence at T = %g + top-1), forward + backward, us per call (median [min .. max] of %d "
             "round medians, %d iterations after %d warm-up each, the routes alternating), teacher logits fp32, %s"
             % (T, a.rounds, a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# student dtype B K | fused | stock | stock/fused | verdict (fused <= stock + the stock chain's spread) | one C-ABI call "
             "each, us (launches included): fwd bwd | kernels per call: fused, stock"]
    losers = []
    crit_cls, crit_div = nn.CrossEntropyLoss(), DistillKL(T)
    for name, dtype in DTYPES.items():
        for B in BATCHES:
            for K in CLASSES:
                torch.manual_seed(0)
                zs = torch.randn(B, K, device=dev).to(dtype).requires_grad_(True)
                zt = torch.randn(B, K, device=dev)
                y = torch.randint(0, K, (B,), device=dev)
                head = StudentHead(T)
                head.native = lambda *_a: True                       # the kernels whatever ops.kd_head_native says: this run is what fills it
                keep = []

                def stock():
                    zs.grad = None
                    out = zs.float()
                    loss = 1.0 * crit_cls(out, y) + 1.0 * crit_div(out, zt)
                    keep[:] = [accuracy(out, y, topk=(1,))[0].squeeze(0)]
                    loss.backward()

                def fused():
                    zs.grad = None
                    loss_cls, loss_div, acc = head(zs, zt, y)
                    keep[:] = [acc]
                    (1.0 * loss_cls + 1.0 * loss_div).backward()

                routes = {"stock": stock, "fused": fused}
                got = {k: [] for k in routes}
                for _ in range(a.rounds):
                    for k, fn in routes.items():
                        got[k].append(timed(fn, a.iters, a.warmup))
                k = abi_times(zs, zt, y, a.iters, a.warmup)
                nk = "-"
                if a.count_launches:
                    nk = "%d, %d" % tuple(count_kernels(routes[r]) for r in ("fused", "stock"))
                holds = med(got["fused"]) <= med(got["stock"]) + (max(got["stock"]) - min(got["stock"]))
                if not holds:
                    losers.append("%s B %d K %d" % (name, B, K))
                lines.append("%s %d %d | %s | %s | %.2fx | %s | fwd %.1f  bwd %.1f | %s" % (
                    name, B, K, f(got["fused"]), f(got["stock"]), med(got["stock"]) / med(got["fused"]), "holds" if holds else "LOSES",
                    k["fwd"], k["bwd"], nk))
                print(lines[-1], flush=True)
    lines.append("# rows where the fused head is slower than the stock chain by more than the stock chain's spread: %s"
                 % (", ".join(losers) or "none"))
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

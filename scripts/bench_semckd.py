#!/usr/bin/env python3
"""What `--distill semckd` adds on one GPU: the criterion's tail -- the attention-weighted per-sample MSE of all 16 (student map,
teacher map) pairs, forward + backward -- as the grouped pair (ops.semckd_weighted_mse: moma_semckd_fwd forward, moma_semckd_bwd
backward) against the stock form (distiller_zoo.SemCKDLoss: per pair MSELoss(reduction='none') -> reshape -> mean -> a strided write,
autograd in the storage's dtype), and the batch Gram matrices in front of the heads (ops.batch_gram: moma_sp_gram + moma_sp_gram_sum,
moma_sp_bwd) against x.reshape(B, -1) @ its transpose with autograd.

    python scripts/bench_semckd.py [--out profiles/semckd_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--batch 64] [--series 2]

Shapes: the EfficientNet-B0 pair of the benchmark at 224 pixels, B = 64: feat[1:-1] = 24 x 56 x 56, 40 x 28 x 28, 112 x 14 x 14,
1280 x 7 x 7 on both sides; pair (i, j) lives on the smaller of the two grids with the teacher's channels (n_p from 24 x 7 x 7 =
1176 to 24 x 56 x 56 = 75264 elements per sample), in fp32 and bf16 storage, NCHW and channels_last.  Rows: `tail` (the 16 pairs:
gradients to every s_value and to the weight), `grams` (the 8 Gram matrices of a step: the student's four with their backward, the
teacher's four without) and one row per map for the Gram alone (forward + backward).
Timed with HIP events around the whole forward + backward after warm-up.  The routes alternate inside one process, `rounds` times
over (stock, fused, stock, ...); a route's figure is the median of its round medians, its spread their min .. max.  The whole table is
taken `series` times.  Verdict per row, the project's standing one: the fused route `holds` when its median is at most the stock
form's plus the stock form's own spread (max - min of its round medians), `LOSES` otherwise; a class of rows that loses in every
series belongs to the composite."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAPS = [(24, 56), (40, 28), (112, 14), (1280, 7)]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
LAYOUTS = {"NCHW": torch.contiguous_format, "channels_last": torch.channels_last}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--series", type=int, default=2)
    a = ap.parse_args()
    from moma_amd import ops
    from moma_amd.distiller_zoo import SemCKDLoss
    if not torch.cuda.is_available():
        raise SystemExit("bench_semckd: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    B, S, T = a.batch, len(MAPS), len(MAPS)
    crit = SemCKDLoss()
    lines = ["# semckd: the tail over 16 pairs and the batch Gram matrices, us per forward + backward (median [min .. max] of %d round "
             "medians, %d iterations after %d warm-up each, the routes alternating), B = %d, %s" % (
                 a.rounds, a.iters, a.warmup, B, torch.cuda.get_device_name(0)),
             "# series dtype layout row | fused | stock ops | stock/fused | verdict (fused <= stock + the stock form's spread)"]
    lost = {}

    def row(series, name, lay, what, routes):
        got = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                got[k].append(timed(fn, a.iters, a.warmup))
        holds = med(got["fused"]) <= med(got["stock"]) + (max(got["stock"]) - min(got["stock"]))
        if not holds:
            lost.setdefault("%s %s %s" % (name, lay, what), []).append(series)
        lines.append("%d %s %s %s | %s | %s | %.2fx | %s" % (series, name, lay, what, f(got["fused"]), f(got["stock"]),
                                                             med(got["stock"]) / med(got["fused"]), "holds" if holds else "LOSES"))
        print(lines[-1], flush=True)

    for series in range(1, a.series + 1):
        for name, dtype in DTYPES.items():
            for lay, mf in LAYOUTS.items():
                torch.manual_seed(0)
                mk = lambda c, h: torch.randn(B, c, h, h, device=dev).to(dtype).contiguous(memory_format=mf)      # noqa: E731
                xs = [[mk(MAPS[j][0], min(MAPS[i][1], MAPS[j][1])).requires_grad_(True) for j in range(T)] for i in range(S)]
                ts = [[mk(MAPS[j][0], min(MAPS[i][1], MAPS[j][1])) for j in range(T)] for i in range(S)]
                w = torch.softmax(torch.randn(B, S, T, device=dev), -1).requires_grad_(True)
                leaves = [x for r in xs for x in r] + [w]

                def clear():
                    for t in leaves:
                        t.grad = None

                def tail_stock():
                    clear()
                    crit(xs, ts, w).backward()

                def tail_fused():
                    clear()
                    ops.semckd_weighted_mse(xs, ts, w)[0].backward()

                row(series, name, lay, "tail 16 pairs", {"stock": tail_stock, "fused": tail_fused})
                fs = [mk(c, h).requires_grad_(True) for c, h in MAPS]
                ft = [mk(c, h) for c, h in MAPS]
                dG = torch.randn(B, B, device=dev)

                def stock_gram(x):
                    v = x.reshape(B, -1)
                    return torch.matmul(v, v.t())

                def grams(gram, maps_s, maps_t):
                    for x in maps_s:
                        x.grad = None
                    gs = [gram(x) for x in maps_s]
                    with torch.no_grad():
                        for x in maps_t:
                            gram(x)
                    torch.autograd.backward(gs, [dG.to(g.dtype) for g in gs])

                row(series, name, lay, "grams 4 + 4", {"stock": lambda: grams(stock_gram, fs, ft), "fused": lambda: grams(ops.batch_gram, fs, ft)})
                for x, (c, h) in zip(fs, MAPS):
                    row(series, name, lay, "gram %d x %d x %d" % (c, h, h),
                        {"stock": lambda x=x: grams(stock_gram, [x], []), "fused": lambda x=x: grams(ops.batch_gram, [x], [])})
                del xs, ts, w, leaves, fs, ft
                torch.cuda.empty_cache()
    both = [k for k, v in lost.items() if len(v) == a.series]
    lines.append("# rows that lose in every series: %s" % (", ".join(both) or "none"))
    lines.append("# rows that lose in some series only: %s" % (", ".join(k for k, v in lost.items() if len(v) < a.series) or "none"))
    print("\n".join(lines[-2:]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

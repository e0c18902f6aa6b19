#!/usr/bin/env python3
"""Similarity-Preserving distillation criterion on one GPU: the fused path (ops.sp_loss: sp_gram x 2, sp_terms, sp_bwd) against two
baselines in stock PyTorch ops with autograd:
  (a) the criterion's composite (Similarity.composite as the criterion runs it: reshape, float64 mm, F.normalize);
  (b) the published form (Tung & Mori, ICCV 2019, as the reference's distiller_zoo/SP.py states it) in fp32: flatten (reshape where
      the reference would view: view raises on a channels_last map), widen to fp32, mm with the transpose, F.normalize(dim=1) per
      side, mean squared difference.

    python scripts/bench_sp.py [--out profiles/sp_bench.txt] [--iters 20] [--warmup 3] [--rounds 3]

Shapes: B in {64, 256}, student 1280 x 7 x 7 (EfficientNet-B0's head map at 224 px), teacher 1280 x 7 x 7 and 2560 x 7 x 7, fp32 and
bf16 storage, NCHW and channels_last.  Criterion forward + backward (gradient to the student only, the teacher's map detached),
timed with HIP events around the whole call after warm-up.  The three routes alternate inside one process, `rounds` times over
(stock, fused, composite, stock, fused, ...); a route's figure is the median of its round medians, its spread their min .. max.
Verdict per row: the fused route is `ok` when its median is no larger than the stock form's plus the stock form's own spread
(max - min of its round medians), `SLOWER` otherwise.  The four C-ABI calls are then timed one by one on preallocated buffers
(events around ONE call: the launch is inside, so these are upper bounds of the kernels' times) and set against the HBM floor of
the shapes at 8 TB/s: sp_gram B K e bytes, sp_bwd 2 B K e bytes (e = bytes per element)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0
CONFIGS = [(B, 1280, Ct) for B in (64, 256) for Ct in (1280, 2560)]
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


def inputs(B, Cs, Ct, dtype, mf, dev):
    torch.manual_seed(0)
    silu = torch.nn.functional.silu                                  # the head map is post-SiLU
    s = silu(torch.randn(B, Cs, 7, 7, device=dev)).to(dtype).contiguous(memory_format=mf).requires_grad_(True)
    return s, silu(torch.randn(B, Ct, 7, 7, device=dev)).to(dtype).contiguous(memory_format=mf)


def published(f_s, f_t):
    def normalised_gram(f):
        x = f.reshape(f.shape[0], -1).float()
        return torch.nn.functional.normalize(torch.mm(x, x.t()), dim=1)
    with torch.no_grad():
        g_t = normalised_gram(f_t)
    d = g_t - normalised_gram(f_s)
    return (d * d).sum() / (f_s.shape[0] ** 2)


def step_of(fn, s, t):
    def step():
        s.grad = None
        fn(s, t).backward()
    return step


def abi_times(s, t, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    s, dev, B = s.detach(), s.device, s.shape[0]
    Ks, Kt = s.numel() // B, t.numel() // B
    n_s, n_t = lib.moma_sp_workspace_bytes(B, Ks), lib.moma_sp_workspace_bytes(B, Kt)
    ws_s, ws_t = torch.empty(n_s // 4, device=dev), torch.empty(n_t // 4, device=dev)
    G, H = torch.empty(2, B, B, device=dev, dtype=torch.float64), torch.empty(2, B, B, device=dev, dtype=torch.float64)
    rows, M = torch.empty(4, B, device=dev, dtype=torch.float64), torch.empty(B, B, device=dev, dtype=torch.float64)
    loss, g = torch.empty((), device=dev), torch.ones((), device=dev)
    dF = torch.empty_like(s)
    cs, ct = _DT_CODES[s.dtype], _DT_CODES[t.dtype]
    calls = {
        "gram_s": lambda: _lib.check(lib.moma_sp_gram(_ptr(s), B, Ks, cs, _ptr(ws_s), n_s, _stream()), "gram"),
        "gram_t": lambda: _lib.check(lib.moma_sp_gram(_ptr(t), B, Kt, ct, _ptr(ws_t), n_t, _stream()), "gram"),
        "terms": lambda: _lib.check(lib.moma_sp_terms(_ptr(ws_s), n_s, Ks, _ptr(ws_t), n_t, Kt, B, _ptr(G), _ptr(H), _ptr(rows), _ptr(M),
                                                      _ptr(loss), _stream()), "terms"),
        "bwd": lambda: _lib.check(lib.moma_sp_bwd(_ptr(s), _ptr(M), _ptr(g), _ptr(dF), B, Ks, cs, _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup) for k, fn in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from moma_amd import ops
    from moma_amd.distiller_zoo import Similarity
    dev = torch.device("cuda", 0)
    crit = Similarity()
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    lines = ["# Similarity-Preserving criterion, us per forward + backward (median [min .. max] of %d round medians, %d iterations after "
             "%d warm-up each, the routes alternating), %s" % (a.rounds, a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# dtype layout B Cs Ct | fused | (b) stock fp32 | (b)/fused | verdict (fused <= stock + stock's spread) | (a) composite "
             "float64 | (a)/fused | fused forward only | one C-ABI call each, us (launch included): gram_s [x the HBM floor at %.0f TB/s] "
             "gram_t [..] terms bwd [..]" % PEAK_TBS]
    worst = 0.0
    for name, dtype in DTYPES.items():
        for lay, mf in LAYOUTS.items():
            for B, Cs, Ct in CONFIGS:
                s, t = inputs(B, Cs, Ct, dtype, mf, dev)
                routes = {"stock": step_of(published, s, t), "fused": step_of(ops.sp_loss, s, t), "comp": step_of(crit.composite, s, t)}
                got = {k: [] for k in routes}
                for _ in range(a.rounds):
                    for k, fn in routes.items():
                        got[k].append(timed(fn, a.iters, a.warmup))

                def fwd():
                    with torch.no_grad():
                        ops.sp_loss(s, t)
                ffwd = timed(fwd, a.iters, a.warmup)
                k = abi_times(s, t, a.iters, a.warmup)
                e = s.element_size()
                floor = {"gram_s": B * Cs * 49 * e, "gram_t": B * Ct * 49 * e, "bwd": 2 * B * Cs * 49 * e}
                per = "  ".join("%s %.1f" % (c, k[c]) + (" [%.1fx]" % (k[c] * 1e-6 * PEAK_TBS * 1e12 / floor[c]) if c in floor else "")
                                for c in k)
                spread = max(got["stock"]) - min(got["stock"])
                ok = med(got["fused"]) <= med(got["stock"]) + spread
                worst = max(worst, med(got["fused"]) / med(got["stock"]))
                lines.append("%s %s %d %d %d | %s | %s | %.2fx | %s | %s | %.2fx | %.1f | %s" % (
                    name, lay, B, Cs, Ct, f(got["fused"]), f(got["stock"]), med(got["stock"]) / med(got["fused"]), "ok" if ok else "SLOWER",
                    f(got["comp"]), med(got["comp"]) / med(got["fused"]), ffwd, per))
                print(lines[-1], flush=True)
                del s, t, routes
                torch.cuda.empty_cache()
    lines.append("# worst fused / stock over the rows: %.2f" % worst)
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

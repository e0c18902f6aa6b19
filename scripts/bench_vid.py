#!/usr/bin/env python3
"""The Gaussian likelihood of Variational Information Distillation on one GPU: the fused pair (ops.vid_nll: moma_vid_nll forward,
moma_vid_bwd backward) against the criterion's composite (VIDLoss.composite: the same formula in stock torch ops with autograd,
evaluated in float64) and against the reference's own statement of it in the storage's compute type (distiller_zoo/VID.py: softplus,
square, divide, log, mean in fp32 -- under bf16 storage the maps are widened to fp32 first, as autocast would for the loss).

    python scripts/bench_vid.py [--out profiles/vid_layer_microbench.txt] [--iters 20] [--warmup 3] [--rounds 3] [--batch 64] [--dtypes fp32,bf16]

Shapes: the four pairs feat[1:-1] of EfficientNet-B0 at the reference's default batch (64 images of 512 pixels): 24 x 128 x 128,
40 x 64 x 64, 112 x 32 x 32 and 1280 x 16 x 16, in fp32 and bf16 storage, NCHW and channels_last (both sides alike).  Forward +
backward of the likelihood alone (gradients to the mean and to log_scale, the target detached), timed with HIP events around the whole
call after warm-up.  The routes alternate inside one process, `rounds` times over (composite, fused, reference form, composite, ...); a
route's figure is the median of its round medians, its spread their min .. max.  Verdict per row: the fused route `wins` when its
median is below the composite's by more than the larger of the two spreads (max - min of the round medians), `NO` otherwise.
Algorithmic bytes of the fused pair: two reads forward, two reads and one write backward = 5 B C P e (e = bytes per element); the
fraction of the HBM rate is those bytes over the fused route's time, against 8 TB/s.  The two C-ABI calls are then timed one by one on
preallocated buffers (events around ONE call: the launches are inside, so these are upper bounds of the kernels' times)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0
PAIRS = [(24, 128, 128), (40, 64, 64), (112, 32, 32), (1280, 16, 16)]
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


def inputs(B, C, H, W, dtype, mf, dev):
    torch.manual_seed(0)
    m = torch.randn(B, C, H, W, device=dev).to(dtype).contiguous(memory_format=mf).requires_grad_(True)
    t = torch.relu(torch.randn(B, C, H, W, device=dev)).to(dtype).contiguous(memory_format=mf)
    return m, t


def reference_form(log_scale, eps):
    def f(m, t):
        var = (torch.log(1.0 + torch.exp(log_scale)) + eps).view(1, -1, 1, 1)
        return torch.mean(0.5 * ((m.float() - t.float()) ** 2 / var + torch.log(var)))
    return f


def step_of(fn, m, t, log_scale):
    def step():
        m.grad = None
        log_scale.grad = None
        fn(m, t).backward()
    return step


def abi_times(m, t, log_scale, eps, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _map_side, _ptr, _stream
    lib = _lib.load()
    m, ls, dev = m.detach(), log_scale.detach(), m.device
    B, C, H, W = m.shape
    lay_m, lay_t = (_map_side(f, nm, "vid_nll", "VIDLoss") for f, nm in ((m, "mean"), (t, "target")))
    codes = (_DT_CODES[m.dtype], lay_m, _DT_CODES[t.dtype], lay_t)
    n = lib.moma_vid_workspace_bytes(B, C, H * W, *codes)
    ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
    sq, var, gls = (torch.empty(C, device=dev) for _ in range(3))
    loss, g = torch.empty((), device=dev), torch.ones((), device=dev)
    d_mean = torch.empty_like(m)
    calls = {
        "nll": lambda: _lib.check(lib.moma_vid_nll(_ptr(m), _ptr(t), _ptr(ls), eps, B, C, H * W, *codes, _ptr(ws), n, _ptr(sq), _ptr(var),
                                                   _ptr(gls), _ptr(loss), _stream()), "nll"),
        "bwd": lambda: _lib.check(lib.moma_vid_bwd(_ptr(m), _ptr(t), _ptr(var), _ptr(g), _ptr(d_mean), B, C, H * W, *codes, _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup) for k, fn in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtypes", default="fp32,bf16", help="storage types in the order they are timed")
    a = ap.parse_args()
    from moma_amd import ops
    from moma_amd.distiller_zoo import VIDLoss
    if not torch.cuda.is_available():
        raise SystemExit("bench_vid: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    B = a.batch
    lines = ["# VID likelihood, us per forward + backward (median [min .. max] of %d round medians, %d iterations after %d warm-up "
             "each, the routes alternating), B = %d, %s" % (a.rounds, a.iters, a.warmup, B, torch.cuda.get_device_name(0)),
             "# dtype layout C H W | fused | (a) composite float64 | (a)/fused | verdict (composite - fused > the larger spread) | "
             "(b) reference form fp32 | (b)/fused | algorithmic MB (5 B C P e) | fused: fraction of %.0f TB/s | one C-ABI call each, us "
             "(launches included): nll [fraction of the HBM rate at 2 B C P e] bwd [.. at 3 B C P e]" % PEAK_TBS]
    losers = []
    for name in a.dtypes.split(","):
        dtype = DTYPES[name]
        for lay, mf in LAYOUTS.items():
            for C, H, W in PAIRS:
                crit = VIDLoss(C, 8, C).to(dev)                                     # (the regressor is not timed: its width is idle)
                with torch.no_grad():
                    crit.log_scale.copy_(torch.linspace(-3, 8, C))
                ls, eps = crit.log_scale, crit.eps
                m, t = inputs(B, C, H, W, dtype, mf, dev)
                routes = {"comp": step_of(crit.composite, m, t, ls), "fused": step_of(lambda x, y: ops.vid_nll(x, y, ls, eps), m, t, ls),
                          "ref": step_of(reference_form(ls, eps), m, t, ls)}
                got = {k: [] for k in routes}
                for _ in range(a.rounds):
                    for k, fn in routes.items():
                        got[k].append(timed(fn, a.iters, a.warmup))
                k = abi_times(m, t, ls, eps, a.iters, a.warmup)
                e = m.element_size()
                unit = B * C * H * W * e
                frac = lambda us, nbytes: nbytes / (us * 1e-6) / (PEAK_TBS * 1e12)   # noqa: E731
                spread = max(max(got["comp"]) - min(got["comp"]), max(got["fused"]) - min(got["fused"]))
                wins = med(got["comp"]) - med(got["fused"]) > spread
                if not wins:
                    losers.append("%s %s %d x %d x %d" % (name, lay, C, H, W))
                lines.append("%s %s %d %d %d | %s | %s | %.2fx | %s | %s | %.2fx | %.1f | %.3f | nll %.1f [%.3f]  bwd %.1f [%.3f]" % (
                    name, lay, C, H, W, f(got["fused"]), f(got["comp"]), med(got["comp"]) / med(got["fused"]), "wins" if wins else "NO",
                    f(got["ref"]), med(got["ref"]) / med(got["fused"]), 5 * unit / 1e6, frac(med(got["fused"]), 5 * unit),
                    k["nll"], frac(k["nll"], 2 * unit), k["bwd"], frac(k["bwd"], 3 * unit)))
                print(lines[-1], flush=True)
                del m, t, routes, crit
                torch.cuda.empty_cache()
    lines.append("# rows where the fused pair does not beat the composite by more than the spread: %s" % (", ".join(losers) or "none"))
    print(lines[-1])
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

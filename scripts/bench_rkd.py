#!/usr/bin/env python3
"""Relational Knowledge Distillation criterion on one GPU: the fused path (ops.rkd_loss: rkd_dist x 2, rkd_terms, rkd_bwd) against
two baselines in stock PyTorch ops with autograd:
  (a) the criterion's composite (RKDLoss.composite as the criterion runs it: float64, S from the differences, [B, B, B] temporaries);
  (b) the published formulation written out directly (Park et al., CVPR 2019, eq. 5-8: the [B, B, D] tensor of pairwise differences,
      its norms as the distances, the normalised differences batch-multiplied with themselves as the angles, Huber loss on both, in
      float32), run in a CHILD process per configuration so that an out-of-memory error ends that row alone, and only where five
      [B, B, D] fp32 temporaries per side fit half of the free memory.

    python scripts/bench_rkd.py [--out profiles/rkd_bench.txt] [--iters 30] [--warmup 5]

Shapes: B in {64, 256}, (Ds, Dt) in {(1280, 1280), (512, 2048)} (EfficientNet-B0's feat[-1] against itself, a ResNet-18 student
against a ResNet-50 teacher), fp32 and bf16 storage.  Criterion forward + backward (gradient to the student only, the teacher's
feature detached), timed with HIP events around the whole call after warm-up, median [min .. max]; fused and composite alternate
inside one process (composite, fused, composite, fused: the better median of each side makes the ratio).  The four C-ABI calls are
then timed one by one on preallocated buffers (events around ONE call: the launch is inside, so these are upper bounds of the
kernels' times), and set against what the shapes need: rkd_dist 3 D B (B + 16) / 2 FP64 vector operations and B D e + 8 B^2 bytes;
rkd_terms about 38 B^3 FP64 vector operations (the two triples of the angle pass) and 56 B^2 bytes; rkd_bwd 2 B^2 D FP64 matrix
operations and 2 B D e + 8 B^2 bytes -- as shares of 78.6 TF (the public FP64 vector and matrix rate of the MI355X) and of 8 TB/s."""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F64_TF, PEAK_TBS = 78.6, 8.0
CONFIGS = [(B, Ds, Dt) for B in (64, 256) for Ds, Dt in ((1280, 1280), (512, 2048))]
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
    return ts[len(ts) // 2], ts[0], ts[-1]


def inputs(B, Ds, Dt, dtype, dev):
    torch.manual_seed(0)
    s = torch.randn(B, Ds, device=dev).to(dtype).requires_grad_(True)
    return s, torch.randn(B, Dt, device=dev).to(dtype)


def published(f_s, f_t, w_d=25.0, w_a=50.0):
    """eq. 5-8 of the paper as broadcast, normalise and bmm, in float32"""
    huber = torch.nn.functional.smooth_l1_loss

    def relations(x):
        x = x.float()
        diff = x.unsqueeze(0) - x.unsqueeze(1)                        # [B, B, D]
        dist = diff.norm(dim=2)
        mu = dist.sum() / (dist.shape[0] * (dist.shape[0] - 1))
        e = diff / dist.clamp(min=1e-12).unsqueeze(2)
        return dist / mu, torch.bmm(e, e.transpose(1, 2))
    with torch.no_grad():
        d_t, a_t = relations(f_t)
    d_s, a_s = relations(f_s)
    return w_d * huber(d_s, d_t) + w_a * huber(a_s, a_t)


def step_of(fn, s, t):
    def step():
        s.grad = None
        fn(s, t).backward()
    return step


def child(B, Ds, Dt, dt, iters, warmup):
    dev = torch.device("cuda", 0)
    s, t = inputs(B, Ds, Dt, DTYPES[dt], dev)
    need = 5 * 4.0 * B * B * (Ds + Dt)
    free, _total = torch.cuda.mem_get_info()
    if need > free / 2:
        print(json.dumps({"skipped": "five [B,B,D] fp32 temporaries per side need %.1f GB" % (need / 1e9)}))
        return
    try:
        r = timed(step_of(published, s, t), iters, warmup)
        print(json.dumps({"us": [1e3 * v for v in r], "peak_GB": torch.cuda.max_memory_allocated() / 1e9}))
    except torch.cuda.OutOfMemoryError:
        print(json.dumps({"skipped": "out of memory"}))


def abi_times(B, Ds, Dt, dtype, dev, iters, warmup):
    """median us of each C-ABI call on preallocated buffers"""
    from moma_amd import _lib
    from moma_amd.ops import _DT_CODES, _ptr, _stream
    lib = _lib.load()
    s, t = inputs(B, Ds, Dt, dtype, dev)
    s = s.detach()
    S = torch.empty(2, B, B, device=dev, dtype=torch.float64)
    Q = torch.empty(B, B, device=dev, dtype=torch.float64)
    n = lib.moma_rkd_workspace_bytes(B)
    ws = torch.empty(n // 8, device=dev, dtype=torch.float64)
    terms, loss, g = torch.empty(2, device=dev), torch.empty((), device=dev), torch.ones((), device=dev)
    dF = torch.empty_like(s)
    code = _DT_CODES[dtype]
    calls = {
        "dist_s": lambda: _lib.check(lib.moma_rkd_dist(_ptr(s), B, Ds, code, _ptr(S[0]), _stream()), "dist"),
        "dist_t": lambda: _lib.check(lib.moma_rkd_dist(_ptr(t), B, Dt, code, _ptr(S[1]), _stream()), "dist"),
        "terms": lambda: _lib.check(lib.moma_rkd_terms(_ptr(S[0]), _ptr(S[1]), B, 25.0, 50.0, _ptr(ws), n, _ptr(Q), _ptr(terms), _ptr(loss),
                                                       _stream()), "terms"),
        "bwd": lambda: _lib.check(lib.moma_rkd_bwd(_ptr(s), _ptr(Q), _ptr(g), _ptr(dF), B, Ds, code, _stream()), "bwd"),
    }
    return {k: timed(fn, iters, warmup)[0] * 1e3 for k, fn in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", nargs=4, default=None, metavar=("B", "Ds", "Dt", "dtype"))
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.child[3], a.iters, a.warmup)
    from moma_amd import ops
    from moma_amd.distiller_zoo import RKDLoss
    dev = torch.device("cuda", 0)
    crit = RKDLoss()
    f = lambda r: "%.1f [%.1f .. %.1f]" % tuple(1e3 * v for v in r)                # noqa: E731
    lines = ["# RKD criterion, us per call (median [min .. max] over %d iterations after %d warm-up, fused and composite alternating), %s"
             % (a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# dtype B Ds Dt | fused fwd+bwd us, 1st and 2nd run | fused fwd us | (a) composite float64 fwd+bwd us, 1st and 2nd run | (a)/fused | "
             "(b) published form fp32 fwd+bwd us in a child process (peak GB) | (b)/fused | one C-ABI call each, us (launch included): "
             "dist_s [%% of %.1f TF FP64, %% of %.0f TB/s] dist_t [..] terms [..] bwd [..]" % (PEAK_F64_TF, PEAK_TBS)]
    for name, dtype in DTYPES.items():
        for B, Ds, Dt in CONFIGS:
            s, t = inputs(B, Ds, Dt, dtype, dev)
            run_comp, run_fused = step_of(crit.composite, s, t), step_of(ops.rkd_loss, s, t)
            comp1 = timed(run_comp, a.iters, a.warmup)
            fused1 = timed(run_fused, a.iters, a.warmup)
            comp2 = timed(run_comp, a.iters, a.warmup)
            fused2 = timed(run_fused, a.iters, a.warmup)
            comp, fused = min(comp1, comp2), min(fused1, fused2)

            def fwd():
                with torch.no_grad():
                    ops.rkd_loss(s, t)
            ffwd = timed(fwd, a.iters, a.warmup)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(Ds), str(Dt), name, "--iters",
                                str(a.iters), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
            try:
                pub = json.loads(r.stdout.strip().splitlines()[-1])
            except (IndexError, ValueError):
                pub = {"skipped": "child failed (rc %d): %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or "")}
            if "us" in pub:
                pub_txt = "%.1f [%.1f .. %.1f] (%.2f GB) | %.2fx" % (*pub["us"], pub["peak_GB"], pub["us"][0] / (1e3 * fused[0]))
            else:
                pub_txt = "not run: %s | -" % pub["skipped"]
            k = abi_times(B, Ds, Dt, dtype, dev, a.iters, a.warmup)
            e = s.element_size()
            need = {"dist_s": (3.0 * Ds * B * (B + 16) / 2, B * Ds * e + 8.0 * B * B), "dist_t": (3.0 * Dt * B * (B + 16) / 2, B * Dt * e + 8.0 * B * B),
                    "terms": (38.0 * B ** 3, 56.0 * B * B), "bwd": (2.0 * B * B * Ds, 2.0 * B * Ds * e + 8.0 * B * B)}
            per = "  ".join("%s %.1f [%.2f%%, %.2f%%]" % (c, k[c], 100 * need[c][0] / (k[c] * 1e-6) / (PEAK_F64_TF * 1e12),
                                                         100 * need[c][1] / (k[c] * 1e-6) / (PEAK_TBS * 1e12)) for c in k)
            lines.append("%s %d %d %d | %s, %s | %s | %s, %s | %.2fx | %s | %s" % (
                name, B, Ds, Dt, f(fused1), f(fused2), f(ffwd), f(comp1), f(comp2), comp[0] / fused[0], pub_txt, per))
            print(lines[-1], flush=True)
            del s, t
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

"""BN1 + SiLU -> squeeze-excite gate of the 16 MBConv blocks of EfficientNet-B0 (B = 256, bf16): the fused pair
(ops.bn_act_mean / ops.bn_act_gate, csrc/bnse.hip) against the two calls it replaces (ops.bn_act with the plane means, ops.se_gate).

    python scripts/bench_bnse.py [batch]

Per distinct (channels, plane, number of blocks of that shape): HIP-event time per call of the no-grad forward and of forward +
backward, the two routes alternating in windows of at least 0.5 s each (two windows per route, their mean).  The gate logits
come from the plane means through a per-channel scale, so both gradient branches of the pair are live; the squeeze-excite
convolutions themselves are the same on both routes and left out.  The shapes of one plane size are timed in a child process of
their own under a time limit; the first child that does not end cleanly ends the run (nothing is tried again after a fault)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (mid channels, plane of the depthwise output, blocks of that shape)
SHAPES = [(32, 112, 1), (96, 56, 1), (144, 56, 1), (144, 28, 1), (240, 28, 1), (240, 14, 1), (480, 14, 3), (672, 14, 2), (672, 7, 1),
          (1152, 7, 4)]
GROUPS = [[s for s in SHAPES if s[1] == h] for h in (112, 56, 28, 14, 7)]
LIMIT_S = 240
WINDOW_MS = 500.0


def _window(fn):
    """us per call over one window of at least WINDOW_MS"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 5
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= WINDOW_MS:
            return ms / n * 1e3
        n = max(n + 1, int(n * 1.1 * WINDOW_MS / max(ms, 1e-3)) + 1)


def _pair(plain, fused):
    import torch
    for fn in (plain, fused):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = [0.0, 0.0]
    for _ in range(2):
        t[0] += _window(plain) / 2
        t[1] += _window(fused) / 2
    return t


def group(gi, N):
    import torch
    from moma_amd import ops
    for C, H, reps in GROUPS[gi]:
        d = (torch.randn(N, C, H, H, device="cuda") * 1.5 + 0.3).bfloat16().requires_grad_(True)
        gamma = (torch.rand(C, device="cuda") + 0.5).requires_grad_(True)
        beta = (torch.randn(C, device="cuda") * 0.1 + 0.7).requires_grad_(True)
        ws = torch.randn(1, C, 1, 1, device="cuda").bfloat16().requires_grad_(True)
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        dG = torch.randn(N, C, H, H, device="cuda").bfloat16()

        def plain():
            a, pooled = ops.bn_act(d, gamma, beta, rm, rv, True, 0.01, 1e-3, "silu", want_mean=True)
            return ops.se_gate(a, pooled * ws)

        def fused():
            pooled, link = ops.bn_act_mean(d, gamma, beta, rm, rv, True, 0.01, 1e-3, "silu")
            return ops.bn_act_gate(d, link, pooled * ws)

        def nograd(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def both(f):
            def run():
                torch.autograd.grad(f(), [d, gamma, beta, ws], dG)
            return run

        f0, f1 = _pair(nograd(plain), nograd(fused))
        b0, b1 = _pair(both(plain), both(fused))
        mb = d.numel() * 2 / 1e6
        print(f"{C:5d} x {H:3d}x{H:<3d} x{reps}: {mb:6.1f} MB/pass | forward {f0:8.1f} -> {f1:8.1f} us  x{f0 / f1:5.2f} | forward + backward "
              f"{b0:8.1f} -> {b1:8.1f} us  x{b0 / b1:5.2f} | {mb * 3 / f1 * 1e3:6.0f} / {mb * 8 / b1 * 1e3:6.0f} GB/s fused")
        print("RESULT", reps, "%.2f %.2f %.2f %.2f" % (f0, f1, b0, b1), flush=True)
        del d, dG


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    tot = [0.0] * 4
    for gi in range(len(GROUPS)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", str(gi), str(N)], capture_output=True, text=True,
                               timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"group {gi}: no result within {LIMIT_S} s -- stopping")
        print("\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("RESULT")), flush=True)
        if r.returncode != 0:
            sys.exit(f"group {gi}: child ended with {r.returncode} -- stopping\n{r.stderr[-2000:]}")
        for res in (ln.split() for ln in r.stdout.splitlines() if ln.startswith("RESULT")):
            for k in range(4):
                tot[k] += int(res[1]) * float(res[2 + k])
    print(f"per backbone (16 blocks): forward {tot[0]:.0f} -> {tot[1]:.0f} us, forward + backward {tot[2]:.0f} -> {tot[3]:.0f} us")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--group":
        group(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 256)
    else:
        main()

"""BN0 + SiLU -> depthwise on the fifteen expanded layers of EfficientNet-B0 (B = 256, bf16): the two calls against the fused op.

    python scripts/bench_bndw.py [batch]

Per layer (C, H, k, s), HIP-event time per call after warm-up, algorithmic bytes from the shapes and the achieved TB/s on them:
  (a) ops.bn_act + ops.dwconv          forward: 4 E + D  (statistics read, apply read + write, depthwise read; D = the result)
  (b) ops.bn_act_dwconv                forward: 2 E + D  (statistics read, depthwise read)
and the same for forward + backward (the backward is 7 E + 2 D either way: backward-data, backward-weight, the BN backward's
reduce and apply passes).  Every layer is timed in a child process of its own under a time limit; the first child that does not
end cleanly ends the run (nothing is tried again after a fault)."""
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (C, H, k, s, blocks of that shape in the network)
LAYERS = [(96, 112, 3, 2, 1), (144, 56, 3, 1, 1), (144, 56, 5, 2, 1), (240, 28, 5, 1, 1), (240, 28, 3, 2, 1), (480, 14, 3, 1, 2),
          (480, 14, 5, 1, 1), (672, 14, 5, 1, 2), (672, 14, 5, 2, 1), (1152, 7, 5, 1, 3), (1152, 7, 3, 1, 1)]
LIMIT_S = 120


def _time(fn, n=10):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                        # us


def layer(i, N):
    import torch
    from moma_amd import ops
    C, H, K, S, reps = LAYERS[i]
    OH = math.ceil(H / S)
    pad = max((OH - 1) * S + K - H, 0) // 2
    e = (torch.randn(N, C, H, H, device="cuda") * 1.5 + 0.3).bfloat16().requires_grad_(True)
    g = (torch.rand(C, device="cuda") + 0.5).requires_grad_(True)
    b = torch.full((C,), 0.7, device="cuda").requires_grad_(True)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    w = (torch.randn(C, 1, K, K, device="cuda") * 0.3).requires_grad_(True)
    dd = torch.randn(N, C, OH, OH, device="cuda").bfloat16()

    def two():
        return ops.dwconv(ops.bn_act(e, g, b, rm, rv, True, 0.01, 1e-3, "silu"), w, S, pad, pad, OH, OH)

    def one():
        return ops.bn_act_dwconv(e, g, b, rm, rv, True, 0.01, 1e-3, "silu", w, S, pad, pad, OH, OH)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def both(fn):
        return lambda: torch.autograd.grad(fn(), [e, g, b, w], dd)

    t = [_time(no_grad(two)), _time(no_grad(one)), _time(both(two)), _time(both(one))]
    eb, db = e.numel() * 2, dd.numel() * 2
    by = [4 * eb + db, 2 * eb + db, 11 * eb + 3 * db, 9 * eb + 3 * db]
    tb = [by[j] / t[j] / 1e6 for j in range(4)]
    print(f"C={C:5d} {H:3d}x{H:<3d} k{K} s{S} x{reps}: E {eb / 1e6:6.1f} MB | fwd  two calls {t[0]:7.1f} us {tb[0]:5.2f} TB/s, fused "
          f"{t[1]:7.1f} us {tb[1]:5.2f} TB/s | fwd+bwd  two calls {t[2]:7.1f} us {tb[2]:5.2f} TB/s, fused {t[3]:7.1f} us {tb[3]:5.2f} TB/s")
    print("RESULT", reps, *("%.2f" % v for v in t), flush=True)


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    tot = [0.0] * 4
    for i in range(len(LAYERS)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--layer", str(i), str(N)], capture_output=True, text=True,
                               timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"layer {LAYERS[i]}: no result within {LIMIT_S} s -- stopping")
        out = [ln for ln in r.stdout.splitlines() if not ln.startswith("RESULT")]
        print("\n".join(out), flush=True)
        if r.returncode != 0:
            sys.exit(f"layer {LAYERS[i]}: child ended with {r.returncode} -- stopping\n{r.stderr[-2000:]}")
        res = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0]
        for j in range(4):
            tot[j] += int(res[1]) * float(res[2 + j])
    print(f"per backbone pass (fifteen layers): fwd  two calls {tot[0]:.0f} us, fused {tot[1]:.0f} us | fwd+bwd  two calls "
          f"{tot[2]:.0f} us, fused {tot[3]:.0f} us")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--layer":
        layer(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 256)
    else:
        main()

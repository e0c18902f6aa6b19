"""Weight gradient of the pointwise convolutions of EfficientNet-B0 (B = 256, bf16): the library's split-K MFMA kernel
(ops.pwconv_bwd_weight) against stock aten.convolution_backward (weights only; MIOpen's solver with its transposes, fills and cast).

    python scripts/bench_pw.py [batch]

Per distinct layer shape (Cin, Cout, plane, number of layers of that shape): HIP-event time per call after warm-up over a timed
window of at least 0.5 s, and the achieved GB/s on the algorithmic bytes (x and dy read once).  The layers of one plane size are
timed in a child process of their own under a time limit; the first child that does not end cleanly ends the run (nothing is
tried again after a fault)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (Cin, Cout, H, layers of that shape in the network): expand / project convolutions and the head ...
SPATIAL = [(32, 16, 112, 1), (16, 96, 112, 1), (96, 24, 56, 1), (24, 144, 56, 2), (144, 24, 56, 1), (144, 40, 28, 1), (40, 240, 28, 2),
           (240, 40, 28, 1), (240, 80, 14, 1), (80, 480, 14, 3), (480, 80, 14, 2), (480, 112, 14, 1), (112, 672, 14, 3),
           (672, 112, 14, 2), (672, 192, 7, 1), (192, 1152, 7, 4), (1152, 192, 7, 3), (1152, 320, 7, 1), (320, 1280, 7, 1)]
# ... and the squeeze-excite pairs (reduce, expand) on 1 x 1 planes
_SE = [(32, 8, 1), (96, 4, 1), (144, 6, 2), (240, 10, 2), (480, 20, 3), (672, 28, 3), (1152, 48, 4)]
SE = [(c, s, 1, r) for c, s, r in _SE] + [(s, c, 1, r) for c, s, r in _SE]
GROUPS = [[l for l in SPATIAL if l[2] == h] for h in (112, 56, 28, 14, 7)] + [SE]
LIMIT_S = 240
WINDOW_S = 0.55


def _time(fn):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 5
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 500.0:
            return ms / n * 1e3                                  # us
        n = max(n + 1, int(n * WINDOW_S * 1e3 / max(ms, 1e-3)) + 1)


def group(gi, N):
    import torch
    from moma_amd import ops
    for Cin, Cout, H, reps in GROUPS[gi]:
        x = torch.randn(N, Cin, H, H, device="cuda").bfloat16()
        dy = torch.randn(N, Cout, H, H, device="cuda").bfloat16()
        w = torch.randn(Cout, Cin, 1, 1, device="cuda").bfloat16()

        def stock():
            return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])[1]

        def native():
            return ops.pwconv_bwd_weight(x, dy)

        diff = float((native().float() - stock().float()).abs().max()), float(stock().float().abs().max())
        t_stock, t_native = _time(stock), _time(native)
        mb = (x.numel() + dy.numel()) * 2 / 1e6
        print(f"{Cin:5d} -> {Cout:5d} {H:3d}x{H:<3d} x{reps}: {mb:7.1f} MB | stock {t_stock:8.1f} us {mb / t_stock * 1e3:7.0f} GB/s | native "
              f"{t_native:8.1f} us {mb / t_native * 1e3:7.0f} GB/s | x{t_stock / t_native:5.2f} | max |diff| {diff[0]:.3g} of {diff[1]:.3g}")
        print("RESULT", reps, "%.2f %.2f" % (t_stock, t_native), flush=True)
        del x, dy, w


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    tot = [0.0, 0.0]
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
            tot[0] += int(res[1]) * float(res[2])
            tot[1] += int(res[1]) * float(res[3])
    print(f"per backbone backward (64 layers): stock {tot[0]:.0f} us, native {tot[1]:.0f} us")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--group":
        group(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 256)
    else:
        main()

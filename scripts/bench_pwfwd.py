"""Forward and input gradient of the bias-free pointwise convolutions of EfficientNet-B0 (B = 256, bf16): the library's streaming
MFMA kernel (ops.pwconv_fwd / ops.pwconv_bwd_data) against stock F.conv2d / aten.convolution_backward (MIOpen's strided GEMMs;
on the 7 x 7 planes its igemm solver with transposes).

    python scripts/bench_pwfwd.py [batch]

Per distinct spatial layer shape (Cin, Cout, plane, number of layers of that shape) and per direction: HIP-event time per call, the
two routes alternated (stock, native, stock, native) in timed windows of at least 0.5 s each after warm-up, the mean of a route's two
windows reported, and the achieved GB/s on the algorithmic bytes (input and output once).  The layers of one plane size are timed in
a child process of their own under a time limit; the first child that does not end cleanly ends the run (nothing is tried again
after a fault)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (Cin, Cout, H, layers of that shape in the network): expand / project convolutions and the head
SPATIAL = [(32, 16, 112, 1), (16, 96, 112, 1), (96, 24, 56, 1), (24, 144, 56, 2), (144, 24, 56, 1), (144, 40, 28, 1), (40, 240, 28, 2),
           (240, 40, 28, 1), (240, 80, 14, 1), (80, 480, 14, 3), (480, 80, 14, 2), (480, 112, 14, 1), (112, 672, 14, 3),
           (672, 112, 14, 2), (672, 192, 7, 1), (192, 1152, 7, 4), (1152, 192, 7, 3), (1152, 320, 7, 1), (320, 1280, 7, 1)]
GROUPS = [[l for l in SPATIAL if l[2] == h] for h in (112, 56, 28, 14, 7)]
LIMIT_S = 240
WINDOW_MS = 500.0


def _window(fn, n):
    """(us per call, calls) over one window of at least WINDOW_MS, starting from n calls"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= WINDOW_MS:
            return ms / n * 1e3, n
        n = max(n + 1, int(n * 1.1 * WINDOW_MS / max(ms, 1e-3)) + 1)


def _alternate(stock, native):
    import torch
    for fn in (stock, native):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ns = nn = 5
    t = {"s": [], "n": []}
    for _ in range(2):
        us, ns = _window(stock, ns)
        t["s"].append(us)
        us, nn = _window(native, nn)
        t["n"].append(us)
    return sum(t["s"]) / 2, sum(t["n"]) / 2


def group(gi, N):
    import torch
    import torch.nn.functional as F
    from moma_amd import ops
    for Cin, Cout, H, reps in GROUPS[gi]:
        x = torch.randn(N, Cin, H, H, device="cuda").bfloat16()
        dy = torch.randn(N, Cout, H, H, device="cuda").bfloat16()
        w = (torch.randn(Cout, Cin, 1, 1, device="cuda") * 0.1).bfloat16()
        routes = {
            "fwd": (lambda: F.conv2d(x, w), lambda: ops.pwconv_fwd(x, w)),
            "dx ": (lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                                [True, False, False])[0],
                    lambda: ops.pwconv_bwd_data(dy, w)),
        }
        mb = (x.numel() + dy.numel()) * 2 / 1e6
        for name, (stock, native) in routes.items():
            diff = float((native().float() - stock().float()).abs().max()), float(stock().float().abs().max())
            t_stock, t_native = _alternate(stock, native)
            print(f"{name} {Cin:5d} -> {Cout:5d} {H:3d}x{H:<3d} x{reps}: {mb:7.1f} MB | stock {t_stock:8.1f} us {mb / t_stock * 1e3:7.0f} GB/s | "
                  f"native {t_native:8.1f} us {mb / t_native * 1e3:7.0f} GB/s | x{t_stock / t_native:5.2f} | max |diff| {diff[0]:.3g} of "
                  f"{diff[1]:.3g}")
            print("RESULT", name.strip(), reps, "%.2f %.2f" % (t_stock, t_native), int(ops.pwconv_fwd_native(N, Cin, Cout, H * H)),
                  flush=True)
        del x, dy, w


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    tot = {}
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
            t = tot.setdefault(res[1], [0.0, 0.0, 0.0])
            t[0] += int(res[2]) * float(res[3])
            t[1] += int(res[2]) * float(res[4])
            t[2] += int(res[2]) * float(res[4] if res[5] == "1" else res[3])
    for name, t in tot.items():
        print(f"{name} per backbone pass (32 layers): stock {t[0]:.0f} us, native everywhere {t[1]:.0f} us, "
              f"as routed by ops.pwconv_fwd_native {t[2]:.0f} us")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--group":
        group(int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 256)
    else:
        main()

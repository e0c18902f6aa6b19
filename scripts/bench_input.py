#!/usr/bin/env python3
"""The input batch of a data pack on one GPU: ops.input_batch (one launch of csrc/input.hip) against the chain of stock torch operators
it replaces (tests/input_ref.py: torch_chain -- index_select, slicing, where / flip, permute, .float(), div, sub, div, the layout,
the cast), on the same resident uint8 split.

    python scripts/bench_input.py [--out profiles/input_microbench.txt] [--iters 50] [--warmup 5] [--rounds 3] [--images 2048]

Shapes: B 256 at 224 x 224 from 256 x 256 images, and B 64 at 512 x 512 from 512 x 512 images; fp32 / NCHW and bf16 / channels_last;
random rows, random flips, the centred window.  Timed with HIP events around the whole call after warm-up; the routes alternate inside
one process, `rounds` times over; a route's figure is the median of its round medians, its spread their min .. max.  The resident split
(`--images` rows) is larger than the Infinity Cache, so the reads come from HBM.
Bytes of the kernel: 3 S S B read (+ 8 B of idx, B of flip, the 3 KiB table) and 3 S S B elements written.  `of roof` is (bytes read +
bytes written) / 6.29 TB/s, the float4-copy rate of this part, over the kernel route's median: the events sit around ONE call, launch
included, so it is a lower bound of the kernel's share.  The outputs of both routes are compared bit for bit before anything is timed."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.bench_ce import timed  # noqa: E402
from tests.input_ref import MEAN, STD, torch_chain  # noqa: E402

HBM_BYTES_PER_US = 6.29e6
SHAPES = ((256, 224, 256), (64, 512, 512))                       # (B, S, side of the pack's images)
FORMATS = (("fp32 NCHW", torch.float32, False), ("bf16 channels_last", torch.bfloat16, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=2048, help="rows of the resident split at 256 x 256 (a quarter of it at 512 x 512)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input: needs the GPU (a timing taken elsewhere says nothing)")
    from moma_amd import ops
    dev = torch.device("cuda", 0)
    med = lambda v: sorted(v)[len(v) // 2]                                          # noqa: E731
    f = lambda v: "%.1f [%.1f .. %.1f]" % (med(v), min(v), max(v))                  # noqa: E731
    lut = ops.input_lut(MEAN, STD, dev)
    mean = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    scale = torch.full((), 255.0, device=dev)
    lines = ["# input batch from a resident uint8 split, us per call (median [min .. max] of %d round medians, %d iterations after %d "
             "warm-up each, the routes alternating), %s" % (a.rounds, a.iters, a.warmup, torch.cuda.get_device_name(0)),
             "# shape | format | kernel | torch chain | chain/kernel | MB read + written by the kernel | of roof (6.29 TB/s)"]
    for B, S, side in SHAPES:
        n = max(B, a.images * 256 * 256 // (side * side))
        g = torch.Generator(device=dev).manual_seed(1)
        resident = torch.randint(0, 256, (n, side, side, 3), device=dev, dtype=torch.uint8, generator=g)
        idx = torch.randint(0, n, (B,), device=dev, generator=g)
        flip = torch.rand(B, device=dev, generator=g) < 0.5
        flip8 = flip.to(torch.uint8)
        top = left = int(round((side - S) / 2.0))
        for name, dtype, cl in FORMATS:
            kernel = lambda: ops.input_batch(resident, lut, S, idx=idx, flip=flip8, dtype=dtype, channels_last=cl)   # noqa: E731
            chain = lambda: torch_chain(resident, idx, flip, top, left, S, mean, std, dtype, cl, scale)                      # noqa: E731
            x, y = kernel(), chain()
            same = torch.equal(x, y) and x.stride() == y.stride()
            routes = {"kernel": kernel, "chain": chain}
            got = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    got[k].append(timed(fn, a.iters, a.warmup))
            moved = 3 * S * S * B * (1 + x.element_size()) + 9 * B + 3072
            lines.append("B %d %dx%d from %dx%d (%d rows) | %s | %s | %s | %.2fx | %.1f | %.0f%% | outputs %s" % (
                B, S, S, side, side, n, name, f(got["kernel"]), f(got["chain"]), med(got["chain"]) / med(got["kernel"]), moved / 1e6,
                100.0 * moved / HBM_BYTES_PER_US / med(got["kernel"]), "bit-equal" if same else "DIFFER"))
            print(lines[-1], flush=True)
        del resident
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

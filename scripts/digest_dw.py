"""Digests of the depthwise-conv results over a seeded sweep of shapes, to compare two builds of the library bit for bit:

    MOMA_HIP_LIB=/path/to/libmoma_hip.so python scripts/digest_dw.py out.txt [cases]

One line per case: the shape and the SHA-256 of y, dx, dw and the fused (BN + SiLU prologue, running statistics) y.  Both storage
types, k 3 / 5, stride 1 / 2, planes 7 .. 112 (odd sizes too), ragged N * C; every fifth case has enough planes that the waves of
a launch walk over several work items.  `diff` of two such files is the comparison."""
import hashlib
import math
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from moma_amd import ops


def digest(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    out, cases = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rng = random.Random(20240611)
    sizes = [7, 8, 13, 14, 15, 27, 28, 29, 56, 57, 112]
    with open(out, "w") as f:
        for i in range(cases):
            dtype = rng.choice([torch.bfloat16, torch.float32])
            K, S, H = rng.choice([3, 5]), rng.choice([1, 2]), rng.choice(sizes)
            budget = (6 << 20) if i % 5 == 0 else (1 << 19)          # elements of x
            C = rng.choice([1, 3, 5, 7, 12, 37])
            N = max(1, rng.randrange(budget // 2, budget) // (C * H * H))
            OH = math.ceil(H / S)
            p = max((OH - 1) * S + K - H, 0) // 2
            g = torch.Generator(device="cuda").manual_seed(i)
            x = torch.randn(N, C, H, H, device="cuda", generator=g).to(dtype).requires_grad_(True)
            w = (torch.randn(C, 1, K, K, device="cuda", generator=g) * 0.3).requires_grad_(True)
            dy = torch.randn(N, C, OH, OH, device="cuda", generator=g).to(dtype)
            y = ops.dwconv(x, w, S, p, p, OH, OH)
            dx, dw = torch.autograd.grad(y, [x, w], dy)
            gamma = torch.rand(C, device="cuda", generator=g) + 0.5
            beta = torch.randn(C, device="cuda", generator=g) * 0.3
            with torch.no_grad():
                fy = ops.bn_act_dwconv(x, gamma, beta, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), False, 0.01, 1e-3,
                                       "silu", w, S, p, p, OH, OH)
            f.write(f"{i} {str(dtype)[6:]} N{N} C{C} H{H} k{K} s{S} y {digest(y)} dx {digest(dx)} dw {digest(dw)} fused {digest(fy)}\n")
    print("wrote", out, cases, "cases")


if __name__ == "__main__":
    main()

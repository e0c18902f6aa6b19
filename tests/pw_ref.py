"""Reference and shapes for the pointwise-convolution weight gradient (moma_pwconv_bwd_weight):
    dw[co, ci] = sum_{n, y, x} dy[n, co, y, x] * x[n, ci, y, x]
in float64, plus the data generators the GPU and CPU tests share."""
import torch

# (N, Cin, Cout, H, W): the smallest shapes at which each mechanism of the kernel can go wrong
SHAPES = [
    (3, 16, 96, 8, 8),        # aligned baseline
    (2, 5, 7, 7, 7),          # channels below one MFMA tile, 49-element planes (2-byte-aligned rows)
    (3, 24, 40, 14, 14),      # 196-element planes (8-byte aligned), channels not a multiple of 16
    (5, 33, 17, 3, 5),        # K tail shorter than one MFMA step, ragged in every dimension
    (11, 16, 16, 28, 28),     # a prime N: uneven image ranges of the K split
    (2, 192, 130, 7, 7),      # several output tiles in both directions with ragged edge tiles
    (7, 48, 20, 1, 1),        # the squeeze-excite case, HW = 1
    (4, 6, 144, 1, 1),
]


def wgrad_f64(x, dy):
    """[Cout, Cin] float64 from x [N, Cin, H, W] and dy [N, Cout, H, W] (any float dtype: the values as stored)"""
    return torch.einsum("nohw,nihw->oi", dy.double(), x.double())


def wgrad_abs_f64(x, dy):
    """S[co, ci] = sum |dy * x| in float64: the scale of the accumulation error of an fp32 sum of the same products"""
    return torch.einsum("nohw,nihw->oi", dy.double().abs(), x.double().abs())


def exact_data(shape, seed=0):
    """Integers in [-3, 3], asymmetric between the operands (x mostly positive, dy mostly negative, different generators), so that
    every partial sum is exact in fp32 and a swapped row / column or operand shows."""
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randint(-1, 4, (N, Cin, H, W), generator=g).float()
    dy = torch.randint(-3, 2, (N, Cout, H, W), generator=g).float()
    return x, dy


def random_data(shape, seed=0):
    """Normal data rounded to bf16 (returned as bf16)"""
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(N, Cin, H, W, generator=g).bfloat16()
    dy = (torch.randn(N, Cout, H, W, generator=g) * 0.5 + 0.1).bfloat16()
    return x, dy


def bound(ref, S, L):
    """|got - ref| <= 2^-8 |ref| + L 2^-23 S: twice the worst case of one bf16 rounding (2^-9 |ref|) plus any-order fp32
    accumulation of L exact products (L 2^-24 S)."""
    return 2.0 ** -8 * ref.abs() + L * 2.0 ** -23 * S

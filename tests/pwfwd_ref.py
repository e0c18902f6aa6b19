"""Reference, shapes and data for the pointwise-convolution forward and input gradient (moma_pwconv_fwd, moma_pwconv_bwd_data):
    y[n, co, p]  = sum_ci w[co, ci] * x[n, ci, p]          dx[n, ci, p] = sum_co w[co, ci] * dy[n, co, p]
in float64, plus the generators the GPU and CPU tests share.  "Direction" below: False = forward (the activation has Cin channels
and the sum runs over K = Cin), True = input gradient (the activation has Cout channels, K = Cout)."""
import torch

# (N, Cin, Cout, H, W): the smallest shapes at which each mechanism of the kernel can go wrong
SHAPES = [
    (3, 16, 96, 8, 8),        # aligned; K below one MFMA step
    (2, 24, 144, 14, 14),     # K tail; 8-byte-aligned 196-pixel rows; pixel-tile tail
    (3, 40, 240, 4, 4),       # two K steps with a tail
    (2, 96, 24, 12, 12),      # project form; Cout not a multiple of 16
    (5, 33, 17, 3, 5),        # ragged everywhere; 2-byte-aligned rows
    (2, 192, 130, 7, 7),      # 49-pixel planes; several K steps; ragged Cout tiles
    (2, 16, 672, 4, 4),       # the Cout loop across waves and workgroups
    (11, 16, 16, 28, 28),     # prime N; several pixel tiles per image
]
DIRECTIONS = [False, True]


def product_f64(a, w, transposed):
    """float64 result from the activation a and w [Cout, Cin] (any float dtype: the values as stored)"""
    return torch.einsum("oi,nohw->nihw" if transposed else "oi,nihw->nohw", w.double(), a.double())


def product_abs_f64(a, w, transposed):
    """S = sum |w * a| per output in float64: the scale of the accumulation error of an fp32 sum of the same products"""
    return product_f64(a.double().abs(), w.double().abs(), transposed)


def depth(shape, transposed):
    """K, the number of products per output"""
    return shape[2] if transposed else shape[1]


def _act_shape(shape, transposed):
    N, Cin, Cout, H, W = shape
    return (N, Cout if transposed else Cin, H, W)


def exact_data(shape, transposed, seed=0):
    """Integers, asymmetric between the operands (activation in [0, 3], weight in [-2, 1], different draws), thinned with K so that
    every output is an integer of magnitude <= 256 (asserted by the CPU test): the fp32 sum and its bf16 rounding are exact."""
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(3000 + seed + (500 if transposed else 0))
    keep = min(1.0, (40.0 / depth(shape, transposed)) ** 0.5)
    a = torch.randint(0, 4, _act_shape(shape, transposed), generator=g).float()
    a = a * (torch.rand(a.shape, generator=g) < keep)
    w = torch.randint(-2, 2, (Cout, Cin), generator=g).float()
    w = w * (torch.rand(w.shape, generator=g) < keep)
    return a, w


def random_data(shape, transposed, seed=0):
    """Normal data rounded to bf16 (returned as bf16): activation and weight [Cout, Cin]"""
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(4000 + seed + (500 if transposed else 0))
    a = (torch.randn(_act_shape(shape, transposed), generator=g) + 0.1).bfloat16()
    w = (torch.randn(Cout, Cin, generator=g) * 0.2).bfloat16()
    return a, w


def bound(ref, S, K):
    """|got - ref| <= 2^-8 |ref| + K 2^-23 S: twice the worst case of one bf16 rounding (2^-9 |ref|) plus any-order fp32
    accumulation of K exact products (K 2^-24 S) -- the derivation of tests/pw_ref.bound."""
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S


def bf16_ulp(ref):
    """one bf16 unit in the last place at the magnitude of ref (float64)"""
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -120))) - 7)

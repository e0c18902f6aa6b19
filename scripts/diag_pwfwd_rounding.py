"""Who rounds how: the streaming pointwise kernel (ops.pwconv_fwd / ops.pwconv_bwd_data) and stock F.conv2d /
aten.convolution_backward (whatever solver MIOpen's find step picks in this process) against the float64 product of the same bf16
values.

    python scripts/diag_pwfwd_rounding.py > profiles/pwfwd_rounding_vs_float64.txt

Part 1: the 16 cases of tests/pwfwd_ref.py (8 shapes x forward / input gradient), max error / bound per route (the bound of
tests/test_gpu_pwconv_fwd.py), the mean SIGNED relative error in the direction of the value (0 for round-to-nearest, about -2.8e-3
for truncation to bf16) and the share of elements in which the two routes differ.
Part 2: the same, layer by layer, inside the small backbone of tests/test_gpu_pwconv_fwd.py (4 x 3 x 64 x 64, eval, bf16 autocast,
switch on): every bias-free pointwise convolution on the input it actually receives.
Part 3: the two pointwise convolutions of the MBConv block of tests/test_gpu_pwconv.py (4 x 16 x 14 x 14), forward and input gradient."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

from moma_amd import ops
from tests import pwfwd_ref as R


def stock(a, w4, transposed):
    if not transposed:
        return F.conv2d(a, w4)
    x = torch.zeros(a.shape[0], w4.shape[1], a.shape[2], a.shape[3], dtype=a.dtype, device=a.device)
    return torch.ops.aten.convolution_backward(a, x, w4, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])[0]


def line(name, a, w, transposed):
    """a: activation bf16 on the GPU, w: [Cout, Cin] bf16 on the GPU"""
    Cout, Cin = w.shape
    w4 = w.view(Cout, Cin, 1, 1)
    ref, S = R.product_f64(a.cpu(), w.cpu(), transposed), R.product_abs_f64(a.cpu(), w.cpu(), transposed)
    lim = R.bound(ref, S, Cout if transposed else Cin)
    nat = (ops.pwconv_bwd_data if transposed else ops.pwconv_fwd)(a, w4)
    stk = stock(a, w4, transposed)
    out = []
    sel = ref.abs() > 1e-3 * ref.abs().max()
    for got in (nat, stk):
        e = got.cpu().double() - ref
        out.append((float((e.abs() / lim).max()), float((e * ref.sign() / ref.abs().clamp_min(1e-300))[sel].mean())))
    differ = float((nat != stk).float().mean())
    print(f"{name:<44s} {'dx ' if transposed else 'fwd'} kernel {out[0][0]:5.3f} {out[0][1]:+9.2e} | stock {out[1][0]:5.3f} {out[1][1]:+9.2e} | "
          f"differ {100 * differ:6.2f} %", flush=True)


def main():
    print("columns: max error / bound, mean signed relative error (kernel | stock), share of elements in which the routes differ")
    print("\npart 1: the cases of tests/pwfwd_ref.py")
    for shape in R.SHAPES:
        for transposed in R.DIRECTIONS:
            a, w = R.random_data(shape, transposed)
            line(str(shape), a.cuda(), w.cuda(), transposed)

    from moma_amd.backbones import efficientnet as E
    print("\npart 2: the bias-free pointwise convolutions of efficientnet_b0 on 4 x 3 x 64 x 64 (eval, bf16 autocast), each on its own input")
    torch.manual_seed(31)
    model = E.efficientnet_b0(num_classes=10).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(32)
    x = torch.randn(4, 3, 64, 64, generator=g, device="cuda")
    seen, hooks = [], []
    for n, m in model.named_modules():
        if isinstance(m, E.SamePadConv2d) and m.kernel_size == (1, 1) and m.bias is None:
            hooks.append(m.register_forward_pre_hook(lambda mod, args, n=n: seen.append((n, mod, args[0].detach().bfloat16().clone()))))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(x, is_feat=True)
    for h in hooks:
        h.remove()
    for n, m, a in seen:
        w = m.weight.detach().bfloat16().view(m.out_channels, m.in_channels)
        routed = ops.pwconv_fwd_native(a.shape[0], m.in_channels, m.out_channels, a.shape[2] * a.shape[3])
        line(f"{n} {m.in_channels}->{m.out_channels} {a.shape[2]}x{a.shape[3]}{'' if routed else ' (not routed)'}", a, w, False)

    print("\npart 3: the pointwise convolutions of MBConvBlock(3, 1, 6, 16, 16) on 4 x 16 x 14 x 14")
    for Cin, Cout in ((16, 96), (96, 16)):
        for transposed in R.DIRECTIONS:
            a, w = R.random_data((4, Cin, Cout, 14, 14), transposed, seed=7)
            line(f"{Cin}->{Cout} 14x14 batch 4", a.cuda(), w.cuda(), transposed)


if __name__ == "__main__":
    main()

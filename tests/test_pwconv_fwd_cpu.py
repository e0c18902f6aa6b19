"""CPU checks around the pointwise-convolution forward and input gradient on the streaming kernel: the float64 reference the GPU
tests compare against is autograd's conv2d, the exact data keeps its promise, and the routing predicate of SamePadConv2d picks the
spatial bias-free pointwise convolutions of the layer table (asked without a device).  That the library builds for gfx950 with the
new symbols declared, bound and exported, and that they refuse NULL / negative / zero arguments, is test_abi_cpu.py's table."""
import pytest
import torch
import torch.nn.functional as F

from tests import pwfwd_ref as R


@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_is_autograds_conv2d(shape):
    N, Cin, Cout, H, W = shape
    x, w = R.random_data(shape, False)
    dy, _ = R.random_data(shape, True)
    x = x.double().requires_grad_(True)
    y = F.conv2d(x, w.double().view(Cout, Cin, 1, 1))
    torch.testing.assert_close(y, R.product_f64(x.detach(), w, False), rtol=1e-13, atol=1e-13)
    y.backward(dy.double())
    torch.testing.assert_close(x.grad, R.product_f64(dy, w, True), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("transposed", R.DIRECTIONS)
def test_exact_data_is_exact_in_bf16_and_asymmetric(transposed):
    for shape in R.SHAPES:
        a, w = R.exact_data(shape, transposed)
        assert torch.equal(a, a.bfloat16().float()) and torch.equal(w, w.bfloat16().float())
        assert R.product_abs_f64(a, w, transposed).max() <= 256   # every partial sum and every output: an integer bf16 holds
        ref = R.product_f64(a, w, transposed)
        assert torch.equal(ref, ref.bfloat16().double()) and ref.abs().max() >= 8
        assert a.min() == 0 and a.max() == 3 and w.min() == -2 and w.max() == 1


def _plane_sizes(model, size):
    """name -> (N, pixels) of the input of every SamePadConv2d in a forward at size x size"""
    from moma_amd.backbones.efficientnet import SamePadConv2d
    seen, hooks = {}, []
    for n, m in model.named_modules():
        if isinstance(m, SamePadConv2d):
            hooks.append(m.register_forward_pre_hook(
                lambda mod, args, n=n: seen.__setitem__(n, (args[0].shape[0], args[0].shape[2] * args[0].shape[3]))))
    with torch.no_grad():
        model.eval()(torch.zeros(1, 3, size, size))
    for h in hooks:
        h.remove()
    return seen


def _routed(model, planes, live):
    from moma_amd.backbones.efficientnet import SamePadConv2d
    out = set()
    for n, m in model.named_modules():
        if isinstance(m, SamePadConv2d):
            m._wc_live = live and not (m.groups > 1)             # what _refresh_weight_cache sets for a bf16-autocast GPU forward
            N, hw = 256, planes[n][1]                            # the plane sizes of a 224 x 224 input at the benchmark's batch
            if m._takes_pwfwd(True, torch.bfloat16, N, hw):
                out.add(n)
            assert not m._takes_pwfwd(False, torch.bfloat16, N, hw) and not m._takes_pwfwd(True, torch.float32, N, hw)
            m._wc_live = False
    return out


def test_routing_selects_the_spatial_bias_free_pointwise_convolutions_of_the_table(monkeypatch):
    from moma_amd.backbones import efficientnet as E
    model = E.efficientnet_b0(num_classes=4)
    planes = _plane_sizes(model, 224)
    monkeypatch.setattr(E, "_PW_MODE", "hip")
    monkeypatch.setattr(E, "_PW_FWD", "1")
    # the layer table: expand / project / head convolutions on the 112^2, 56^2, 28^2 and 14^2 planes; the 7^2 ones keep MIOpen
    table = {n for n, m in model.named_modules()
             if isinstance(m, E.SamePadConv2d) and m.kernel_size == (1, 1) and m.bias is None
             and planes[n][1] in (112 * 112, 56 * 56, 28 * 28, 14 * 14) and m.out_channels > 16}
    assert len(table) == 21                                       # all 22 of those planes but 32 -> 16, which keeps MIOpen's rounding
    routed = _routed(model, planes, live=True)
    assert routed == table
    assert not any(n.endswith(("_se_reduce", "_se_expand")) for n in routed)            # never a squeeze-excite layer
    assert "_conv_stem" not in routed and not any("_depthwise_conv" in n for n in routed)
    assert "_blocks.0._project_conv" not in routed and "_blocks.1._project_conv" in routed and "_blocks.1._expand_conv" in routed and "_conv_head" not in routed
    # _takes_pwconv keeps its meaning: all 64 pointwise convolutions, whatever the new switch says
    for flag in ("1", "0"):
        monkeypatch.setattr(E, "_PW_FWD", flag)
        for m in model.modules():
            if isinstance(m, E.SamePadConv2d):
                m._wc_live = m.groups == 1
        assert sum(m._takes_pwconv(True, torch.bfloat16) for m in model.modules() if isinstance(m, E.SamePadConv2d)) == 64
    # the switch off or MOMA_PW=miopen: none; the weight cache does not enter (it must stay transparent)
    assert _routed(model, planes, live=True) == set() and _routed(model, planes, live=False) == set()
    monkeypatch.setattr(E, "_PW_FWD", "1")
    assert _routed(model, planes, live=False) == table
    monkeypatch.setattr(E, "_PW_MODE", "miopen")
    assert _routed(model, planes, live=True) == set()


def test_shape_predicate_names_the_classes_of_the_layer_table():
    from moma_amd import ops
    for hw in (112 * 112, 56 * 56, 28 * 28, 14 * 14):
        assert ops.pwconv_fwd_native(256, 16, 96, hw) and ops.pwconv_fwd_native(256, 672, 112, hw)
    assert not ops.pwconv_fwd_native(256, 192, 1152, 49)         # 7 x 7: element accesses, measured slower
    assert not ops.pwconv_fwd_native(256, 480, 20, 1)            # squeeze-excite planes
    assert not ops.pwconv_fwd_native(256, 32, 16, 112 * 112)     # at most 16 output channels: MIOpen's rounding is kept
    assert ops.pwconv_fwd_native(4, 16, 96, 14 * 14) and ops.pwconv_fwd_native(1, 16, 96, 4)      # the batch does not enter

"""CPU checks around the pointwise-convolution weight gradient: the float64 reference the GPU tests compare against is autograd's
conv2d weight gradient, and the routing predicate of SamePadConv2d picks exactly the pointwise convolutions (asked without a
device).  That the library builds for gfx950 with the new symbols declared, bound and exported is test_abi_cpu.py's table."""
import pytest
import torch
import torch.nn.functional as F

from tests import pw_ref as R


@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_is_autograds_conv2d_weight_gradient(shape):
    N, Cin, Cout, H, W = shape
    x, dy = R.random_data(shape)
    x, dy = x.double(), dy.double()
    w = torch.zeros(Cout, Cin, 1, 1, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w).backward(dy)
    ref = R.wgrad_f64(x, dy)
    assert ref.shape == (Cout, Cin)
    torch.testing.assert_close(w.grad[:, :, 0, 0], ref, rtol=1e-13, atol=1e-13)


def test_exact_data_is_exact_in_fp32_and_asymmetric():
    for shape in R.SHAPES:
        x, dy = R.exact_data(shape)
        assert R.wgrad_abs_f64(x, dy).max() < 2 ** 24            # every partial sum of the products is an fp32 integer
        assert x.mean() > 0.5 and dy.mean() < -0.5


def _pointwise_names(model):
    from moma_amd.backbones.efficientnet import SamePadConv2d
    return {n for n, m in model.named_modules() if isinstance(m, SamePadConv2d) and m.kernel_size == (1, 1)}


def _routed(model, live):
    from moma_amd.backbones.efficientnet import SamePadConv2d
    out = set()
    for n, m in model.named_modules():
        if isinstance(m, SamePadConv2d):
            m._wc_live = live and not (m.groups > 1)             # what _refresh_weight_cache sets for a bf16-autocast GPU forward
            if m._takes_pwconv(True, torch.bfloat16):
                out.add(n)
            assert not m._takes_pwconv(False, torch.bfloat16) and not m._takes_pwconv(True, torch.float32)
            m._wc_live = False
    return out


def test_routing_selects_exactly_the_64_pointwise_convolutions(monkeypatch):
    from moma_amd.backbones import efficientnet as E
    model = E.efficientnet_b0(num_classes=4)
    monkeypatch.setattr(E, "_PW_MODE", "hip")
    names = _pointwise_names(model)
    assert len(names) == 64
    assert sum(n.endswith(("_se_reduce", "_se_expand")) for n in names) == 32
    assert _routed(model, live=True) == names
    assert "_conv_stem" not in names and not any("_depthwise_conv" in n for n in names)
    # the weight cache off (MOMA_WCACHE=0: no forward ever sets _wc_live) or MOMA_PW=miopen: none
    assert _routed(model, live=False) == set()
    monkeypatch.setattr(E, "_PW_MODE", "miopen")
    assert _routed(model, live=True) == set()


def test_weight_cache_switch_keeps_the_cache_dead_on_cpu(monkeypatch):
    """_wc_live only ever comes from _refresh_weight_cache, which needs _WCACHE, a GPU input and bf16 autocast"""
    from moma_amd.backbones import efficientnet as E
    model = E.efficientnet_b0(num_classes=4)
    for flag in (True, False):
        monkeypatch.setattr(E, "_WCACHE", flag)
        model._refresh_weight_cache(torch.zeros(1, 3, 32, 32))
        assert not any(m._wc_live for m in model.modules() if isinstance(m, E.SamePadConv2d))

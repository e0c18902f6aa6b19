"""BN1 + activation inside the squeeze-excite gate (ops.bn_act_mean / ops.bn_act_gate, csrc/bnse.hip), what holds without a GPU:
the plane-sum decomposition the backward kernels implement reproduces torch.autograd of the composite in fp64; the ops refuse CPU
tensors; a block on the CPU keeps the stock path.  (tests/test_abi_cpu.py walks the new entry points with every other one.)"""
import pytest
import torch

from tests import bnse_ref

EPS = 1e-3


def _operands(shape, seed=0):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    D = torch.randn(shape, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gamma = torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 1.0
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.1 + 0.7
    rm = torch.randn(C, generator=g, dtype=torch.float64) * 0.2 + 0.3
    rv = torch.randn(C, generator=g, dtype=torch.float64).abs() + 0.5
    M = torch.randn(C, C, generator=g, dtype=torch.float64) / C ** 0.5
    dG = torch.randn(shape, generator=g, dtype=torch.float64)
    return D, gamma, beta, rm, rv, M, dG


@pytest.mark.parametrize("act", ["silu", "none"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(3, 5, 9, 9), (2, 4, 14, 14), (70, 3, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_plane_sum_decomposition_is_the_gradient_of_the_composite(shape, training, act):
    D, gamma, beta, rm, rv, M, dG = _operands(shape)
    leaves = [t.clone().requires_grad_(True) for t in (D, gamma, beta, M)]
    G, pooled, s = bnse_ref.composite(leaves[0], leaves[1], leaves[2], rm, rv, leaves[3], training, act, EPS)
    want = torch.autograd.grad(G, leaves + [s], dG)
    got = bnse_ref.decomposed_grads(D, gamma, beta, rm, rv, M, dG, training, act, EPS)
    dD, dgamma, dbeta, ds, dM = got
    for name, g, w in zip(("dD", "dgamma", "dbeta", "dM", "ds"), (dD, dgamma, dbeta, dM, ds), want):
        torch.testing.assert_close(g, w, rtol=1e-10, atol=1e-11 * max(1.0, w.abs().max().item()), msg=lambda m, n=name: f"{n}: {m}")


def test_ops_refuse_cpu_tensors():
    from moma_amd import _lib, ops
    d = torch.zeros(2, 3, 4, 4)
    with pytest.raises(_lib.MomaHipError):
        ops.bn_act_mean(d, torch.ones(3), torch.zeros(3), torch.zeros(3), torch.ones(3), True, 0.1, EPS, "silu")
    with pytest.raises(_lib.MomaHipError):
        ops.bn_act_gate(d, torch.zeros(3, 2), torch.zeros(2, 3, 1, 1))


@pytest.mark.parametrize("mode", ["1", "all", "nograd"])
def test_block_on_the_cpu_keeps_the_stock_path(mode, monkeypatch):
    from moma_amd import ops
    from moma_amd.backbones import efficientnet as E

    def refuse(*a, **k):
        raise AssertionError("the fused path was taken on the CPU")
    monkeypatch.setattr(ops, "bn_act_mean", refuse)
    monkeypatch.setattr(ops, "bn_act_gate", refuse)
    monkeypatch.setattr(E, "_SE_FUSE", mode)
    torch.manual_seed(0)
    blk = E.MBConvBlock(3, 1, 6, 8, 8, 0.25)
    x = torch.randn(2, 8, 10, 10)
    with torch.no_grad():
        y = blk(x)
    assert y.shape == x.shape and torch.isfinite(y).all()
    blk(x).sum().backward()
    assert blk._bn1.weight.grad is not None


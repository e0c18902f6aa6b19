"""BN0 + SiLU applied inside the depthwise kernels (ops.bn_act_dwconv, MBConvBlock's fused path): every result must equal the
unfused chain of the same build, ops.dwconv(ops.bn_act(E, ...), ...), BIT FOR BIT -- the fused kernels round each normalised,
activated element to the storage type before it enters the tile, so the tile holds what it held after loading the materialised
activation.  beta sits around 0.7: a padding element that went through the activation (act(shift) != 0) changes the border
outputs.  The unfused chain itself is pinned by test_gpu_kernels / test_gpu_step / the golden step traces."""
import copy
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_guard import _Guarded, guard, _in, _rand  # noqa: F401  (`guard` is a fixture)

pytestmark = pytest.mark.gpu

# (N, C, H, W, K, S) and the code path each is the smallest shape of
SHAPES = [
    (3, 5, 9, 9, 3, 1),         # odd plane: scalar loads
    (2, 6, 16, 16, 5, 2),       # asymmetric SAME padding, 16-byte vectors
    (2, 3, 30, 30, 3, 2),       # 4-byte vectors in bf16
    (2, 4, 14, 14, 5, 1),       # dw_small_kernel, 14 x 14
    (9, 3, 7, 7, 3, 1),         # dw_small_kernel, 7 x 7: 27 planes, a ragged last group of 8
    (1, 2, 56, 56, 3, 1),       # two bands per plane: zero_rows with the prologue; backward-weight through the dy tile
    (2, 3, 28, 28, 5, 1),
]
MOM, EPS = 0.1, 1e-3


def _same(H, W, K, S):
    """(pad_top, pad_left, OH, OW) of TensorFlow SAME padding"""
    oh, ow = math.ceil(H / S), math.ceil(W / S)
    ph, pw = max((oh - 1) * S + K - H, 0), max((ow - 1) * S + K - W, 0)
    return ph // 2, pw // 2, oh, ow


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    a, b = _bits(a), _bits(b)
    if not torch.equal(a, b):
        bad = (a != b)
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} elements differ, largest distance "
                             f"{int((a.int() - b.int()).abs().max())} ulp")


def _operands(shape, dtype, seed=0):
    N, C, H, W, K, S = shape
    rng = np.random.default_rng(seed + sum(shape))
    E = (_rand(rng, N, C, H, W, scale=1.5) + 0.3).to(dtype)
    gamma = _rand(rng, C) * 0.5 + 1.0
    beta = _rand(rng, C) * 0.1 + 0.7
    rm, rv = _rand(rng, C) * 0.2 + 0.3, _rand(rng, C).abs() + 0.5
    w = _rand(rng, C, 1, K, K, scale=0.4)
    pt, pl, oh, ow = _same(H, W, K, S)
    dD = _rand(rng, N, C, oh, ow).to(dtype)
    return E, gamma, beta, rm, rv, w, dD, (S, pt, pl, oh, ow)


def _run(fused, ops, E, gamma, beta, rm, rv, w, dD, geo, training, act):
    """forward + backward on fresh leaves -> (D, dE, dgamma, dbeta, dW, running_mean, running_var)"""
    E, gamma, beta, w = (t.clone().requires_grad_(True) for t in (E, gamma, beta, w))
    rm, rv = rm.clone(), rv.clone()
    if fused:
        D = ops.bn_act_dwconv(E, gamma, beta, rm, rv, training, MOM, EPS, act, w, *geo)
    else:
        D = ops.dwconv(ops.bn_act(E, gamma, beta, rm, rv, training, MOM, EPS, act), w, *geo)
    grads = torch.autograd.grad(D, [E, gamma, beta, w], dD)
    return (D.detach(), *grads, rm, rv)


NAMES = ("D", "dE", "dgamma", "dbeta", "dW", "running_mean", "running_var")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act", ["silu", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_equals_the_unfused_chain_bit_for_bit(shape, act, training, dtype):
    from moma_amd import ops
    args = _operands(shape, dtype)
    want = _run(False, ops, *args, training, act)
    got = _run(True, ops, *args, training, act)
    assert got[4].dtype == torch.float32 and got[2].dtype == torch.float32
    for name, g, w_ in zip(NAMES, got, want):
        _same_bits(g, w_, f"{name} {shape} {act} training={training} {dtype}")
    # the padding is zero of the ACTIVATION: with beta ~ 0.7 a transformed halo would have moved the border outputs
    assert torch.isfinite(got[0].float()).all()


def test_only_the_weight_or_only_the_input_gradient():
    """needs_input_grad: each subset of gradients is produced by the calls it needs, with the same bits"""
    from moma_amd import ops
    E, gamma, beta, rm, rv, w, dD, geo = _operands((2, 6, 16, 16, 5, 2), torch.bfloat16)
    full = _run(True, ops, E, gamma, beta, rm, rv, w, dD, geo, True, "silu")
    for pick in ((0,), (3,), (1, 2)):
        leaves = [t.clone() for t in (E, gamma, beta, w)]
        for i in pick:
            leaves[i].requires_grad_(True)
        D = ops.bn_act_dwconv(leaves[0], leaves[1], leaves[2], rm.clone(), rv.clone(), True, MOM, EPS, "silu", leaves[3], *geo)
        grads = torch.autograd.grad(D, [leaves[i] for i in pick], dD)
        for i, g in zip(pick, grads):
            _same_bits(g, full[1 + i], f"gradient {i} alone")


# ---- the block and the model ------------------------------------------------------------------------------------
def _randomise_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1 + 0.7)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _flat(o)]


def _forward(module, x, fuse, train, amp, grad, monkeypatch, **kw):
    from moma_amd.backbones import efficientnet as E
    m = copy.deepcopy(module).train(train)
    monkeypatch.setattr(E, "_BNDW_FUSE", "grad" if fuse else "0")       # ("1", the default: test_default_fuses_...)
    if grad:
        # MIOpen's default fp32 weight gradients of the 1x1 convolutions around the pair differ from run to run of the SAME path;
        # deterministic solver selection leaves the code under test as the only difference.  Still bit for bit.
        monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(1234)                                     # stochastic depth / dropout draw the same numbers
    x = x.clone().requires_grad_(grad)
    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        outs = _flat(m(x, **kw))
    grads = {}
    if grad:
        sum(o.float().square().sum() for o in outs).backward()
        grads = {n: p.grad for n, p in m.named_parameters()}
        grads["input"] = x.grad
    return [o.detach() for o in outs], m.state_dict(), grads


def _calls(monkeypatch):
    """count the fused op's calls (the comparison must not compare the unfused path with itself)"""
    from moma_amd import ops
    n = [0]
    real = ops.bn_act_dwconv

    def counted(*a, **k):
        n[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "bn_act_dwconv", counted)
    return n


@pytest.mark.parametrize("amp", [True, False], ids=["bf16-autocast", "fp32"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_block_is_unchanged_by_the_fusion(train, amp, monkeypatch):
    from moma_amd.backbones.efficientnet import MBConvBlock
    torch.manual_seed(0)
    blk = MBConvBlock(5, 2, 6, 8, 12, 0.25).cuda()
    _randomise_bn(blk, 1)
    x = torch.randn(4, 8, 18, 18, device="cuda")
    n = _calls(monkeypatch)
    for grad in (False, True):
        before = n[0]
        o1, sd1, g1 = _forward(blk, x, True, train, amp, grad, monkeypatch)
        assert n[0] == before + 1
        o0, sd0, g0 = _forward(blk, x, False, train, amp, grad, monkeypatch)
        assert n[0] == before + 1
        for a, b in zip(o1, o0):
            _same_bits(a, b, f"block output grad={grad}")
        assert sd1.keys() == sd0.keys()
        for k in sd1:
            assert torch.equal(sd1[k], sd0[k]), k               # BN buffers, num_batches_tracked included
        assert g1.keys() == g0.keys()
        for k in g1:
            assert (g1[k] is None) == (g0[k] is None), k
            if g1[k] is not None:
                _same_bits(g1[k], g0[k], f"gradient of {k}")


@pytest.mark.parametrize("amp", [True, False], ids=["bf16-autocast", "fp32"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_model_forward_is_unchanged_by_the_fusion(train, amp, monkeypatch):
    """(no gradients here: MIOpen's weight gradients are not deterministic from run to run)"""
    from moma_amd.backbones.efficientnet import efficientnet_b0
    torch.manual_seed(0)
    model = efficientnet_b0(num_classes=5).cuda()
    _randomise_bn(model, 2)
    x = torch.randn(4, 3, 64, 64, device="cuda")
    n = _calls(monkeypatch)
    o1, sd1, _ = _forward(model, x, True, train, amp, False, monkeypatch, is_feat=True)
    assert n[0] == 15                                           # every block with an expansion
    o0, sd0, _ = _forward(model, x, False, train, amp, False, monkeypatch, is_feat=True)
    assert n[0] == 15
    assert len(o1) == len(o0) == 7
    for i, (a, b) in enumerate(zip(o1, o0)):
        _same_bits(a, b, f"feature {i}")
    for k in sd1:
        assert torch.equal(sd1[k], sd0[k]), k
    if train:
        assert int(sd1["_blocks.1._bn0.num_batches_tracked"]) == 1


# ---- graph capture ----------------------------------------------------------------------------------------------
def test_forward_and_backward_capture_into_a_graph():
    from moma_amd import ops
    E, gamma, beta, rm, rv, w, dD, geo = _operands((2, 6, 16, 16, 5, 2), torch.bfloat16)
    want = _run(True, ops, E, gamma, beta, rm, rv, w, dD, geo, True, "silu")
    leaves = [t.clone().requires_grad_(True) for t in (E, gamma, beta, w)]
    rm_g, rv_g = rm.clone(), rv.clone()

    def step():
        D = ops.bn_act_dwconv(leaves[0], leaves[1], leaves[2], rm_g, rv_g, True, MOM, EPS, "silu", leaves[3], *geo)
        return (D.detach(), *torch.autograd.grad(D, leaves, dD))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, g, w_ in zip(NAMES, outs, want):
            _same_bits(g, w_, f"replayed {name}")


# ---- writes stay inside, reads stay inside -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [((5, 3, 9, 11, 3, 1), torch.float32), ((3, 24, 28, 28, 5, 2), torch.bfloat16)],
                         ids=["5x3x9x11-fp32", "3x24x28x28-bf16"])
def test_fused_op_between_guards(guard, shape, dtype, monkeypatch):
    """operands between NaN guards, outputs / workspaces / saved tensors between canaries (tests/test_gpu_guard.py)"""
    from moma_amd import ops
    E, gamma, beta, rm, rv, w, dD, geo = _operands(shape, dtype)
    with monkeypatch.context() as m:
        m.setattr(ops, "torch", torch)                          # the same call on ordinary allocations
        want = _run(True, ops, E, gamma, beta, rm, rv, w, dD, geo, True, "silu")
    gE, gg, gb, gw = (_in(guard, t).requires_grad_(True) for t in (E, gamma, beta, w))
    grm, grv, gdD = _in(guard, rm), _in(guard, rv), _in(guard, dD)
    D = ops.bn_act_dwconv(gE, gg, gb, grm, grv, True, MOM, EPS, "silu", gw, *geo)
    assert guard.check(f"fused forward {shape}") >= 7 + 5       # the operands + y, statistics, scale_shift, workspace
    grads = torch.autograd.grad(D, [gE, gg, gb, gw], gdD)
    assert guard.check(f"fused backward {shape}") >= 7          # dA, dE, dgamma, dbeta, dW and the two workspaces
    for name, g, w_ in zip(NAMES, (D.detach(), *grads, grm, grv), want):
        _same_bits(g, w_, f"guarded {name}")


def test_default_fuses_only_where_no_gradient_is_recorded(monkeypatch):
    """MOMA_BNDW=1: the fused op serves forwards without a recorded gradient (the teacher's passes); a training forward keeps
    the two calls, whose backward-weight kernel is the faster one"""
    from moma_amd.backbones import efficientnet as E
    from moma_amd.backbones.efficientnet import MBConvBlock
    monkeypatch.setattr(E, "_BNDW_FUSE", "1")
    torch.manual_seed(0)
    blk = MBConvBlock(5, 2, 6, 8, 12, 0.25).cuda()
    x = torch.randn(4, 8, 18, 18, device="cuda")
    n = _calls(monkeypatch)
    with torch.no_grad():
        blk(x)
    assert n[0] == 1
    blk(x).sum().backward()
    assert n[0] == 1 and blk._depthwise_conv.weight.grad is not None
    for p in blk.parameters():
        p.requires_grad_(False)
    blk(x)                                                       # grad mode on, nothing to record
    assert n[0] == 2

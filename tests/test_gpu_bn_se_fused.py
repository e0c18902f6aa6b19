"""BN1 + activation applied inside the squeeze-excite gate (ops.bn_act_mean / ops.bn_act_gate, MBConvBlock's fused path).
Forward: pooled, G and the running statistics must equal the unfused chain of the same build,
ops.se_gate(*ops.bn_act(D, ..., want_mean=True) ...), BIT FOR BIT -- the read-only pass adds up the unrounded activations in
bn_apply_mean_kernel's walk, and the gate rounds every activation to the storage type before it multiplies.  Backward: against the
fp64 composite in stock ops (tests/bnse_ref.py) with the tolerances tests/test_gpu_kernels.py uses for the same quantities
(test_bn_act_with_plane_mean: dD, dgamma, dbeta; test_se_gate_and_plane_mean_match_torch: what passes through the gate's logits),
and never more than twice as far from fp64 as the unfused chain on the same operands: the fused chain skips the rounding of the
activation's gradient to the storage type, the factor allows for reordered fp32 sums.  beta sits around 0.7, the inputs off-centre.

The map from the plane means to the logits stands in for layers outside the code under test: it runs in double (so that it adds
no rounding of its own to what is measured) and is small (tests/bnse_ref.py: SCALE, with the reasoning)."""
import numpy as np
import pytest
import torch

from tests import bnse_ref
from tests.test_gpu_bn_dw_fused import _flat, _randomise_bn, _same_bits
from tests.test_gpu_guard import _Guarded, guard, _in, _rand  # noqa: F401  (`guard` is a fixture)

pytestmark = pytest.mark.gpu

# (N, C, H, W) and the code path each is the smallest shape of
SHAPES = [
    (3, 5, 9, 9),          # odd plane: scalar loads, two trips per lane, ragged
    (2, 6, 16, 16),        # 16-byte vectors, fewer vectors than lanes
    (2, 3, 30, 30),        # 4-element vectors
    (2, 4, 14, 14),        # the workload's small planes
    (9, 3, 7, 7),          # 27 planes: a ragged last workgroup
    (1, 2, 56, 56),        # several trips per lane
    (8, 2, 56, 56),        # more than one statistics split
    (70, 3, 4, 4),         # the per-channel combine over N > 64
]
MOM, EPS = 0.1, 1e-3
GRADS = ("dD", "dgamma", "dbeta", "dM", "ds")


def _operands(shape, dtype, seed=0):
    N, C, H, W = shape
    rng = np.random.default_rng(seed + sum(shape))
    D = (_rand(rng, N, C, H, W, scale=1.5) + 0.3).to(dtype)
    gamma = _rand(rng, C) * 0.5 + 1.0
    beta = _rand(rng, C) * 0.1 + 0.7
    rm, rv = _rand(rng, C) * 0.2 + 0.3, _rand(rng, C).abs() + 0.5
    M = _rand(rng, C, C) / C ** 0.5
    dG = _rand(rng, N, C, H, W).to(dtype)
    return D, gamma, beta, rm, rv, M, dG


def _chain(fused, ops, D, gamma, beta, rm, rv, M, training, act):
    """-> (G, pooled, s): s from pooled through a small linear map, so both branches carry gradient.  The map (M: float64) runs in
    double: it stands in for layers outside the code under test and must add no rounding of its own to what is measured; s and
    the gradient of pooled are rounded to the tensors' type where they enter the ops, as in the block."""
    if fused:
        pooled, link = ops.bn_act_mean(D, gamma, beta, rm, rv, training, MOM, EPS, act)
        s = bnse_ref.smap(pooled.double(), M).to(D.dtype)
        return ops.bn_act_gate(D, link, s), pooled, s
    A, pooled = ops.bn_act(D, gamma, beta, rm, rv, training, MOM, EPS, act, want_mean=True)
    s = bnse_ref.smap(pooled.double(), M).to(D.dtype)
    return ops.se_gate(A, s), pooled, s


def _run(fused, ops, D, gamma, beta, rm, rv, M, dG, training, act, pick=(0, 1, 2, 3)):
    """forward + backward on fresh leaves -> {G, pooled, running_*, and the gradients of the picked leaves (and ds)}"""
    leaves = [t.clone() for t in (D, gamma, beta, M.double())]
    for i in pick:
        leaves[i].requires_grad_(True)
    rm, rv = rm.clone(), rv.clone()
    G, pooled, s = _chain(fused, ops, *leaves[:3], rm, rv, leaves[3], training, act)
    grads = torch.autograd.grad(G, [leaves[i] for i in pick] + [s], dG)
    out = {"G": G.detach(), "pooled": pooled.detach(), "running_mean": rm, "running_var": rv, "ds": grads[-1]}
    out.update({GRADS[i]: g for i, g in zip(pick, grads)})
    return out


_REF = {}


def _reference(shape, dtype, training, act):
    """the fp64 composite on the same operands, computed once per case"""
    key = (shape, dtype, training, act)
    if key not in _REF:
        D, gamma, beta, rm, rv, M, dG = (t.double() for t in _operands(shape, dtype))
        leaves = [t.requires_grad_(True) for t in (D, gamma, beta, M)]
        G, pooled, s = bnse_ref.composite(*leaves[:3], rm, rv, leaves[3], training, act, EPS)
        grads = torch.autograd.grad(G, leaves + [s], dG)
        _REF[key] = dict(zip(GRADS, grads))
    return _REF[key]


def _tolerances(name, ref, shape, dtype):
    """(rtol, atol) of tests/test_gpu_kernels.py for the same quantity"""
    f32 = dtype == torch.float32
    if name == "dD":                                             # test_bn_act_with_plane_mean: the input gradient
        rtol, atol = (2e-5, 2e-5) if f32 else (1e-2, 1e-2)
        return rtol, atol * max(1.0, ref.abs().max().item())
    if name in ("dgamma", "dbeta"):                              # test_bn_act_with_plane_mean: the parameter gradients
        n_el = shape[0] * shape[2] * shape[3]
        return 1e-3, 2e-4 * n_el ** 0.5 * (1 if f32 else 30)
    rtol, atol = (2e-5, 2e-5) if f32 else (1.6e-2, 1.6e-2)      # test_se_gate_and_plane_mean_match_torch: through the gate
    return rtol, atol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act", ["silu", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_bits_and_backward_against_fp64(shape, act, training, dtype):
    _check(shape, act, training, dtype)


def test_more_planes_than_one_grid_sweep():
    """70 x 480 = 33600 planes against the 32768 that one sweep of the largest grid (8192 workgroups of four waves) covers: the
    second trip of the plane loop of every kernel, as the 28 x 28 layers of the workload take it at B = 256 (61440 planes)"""
    _check((70, 480, 2, 2), "silu", True, torch.bfloat16)


def _check(shape, act, training, dtype):
    from moma_amd import ops
    args = _operands(shape, dtype)
    want = _run(False, ops, *args, training, act)
    got = _run(True, ops, *args, training, act)
    for name in ("pooled", "G", "running_mean", "running_var"):
        _same_bits(got[name], want[name], f"{name} {shape} {act} training={training} {dtype}")
    assert got["dgamma"].dtype == torch.float32 and got["dD"].dtype == dtype and got["ds"].dtype == dtype
    ref = _reference(shape, dtype, training, act)
    errs = {}
    for name in GRADS:
        r = ref[name].reshape(got[name].shape)
        errs[name] = ((got[name].double() - r).abs().max().item(), (want[name].double() - r).abs().max().item())
        print(f"{name}: fused {errs[name][0]:.3e}  unfused {errs[name][1]:.3e}  (max |ref| {r.abs().max().item():.3e})")
    for name in GRADS:
        r = ref[name].reshape(got[name].shape)
        rtol, atol = _tolerances(name, r, shape, dtype)
        torch.testing.assert_close(got[name].double(), r, rtol=rtol, atol=atol, msg=lambda m, n=name: f"{n}: {m}")
    for name in GRADS:
        assert errs[name][0] <= 2.0 * errs[name][1], (name, errs[name])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_subsets_and_repeated_runs_have_the_same_bits(dtype):
    """needs_input_grad: only D, only gamma / beta, only the logits (through the map alone); and the same call twice"""
    from moma_amd import ops
    args = _operands((3, 5, 9, 9), dtype)
    full = _run(True, ops, *args, True, "silu")
    again = _run(True, ops, *args, True, "silu")
    for name in full:
        _same_bits(again[name], full[name], f"second run: {name}")
    for pick in ((0,), (1, 2), (3,)):
        part = _run(True, ops, *args, True, "silu", pick=pick)
        assert set(part) == {"G", "pooled", "running_mean", "running_var", "ds"} | {GRADS[i] for i in pick}
        for name in part:
            _same_bits(part[name], full[name], f"gradients {pick} alone: {name}")


def test_plane_means_alone_still_backpropagate():
    """a loss that never touches the gate's output: the BatchNorm's backward runs without a parked gate gradient"""
    from moma_amd import ops
    D, gamma, beta, rm, rv, M, dG = _operands((2, 4, 14, 14), torch.float32)
    dpl = torch.randn(2, 4, 1, 1, device="cuda")
    a = [t.clone().requires_grad_(True) for t in (D, gamma, beta)]
    b = [t.clone().requires_grad_(True) for t in (D, gamma, beta)]
    pooled, _ = ops.bn_act_mean(*a, rm.clone(), rv.clone(), True, MOM, EPS, "silu")
    _, pooled0 = ops.bn_act(*b, rm.clone(), rv.clone(), True, MOM, EPS, "silu", want_mean=True)
    for g1, g0 in zip(torch.autograd.grad(pooled, a, dpl), torch.autograd.grad(pooled0, b, dpl)):
        _same_bits(g1, g0, "gradient through the plane means alone")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 9, 9), (2, 4, 14, 14), (8, 2, 56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_gradient_of_the_plane_means_at_full_scale(shape, dtype):
    """The small map above keeps the gradient of the plane means small next to dG.  Here the plane means ALSO enter the loss
    directly, with a cotangent of three times a unit normal handed over exactly -- the operands of test_bn_act_with_plane_mean,
    whose tolerances these are -- so the P2 / P4 terms of the channel sums and dpooled / HW in the apply pass carry full weight."""
    from moma_amd import ops
    D, gamma, beta, rm, rv, M, dG = _operands(shape, dtype)
    rng = np.random.default_rng(7 + sum(shape))
    dmean = (_rand(rng, shape[0], shape[1], 1, 1) * 3.0).to(dtype)
    leaves = [t.clone().requires_grad_(True) for t in (D, gamma, beta)]
    G, pooled, _ = _chain(True, ops, *leaves, rm.clone(), rv.clone(), M.double(), True, "silu")
    got = torch.autograd.grad([G, pooled], leaves, [dG, dmean])
    ref_leaves = [t.double().requires_grad_(True) for t in (D, gamma, beta)]
    Gr, pr, _ = bnse_ref.composite(*ref_leaves, rm.double(), rv.double(), M.double(), True, "silu", EPS)
    want = torch.autograd.grad([Gr, pr], ref_leaves, [dG.double(), dmean.double()])
    for name, g, r in zip(GRADS, got, want):
        rtol, atol = _tolerances(name, r, shape, dtype)
        print(f"{name}: {(g.double() - r).abs().max().item():.3e} (max |ref| {r.abs().max().item():.3e}, atol {atol:.3e})")
        torch.testing.assert_close(g.double(), r, rtol=rtol, atol=atol, msg=lambda m, n=name: f"{n}: {m}")


def test_nothing_stays_parked_when_the_batchnorm_node_never_runs():
    """a gradient asked of the logits alone, with D requiring one: the gate's backward parks dG for a node this pass never reaches"""
    from moma_amd import ops
    D, gamma, beta, rm, rv, M, dG = _operands((3, 5, 9, 9), torch.bfloat16)
    leaves = [t.clone().requires_grad_(True) for t in (D, gamma, beta)]
    pooled, link = ops.bn_act_mean(*leaves, rm.clone(), rv.clone(), True, MOM, EPS, "silu")
    s = bnse_ref.smap(pooled.double(), M.double()).to(D.dtype)
    G = ops.bn_act_gate(leaves[0], link, s)
    (ds,) = torch.autograd.grad(G, [s], dG, retain_graph=True)
    assert link._moma_bnse.pending is None
    full = torch.autograd.grad(G, leaves + [s], dG)                # the whole backward still works afterwards, same ds
    _same_bits(full[-1], ds, "ds")
    assert link._moma_bnse.pending is None and all(torch.isfinite(g.float()).all() for g in full)


@pytest.mark.parametrize("shape,dtype", [((3, 5, 9, 9), torch.float32), ((3, 5, 9, 9), torch.bfloat16), ((9, 3, 7, 7), torch.bfloat16),
                                         ((70, 3, 4, 4), torch.float32)],
                         ids=["3x5x9x9-fp32", "3x5x9x9-bf16", "9x3x7x7-bf16", "70x3x4x4-fp32"])
def test_entry_points_between_guards(guard, shape, dtype, monkeypatch):
    """operands between NaN guards, outputs / workspaces / saved tensors between canaries (tests/test_gpu_guard.py)"""
    from moma_amd import ops
    D, gamma, beta, rm, rv, M, dG = _operands(shape, dtype)
    with monkeypatch.context() as m:
        m.setattr(ops, "torch", torch)                          # the same calls on ordinary allocations
        want = _run(True, ops, D, gamma, beta, rm, rv, M, dG, True, "silu")
    gD, gg, gb = (_in(guard, t).requires_grad_(True) for t in (D, gamma, beta))
    gM = M.double().requires_grad_(True)
    grm, grv, gdG = _in(guard, rm), _in(guard, rv), _in(guard, dG)
    G, pooled, s = _chain(True, ops, gD, gg, gb, grm, grv, gM, True, "silu")
    assert guard.check(f"fused forward {shape}") >= 6 + 6       # the operands + statistics (2), scale / shift, pooled, workspace, G
    grads = torch.autograd.grad(G, [gD, gg, gb, gM, s], gdG)
    assert guard.check(f"fused backward {shape}") >= 5          # ds, the plane-sum workspace, dD, dgamma, dbeta
    got = dict(zip(GRADS, grads), G=G.detach(), pooled=pooled.detach(), running_mean=grm, running_var=grv)
    for name in got:
        _same_bits(got[name], want[name], f"guarded {name}")


# ---- the block and the model ------------------------------------------------------------------------------------
def _calls(monkeypatch):
    """count the fused op's calls (the comparison must not compare the unfused path with itself)"""
    from moma_amd import ops
    n = [0]
    real = ops.bn_act_gate

    def counted(*a, **k):
        n[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "bn_act_gate", counted)
    return n


def _forward(module, x, fuse, train, amp, grad, monkeypatch, **kw):
    import copy
    from moma_amd.backbones import efficientnet as E
    m = copy.deepcopy(module).train(train)
    monkeypatch.setattr(E, "_SE_FUSE", "all" if fuse else "0")       # ("1", the default: test_default_follows_...)
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


def _compare(a, b, amp, what):
    """forward outputs and BN buffers bit for bit; gradients within the bounds of tests/effnet_stock_compare.py"""
    (o1, sd1, g1), (o0, sd0, g0) = a, b
    assert len(o1) == len(o0)
    for i, (p, q) in enumerate(zip(o1, o0)):
        _same_bits(p, q, f"{what}: output {i}")
    assert sd1.keys() == sd0.keys()
    for k in sd1:
        assert torch.equal(sd1[k], sd0[k]), (what, k)           # BN buffers, num_batches_tracked included
    assert g1.keys() == g0.keys()
    if not g0:
        return
    gmax = max(g.abs().max().item() for g in g0.values() if g is not None)
    for k in g0:
        assert (g1[k] is None) == (g0[k] is None), k
        if g0[k] is not None:
            e = ((g1[k] - g0[k]).abs().max() / g0[k].abs().max().clamp_min((3e-2 if amp else 1e-4) * gmax)).item()
            assert e < (0.6 if amp else 2e-2), (what, k, e)


@pytest.mark.parametrize("amp", [True, False], ids=["bf16-autocast", "fp32"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("stride,cout", [(1, 8), (2, 12)], ids=["stride1-skip", "stride2"])
def test_block_is_unchanged_by_the_fusion(stride, cout, train, amp, monkeypatch):
    from moma_amd.backbones.efficientnet import MBConvBlock
    torch.manual_seed(0)
    blk = MBConvBlock(5, stride, 6, 8, cout, 0.25).cuda()
    _randomise_bn(blk, 1)
    x = torch.randn(4, 8, 18, 18, device="cuda")
    n = _calls(monkeypatch)
    for grad in (False, True):
        before = n[0]
        fused = _forward(blk, x, True, train, amp, grad, monkeypatch)
        assert n[0] == before + 1
        plain = _forward(blk, x, False, train, amp, grad, monkeypatch)
        assert n[0] == before + 1
        _compare(fused, plain, amp, f"block grad={grad}")


@pytest.mark.parametrize("amp", [True, False], ids=["bf16-autocast", "fp32"])
@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "grad"])
def test_model_is_unchanged_by_the_fusion(grad, amp, monkeypatch):
    from moma_amd.backbones.efficientnet import efficientnet_b0
    torch.manual_seed(0)
    model = efficientnet_b0(num_classes=5).cuda()
    _randomise_bn(model, 2)
    x = torch.randn(2, 3, 64, 64, device="cuda")
    n = _calls(monkeypatch)
    fused = _forward(model, x, True, True, amp, grad, monkeypatch, is_feat=True)
    assert n[0] == 16                                           # every block
    plain = _forward(model, x, False, True, amp, grad, monkeypatch, is_feat=True)
    assert n[0] == 16
    _compare(fused, plain, amp, f"model grad={grad}")


def test_nograd_mode_fuses_only_where_no_gradient_is_recorded(monkeypatch):
    from moma_amd.backbones import efficientnet as E
    monkeypatch.setattr(E, "_SE_FUSE", "nograd")
    torch.manual_seed(0)
    blk = E.MBConvBlock(3, 1, 6, 4, 4, 0.25).cuda()
    x = torch.randn(2, 4, 56, 56, device="cuda")
    n = _calls(monkeypatch)
    with torch.no_grad():
        blk(x)
    assert n[0] == 1
    blk(x).sum().backward()
    assert n[0] == 1 and blk._bn1.weight.grad is not None
    monkeypatch.setattr(E, "_SE_FUSE", "1")
    blk(x).sum().backward()
    assert n[0] == 2


def test_default_follows_the_layer_table(monkeypatch):
    """MOMA_SEFUSE=1: planes of 56 x 56 and up everywhere, 28 x 28 and up where a gradient is recorded, the two calls below"""
    from moma_amd import ops
    from moma_amd.backbones import efficientnet as E
    assert ops.bn_se_native(56 * 56, False) and ops.bn_se_native(112 * 112, True) and ops.bn_se_native(28 * 28, True)
    assert not ops.bn_se_native(28 * 28, False) and not ops.bn_se_native(14 * 14, True) and not ops.bn_se_native(7 * 7, False)
    monkeypatch.setattr(E, "_SE_FUSE", "1")
    torch.manual_seed(0)
    blk = E.MBConvBlock(3, 1, 6, 4, 4, 0.25).cuda()
    n = _calls(monkeypatch)
    for side, nograd, grad in ((56, 1, 1), (28, 0, 1), (14, 0, 0)):
        x = torch.randn(2, 4, side, side, device="cuda")
        before = n[0]
        with torch.no_grad():
            blk(x)
        assert n[0] == before + nograd, side
        blk(x).sum().backward()
        assert n[0] == before + nograd + grad, side

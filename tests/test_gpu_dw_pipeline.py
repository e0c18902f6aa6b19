"""The depthwise kernels when one wave walks over MANY work items (planes x bands), as it does once the launch is sized to the
resident waves and an item's loads are issued while the item before it is computed: an item fetched but never or wrongly
committed, a fetch past the last item, a ragged last group of planes, a short last band, and the vector-width fall-backs of the
contiguous-span fill.  The shapes of the other suites give every wave one item at most and cannot see any of these, so N * C
is chosen here such that the item count exceeds 3 * 16384 (the most waves any launch of these kernels ever had) and is not a
multiple of 4 (the waves of a workgroup) nor N * C of the planes per item.

1. exact arithmetic: small integers in x, dy and w make every partial sum an integer below 2^24, so y, dx and dw cannot depend
   on the order of the sums and must EQUAL a reference built from shifted, strided slices of the zero-padded input in plain
   fp32 torch ops (no library convolution: its algorithm need not be exact);
2. independence of the batch: on random data the call on the whole tensor equals, bit for bit, the calls on consecutive chunks
   of it that give every wave one item at most -- also from a base pointer that is offset by one element, where the 16-byte
   loads fall back;
3. the fused BN + activation prologue equals the two calls bit for bit at the multi-item shapes;
4. operands between NaN guards and results between canaries at ragged shapes (tests/test_gpu_guard.py).
"""
import functools
import math

import pytest
import torch

from tests.test_gpu_guard import _Guarded, guard, _in  # noqa: F401  (`guard` is a fixture)

pytestmark = pytest.mark.gpu

# name: (N, C, H, K, S); the item counts are checked on the CPU by test_the_shapes_have_more_items_than_waves
#   planes per item / bands per plane of the forward launch as planned by moma_amd/csrc/dwconv.hip
SHAPES = {
    "7x7_k5_s1": (28087, 14, 7, 5, 1),        # small planes, 8 planes per item: 393218 planes, 49153 items
    "14x14_k3_s1": (19661, 10, 14, 3, 1),     # small planes, 4 per item: 196610 planes, 49153 items
    "14x14_k5_s1": (19661, 10, 14, 5, 1),
    "28x28_k5_s1": (2979, 33, 28, 5, 1),      # strips, 2 per item: 98307 planes, 49154 items
    "14x14_k5_s2": (19661, 10, 14, 5, 2),     # strips on a 7 x 7 result, 4 per item
    "57x57_k3_s2": (3511, 7, 57, 3, 2),       # 2 bands per plane, odd width (element fills): 24577 planes, 49154 items
    "112x112_k3_s2": (2341, 3, 112, 3, 2),    # 7 bands per plane: 7023 planes, 49161 items
}
ITEMS = {"7x7_k5_s1": (8, 1), "14x14_k3_s1": (4, 1), "14x14_k5_s1": (4, 1), "28x28_k5_s1": (2, 1), "14x14_k5_s2": (4, 1),
         "57x57_k3_s2": (1, 2), "112x112_k3_s2": (1, 7)}
MOST_WAVES = 16384
DTYPES = [torch.bfloat16, torch.float32]


def _geom(H, K, S):
    OH = math.ceil(H / S)
    total = max((OH - 1) * S + K - H, 0)
    return OH, total // 2, total                                   # result size, top / left padding, rows / columns added in all


def test_the_shapes_have_more_items_than_waves():
    for name, (N, C, H, K, S) in SHAPES.items():
        pb, nbands = ITEMS[name]
        items = -(-(N * C) // pb) * nbands
        assert items > 3 * MOST_WAVES and items % 4 != 0 and (N * C) % 4 != 0 and (pb == 1 or (N * C) % pb != 0), (name, items)


def _ints(shape, lo, hi, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g).to(dtype)


def _pad(x, H, K, S):
    OH, p, total = _geom(H, K, S)
    return torch.nn.functional.pad(x.float(), (p, total - p, p, total - p))


def _ref_fwd(x, w, H, K, S):
    """sum_{ky,kx} w[c,ky,kx] * xpad[..., ky::S, kx::S] in fp32"""
    OH = _geom(H, K, S)[0]
    xp = _pad(x, H, K, S)
    y = torch.zeros(x.shape[0], x.shape[1], OH, OH, device=x.device)
    for ky in range(K):
        for kx in range(K):
            y += w[:, 0, ky, kx].view(1, -1, 1, 1) * xp[..., ky:ky + (OH - 1) * S + 1:S, kx:kx + (OH - 1) * S + 1:S]
    return y


def _ref_dx(dy, w, H, K, S):
    OH, p, total = _geom(H, K, S)
    dxp = torch.zeros(dy.shape[0], dy.shape[1], H + total, H + total, device=dy.device)
    g = dy.float()
    for ky in range(K):
        for kx in range(K):
            dxp[..., ky:ky + (OH - 1) * S + 1:S, kx:kx + (OH - 1) * S + 1:S] += w[:, 0, ky, kx].view(1, -1, 1, 1) * g
    return dxp[..., p:p + H, p:p + H]


def _ref_dw(x, dy, H, K, S):
    OH = _geom(H, K, S)[0]
    xp = _pad(x, H, K, S)
    g = dy.float()
    dw = torch.empty(x.shape[1], 1, K, K, device=x.device)
    for ky in range(K):
        for kx in range(K):
            dw[:, 0, ky, kx] = (g * xp[..., ky:ky + (OH - 1) * S + 1:S, kx:kx + (OH - 1) * S + 1:S]).sum(dim=(0, 2, 3))
    return dw


@functools.lru_cache(maxsize=1)
def _exact_case(name):
    """integer operands and the fp32 references, shared by both storage types (small integers are exact in bf16)"""
    N, C, H, K, S = SHAPES[name]
    OH = _geom(H, K, S)[0]
    x = _ints((N, C, H, H), -4, 4, torch.float32, 1)
    dy = _ints((N, C, OH, OH), -4, 4, torch.float32, 2)
    w = _ints((C, 1, K, K), -2, 2, torch.float32, 3)
    # dw: narrower values, so that N * OH * OW * max|x| * max|dy| stays below 2^24
    x2, dy2 = x.clamp(-2, 2), dy.sign()
    assert N * OH * OH * 2 * 1 < 2 ** 24, name
    assert K * K * 4 * 2 <= 200
    return x, dy, w, _ref_fwd(x, w, H, K, S), _ref_dx(dy, w, H, K, S), x2, dy2, _ref_dw(x2, dy2, H, K, S)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_arithmetic(name, dtype):
    from moma_amd import ops
    N, C, H, K, S = SHAPES[name]
    OH, p, _ = _geom(H, K, S)
    x, dy, w, y_ref, dx_ref, x2, dy2, dw_ref = _exact_case(name)
    xt = x.to(dtype).requires_grad_(True)
    y = ops.dwconv(xt, w, S, p, p, OH, OH)
    assert y.dtype == dtype and torch.equal(y.float(), y_ref), f"{name}: y differs in {int((y.float() != y_ref).sum())} elements"
    dx, = torch.autograd.grad(y, xt, dy.to(dtype))
    assert torch.equal(dx.float(), dx_ref), f"{name}: dx differs in {int((dx.float() != dx_ref).sum())} elements"
    del y, dx
    wt = w.clone().requires_grad_(True)
    y2 = ops.dwconv(x2.to(dtype), wt, S, p, p, OH, OH)
    dw, = torch.autograd.grad(y2, wt, dy2.to(dtype))
    assert torch.equal(dw, dw_ref), f"{name}: dw differs by up to {float((dw - dw_ref).abs().max())}"


def _bn_params(C):
    g = torch.Generator(device="cuda").manual_seed(7)
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g) * 0.3
    rm = torch.randn(C, device="cuda", generator=g) * 0.2
    rv = torch.rand(C, device="cuda", generator=g) + 0.5
    return gamma, beta, rm, rv


@functools.lru_cache(maxsize=1)
def _random_case(name, dtype):
    N, C, H, K, S = SHAPES[name]
    OH = _geom(H, K, S)[0]
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(N, C, H, H, device="cuda", generator=g).to(dtype)
    dy = torch.randn(N, C, OH, OH, device="cuda", generator=g).to(dtype)
    w = torch.randn(C, 1, K, K, device="cuda", generator=g) * 0.3
    return x, dy, w


def _three(x, dy, w, K, S, H, bn):
    """forward, dx and the prologue form (running statistics: the same scale / shift whatever the batch) of one call"""
    from moma_amd import ops
    OH, p, _ = _geom(H, K, S)
    xt = x.detach().requires_grad_(True)
    y = ops.dwconv(xt, w, S, p, p, OH, OH)
    dx, = torch.autograd.grad(y, xt, dy)
    gamma, beta, rm, rv = bn
    with torch.no_grad():
        f = ops.bn_act_dwconv(x, gamma, beta, rm.clone(), rv.clone(), False, 0.01, 1e-3, "silu", w, S, p, p, OH, OH)
    return y.detach(), dx, f


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_whole_batch_equals_its_chunks(name, dtype):
    N, C, H, K, S = SHAPES[name]
    pb, nbands = ITEMS[name]
    x, dy, w = _random_case(name, dtype)
    bn = _bn_params(C)
    whole = _three(x, dy, w, K, S, H, bn)
    # chunks of at most 1024 items: fewer than the waves of any launch, every wave has one item or none
    n = max(1, (1024 * pb // nbands) // C)
    parts = [_three(x[i:i + n], dy[i:i + n], w, K, S, H, bn) for i in range(0, N, n)]
    for k, what in enumerate(("y", "dx", "fused y")):
        assert torch.equal(whole[k], torch.cat([q[k] for q in parts])), f"{name}: {what} of the whole batch differs from its chunks"
    # the same operands 1, 2 and 4 elements off their allocation's start: the span fill of the small planes falls back to
    # element loads (2 bytes off), to 4-byte vectors and to 8-byte vectors, each with several items per wave
    def shifted(t, k):
        buf = torch.empty(t.numel() + k, device="cuda", dtype=t.dtype)
        buf[k:].copy_(t.reshape(-1))
        return buf[k:].view(t.shape)
    for off in ((1, 2, 4) if dtype == torch.bfloat16 else (1, 2)):
        assert x.data_ptr() % 16 == 0 and shifted(x, off).data_ptr() % 16 == off * x.element_size()
        got = _three(shifted(x, off), shifted(dy, off), w, K, S, H, bn)
        for k, what in enumerate(("y", "dx", "fused y")):
            assert torch.equal(whole[k], got[k]), f"{name}: {what} changes with the operands {off} elements off a 16-byte boundary"


@pytest.mark.parametrize("training", [True, False], ids=["batch_stats", "running_stats"])
@pytest.mark.parametrize("name", ["7x7_k5_s1", "14x14_k3_s1", "14x14_k5_s1", "28x28_k5_s1"])
def test_fused_equals_the_two_calls(name, training):
    from moma_amd import ops
    N, C, H, K, S = SHAPES[name]
    OH, p, _ = _geom(H, K, S)
    x, dy, w = _random_case(name, torch.bfloat16)
    gamma, beta, rm, rv = _bn_params(C)
    with torch.no_grad():
        rm1, rv1, rm2, rv2 = rm.clone(), rv.clone(), rm.clone(), rv.clone()
        two = ops.dwconv(ops.bn_act(x, gamma, beta, rm1, rv1, training, 0.01, 1e-3, "silu"), w, S, p, p, OH, OH)
        one = ops.bn_act_dwconv(x, gamma, beta, rm2, rv2, training, 0.01, 1e-3, "silu", w, S, p, p, OH, OH)
    assert torch.equal(one, two), f"{name}: {int((one != two).sum())} elements differ"
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2)


# ragged: odd planes, stride 2, k = 5, N * C no multiple of the planes per item.  The first two are the small-plane kernel with
# 4127 items (33011 planes by 8, 16505 by 4) for the 4096 waves it launches at most, and at least as many channels as planes per
# item: waves fetch a second item ahead, and the last group is short
GUARDED = [(3001, 11, 7, 5, 1), (3301, 5, 14, 5, 1), (3, 5, 14, 3, 1), (7, 3, 15, 5, 2), (5, 3, 29, 3, 2), (3, 7, 28, 5, 1),
           (2, 3, 57, 5, 2), (1, 3, 113, 3, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", GUARDED, ids=lambda s: "x".join(map(str, s)))
def test_operands_between_guards(guard, shape, dtype):
    from moma_amd import ops
    N, C, H, K, S = shape
    OH, p, _ = _geom(H, K, S)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, C, H, H, device="cuda", generator=g).to(dtype)
    dy = torch.randn(N, C, OH, OH, device="cuda", generator=g).to(dtype)
    w = torch.randn(C, 1, K, K, device="cuda", generator=g) * 0.3

    def run(x_, dy_, w_):
        x_ = x_.requires_grad_(True)
        w_ = w_.requires_grad_(True)
        y = ops.dwconv(x_, w_, S, p, p, OH, OH)
        dx, dw = torch.autograd.grad(y, [x_, w_], dy_)
        return y.detach(), dx, dw

    plain = run(x.clone(), dy, w.clone())
    guard.records.clear()                                        # (the plain call's buffers were carved too; only the next call counts)
    got = run(_in(guard, x), _in(guard, dy), _in(guard, w))
    assert guard.check(f"dwconv {shape}") >= 3 + 4              # the operands + y, dx, dw and the workspace
    for a, b, what in zip(got, plain, ("y", "dx", "dw")):
        assert not torch.isnan(a.float()).any(), f"{shape}: NaN in {what}: a read outside an operand"
        assert torch.equal(a, b), f"{shape}: guarded {what} differs"

"""GPU tests of the classification-head kernels (csrc/ce.hip) through the C ABI, ops.ce_head, helper.ce_head.CrossEntropyHead and one
step of train_vanilla.

Yardstick: the float64 evaluation of the formulas (tests/ce_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_loss / _dz`) that the reference's own fp32 results keep from float64 over the cases of the golden
fixture, never below one fp32 ulp (2^-23, relative).  Metric: the loss relative to its own value, dz in crd_ref.rel's units (the
yardstick's largest element).  A dz stored in bf16 adds that rounding: at most 2^-8 of the element.  lse and 1 / n_valid are doubles
computed in double: compared at 1e-12.  pred, hits, counts and conf are compared exactly (every row's maximum is unique by
construction).
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from moma_amd.helper.ce_head import CrossEntropyHead
from tests import ce_fixture, ce_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8
N_CASES = ce_fixture.N_CASES
USED = {}                                                                     # kind -> the largest share of its allowance any check used
STATS0 = (10.0, 20.0, 30.0, 40.0)                                             # what stats holds before a call: the call ADDS
CONF0 = 7                                                                     # likewise every cell of conf


def _lib():
    from moma_amd import _lib as L
    return L.load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(name, got, allowed, kind=None):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e}, ratio {got / allowed:.2f})")
    if kind is not None:
        USED[kind] = max(USED.get(kind, 0.0), got / allowed)
    return got <= allowed


def _code(dtype):
    from moma_amd import _lib as L
    return L.DT_BF16 if dtype == BF16 else L.DT_F32


def _carve(guard, shape, dtype, offset):
    """an uninitialised dense [B, K] device tensor between NaN margins, optionally starting one element behind an aligned address"""
    flat = guard.empty(shape[0] * shape[1] + int(offset), device="cuda", dtype=dtype)
    return (flat[1:] if offset else flat).view(*shape)


def _draw(B, K, seed, scale=1.0):
    """the fixture's recipe: normal draws on the 1/32 grid clipped to 4 (exact in bf16), each row's first maximum raised by 1/8; labels:
    the argmax on the even rows, a uniform draw on the odd ones"""
    rng = np.random.default_rng(seed)
    z = np.clip(np.round(rng.standard_normal((B, K)) * 32) / 32, -4, 4).astype(np.float32)
    top = z.argmax(axis=1)
    z[np.arange(B), top] += np.float32(V.MARGIN)
    z *= np.float32(scale)
    y = rng.integers(0, K, B).astype(np.int64)
    y[::2] = top[::2]
    assert V.margin(z) >= V.MARGIN * scale
    return z, y


def run_abi(z, y, dtype=F32, off=False, g_loss=1.0, extras=True, bwd=True):
    """moma_ce_fwd -> moma_ce_bwd on fresh guarded buffers; numpy inputs.  extras: with pred, stats and conf (else NULL)
    -> dict of numpy arrays and the raw device tensors under `raw`"""
    lib, guard = _lib(), _Guarded()
    B, K = z.shape
    tz = _carve(guard, z.shape, dtype, off)
    src = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(dtype)
    assert np.array_equal(src.float().numpy(), z)                            # (the inputs are exact in the storage type)
    tz.copy_(src)
    ty = guard.empty(B, device="cuda", dtype=I64)
    ty.copy_(torch.from_numpy(y))
    nws = lib.moma_ce_workspace_bytes(B, K)
    assert nws > 0
    ws = guard.empty((nws + 7) // 8, device="cuda", dtype=F64)
    loss, lse, inv_n = guard.empty(1, device="cuda", dtype=F32), guard.empty(B, device="cuda", dtype=F64), guard.empty(1, device="cuda", dtype=F64)
    pred = stats = conf = None
    if extras:
        pred = guard.empty(B, device="cuda", dtype=torch.int32)
        stats = guard.empty(4, device="cuda", dtype=F64)
        stats.copy_(torch.tensor(STATS0, dtype=F64))
        conf = guard.empty(K, K, device="cuda", dtype=I64)
        conf.fill_(CONF0)
    rc = lib.moma_ce_fwd(_p(tz), _p(ty), B, K, _code(dtype), _p(ws), ((nws + 7) // 8) * 8, _p(loss), _p(lse), _p(inv_n), _p(pred),
                         _p(stats), _p(conf), _st())
    assert rc == 0, rc
    raw = {"loss": loss, "lse": lse, "inv_n": inv_n}
    if extras:
        raw.update(pred=pred, stats=stats, conf=conf)
    if bwd:
        gl = torch.full((1,), float(g_loss), device="cuda")
        dz = _carve(guard, z.shape, dtype, off)
        rc = lib.moma_ce_bwd(_p(tz), _p(ty), _p(lse), _p(inv_n), _p(gl), _p(dz), B, K, _code(dtype), _st())
        assert rc == 0, rc
        raw["dz"] = dz
    assert guard.check("ce C ABI") > 0                                        # every margin untouched
    out = {k: (v.float() if v.dtype == BF16 else v).cpu().numpy() for k, v in raw.items()}
    out["loss"] = float(out["loss"][0])
    out["raw"] = raw
    return out


def check(tag, got, want, allow, g_loss=1.0, bf16_out=False):
    """want: V.ce at g_loss = 1"""
    if np.isnan(want["loss"]):
        ok = np.isnan(got["loss"])
    else:
        ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / max(abs(want["loss"]), 1e-300), allow["loss"], "loss")
    assert np.abs(got["lse"] - want["lse"]).max() <= 1e-12 * max(1.0, np.abs(want["lse"]).max()), tag
    if want["n_valid"]:
        assert got["inv_n"][0] == 1.0 / want["n_valid"], tag
    if "dz" in got:
        w = g_loss * want["dz"]
        err = np.abs(got["dz"].astype(np.float64) - w)
        if bf16_out:
            err = np.maximum(err - HALF_ULP_BF16 * np.abs(w), 0)              # the rounding of the stored gradient
        ok &= _report(f"{tag} dz", float(err.max() / max(np.abs(w).max(), 1e-300)), allow["dz"], "dz")
        assert not got["dz"][want["_valid_labels"] < 0].any(), tag             # rows that are not valid: exact zeros
    if "pred" in got:
        assert np.array_equal(got["pred"], want["pred"]), tag
        s = got["stats"] - np.asarray(STATS0)
        assert s[1] == want["hits"] and s[2] == want["n_valid"] and s[3] == want["n_bad"], (tag, s)
        assert abs(s[0] - want["sum"]) <= 1e-12 * max(1.0, abs(want["sum"])), (tag, s[0], want["sum"])
        assert np.array_equal(got["conf"] - CONF0, want["conf"]), tag
    return ok


def _want(z, y):
    """V.ce with `_valid_labels` [B]: the label where the row is valid, -1 elsewhere"""
    w = V.ce(z, y)
    K = z.shape[1]
    w["_valid_labels"] = np.where((y >= 0) & (y < K), y, -1)
    return w


def teardown_module(_m):
    print("largest share of an allowance used, per kind:", {k: round(v, 3) for k, v in sorted(USED.items())})


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """every fixture case against float64, through the C ABI in both dtypes, with and without a one-element offset of the base address,
    with and without pred / stats / conf, and through the op and the module; the inputs are exact in bf16, so one yardstick serves both"""
    from moma_amd import ops
    cases, allow = ce_fixture.load()
    c = cases[ci]
    z, y = c["logits"], c["labels"]
    want = _want(z, y)
    print(f"case {ci} B {c['B']} K {c['K']}")
    ok = True
    for dtype in (F32, BF16):
        for off in (False, True):
            got = run_abi(z, y, dtype, off, g_loss=3.0)
            assert got["raw"]["dz"].dtype == dtype
            ok &= check(f"abi {dtype} off {int(off)}", got, want, allow, g_loss=3.0, bf16_out=dtype == BF16)
            bare = run_abi(z, y, dtype, off, g_loss=3.0, extras=False)
            assert all(torch.equal(bare["raw"][k], got["raw"][k]) for k in ("loss", "lse", "inv_n", "dz"))      # the extras change nothing
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    got = run_abi(z, y)
    ok &= _report("loss vs reference", abs(got["loss"] - c["loss"]) / max(abs(c["loss"]), 1e-300), allow["loss"] + c["ref_vs_f64_loss"])
    ok &= _report("dz vs reference", rel(got["dz"], c["dz"]), allow["dz"] + c["ref_vs_f64_dz"])
    assert np.array_equal(got["conf"] - CONF0, c["conf"]) and abs(100.0 * (got["stats"][1] - STATS0[1]) / c["B"] - c["acc"]) < 1e-4
    # the op: the same bits as the C ABI, and the composite within the allowance
    for dtype in (F32, BF16):
        tz = torch.from_numpy(z).to(dtype).cuda().requires_grad_(True)
        ty = torch.from_numpy(y).cuda()
        head = CrossEntropyHead(c["K"], meter=True).cuda()                          # (its buffers; the module's routing is tested below)
        loss = ops.ce_head(tz, ty, head.stats, head.conf)
        assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
        (loss * 3.0).backward()
        ref = run_abi(z, y, dtype, g_loss=3.0)
        assert torch.equal(loss.detach().reshape(1), ref["raw"]["loss"]) and torch.equal(tz.grad, ref["raw"]["dz"]) and tz.grad.dtype == dtype
        assert torch.equal(head.stats[1:], (ref["raw"]["stats"] - torch.tensor(STATS0, dtype=F64, device="cuda"))[1:])
        assert abs(float(head.stats[0]) - want["sum"]) <= 1e-12 * max(1.0, abs(want["sum"]))
        assert torch.equal(head.conf, ref["raw"]["conf"] - CONF0)
        assert torch.equal(ops.ce_head(tz.detach(), ty), loss.detach())
        comp = CrossEntropyHead(c["K"], meter=True).cuda()
        tc = torch.from_numpy(z).to(dtype).cuda().requires_grad_(True)
        closs = comp.composite(tc, ty, comp.stats, comp.conf)
        (closs * 3.0).backward()
        ok &= _report(f"{dtype} loss vs the composite", abs(float(loss) - float(closs)) / max(abs(float(closs)), 1e-300),
                      allow["loss"] + ULP32 / 2)
        err = np.abs(tz.grad.double().cpu().numpy() - tc.grad.double().cpu().numpy())
        if dtype == BF16:
            err = np.maximum(err - 2 * HALF_ULP_BF16 * np.abs(3.0 * want["dz"]), 0)          # (both sides store bf16)
        ok &= _report(f"{dtype} dz vs the composite", float(err.max() / max(np.abs(3.0 * want["dz"]).max(), 1e-300)), allow["dz"] + ULP32 / 2)
        assert torch.equal(head.conf, comp.conf) and torch.equal(head.stats[1:], comp.stats[1:])
        assert abs(float(head.stats[0]) - float(comp.stats[0])) <= 1e-12 * max(1.0, abs(float(comp.stats[0])))
    assert ok


EDGES = [  # (B, K): sizes at which the kernels take another path
    (300, 4),       # one lane per row, 256 rows per workgroup: a second workgroup; two rows per thread of the finalize
    (5, 16),        # the longest row of one lane
    (5, 17),        # two lanes per row, the second with one element
    (70, 40),       # four lanes per row, 64 rows per workgroup: a second workgroup
    (9, 512),       # 32 lanes: the shuffles stay inside half a wave
    (9, 513),       # 64 lanes, the last ones idle
    (6, 1032),      # two walks, 16-byte accesses in bf16 and fp32, one more trip for the first lanes
    (600, 3),       # element accesses, three workgroups, three rows per thread of the finalize
]


@pytest.mark.parametrize("ei", range(len(EDGES)))
def test_edges_against_the_restatement(ei):
    _cases, allow = ce_fixture.load()
    B, K = EDGES[ei]
    z, y = _draw(B, K, 500 + ei)
    y[1::7] = V.IGNORE
    want = _want(z, y)
    ok = True
    for dtype in (F32, BF16):
        got = run_abi(z, y, dtype, off=bool(ei % 2), g_loss=0.5)
        ok &= check(f"{EDGES[ei]} {dtype}", got, want, allow, g_loss=0.5, bf16_out=dtype == BF16)
    assert ok


def test_stats_and_conf_accumulate_over_two_calls():
    z1, y1 = _draw(33, 9, 1)
    z2, y2 = _draw(20, 9, 2)
    y2[3] = V.IGNORE
    w1, w2 = V.ce(z1, y1), V.ce(z2, y2)
    from moma_amd import ops
    for dtype in (F32, BF16):
        head = CrossEntropyHead(9, meter=True).cuda()
        ops.ce_head(torch.from_numpy(z1).to(dtype).cuda(), torch.from_numpy(y1).cuda(), head.stats, head.conf)
        head(torch.from_numpy(z2).to(dtype).cuda(), torch.from_numpy(y2).cuda())      # (the module: kernels for bf16, the composite for fp32)
        acc, mean, conf = head.read()
        s = head.stats.tolist()
        assert s[1:] == [w1["hits"] + w2["hits"], 52.0, 0.0] and np.array_equal(conf, w1["conf"] + w2["conf"])
        assert abs(s[0] - (w1["sum"] + w2["sum"])) <= 1e-12 * s[0] and acc == 100.0 * s[1] / 52 and mean == s[0] / 52
        head.reset()
        assert not head.stats.any() and not head.conf.any()


def test_one_class_gives_exact_zeros():
    z = np.array([[1.5], [-3.0], [0.0], [4.125], [-0.03125]], np.float32)
    y = np.zeros(5, np.int64)
    for dtype in (F32, BF16):
        got = run_abi(z, y, dtype, g_loss=5.0)
        assert got["loss"] == 0.0 and not got["dz"].any()
        assert np.array_equal(got["lse"], z[:, 0].astype(np.float64)) and not got["pred"].any()
        assert got["stats"][0] == STATS0[0] and got["stats"][1] == STATS0[1] + 5 and got["conf"][0, 0] == CONF0 + 5


def test_two_calls_give_the_same_bits():
    for (B, K, dtype) in [(64, 4, F32), (37, 100, BF16), (8, 1000, F32), (5, 2500, BF16)]:
        z, y = _draw(B, K, B + K)
        a, b = (run_abi(z, y, dtype, g_loss=2.0) for _ in range(2))
        for k in a["raw"]:
            assert torch.equal(a["raw"][k], b["raw"][k]), ((B, K), k)


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.ce_head with every buffer it allocates (workspace + lse + 1 / n_valid, the loss, dz) between NaN margins, at ragged shapes
    and both dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (B, K, dtype) in [(3, 5, F32), (65, 4, BF16), (7, 100, BF16), (5, 1025, F32), (300, 9, F32)]:
        z, y = _draw(B, K, 7 * B + K)
        tz, ty = torch.from_numpy(z).to(dtype).cuda(), torch.from_numpy(y).cuda()

        def run(wrap):
            xx = wrap(tz).requires_grad_(True)
            stats, conf = wrap(torch.zeros(4, dtype=F64, device="cuda")), wrap(torch.zeros(K, K, dtype=I64, device="cuda"))
            loss = ops.ce_head(xx, wrap(ty), stats, conf)
            (loss * 2.5).backward()
            return [loss.detach().clone(), xx.grad.clone(), stats.clone(), conf.clone()]

        plain = run(lambda t: t.clone())
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda t: _in(guard, t))
            assert guard.check(f"ce_head {(B, K)}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_upstream_gradient_scales_exactly():
    """g_loss is a device scalar folded in before the one rounding: 2^k against 1 scales every bit pattern of dz exactly, 0 gives exact
    zeros; through autograd likewise (a GradScaler's factor rides there); no gradient asked, none computed; the guards of the op"""
    from moma_amd import ops
    for (B, K) in [(7, 10), (5, 1025)]:
        z, y = _draw(B, K, 8)
        for dtype in (F32, BF16):
            one = run_abi(z, y, dtype)
            for g in (2.0, 0.5, 1024.0, 65536.0):
                got = run_abi(z, y, dtype, g_loss=g)
                assert torch.equal(got["raw"]["dz"].float(), one["raw"]["dz"].float() * g), (dtype, g)
                assert all(torch.equal(got["raw"][k], one["raw"][k]) for k in ("loss", "lse", "inv_n"))
            assert not run_abi(z, y, dtype, g_loss=0.0)["dz"].any()
    tz, ty = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    grads = []
    for g in (1.0, 4.0):
        x = tz.clone().requires_grad_(True)
        (ops.ce_head(x, ty) * g).backward()
        grads.append(x.grad)
    assert torch.equal(grads[1], grads[0] * 4.0)
    with torch.no_grad():
        assert not ops.ce_head(tz, ty).requires_grad
    from moma_amd._lib import MomaHipError
    with pytest.raises(TypeError):
        ops.ce_head(tz.half(), ty)
    with pytest.raises(TypeError):
        ops.ce_head(tz, ty.int())
    with pytest.raises(ValueError):
        ops.ce_head(tz.t().contiguous().t(), ty)
    with pytest.raises(ValueError):
        ops.ce_head(tz, ty[:3])
    with pytest.raises(ValueError):
        ops.ce_head(tz, ty, conf=torch.zeros(3, 3, dtype=I64, device="cuda"))
    with pytest.raises(MomaHipError):
        ops.ce_head(tz.cpu(), ty.cpu())


def test_refusals_write_nothing():
    """B < 1 or K < 1: MOMA_E_SHAPE; an unknown dtype: MOMA_E_DTYPE; past the caps: MOMA_E_UNSUPPORTED; from both entry points,
    nothing launched, nothing written"""
    from moma_amd import _lib as L
    lib, guard = _lib(), _Guarded()
    e = lambda n, dt=F32: guard.empty(n, device="cuda", dtype=dt)             # noqa: E731
    z, y, d, f, c = e(16), e(8, I64), e(16, F64), e(8), e(16, I64)
    z.fill_(1.5); d.fill_(1.5); f.fill_(1.5); y.fill_(1); c.fill_(3)
    big = 1 << 30

    def fwd(B, K, dt=0):
        return lib.moma_ce_fwd(_p(z), _p(y), B, K, dt, _p(d), big, _p(f), _p(d), _p(d), _p(c), _p(d), _p(c), _st())

    def bwd(B, K, dt=0):
        return lib.moma_ce_bwd(_p(z), _p(y), _p(d), _p(d), _p(f), _p(z), B, K, dt, _st())

    for shape in ((0, 4), (4, 0), (-1, 4)):
        assert lib.moma_ce_workspace_bytes(*shape) == 0 and fwd(*shape) == -2 and bwd(*shape) == -2
    assert fwd(2, 4, 2) == -3 and bwd(2, 4, 2) == -3 and fwd(2, 4, -1) == -3
    for shape in ((L.CE_MAX_B + 1, 2), (2, L.CE_MAX_K + 1)):
        assert lib.moma_ce_workspace_bytes(*shape) == 0 and fwd(*shape) == -6 and bwd(*shape) == -6
    assert lib.moma_ce_workspace_bytes(L.CE_MAX_B, L.CE_MAX_K) == 16 * L.CE_MAX_B
    assert lib.moma_ce_fwd(_p(z), _p(y), 2, 4, 0, _p(d), 8, _p(f), _p(d), _p(d), None, None, None, _st()) == -5      # a workspace too small
    assert guard.check("refused shapes") > 0
    torch.cuda.synchronize()
    assert all(bool((t == 1.5).all()) for t in (z, d, f)) and bool((y == 1).all()) and bool((c == 3).all())      # nothing written


def test_a_bad_label_is_never_an_index():
    """labels outside [0, K) other than -100: the loss is NaN, the row's gradient zero, stats[3] counts them, conf and the margins of
    every buffer stay untouched by them; the other rows keep their loss term, gradient and cell"""
    _cases, allow = ce_fixture.load()
    z, y = _draw(9, 5, 77)
    y[[1, 4, 6]] = (5, -1, 1 << 40)
    y[7] = V.IGNORE
    want = _want(z, y)
    assert want["n_bad"] == 3 and want["n_valid"] == 5 and np.isnan(want["loss"])
    for dtype in (F32, BF16):
        for off in (False, True):
            got = run_abi(z, y, dtype, off, g_loss=2.0)                       # (run_abi checks the margins, conf's among them)
            assert check(f"bad labels {dtype}", got, want, allow, g_loss=2.0, bf16_out=dtype == BF16)
            assert np.isnan(got["loss"]) and not got["dz"][[1, 4, 6, 7]].any() and (got["conf"] - CONF0).sum() == 5
    # through the module: no exception, the process lives on
    head = CrossEntropyHead(5, meter=True).cuda()
    x = torch.from_numpy(z).bfloat16().cuda().requires_grad_(True)            # (bf16: the module takes the kernels)
    loss = head(x, torch.from_numpy(y).cuda())
    loss.backward()
    assert bool(torch.isnan(loss)) and not x.grad[[1, 4, 6, 7]].any() and head.stats.tolist()[1:] == [want["hits"], 5.0, 3.0] and np.array_equal(head.read()[2], want["conf"])
    # an all-ignored batch: NaN as torch, exact zeros, nothing counted
    ya = np.full(9, V.IGNORE, np.int64)
    got = run_abi(z, ya, F32)
    assert np.isnan(got["loss"]) and not got["dz"].any() and np.array_equal(got["stats"], STATS0) and (got["conf"] == CONF0).all()


def test_module_takes_the_kernels_or_the_composite(monkeypatch):
    from moma_amd import ops
    calls = []
    real = ops.ce_head

    def spy(logits, *a, **kw):
        calls.append(logits.dtype)
        return real(logits, *a, **kw)
    monkeypatch.setattr(ops, "ce_head", spy)
    c = ce_fixture.load()[0][4]
    z, y = torch.from_numpy(c["logits"]).cuda(), torch.from_numpy(c["labels"]).cuda()
    head = CrossEntropyHead()
    ref = c["loss"]
    assert abs(float(head(z.bfloat16(), y)) - ref) < 1e-6 * ref and calls == [BF16]
    assert abs(float(head(z, y)) - ref) < 1e-6 * ref and len(calls) == 1                   # float32: turned away by the microbenchmark
    assert abs(float(head(z.half(), y)) - ref) < 1e-6 * ref and len(calls) == 1            # float16: the composite
    assert head(z.double(), y).dtype == F32 and len(calls) == 1                            # float64 likewise
    assert abs(float(head(z.bfloat16(), y.int())) - ref) < 1e-6 * ref and len(calls) == 1  # int32 labels likewise
    assert abs(float(head(z.cpu(), y.cpu())) - ref) < 1e-6 * ref and len(calls) == 1       # the CPU likewise
    z8, y8 = z[:, :8].bfloat16(), y.clamp(max=7)
    assert abs(float(head(z8.t().contiguous().t(), y8)) - float(head.composite(z8, y8))) < 1e-6 and len(calls) == 2      # strided logits: made contiguous
    assert ops.ce_native(64, 4, BF16) and ops.ce_native(64, 4) and not ops.ce_native(64, 4, F32)
    assert not ops.ce_native(1 << 20, 4, BF16) and not ops.ce_native(4, 1 << 20, BF16) and not ops.ce_native(0, 4)
    monkeypatch.setattr(ops, "ce_native", lambda *a, **kw: False)
    assert abs(float(head(z.bfloat16(), y)) - ref) < 1e-6 * ref and len(calls) == 2        # routed away by the table
    monkeypatch.setattr(ops, "ce_native", lambda *a, **kw: True)
    assert abs(float(head(z, y)) - ref) < 1e-6 * ref and calls[2:] == [F32]                # and float32 onto the kernels, if the table says so


ARGV = ["--model", "resnet8", "--dataset", "cifar100", "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "--print_freq", "100",
        "--learning_rate", "0.01", "--num_workers", "0"]


def test_one_train_vanilla_step_on_the_kernels_against_the_composite(monkeypatch):
    """one step of train_vanilla (resnet8, synthetic 32 x 32, B = 8, bf16 autocast, deterministic convolutions) with the head on the
    kernels and with the head routed to its composite: the same bf16 logits reach both, so the losses agree within the allowance and
    the meters are equal; the same step in fp32 takes the composite (ops.ce_native) and stays finite"""
    from moma_amd import ops, train_teacher as TT
    from moma_amd.backbones import model_dict
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_vanilla import train_vanilla
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    _cases, allow = ce_fixture.load()
    dev = torch.device("cuda", 0)
    seen = []
    real = ops.ce_head

    def spy(logits, *a, **kw):
        seen.append(logits.dtype)
        return real(logits, *a, **kw)
    monkeypatch.setattr(ops, "ce_head", spy)

    def step(extra=()):
        opt = TT.parse_option(ARGV + list(extra))
        opt.gpu, opt.multiprocessing_distributed, opt.device, opt.trace = 0, False, dev, []
        torch.manual_seed(3)
        model = model_dict["resnet8"](num_classes=4).to(dev)
        head = CrossEntropyHead(4, meter=True).to(dev)
        optimizer = TT.make_optimizer(model.parameters(), opt, dev)
        acc, loss = train_vanilla(1, SyntheticLoader(1, 8, 32, 4, 5, dev), model, head, optimizer, opt)
        return acc, loss, float(opt.trace[0]), head.stats.tolist(), head.conf.cpu().numpy()

    k = step(["--amp", "bf16"])
    assert seen == [BF16]                                                                  # (autocast hands the head bf16 logits)
    monkeypatch.setattr(ops, "ce_native", lambda *a, **kw: False)
    c = step(["--amp", "bf16"])
    assert seen == [BF16]                                                                  # (the composite's step called no kernel)
    monkeypatch.undo()
    print("loss of the step: kernels %.9e  composite %.9e" % (k[2], c[2]))
    assert _report("loss of the step", abs(k[2] - c[2]) / c[2], allow["loss"] + ULP32 / 2, "loss")
    assert k[3][1:] == c[3][1:] == [k[3][1], 8.0, 0.0] and np.array_equal(k[4], c[4]) and k[4].sum() == 8
    assert abs(k[3][0] - c[3][0]) <= 1e-9 * c[3][0] and k[0] == c[0] == 100.0 * k[3][1] / 8 and abs(k[1] - k[3][0] / 8) < 1e-12
    monkeypatch.setattr(ops, "ce_head", spy)
    a = step()                                                                             # fp32 logits: the composite, by the table
    assert seen == [BF16] and np.isfinite(a[2]) and a[3][2] == 8.0

"""GPU tests of the student-head kernels (csrc/kdhead.hip) through the C ABI, ops.kd_head, helper.kd_head.StudentHead, one eager step of
MomaStep per head and one graph-served step.

Yardstick: the float64 evaluation of the formulas (tests/kdhead_ref.py).  Allowance for every floating-point result, per kind (cls, div,
dz): TWICE the largest distance of that kind (`ref_vs_f64_<kind>`) that the reference's own fp32 results keep from float64 over the
cases of the golden fixture, never below one fp32 ulp (2^-23, relative) -- computed by tests/kdhead_fixture.py from the .npz.  Metric:
each loss relative to its own value, dz in crd_ref.rel's units (the yardstick's largest element).  A dz stored in bf16 adds that
rounding: at most 2^-8 of the element.  The identical-rows case has loss_div = 0 in float64 and is checked in absolute terms: |loss_div|
at most the larger of the reference's own recorded |loss_div| for that case and 2^-23 T^2 (a row's KL is a sum of terms of order 1,
scaled by T^2), and the KL part of its dz exactly 0.  The saved lse, lseS, lseT and 1 / n_valid are doubles computed in double: compared
at 1e-12.  acc is compared exactly (every student row's maximum is unique by construction).
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched.

Largest share of each allowance used (printed by teardown_module; DESIGN.md, section KD head, quotes it)."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from moma_amd.helper.kd_head import StudentHead
from tests import kdhead_fixture, kdhead_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded
from tests.test_kdhead_cpu import compare_steps, step_of

pytestmark = pytest.mark.gpu
F32, BF16, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8
N_CASES = kdhead_fixture.N_CASES
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]                  # (student, teacher)
USED = {}                                                                     # kind -> the largest share of its allowance any check used


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


def _put(guard, z, dtype, off):
    t = _carve(guard, z.shape, dtype, off)
    src = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(dtype)
    assert np.array_equal(src.float().numpy(), z)                            # (the inputs are exact in the storage type)
    t.copy_(src)
    return t


def _draw(B, K, seed):
    """the fixture's recipe for both sides; labels: the student's argmax on the even rows, a uniform draw on the odd ones"""
    rng = np.random.default_rng(seed)
    zs = np.clip(np.round(rng.standard_normal((B, K)) * 32) / 32, -4, 4).astype(np.float32)
    zt = np.clip(np.round(rng.standard_normal((B, K)) * 32) / 32, -4, 4).astype(np.float32)
    top = zs.argmax(axis=1)
    zs[np.arange(B), top] += np.float32(V.MARGIN)
    y = rng.integers(0, K, B).astype(np.int64)
    y[::2] = top[::2]
    assert V.margin(zs) >= V.MARGIN
    return zs, zt, y


def run_abi(zs, zt, y, T, ds=F32, dt=F32, off=False, g_cls=1.0, g_div=1.0, bwd=True):
    """moma_kdhead_fwd -> moma_kdhead_bwd on fresh guarded buffers; numpy inputs; g_cls / g_div None: a NULL pointer
    -> dict of numpy arrays and the raw device tensors under `raw`"""
    lib, guard = _lib(), _Guarded()
    B, K = zs.shape
    ts, tt = _put(guard, zs, ds, off), _put(guard, zt, dt, off)
    ty = guard.empty(B, device="cuda", dtype=I64)
    ty.copy_(torch.from_numpy(y))
    nws = lib.moma_kdhead_workspace_bytes(B, K)
    assert nws > 0 and nws % 8 == 0
    ws = guard.empty(nws // 8, device="cuda", dtype=F64)
    out, saved = guard.empty(3, device="cuda", dtype=F32), guard.empty(3 * B + 1, device="cuda", dtype=F64)
    rc = lib.moma_kdhead_fwd(_p(ts), _p(tt), _p(ty), B, K, _code(ds), _code(dt), T, _p(ws), nws, _p(out), _p(saved), _st())
    assert rc == 0, rc
    raw = {"out": out, "saved": saved}
    if bwd:
        gc = None if g_cls is None else torch.full((1,), float(g_cls), device="cuda")
        gd = None if g_div is None else torch.full((1,), float(g_div), device="cuda")
        dz = _carve(guard, zs.shape, ds, off)
        rc = lib.moma_kdhead_bwd(_p(ts), _p(tt), _p(ty), _p(saved), _p(gc), _p(gd), _p(dz), B, K, _code(ds), _code(dt), T, _st())
        assert rc == 0, rc
        raw["dz"] = dz
    assert guard.check("kdhead C ABI") > 0                                    # every margin untouched
    res = {k: (v.float() if v.dtype == BF16 else v).cpu().numpy() for k, v in raw.items()}
    res.update(loss_cls=float(res["out"][0]), loss_div=float(res["out"][1]), acc=float(res["out"][2]), raw=raw)
    return res


def check(tag, got, want, allow, c=None, g_cls=1.0, g_div=1.0, bf16_out=False):
    """want: V.head at both weights 1; c: the fixture case (the identical-rows case is checked in absolute terms)"""
    B = want["lse"].shape[0]
    T = None if c is None else c["T"]
    if np.isnan(want["loss_cls"]):
        ok = np.isnan(got["loss_cls"])
    elif want["loss_cls"] == 0.0:
        ok = got["loss_cls"] == 0.0
    else:
        ok = _report(f"{tag} loss_cls", abs(got["loss_cls"] - want["loss_cls"]) / abs(want["loss_cls"]), allow["cls"], "cls")
    if c is not None and c["same"]:
        ok &= _report(f"{tag} loss_div (absolute)", abs(got["loss_div"]), max(c["ref_vs_f64_div"], ULP32 * T * T))
    elif want["loss_div"] == 0.0:
        ok &= got["loss_div"] == 0.0
    else:
        ok &= _report(f"{tag} loss_div", abs(got["loss_div"] - want["loss_div"]) / abs(want["loss_div"]), allow["div"], "div")
    assert got["acc"] == float(np.float32(want["acc"])), (tag, got["acc"], want["acc"])
    sv = got["saved"]
    for i, k in enumerate(("lse", "lseS", "lseT")):
        assert np.abs(sv[i * B:(i + 1) * B] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), (tag, k)
    if want["n_valid"]:
        assert sv[3 * B] == 1.0 / want["n_valid"], tag
    if "dz" in got:
        w = (0.0 if g_cls is None else g_cls) * want["dz_cls"] + (0.0 if g_div is None else g_div) * want["dz_div"]
        err = np.abs(got["dz"].astype(np.float64) - w)
        if bf16_out:
            err = np.maximum(err - HALF_ULP_BF16 * np.abs(w), 0)              # the rounding of the stored gradient
        if np.abs(w).max() == 0.0:
            ok &= not got["dz"].any()
        else:
            ok &= _report(f"{tag} dz", float(err.max() / np.abs(w).max()), allow["dz"], "dz")
    return ok


def teardown_module(_m):
    print("largest share of an allowance used, per kind:", {k: round(v, 3) for k, v in sorted(USED.items())})


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """every fixture case against float64: through the C ABI in all four dtype pairs, with and without a one-element offset of the base
    addresses; g_cls only, g_div only, both, a power of two in both; two runs with the same bits; then the op and the module.  The
    inputs are exact in bf16, so one yardstick serves every pair"""
    from moma_amd import ops
    cases, allow = kdhead_fixture.load()
    c = cases[ci]
    zs, zt, y, T = c["logit_s"], c["logit_t"], c["labels"], c["T"]
    want = V.head(zs, zt, y, T)
    print(f"case {ci} B {c['B']} K {c['K']} T {T}")
    ok = True
    for ds, dt in PAIRS:
        for off in (False, True):
            got = run_abi(zs, zt, y, T, ds, dt, off, g_cls=3.0, g_div=0.5)
            assert got["raw"]["dz"].dtype == ds
            ok &= check(f"abi {ds} {dt} off {int(off)}", got, want, allow, c, 3.0, 0.5, bf16_out=ds == BF16)
    ds, dt = PAIRS[ci % 4]
    off = bool((ci // 4) % 2)
    both = run_abi(zs, zt, y, T, ds, dt, off)
    again = run_abi(zs, zt, y, T, ds, dt, off)
    assert all(torch.equal(both["raw"][k], again["raw"][k]) for k in both["raw"])                    # two runs, the same bits
    only_c = run_abi(zs, zt, y, T, ds, dt, off, g_cls=1.0, g_div=None)
    only_d = run_abi(zs, zt, y, T, ds, dt, off, g_cls=None, g_div=1.0)
    ok &= check("g_cls only", only_c, want, allow, c, 1.0, None, bf16_out=ds == BF16)
    ok &= check("g_div only", only_d, want, allow, c, None, 1.0, bf16_out=ds == BF16)
    zero_d = run_abi(zs, zt, y, T, ds, dt, off, g_cls=1.0, g_div=0.0)
    assert torch.equal(zero_d["raw"]["dz"], only_c["raw"]["dz"])                                     # NULL = 0
    if c["same"]:
        assert not only_d["dz"].any() and torch.equal(both["raw"]["dz"], only_c["raw"]["dz"])       # the KL part: exactly 0
    for s in (4.0, 2.0 ** -5):
        sc = run_abi(zs, zt, y, T, ds, dt, off, g_cls=s, g_div=s)
        assert torch.equal(sc["raw"]["dz"].float(), both["raw"]["dz"].float() * s), s                # every bit pattern scales exactly
        assert torch.equal(sc["raw"]["out"], both["raw"]["out"]) and torch.equal(sc["raw"]["saved"], both["raw"]["saved"])
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    got = run_abi(zs, zt, y, T)
    if c["loss_cls"] != 0.0:
        ok &= _report("loss_cls vs reference", abs(got["loss_cls"] - c["loss_cls"]) / abs(c["loss_cls"]), allow["cls"] + c["ref_vs_f64_cls"])
    if not c["same"] and c["loss_div"] != 0.0:
        ok &= _report("loss_div vs reference", abs(got["loss_div"] - c["loss_div"]) / abs(c["loss_div"]), allow["div"] + c["ref_vs_f64_div"])
    ok &= _report("dz vs reference", rel(got["dz"], c["dz"]) if np.abs(c["dz"]).max() else 0.0, allow["dz"] + c["ref_vs_f64_dz"])
    assert abs(got["acc"] - c["acc"]) < 1e-4
    # the op: the same bits as the C ABI; the module takes it; the composite within the allowance
    for ds, dt in PAIRS:
        xs = torch.from_numpy(zs).to(ds).cuda().requires_grad_(True)
        xt, ty = torch.from_numpy(zt).to(dt).cuda(), torch.from_numpy(y).cuda()
        lc, ld, acc = ops.kd_head(xs, xt, ty, T)
        assert all(t.dtype == F32 and t.dim() == 0 and t.is_cuda for t in (lc, ld, acc)) and not acc.requires_grad
        (3.0 * lc + 0.5 * ld).backward()
        ref = run_abi(zs, zt, y, T, ds, dt, g_cls=3.0, g_div=0.5)
        assert torch.equal(torch.stack([lc.detach(), ld.detach(), acc]), ref["raw"]["out"])
        assert torch.equal(xs.grad, ref["raw"]["dz"]) and xs.grad.dtype == ds
        x2 = torch.from_numpy(zs).to(ds).cuda().requires_grad_(True)
        ops.kd_head(x2, xt, ty, T)[1].backward()                                                     # one output used: the other's gradient is None
        assert torch.equal(x2.grad, run_abi(zs, zt, y, T, ds, dt, g_cls=None, g_div=1.0)["raw"]["dz"])
        mc, md, macc = StudentHead(T)(xs.detach(), xt, ty)
        assert torch.equal(mc, lc.detach()) and torch.equal(md, ld.detach()) and torch.equal(macc, acc)
        xc = torch.from_numpy(zs).to(ds).cuda().requires_grad_(True)
        cc, cd, cacc = StudentHead.composite(xc, xt, ty, T)
        (3.0 * cc + 0.5 * cd).backward()
        lc, ld, cc, cd = lc.detach(), ld.detach(), cc.detach(), cd.detach()
        if want["loss_cls"]:
            ok &= _report(f"{ds} loss_cls vs the composite", abs(float(lc) - float(cc)) / abs(float(cc)), allow["cls"] + ULP32 / 2)
        if want["loss_div"]:
            ok &= _report(f"{ds} loss_div vs the composite", abs(float(ld) - float(cd)) / abs(float(cd)), allow["div"] + ULP32 / 2)
        w = 3.0 * want["dz_cls"] + 0.5 * want["dz_div"]
        err = np.abs(xs.grad.double().cpu().numpy() - xc.grad.double().cpu().numpy())
        if ds == BF16:
            err = np.maximum(err - 2 * HALF_ULP_BF16 * np.abs(w), 0)                                 # (both sides store bf16)
        if np.abs(w).max():
            ok &= _report(f"{ds} dz vs the composite", float(err.max() / np.abs(w).max()), allow["dz"] + ULP32 / 2)
        assert float(acc) == float(cacc)
    assert ok


EDGES = [  # (B, K, T): sizes at which the kernels take another path and more than one workgroup
    (300, 4, 4.0),      # one lane per row, 256 rows per workgroup: a second workgroup; two rows per thread of the finalize
    (5, 17, 2.0),       # two lanes per row, the second with one element
    (70, 40, 4.0),      # four lanes per row, 64 rows per workgroup: a second workgroup
    (9, 513, 3.0),      # 64 lanes, the last ones idle
    (6, 1032, 4.0),     # two walks, 16-byte accesses in bf16 and fp32, one more trip for the first lanes
    (600, 3, 1.5),      # element accesses, three workgroups, three rows per thread of the finalize
]


@pytest.mark.parametrize("ei", range(len(EDGES)))
def test_edges_against_the_restatement(ei):
    _cases, allow = kdhead_fixture.load()
    B, K, T = EDGES[ei]
    zs, zt, y = _draw(B, K, 600 + ei)
    y[1::7] = V.IGNORE
    want = V.head(zs, zt, y, T)
    ok = True
    for ds, dt in ((F32, BF16), (BF16, F32), (BF16, BF16)):
        got = run_abi(zs, zt, y, T, ds, dt, off=bool(ei % 2), g_cls=0.5, g_div=2.0)
        ok &= check(f"{EDGES[ei]} {ds} {dt}", got, want, allow, None, 0.5, 2.0, bf16_out=ds == BF16)
    assert ok


def test_a_bad_label_is_never_an_index():
    _cases, allow = kdhead_fixture.load()
    zs, zt, y = _draw(9, 5, 77)
    y[[1, 4, 6]] = (5, -1, 1 << 40)
    y[7] = V.IGNORE
    want = V.head(zs, zt, y, 4.0)
    assert want["n_bad"] == 3 and want["n_valid"] == 5 and np.isnan(want["loss_cls"]) and np.isfinite(want["loss_div"])
    for ds, dt in PAIRS:
        got = run_abi(zs, zt, y, 4.0, ds, dt, off=ds == BF16, g_cls=2.0, g_div=None)         # (run_abi checks the margins)
        assert check(f"bad labels {ds}", got, want, allow, None, 2.0, None, bf16_out=ds == BF16)
        assert np.isnan(got["loss_cls"]) and np.isfinite(got["loss_div"]) and not got["dz"][[1, 4, 6, 7]].any()
        assert check(f"bad labels {ds}, both", run_abi(zs, zt, y, 4.0, ds, dt), want, allow, None, bf16_out=ds == BF16)
    # through the module: no exception, the process lives on
    x = torch.from_numpy(zs).bfloat16().cuda().requires_grad_(True)
    lc, ld, acc = StudentHead(4.0)(x, torch.from_numpy(zt).cuda(), torch.from_numpy(y).cuda())
    lc.backward()
    assert bool(torch.isnan(lc)) and bool(torch.isfinite(ld)) and not x.grad[[1, 4, 6, 7]].any() and float(acc) == np.float32(want["acc"])
    # an all-ignored batch: NaN as torch, no CE gradient
    ya = np.full(9, V.IGNORE, np.int64)
    got = run_abi(zs, zt, ya, 4.0, g_cls=1.0, g_div=None)
    assert np.isnan(got["loss_cls"]) and not got["dz"].any() and got["acc"] == 0.0


def test_refusals_write_nothing():
    """B < 1, K < 1 or a T that is not finite and > 0: MOMA_E_SHAPE; an unknown dtype: MOMA_E_DTYPE; past the caps: MOMA_E_UNSUPPORTED;
    from both entry points, nothing launched, nothing written"""
    from moma_amd import _lib as L
    lib, guard = _lib(), _Guarded()
    e = lambda n, dt=F32: guard.empty(n, device="cuda", dtype=dt)             # noqa: E731
    z, y, d, f = e(16), e(8, I64), e(16, F64), e(8)
    z.fill_(1.5); d.fill_(1.5); f.fill_(1.5); y.fill_(1)
    big = 1 << 30

    def fwd(B, K, a=0, b=0, T=4.0):
        return lib.moma_kdhead_fwd(_p(z), _p(z), _p(y), B, K, a, b, T, _p(d), big, _p(f), _p(d), _st())

    def bwd(B, K, a=0, b=0, T=4.0):
        return lib.moma_kdhead_bwd(_p(z), _p(z), _p(y), _p(d), _p(f), _p(f), _p(z), B, K, a, b, T, _st())

    for shape in ((0, 4), (4, 0), (-1, 4)):
        assert lib.moma_kdhead_workspace_bytes(*shape) == 0 and fwd(*shape) == -2 and bwd(*shape) == -2
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert fwd(2, 4, T=T) == -2 and bwd(2, 4, T=T) == -2
    assert fwd(2, 4, 2, 0) == -3 and fwd(2, 4, 0, 2) == -3 and bwd(2, 4, 0, -1) == -3 and bwd(2, 4, 7, 0) == -3
    for shape in ((L.KDHEAD_MAX_B + 1, 2), (2, L.KDHEAD_MAX_K + 1)):
        assert lib.moma_kdhead_workspace_bytes(*shape) == 0 and fwd(*shape) == -6 and bwd(*shape) == -6
    assert lib.moma_kdhead_workspace_bytes(L.KDHEAD_MAX_B, L.KDHEAD_MAX_K) == 20 * L.KDHEAD_MAX_B
    assert lib.moma_kdhead_fwd(_p(z), _p(z), _p(y), 2, 4, 0, 0, 4.0, _p(d), 8, _p(f), _p(d), _st()) == -5       # a workspace too small
    assert lib.moma_kdhead_bwd(_p(z), _p(z), _p(y), _p(d), None, None, _p(z), 2, 4, 0, 0, 4.0, _st()) == -1      # no upstream gradient at all
    assert guard.check("refused shapes") > 0
    torch.cuda.synchronize()
    assert all(bool((t == 1.5).all()) for t in (z, d, f)) and bool((y == 1).all())      # nothing written


def test_the_guards_of_the_op_and_the_routing_of_the_module(monkeypatch):
    from moma_amd import ops
    from moma_amd._lib import MomaHipError
    c = kdhead_fixture.load()[0][4]
    zs, zt, y = torch.from_numpy(c["logit_s"]).cuda(), torch.from_numpy(c["logit_t"]).cuda(), torch.from_numpy(c["labels"]).cuda()
    with pytest.raises(ValueError, match="no gradient to logit_t"):
        ops.kd_head(zs, zt.clone().requires_grad_(True), y, 1.0)
    with torch.no_grad():
        assert not ops.kd_head(zs, zt.clone().requires_grad_(True), y, 1.0)[0].requires_grad
    with pytest.raises(ValueError, match="not contiguous"):
        ops.kd_head(zs.t().contiguous().t(), zt, y, 1.0)
    with pytest.raises(ValueError, match="not contiguous"):
        ops.kd_head(zs, zt.t().contiguous().t(), y, 1.0)
    with pytest.raises(TypeError):
        ops.kd_head(zs.half(), zt, y, 1.0)
    with pytest.raises(TypeError):
        ops.kd_head(zs, zt, y.int(), 1.0)
    with pytest.raises(ValueError):
        ops.kd_head(zs, zt[:, :8].contiguous(), y, 1.0)
    with pytest.raises(ValueError):
        ops.kd_head(zs, zt, y[:3], 1.0)
    for T in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.kd_head(zs, zt, y, T)
    with pytest.raises(MomaHipError):
        ops.kd_head(zs.cpu(), zt.cpu(), y.cpu(), 1.0)
    # the module: strided inputs are made dense, what the table or the dtypes turn away takes the composite
    calls = []
    real = ops.kd_head

    def spy(a, b, *r, **kw):
        calls.append((a.dtype, b.dtype, a.is_contiguous() and b.is_contiguous()))
        return real(a, b, *r, **kw)
    monkeypatch.setattr(ops, "kd_head", spy)
    head, ref = StudentHead(1.0), (c["loss_cls"], c["loss_div"])
    near = lambda r: abs(float(r[0]) - ref[0]) < 1e-5 * ref[0] and abs(float(r[1]) - ref[1]) < 1e-4 * ref[1]      # noqa: E731
    assert near(head(zs.bfloat16(), zt, y)) and calls == [(BF16, F32, True)]
    assert near(head(zs.t().contiguous().t(), zt.t().contiguous().t(), y)) and calls[1:] == [(F32, F32, True)]
    n = len(calls)
    assert near(head(zs.half(), zt, y)) and near(head(zs, zt.double(), y)) and near(head(zs, zt, y.int())) and len(calls) == n
    assert near(head(zs.cpu(), zt.cpu(), y.cpu())) and len(calls) == n
    assert near(head(zs, zt.clone().requires_grad_(True), y)) and len(calls) == n                  # a teacher that wants a gradient
    monkeypatch.setattr(ops, "kd_head_native", lambda *a, **kw: False)
    assert near(head(zs.bfloat16(), zt, y)) and len(calls) == n                                     # routed away by the table


@pytest.mark.parametrize("amp", [None, "bf16"])
def test_one_eager_step_per_head(amp, monkeypatch):
    """one MomaStep.run_eager step of --distill kd (resnet8x4 <- resnet32x4, B = 8, n_cls = 4, deterministic convolutions) with
    --student_head fused against the same step with stock: the head sees the student's logits as the backbone left them (bf16 under
    --amp bf16, no .float() cast) and the kernels serve them; loss and student gradients within the allowance.  Under bf16 both
    heads' dz are rounded to bf16 before they enter the backbone's backward: 2^-8 of the element on either side"""
    from moma_amd import ops
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    _cases, allow = kdhead_fixture.load()
    dev = torch.device("cuda", 0)
    seen = []
    real = ops.kd_head

    def spy(a, b, *r, **kw):
        seen.append((a.dtype, b.dtype))
        return real(a, b, *r, **kw)
    monkeypatch.setattr(ops, "kd_head", spy)
    extra = ["--amp", amp] if amp else []
    fused = step_of(dev, "fused", extra)
    assert seen == [(BF16 if amp else F32, F32)]
    stock = step_of(dev, "stock", extra)
    assert len(seen) == 1 and np.isfinite(fused[0]) and fused[0] > 0
    print("loss of the step: fused %.9e  stock %.9e" % (fused[0], stock[0]))
    assert compare_steps(fused, stock, allow, extra_dz=2 * HALF_ULP_BF16 if amp else 0.0)


def _moma_run(graph_student, student_head, steps=7, B=8, K=256, d=64, size=32, lr=0.02):
    """one epoch of the --distill moma loop (resnet8 pair, bf16 policy, two streams): the only configuration MomaStep.graphable()
    serves from HIP graphs (`--distill kd` keeps the eager loop) -> per-step losses, accuracies, the student after the epoch, replays"""
    from moma_amd.backbones import model_dict
    from moma_amd.MoMA.mem_moco import build_mem
    from moma_amd.MoMA.criterion_moco_att import CMO
    from moma_amd.learning.contrast_trainer import ContrastTrainer
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.distiller_zoo import DistillKL
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    ms, mt = model_dict["resnet8"](num_classes=4), model_dict["resnet8"](num_classes=4)
    with torch.no_grad():
        s_dim = ms.eval()(torch.randn(2, 3, size, size), is_feat=True)[0][-1].shape[1]
    opt = argparse.Namespace(distill="moma", head="mlp", feat_dim=d, attn="self", mem="MoCo", nce_k=K, nce_t=0.15, alpha=0.99, cls=1.0,
                             div=1.0, beta=1.0, kd_T=4.0, gpu=0, multiprocessing_distributed=False, print_freq=1000, batch_size=B, rank=0,
                             world_size=1, s_dim=s_dim, t_dim=s_dim, moma_prec="bf16", queue_dtype="bf16", moma_fused=True, trace=[],
                             overlap_teacher=True, graph_teacher=True, graph_student=graph_student, amp=None, student_head=student_head)
    contrast, kd = build_mem(opt), CMO(opt)
    ms, mt, contrast, kd = ms.to(dev), mt.to(dev), contrast.to(dev), kd.to(dev)
    trainer = ContrastTrainer(opt)
    att_names = [n for n in ("atts", "atts_p", "atts_n", "atts_q", "atts_k", "atts_queue") if hasattr(kd, n)]
    trainable = nn.ModuleList([ms] + [getattr(kd, n) for n in att_names] + [kd.embed_s])
    optimizer = torch.optim.SGD(trainable.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    mods, crits = nn.ModuleList([ms, kd.embed_s, kd.embed_t, mt]), nn.ModuleList([nn.CrossEntropyLoss(), DistillKL(4.0), kd])
    gen = torch.Generator().manual_seed(3)
    data = [(torch.randn(B, 3, size, size, generator=gen).to(dev), torch.randint(0, 4, (B,), generator=gen).to(dev)) for _ in range(steps)]
    torch.manual_seed(99)
    train_distill_moma(1, data, mods, crits, trainer, contrast, optimizer, opt)
    torch.cuda.synchronize()
    sg = getattr(trainer, "_step_graphs", None)
    return dict(loss=torch.stack([t[0] for t in opt.trace]).cpu().numpy(), loss_kd=torch.stack([t[2] for t in opt.trace]).cpu().numpy(),
                student=[p.detach().float().cpu().numpy() for p in ms.parameters()], replays=0 if sg is None else sg.replays, runner=sg)


def test_the_graph_served_step_with_the_fused_head():
    """seven steps of the --distill moma loop with --student_head fused, served from HIP graphs from the 5th step on, against the same
    loop issued launch by launch: bit-identical losses and student.  Against the stock head: the first step's loss within the allowance
    (later steps start from weights that already differ).  A runner bound under one head is not reused under the other"""
    from moma_amd.helper.step_graph import StepGraphs
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        _cases, allow = kdhead_fixture.load()
        g = _moma_run(True, "fused")
        e = _moma_run(False, "fused")
        s = _moma_run(False, "stock")
    finally:
        torch.backends.cudnn.deterministic = det
    assert g["replays"] == 3 and e["replays"] == 0
    assert np.array_equal(g["loss"], e["loss"]) and np.array_equal(g["loss_kd"], e["loss_kd"])
    assert all(np.array_equal(a, b) for a, b in zip(g["student"], e["student"]))
    # the first step: loss = loss_cls + loss_div + loss_kd, the last term from the same kernels on the same inputs
    assert e["loss_kd"][0] == s["loss_kd"][0]
    assert _report("first step's loss, fused vs stock", abs(e["loss"][0] - s["loss"][0]) / abs(s["loss"][0]),
                   1.5 * (allow["cls"] + allow["div"]) + ULP32)
    # the runner: bound under the fused head, it is not the stock head's
    runner = g["runner"]
    assert isinstance(runner, StepGraphs) and runner.st.student_head is not None
    other = argparse.Namespace(**{k: getattr(runner.st, k) for k in ("model_s", "model_t", "criterion_kd", "contrast", "optimizer", "trainer")},
                               student_head=None)
    same = argparse.Namespace(**{**vars(other), "student_head": StudentHead(4.0)})
    assert runner.same_objects(same) and not runner.same_objects(other)

"""GPU tests of the Variational Information Distillation kernels (csrc/vid.hip) through the C ABI, ops.vid_nll, the criterion and the
training loop.

Yardstick: the float64 evaluation of the formulas (tests/vid_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_loss / _dmean / _dls / _dx / _dw`) that the reference's own fp32 results keep from that evaluation
over the cases of the golden fixture, never below one fp32 ulp (2^-23, relative): a different but equally valid fp32 order can land
on the other side of the float64 value.  Metric: crd_ref.rel (units of the yardstick's largest element); the loss in units of
abs_terms = 0.5 (mean d^2 / var + mean_c |log var_c|), the sum of its terms by magnitude (it cancels where var < 1).  S_c takes the
`loss` allowance per channel relative to its own value (the loss's data term is S_c scaled by an exact factor); var_c is one
rounding of a double: one fp32 ulp.  A gradient stored in bf16 adds that rounding: half a bf16 ulp (8 significant bits), at most
2^-8 of the element.
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result."""
import ctypes as C

import numpy as np
import pytest
import torch

from moma_amd.distiller_zoo import VIDLoss  # noqa: F401  (the criterion under test: without it nothing here has a subject)
from tests import vid_fixture, vid_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8


def _lib():
    from moma_amd import _lib as L
    return L.load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(name, got, allowed):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e}, ratio {got / allowed:.2f})")
    return got <= allowed


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _r16(a):
    """numpy -> the same values rounded to bf16, as float64"""
    return _np(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16))


def _carve(guard, shape, dtype, cl, offset):
    """an uninitialised device tensor of logical shape [B,C,H,W] between NaN margins: contiguous or channels_last, optionally starting
    one element behind an aligned address (a slice of a larger buffer: no 16-byte access is possible)"""
    B, Cc, H, W = shape
    flat = guard.empty(B * Cc * H * W + int(offset), device="cuda", dtype=dtype)
    flat = flat[1:] if offset else flat
    return flat.view(B, H, W, Cc).permute(0, 3, 1, 2) if cl else flat.view(B, Cc, H, W)


def _place(guard, f, dtype=F32, cl=False, offset=False):
    out = _carve(guard, f.shape, dtype, cl, offset)
    out.copy_(torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dtype))
    return out


def _codes(dtype, cl):
    from moma_amd import _lib as L
    return (L.DT_BF16 if dtype == BF16 else L.DT_F32), (L.LAYOUT_NHWC if cl else L.LAYOUT_NCHW)


def run_abi(mean, target, log_scale, eps=1e-5, cl_m=False, cl_t=False, dt_m=F32, dt_t=F32, off_m=False, off_t=False, g_loss=1.0):
    """moma_vid_nll -> moma_vid_bwd on fresh guarded buffers.  mean, target: numpy [B,C,H,W].  -> dict of numpy float64 arrays S, var,
    d_ls (before g_loss), d_mean, the loss, and the raw device tensors under `raw`"""
    lib, guard = _lib(), _Guarded()
    B, Cc, H, W = mean.shape
    P = H * W
    tm, tt = _place(guard, mean, dt_m, cl_m, off_m), _place(guard, target, dt_t, cl_t, off_t)
    e = lambda *shape: guard.empty(*shape, device="cuda", dtype=F32)          # noqa: E731
    ls = e(Cc)
    ls.copy_(torch.from_numpy(np.asarray(log_scale, np.float32)))
    codes = (*_codes(dt_m, cl_m), *_codes(dt_t, cl_t))
    from moma_amd import _lib as L
    nws = lib.moma_vid_workspace_bytes(B, Cc, P, *codes)
    assert nws == B * -(-P // L.VID_CHUNK) * Cc * 8
    ws = guard.empty(nws // 8, device="cuda", dtype=torch.float64)
    sq, var, g_ls, loss = e(Cc), e(Cc), e(Cc), e(1)
    rc = lib.moma_vid_nll(_p(tm), _p(tt), _p(ls), float(eps), B, Cc, P, *codes, _p(ws), nws, _p(sq), _p(var), _p(g_ls), _p(loss), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    d_mean = _carve(guard, mean.shape, dt_m, cl_m, off_m)                     # dtype and layout of mean
    rc = lib.moma_vid_bwd(_p(tm), _p(tt), _p(var), _p(gl), _p(d_mean), B, Cc, P, *codes, _st())
    assert rc == 0, rc
    assert guard.check("vid C ABI") > 0                                       # every margin untouched
    raw = {"S": sq, "var": var, "d_ls": g_ls, "loss": loss, "d_mean": d_mean, "partials": ws}
    out = {k: _np(v) for k, v in raw.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out["loss"] = float(loss.item())
    out["raw"] = raw
    return out


def run_op(mean, target, log_scale, eps=1e-5, cl_m=False, cl_t=False, dt_m=F32, dt_t=F32, g_loss=1.0):
    from moma_amd import ops
    mk = lambda f, cl, dt: torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dt).cuda().contiguous(    # noqa: E731
        memory_format=torch.channels_last if cl else torch.contiguous_format)
    tm, tt = mk(mean, cl_m, dt_m).requires_grad_(True), mk(target, cl_t, dt_t)
    ls = torch.from_numpy(np.asarray(log_scale, np.float32)).cuda().requires_grad_(True)
    loss = ops.vid_nll(tm, tt, ls, eps)
    (loss * g_loss).backward()
    assert tm.grad.stride() == tm.stride() and tm.grad.dtype == dt_m and tt.grad is None
    assert ls.grad.dtype == F32 and ls.grad.shape == ls.shape
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    return {"loss": float(loss), "d_mean": _np(tm.grad), "d_ls": _np(ls.grad) / g_loss, "raw_d_mean": tm.grad, "raw_loss": loss.detach()}


def check(tag, got, want, allow, g_loss=1.0, bf16_out=False, full=True):
    """want: V.nll at g_loss = 1 (d_ls is compared before the upstream gradient, d_mean after it)"""
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / want["abs_terms"], allow["loss"])
    wd = g_loss * want["d_mean"]
    err = np.abs(got["d_mean"] - wd)
    if bf16_out:
        err = np.maximum(err - HALF_ULP_BF16 * np.abs(wd), 0)                 # the rounding of the stored gradient
    scale = max(np.abs(wd).max(), 1e-300)
    ok &= _report(f"{tag} d_mean", float(err.max() / scale), allow["dmean"])
    ok &= _report(f"{tag} d_log_scale", rel(got["d_ls"], want["d_ls"]), allow["dls"])
    if full:
        s_scale = np.where(want["S"] > 0, want["S"], 1.0)
        ok &= _report(f"{tag} S", float((np.abs(got["S"] - want["S"]) / s_scale).max()), allow["loss"])
        ok &= _report(f"{tag} var", float((np.abs(got["var"] - want["var"]) / want["var"]).max()), ULP32)
    return ok


N_CASES = 11


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """the reference's own pred_mean, the target on the common grid and log_scale, as the criterion hands them to the kernels"""
    cases, allow = vid_fixture.load()
    c = cases[ci]
    t = V.criterion(c["x"], c["target"], c["w"], c["log_scale"], c["eps"])["target"].astype(np.float32)   # (pooled where the case pools)
    want = V.nll(c["pred_mean"], t, c["log_scale"], c["eps"])
    print(f"case {ci} {c['shape']}")
    abi = run_abi(c["pred_mean"], t, c["log_scale"], c["eps"])
    ok = check("abi", abi, want, allow)
    op = run_op(c["pred_mean"], t, c["log_scale"], c["eps"])
    ok &= check("op", op, want, allow, full=False)
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / want["abs_terms"], allow["loss"] + c["ref_vs_f64_loss"])
    ok &= _report("op d_mean vs reference", rel(op["d_mean"], c["d_pred_mean"]), allow["dmean"] + c["ref_vs_f64_dmean"])
    ok &= _report("op d_log_scale vs reference", rel(op["d_ls"], c["d_log_scale"]), allow["dls"] + c["ref_vs_f64_dls"])
    assert ok


_GRID = {}


def _grid_case(ci):
    """(mean, target on the common grid, log_scale, eps, float64 results) of a fixture case -- evaluated once, shared"""
    cases, allow = vid_fixture.load()
    if ci not in _GRID:
        c = cases[ci]
        t = V.criterion(c["x"], c["target"], c["w"], c["log_scale"], c["eps"])["target"].astype(np.float32)
        _GRID[ci] = (c["pred_mean"], t, c["log_scale"], c["eps"], V.nll(c["pred_mean"], t, c["log_scale"], c["eps"]))
    return (*_GRID[ci], allow)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_layouts_agree(ci):
    """all four layout combinations of the two sides: within the allowance of the float64 value and of each other"""
    m, t, ls, eps, want, allow = _grid_case(ci)
    base = run_abi(m, t, ls, eps)
    ok = True
    for cl_m, cl_t in ((False, False), (True, False), (False, True), (True, True)):
        got = run_abi(m, t, ls, eps, cl_m, cl_t, g_loss=3.0)
        tag = f"case {ci} cl_m={int(cl_m)} cl_t={int(cl_t)}"
        ok &= check(tag, got, want, allow, g_loss=3.0)
        ok &= _report(tag + " loss vs NCHW", abs(got["loss"] - base["loss"]) / want["abs_terms"], 2 * allow["loss"])
        ok &= _report(tag + " d_mean vs NCHW", rel(got["d_mean"], 3.0 * base["d_mean"]), 2 * allow["dmean"])
        ok &= _report(tag + " d_log_scale vs NCHW", rel(got["d_ls"], base["d_ls"]), 2 * allow["dls"])
        op = run_op(m, t, ls, eps, cl_m, cl_t)
        ok &= check(tag + " op", op, want, allow, full=False)
    assert ok


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("ci", range(N_CASES))
def test_bf16_storage(ci, cl):
    """inputs rounded to bf16 (the yardstick takes the rounded values): both sides in bf16, either side alone, in both layouts, and
    a bf16 NCHW mean against an fp32 channels_last target; d_mean is stored in mean's dtype"""
    m, t, ls, eps, _want, allow = _grid_case(ci)
    m, t = _r16(m), _r16(t)
    want = V.nll(m, t, ls, eps)
    ok = True
    for dt_m, dt_t, cl_m, cl_t in ((BF16, BF16, cl, cl), (BF16, F32, cl, cl), (F32, BF16, cl, cl), (BF16, F32, False, True)):
        got = run_abi(m, t, ls, eps, cl_m, cl_t, dt_m, dt_t, g_loss=2.0)
        assert got["raw"]["d_mean"].dtype == dt_m
        ok &= check(f"case {ci} {dt_m} {dt_t} cl {int(cl_m)}{int(cl_t)}", got, want, allow, g_loss=2.0, bf16_out=dt_m == BF16)
    op = run_op(m, t, ls, eps, cl, cl, BF16, BF16)
    ok &= check(f"case {ci} op bf16", op, want, allow, bf16_out=True, full=False)
    assert ok


def _chunk():
    from moma_amd import _lib as L
    return L.VID_CHUNK


def _edges():
    K = _chunk()
    return [  # name, shape, layouts
        ("P=1, C=1283", (2, 1283, 1, 1), (False, True)),
        ("P=49: no vector width divides it", (2, 6, 7, 7), (False, True)),
        ("P=15: no vector width divides it", (3, 4, 3, 5), (False, True)),
        ("C=1 channels_last", (2, 1, 6, 6), (True,)),
        ("C=3 channels_last", (2, 3, 6, 6), (True,)),
        ("C=5 channels_last", (2, 5, 5, 7), (True,)),
        ("C=257 channels_last", (2, 257, 3, 3), (True,)),
        ("C=72 channels_last: two tiles of channel vectors", (2, 72, 5, 5), (True,)),
        ("a plane one element longer than a chunk", (1, 2, 1, K + 1), (False, True)),
        ("a plane of three chunks, the last ragged", (2, 3, 1, 2 * K + 40), (False, True)),
        ("a plane of exactly one chunk, 8 channels", (1, 8, 8, K // 8), (False, True)),
        ("B=65 with two channels", (65, 2, 2, 2), (False, True)),
        ("P=36: vectors of 4", (2, 7, 6, 6), (False, True)),
        ("C=12 channels_last: vectors of 4", (2, 12, 3, 3), (True,)),
    ]


@pytest.mark.parametrize("ei", range(14))
def test_edges_against_the_restatement(ei):
    """the smallest shapes at which the kernels take another path, with an upstream gradient of 3 and a log_scale spread over [-3, 8]"""
    name, shape, layouts = _edges()[ei]
    _cases, allow = vid_fixture.load()
    rng = np.random.default_rng(shape[1] * 1000 + shape[2] * 10 + shape[3])
    m = (np.round(rng.standard_normal(shape) * 32) / 32).astype(np.float32)
    t = (np.round(rng.standard_normal(shape) * 32) / 32 + 0.5).astype(np.float32)
    ls = np.linspace(-3, 8, shape[1]).astype(np.float32)
    want = V.nll(m, t, ls)
    ok = True
    for cl in layouts:
        ok &= check(f"{name} {'channels_last' if cl else 'NCHW'}", run_abi(m, t, ls, cl_m=cl, cl_t=cl, g_loss=3.0), want, allow, g_loss=3.0)
    assert ok


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cl", [False, True])
def test_offset_base_pointers(cl, dtype):
    """each side in turn starts one element behind an aligned address, C and P both multiples of 8: no 16-byte access is possible on
    that side, so the pair is walked element by element; then both sides"""
    _cases, allow = vid_fixture.load()
    rng = np.random.default_rng(23 + int(cl))
    m = (np.round(rng.standard_normal((2, 8, 4, 4)) * 32) / 32).astype(np.float32)
    t = (np.round(rng.standard_normal((2, 8, 4, 4)) * 32) / 32 + 0.25).astype(np.float32)
    ls = np.linspace(-2, 6, 8).astype(np.float32)
    want = V.nll(m, t, ls)
    ok = True
    for off_m, off_t in ((True, False), (False, True), (True, True)):
        got = run_abi(m, t, ls, cl_m=cl, cl_t=cl, dt_m=dtype, dt_t=dtype, off_m=off_m, off_t=off_t, g_loss=3.0)
        ok &= check(f"offset mean={int(off_m)} target={int(off_t)}", got, want, allow, g_loss=3.0, bf16_out=dtype == BF16)
    assert ok


@pytest.mark.parametrize("value", [-30.0, 30.0, 100.0])
def test_log_scale_extremes(value):
    """-30: var = eps to fp32; +30 and +100: the softplus is its argument; at +100 the reference's fp32 exp is inf, the kernels
    evaluate it in double and stay finite (the documented deviation)"""
    _cases, allow = vid_fixture.load()
    rng = np.random.default_rng(5)
    m = (np.round(rng.standard_normal((3, 6, 5, 5)) * 32) / 32).astype(np.float32)
    t = (np.round(rng.standard_normal((3, 6, 5, 5)) * 32) / 32).astype(np.float32)
    ls = np.full(6, value, np.float32)
    want = V.nll(m, t, ls)
    assert np.isfinite(want["loss"]) and np.isfinite(want["d_ls"]).all()
    ok = True
    for cl in (False, True):
        got = run_abi(m, t, ls, cl_m=cl, cl_t=cl)
        ok &= check(f"log_scale {value} cl={int(cl)}", got, want, allow)
        if value < 0:
            assert np.all(got["var"] == np.float64(np.float32(1e-5)))
        else:
            assert np.all(got["var"] == np.float64(np.float32(value + 1e-5)))
    op = run_op(m, t, ls)
    ok &= check(f"log_scale {value} op", op, want, allow, full=False)
    assert ok


def test_mean_equal_to_target():
    """S = 0, d_mean exactly 0, d_log_scale = 0.5 / C * sigmoid / var, finite"""
    _cases, allow = vid_fixture.load()
    rng = np.random.default_rng(6)
    m = rng.standard_normal((2, 5, 6, 6)).astype(np.float32)
    ls = np.linspace(-3, 8, 5).astype(np.float32)
    want = V.nll(m, m, ls)
    for cl in (False, True):
        got = run_abi(m, m, ls, cl_m=cl, cl_t=cl, g_loss=7.0)
        assert not got["S"].any() and not got["d_mean"].any() and np.isfinite(got["d_ls"]).all() and (got["d_ls"] > 0).all()
        assert check(f"mean == target cl={int(cl)}", got, want, allow, g_loss=7.0)


def test_upstream_gradient_scales_exactly():
    """g_loss is a device scalar: powers of two scale d_mean exactly, 0 gives exact zeros; through autograd likewise, and
    log_scale's gradient carries it too"""
    rng = np.random.default_rng(8)
    m = rng.standard_normal((3, 12, 7, 7)).astype(np.float32)
    t = rng.standard_normal((3, 12, 7, 7)).astype(np.float32)
    ls = np.linspace(-3, 8, 12).astype(np.float32)
    for cl, dt in ((False, F32), (True, F32), (False, BF16), (True, BF16)):
        one = run_abi(m, t, ls, cl_m=cl, cl_t=cl, dt_m=dt, dt_t=dt)
        for g in (0.5, 1024.0):
            got = run_abi(m, t, ls, cl_m=cl, cl_t=cl, dt_m=dt, dt_t=dt, g_loss=g)
            assert torch.equal(got["raw"]["d_mean"].float(), one["raw"]["d_mean"].float() * g), (cl, dt, g)
            assert torch.equal(got["raw"]["d_ls"], one["raw"]["d_ls"])
        zero = run_abi(m, t, ls, cl_m=cl, cl_t=cl, dt_m=dt, dt_t=dt, g_loss=0.0)
        assert not zero["raw"]["d_mean"].float().abs().sum().item()
    a, b = run_op(m, t, ls), run_op(m, t, ls, g_loss=1024.0)
    assert torch.equal(b["raw_d_mean"], a["raw_d_mean"] * 1024.0) and np.array_equal(b["d_ls"], a["d_ls"])
    from moma_amd import ops
    tm, tt, tl = torch.from_numpy(m).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(ls).cuda()
    with torch.no_grad():
        assert float(ops.vid_nll(tm, tt, tl)) == a["loss"]
    assert not ops.vid_nll(tm, tt, tl).requires_grad
    only_ls = ops.vid_nll(tm, tt, tl.clone().requires_grad_(True))            # log_scale alone wants a gradient
    assert only_ls.requires_grad
    with pytest.raises(TypeError):
        ops.vid_nll(tm.half(), tt.half(), tl)
    with pytest.raises(ValueError):
        ops.vid_nll(tm, tt[:, :, :, :6], tl)
    with pytest.raises(ValueError):
        ops.vid_nll(tm.permute(0, 1, 3, 2), tt.permute(0, 1, 3, 2), tl)       # dense, neither layout
    with pytest.raises(ValueError):
        ops.vid_nll(tm, tt.clone().requires_grad_(True), tl)


def test_two_calls_give_the_same_bits():
    for (shape, cl, dtype) in [((4, 112, 14, 14), False, F32), ((4, 40, 28, 28), True, BF16), ((3, 24, 56, 56), False, BF16),
                               ((2, 1280, 4, 4), True, F32), ((2, 200, 5, 5), False, F32)]:
        rng = np.random.default_rng(shape[1])
        m, t = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
        ls = np.linspace(-3, 8, shape[1]).astype(np.float32)
        a, b = run_abi(m, t, ls, cl_m=cl, cl_t=cl, dt_m=dtype, dt_t=dtype), run_abi(m, t, ls, cl_m=cl, cl_t=cl, dt_m=dtype, dt_t=dtype)
        for k in ("S", "var", "d_ls", "loss", "d_mean", "partials"):
            assert torch.equal(a["raw"][k], b["raw"][k]), (shape, k)
        o1, o2 = run_op(m, t, ls, 1e-5, cl, cl, dtype, dtype), run_op(m, t, ls, 1e-5, cl, cl, dtype, dtype)
        assert torch.equal(o1["raw_loss"], o2["raw_loss"]) and torch.equal(o1["raw_d_mean"], o2["raw_d_mean"])
        assert np.array_equal(o1["d_ls"], o2["d_ls"]) and o1["loss"] == a["loss"]


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.vid_nll with every buffer it allocates (partials, S, var, d log_scale, loss, d_mean) between NaN margins, at ragged
    shapes and both dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (shape, cl, dtype) in [((3, 5, 7, 7), False, F32), ((2, 24, 9, 9), True, BF16), ((2, 200, 5, 5), False, BF16),
                               ((5, 3, 10, 10), True, F32), ((1, 3, 1, _chunk() + 7), False, F32)]:
        rng = np.random.default_rng(shape[1] * 7 + shape[2])
        mf = torch.channels_last if cl else torch.contiguous_format
        a = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf)
        b = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf)
        ls = torch.linspace(-3, 8, shape[1], device="cuda")

        def run(wrap):
            x, y, s = wrap(a).requires_grad_(True), wrap(b), ls.clone().requires_grad_(True)
            loss = ops.vid_nll(x, y, s)
            (loss * 2.5).backward()
            return loss.detach().clone(), x.grad.clone(), s.grad.clone()

        plain = run(lambda t: t.clone(memory_format=torch.preserve_format))
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda t: t.clone(memory_format=torch.preserve_format) if cl else _in(guard, t))
            assert guard.check(f"vid_nll {shape}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def _criterion_of(c):
    from moma_amd.distiller_zoo import VIDLoss
    B, Cs, Ct, H, W = c["shape"]
    crit = VIDLoss(Cs, c["mid"], Ct)
    with torch.no_grad():
        for i, w in zip((0, 2, 4), c["w"]):
            crit.regressor[i].weight.copy_(torch.from_numpy(w).view_as(crit.regressor[i].weight))
        crit.log_scale.copy_(torch.from_numpy(c["log_scale"]))
    return crit.cuda()


def _count_calls(monkeypatch):
    from moma_amd import ops
    calls = []
    real = ops.vid_nll
    monkeypatch.setattr(ops, "vid_nll", lambda m, t, ls, eps=1e-5: (calls.append((m.dtype, t.dtype)), real(m, t, ls, eps))[1])
    return calls


def test_criterion_takes_the_kernels_or_the_composite(monkeypatch):
    """on GPU tensors: the kernels in fp32 and under bf16 autocast (the regressor's output arrives in bf16), in channels_last too;
    the composite for float16 storage and for a target that records a gradient; token lists are refused"""
    calls = _count_calls(monkeypatch)
    c = vid_fixture.load()[0][5]
    crit = _criterion_of(c)
    x, t = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["target"]).cuda()
    ref = float(crit.composite(crit.regressor(x), t))
    out = crit(x, t)
    assert calls == [(F32, F32)] and out.dtype == F32 and out.dim() == 0 and abs(float(out) - ref) < 1e-5 * abs(ref)
    with torch.autocast("cuda", dtype=BF16):
        out = crit(x, t.to(BF16))
    assert calls[1:] == [(BF16, BF16)] and out.dtype == F32 and abs(float(out) - ref) < 2e-2 * abs(ref)
    out = crit(x.contiguous(memory_format=torch.channels_last), t.contiguous(memory_format=torch.channels_last))
    assert len(calls) == 3 and abs(float(out) - ref) < 1e-5 * abs(ref)
    big = torch.from_numpy(np.repeat(np.repeat(c["x"], 2, axis=2), 2, axis=3)).cuda()          # pooled back to the grid first
    assert abs(float(crit(big, t)) - ref) < 1e-5 * abs(ref) and len(calls) == 4
    with torch.autocast("cuda", dtype=torch.float16):
        out = crit(x, t.half())
    assert len(calls) == 4 and out.dtype == F32 and abs(float(out) - ref) < 2e-2 * abs(ref)     # float16: the composite
    tg = t.clone().requires_grad_(True)
    crit(x, tg).backward()
    assert len(calls) == 4 and tg.grad is not None and bool(tg.grad.abs().sum() > 0)            # a target with a gradient: likewise
    with pytest.raises(ValueError, match="feature maps"):
        crit(torch.randn(2, 17, 24, device="cuda"), torch.randn(2, 17, 24, device="cuda"))


@pytest.mark.parametrize("ci", range(N_CASES))
def test_criterion_end_to_end_fp32(ci, monkeypatch):
    """the whole criterion on GPU tensors in fp32 -- pooling, regressor (stock convolutions), the kernels: the loss and the
    gradients of the input, the three weights and log_scale against the float64 chain, within the fixture's allowances"""
    calls = _count_calls(monkeypatch)
    cases, allow = vid_fixture.load()
    c = cases[ci]
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    crit = _criterion_of(c)
    x, t = torch.from_numpy(c["x"]).cuda().requires_grad_(True), torch.from_numpy(c["target"]).cuda()
    loss = crit(x, t)
    loss.backward()
    assert calls == [(F32, F32)]
    w = V.criterion(c["x"], c["target"], c["w"], c["log_scale"], c["eps"])
    print(f"case {ci} {c['shape']}")
    ok = _report("loss", abs(float(loss) - w["loss"]) / w["abs_terms"], allow["chain_loss"])
    ok &= _report("dx", rel(_np(x.grad), w["dx"]), allow["dx"])
    for i, k in enumerate((0, 2, 4)):
        ok &= _report(f"dw{i}", rel(_np(crit.regressor[k].weight.grad).reshape(w["dw"][i].shape), w["dw"][i]), allow["dw"])
    ok &= _report("d_log_scale", rel(_np(crit.log_scale.grad), w["d_ls"]), allow["dls"])
    assert ok


@pytest.mark.parametrize("ci", [1, 5, 6, 9, 10])
def test_criterion_end_to_end_bf16_autocast(ci, monkeypatch):
    """under bf16 autocast the regressor's convolutions run on the streaming kernel where ops.pwconv_fwd_native admits the shape
    (cases 5, 6, 9, 10) and the likelihood on bf16 maps.  Yardstick: the float64 chain over the bf16-rounded operands (input, target,
    weights).  Allowance: twice the distance the same module shows with its convolutions forced to stock F.conv2d, measured here"""
    from moma_amd.backbones import efficientnet as E
    calls = _count_calls(monkeypatch)
    c = vid_fixture.load()[0][ci]
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    xr, tr, wr = _r16(c["x"]), _r16(c["target"]), [_r16(w) for w in c["w"]]
    w = V.criterion(xr, tr, wr, c["log_scale"], c["eps"])

    def run():
        crit = _criterion_of(c)
        x = torch.from_numpy(xr.astype(np.float32)).cuda().requires_grad_(True)
        t = torch.from_numpy(tr.astype(np.float32)).cuda().to(BF16)
        with torch.autocast("cuda", dtype=BF16):
            loss = crit(x, t)
        loss.backward()
        return {"loss": abs(float(loss) - w["loss"]) / w["abs_terms"], "dx": rel(_np(x.grad), w["dx"]),
                "dw": max(rel(_np(crit.regressor[k].weight.grad).reshape(w["dw"][i].shape), w["dw"][i]) for i, k in enumerate((0, 2, 4))),
                "d_log_scale": rel(_np(crit.log_scale.grad), w["d_ls"])}

    native = run()
    monkeypatch.setattr(E, "_PW_FWD", "0")
    stock = run()
    assert calls == [(BF16, BF16)] * 2
    B, Cs, Ct, H, W = c["shape"]
    from moma_amd import ops
    print(f"case {ci} {c['shape']}: the streaming kernel admits the last convolution: {ops.pwconv_fwd_native(B, c['mid'], Ct, H * W)}")
    ok = True
    for k in native:
        print(f"  {k}: stock F.conv2d {stock[k]:.3e}")
        ok &= _report(k, native[k], 2 * max(stock[k], ULP32))
    assert ok


def _loop(extra, steps=1):
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    argv = ["--distill", "vid", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
            "--batch_size", "8", "--steps_per_epoch", str(steps), "-c", "1", "-d", "1", "-b", "1", "--learning_rate", "0.01",
            "--no_graph_teacher", *extra]
    opt = parse_option(argv)
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
    dev = torch.device("cuda", 0)
    opt.device = dev
    torch.manual_seed(31)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
    kd = criterion_list[2]
    before = {n: p.detach().clone() for n, p in kd.named_parameters()}
    feats = {}

    def keep(k):                                                            # the feature lists of the FIRST step
        def hook(_m, _i, out):
            if k not in feats:
                feats[k] = [f.detach().clone() for f in out[0]]
        return hook
    hooks = [m.register_forward_hook(keep(k)) for k, m in (("s", model_s), ("t", model_t))]
    loader = SyntheticLoader(steps, 8, 32, 4, 5, dev)
    opt.trace, opt.print_freq = [], 1000
    train_distill_moma(1, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    for h in hooks:
        h.remove()
    return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace], feats, before, kd


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='vid', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: every pair runs on the
    kernels; loss_kd is the restatement's value on the feature maps the two models produced in that step with the criteria as they
    were before it; the step moves every log_scale and regressor; the same step in channels_last under bf16 autocast hands the
    kernels bf16 maps and stays finite"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    calls = _count_calls(monkeypatch)
    _cases, allow = vid_fixture.load()
    losses, kds, feats, before, kd = _loop([])
    mid_s, mid_t = feats["s"][1:-1], feats["t"][1:-1]
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all()
    assert len(mid_s) >= 2 and calls == [(F32, F32)] * len(mid_s) and len(kd) == len(mid_s)
    want = [V.criterion(a.cpu().numpy(), b.cpu().numpy(), [before[f"{i}.regressor.{k}.weight"].cpu().numpy() for k in (0, 2, 4)],
                        before[f"{i}.log_scale"].cpu().numpy(), kd[i].eps) for i, (a, b) in enumerate(zip(mid_s, mid_t))]
    total, scale = sum(w["loss"] for w in want), sum(w["abs_terms"] for w in want)
    print("loss_kd: %.6e  restatement: %.6e" % (kds[0], total))
    # (the regressors are stock fp32 convolutions here: the chain allowance of the fixture, per pair)
    assert _report("loss_kd of the step", abs(kds[0] - total) / scale, allow["chain_loss"])
    after = dict(kd.named_parameters())
    assert all(not torch.equal(before[n], after[n]) for n in before)
    del calls[:]
    losses, kds, feats, _before, kd = _loop(["--channels_last", "--amp", "bf16"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all()
    print("bf16 / channels_last step: loss_kd %.6e, kernel calls %s" % (kds[0], calls))
    assert calls == [(BF16, BF16)] * len(kd)


def test_cli_runs_with_distill_vid(tmp_path):
    """`python train_student_moma.py --distill vid` on the smallest synthetic configuration: parses, builds, trains and validates"""
    from tests.test_gpu_cli import _run_cli
    r = _run_cli(tmp_path, ["--distill", "vid", "--dataset", "cifar100", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--n_cls", "4",
                            "--batch_size", "8",
                            "--epochs", "1", "--steps_per_epoch", "2"], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout and "nan" not in r.stdout.lower()

"""GPU tests of the Neuron Selectivity Transfer kernels (csrc/nst.hip) through the C ABI, ops.nst_loss, the criterion and the
training loop.

Yardstick: the float64 evaluation of the formulas (tests/nst_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_loss / _grad / _gram`) that the reference's own fp32 results keep from that evaluation over the
cases of the golden fixture, never below one fp32 ulp (2^-23, relative): a different but equally valid fp32 summation order can land
on the other side of the float64 value.  Metric: crd_ref.rel (units of the yardstick's largest element); the scalars relative to
t1 + 2 t2 (the loss is their difference and crosses zero).  G and the norms take the `gram` allowance, the rows' sums of squares
twice that (a sum of squares of entries of G, none above 1), t1 and t2 the `loss` allowance of their own value.
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nst_fixture, nst_ref as N
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


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


def _place(guard, f, dtype=F32, cl=False, offset=False):
    """numpy [B,C,H,W] -> a device tensor of that logical shape between NaN margins: contiguous or channels_last, optionally
    starting one element behind an aligned address (a slice of a larger buffer: no 16-byte access is possible)"""
    t = torch.from_numpy(np.ascontiguousarray(f)).to(dtype)
    B, Cc, H, W = t.shape
    flat = guard.empty(t.numel() + int(offset), device="cuda", dtype=dtype)
    if offset:
        flat[0] = float("nan")
        flat = flat[1:]
    out = flat.view(B, H, W, Cc).permute(0, 3, 1, 2) if cl else flat.view(B, Cc, H, W)
    out.copy_(t)
    return out


def _codes(t, cl):
    from moma_amd import _lib as L
    return (L.DT_BF16 if t.dtype == BF16 else L.DT_F32), (L.LAYOUT_NHWC if cl else L.LAYOUT_NCHW)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def run_abi(f_s, f_t, cl_s=False, cl_t=False, dt_s=F32, dt_t=F32, offset=False, g_loss=1.0):
    """moma_nst_gram -> moma_nst_bwd on fresh guarded buffers.  f_s, f_t: numpy on a common grid.  -> dict of numpy float64 arrays
    G, norms, rows, terms, loss, dF_s, and the raw device tensors under `raw`"""
    from moma_amd import _lib as L
    lib, guard = _lib(), _Guarded()
    B, Cs, H, W = f_s.shape
    Ct, P = f_t.shape[1], H * W
    ts, tt = _place(guard, f_s, dt_s, cl_s, offset), _place(guard, f_t, dt_t, cl_t, offset)
    e = lambda *shape: guard.empty(*shape, device="cuda", dtype=F32)          # noqa: E731
    nws = lib.moma_nst_workspace_bytes(B, Cs, Ct)
    assert nws == B * Cs * (Cs + Ct) * 4
    G, norms, rows = e(B, Cs, Cs + Ct), e(B, Cs + Ct), e(B, Cs, 2)
    partials, terms, loss = e(B, -(-Cs // L.NST_ROW_BLOCK), 2), e(2), e(1)
    codes = (*_codes(ts, cl_s), *_codes(tt, cl_t))
    rc = lib.moma_nst_gram(_p(ts), _p(tt), B, Cs, Ct, P, *codes, _p(G), nws, _p(norms), _p(rows), _p(partials), _p(terms), _p(loss), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    flat = guard.empty(ts.numel() + int(offset), device="cuda", dtype=dt_s)
    flat = flat[1:] if offset else flat
    dF = flat.as_strided(ts.shape, ts.stride())                               # dtype and layout of f_s
    rc = lib.moma_nst_bwd(_p(ts), _p(tt), _p(G), nws, _p(norms), _p(rows), _p(gl), _p(dF), B, Cs, Ct, P, *codes, _st())
    assert rc == 0, rc
    assert guard.check("nst C ABI") > 0                                       # every margin untouched
    raw = {"G": G, "norms": norms, "rows": rows, "partials": partials, "terms": terms, "loss": loss, "dF_s": dF}
    out = {k: _np(v) for k, v in raw.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out["loss"] = float(loss.item())
    out["raw"] = raw
    return out


def run_op(f_s, f_t, cl_s=False, cl_t=False, dt_s=F32, dt_t=F32, g_loss=1.0):
    from moma_amd import ops
    mk = lambda f, cl, dt: torch.from_numpy(np.ascontiguousarray(f)).to(dt).cuda().contiguous(    # noqa: E731
        memory_format=torch.channels_last if cl else torch.contiguous_format)
    ts, tt = mk(f_s, cl_s, dt_s).requires_grad_(True), mk(f_t, cl_t, dt_t)
    loss = ops.nst_loss(ts, tt)
    (loss * g_loss).backward()
    assert ts.grad.stride() == ts.stride() and ts.grad.dtype == dt_s and tt.grad is None
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    return loss.detach(), ts.grad


def check(tag, got, want, allow, full=True, grad_scale=None):
    """grad_scale: what the gradient's error is measured in where the gradient itself vanishes (default: its largest element)"""
    scale = want["t1"] + 2 * want["t2"]
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / scale, allow["loss"])
    if grad_scale is None:
        ok &= _report(f"{tag} dF_s", rel(got["dF_s"], want["dF_s"]), allow["grad"])
    else:
        ok &= _report(f"{tag} dF_s (of the sum's terms)", np.abs(got["dF_s"] - want["dF_s"]).max() / grad_scale, allow["grad"])
    if full:
        ok &= _report(f"{tag} G", rel(got["G"], want["G"]), allow["gram"])
        ok &= _report(f"{tag} norms", rel(got["norms"], want["norms"]), allow["gram"])
        ok &= _report(f"{tag} rows", rel(got["rows"], want["rows"]), 2 * allow["gram"])
        ok &= _report(f"{tag} t1", abs(got["terms"][0] - want["t1"]) / want["t1"], allow["loss"])
        ok &= _report(f"{tag} t2", abs(got["terms"][1] - want["t2"]) / want["t2"], allow["loss"])
    return ok


_WANT = {}


def fixture_case(ci):
    """(case, the pair on its common grid (stock pooling of the student where the heights differ), float64 results of the whole
    pair, float64 results on the common grid) -- evaluated once, shared by the tests"""
    cases, allow = nst_fixture.load()
    if ci not in _WANT:
        c = cases[ci]
        f_s = c["f_s"]
        Hs, Ht = c["shape"][3], c["shape"][5]
        if Hs > Ht:
            f_s = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(f_s), (Ht, Ht)).numpy()
        want = N.pair(c["f_s"], c["f_t"])
        _WANT[ci] = (f_s, want, want if Hs == Ht else N.pair(f_s, c["f_t"]))
    return (cases[ci], *_WANT[ci], allow)


N_CASES = 10


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    c, f_s, want, want_grid, allow = fixture_case(ci)
    print(f"case {ci} {c['shape']}")
    abi = run_abi(f_s, c["f_t"])
    ok = check("abi", abi, want_grid, allow)
    if c["shape"][3] == c["shape"][5]:          # the all-zero row: exactly zero, nothing undefined
        assert not abi["dF_s"][0, 1].any() and not abi["G"][0, 1].any() and not abi["G"][0, :, 1].any() and abi["norms"][0, 1] == np.float32(1e-12)
    loss, dF_s = run_op(c["f_s"], c["f_t"])
    op = {"loss": float(loss), "dF_s": _np(dF_s)}
    ok &= check("op", op, want, allow, full=False)
    assert np.isfinite(op["dF_s"]).all() and not op["dF_s"][0, 1].any()
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    scale = want["t1"] + 2 * want["t2"]
    ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / scale, allow["loss"] + c["ref_vs_f64_loss"])
    ok &= _report("op dF_s vs reference", rel(op["dF_s"], c["dF_s"]), allow["grad"] + c["ref_vs_f64_grad"])
    assert ok


@pytest.mark.parametrize("ci", range(N_CASES))
def test_layouts_agree(ci):
    """f_s and / or f_t in channels_last: the same results as the NCHW run, within the allowance (of the float64 value, and of
    each other: two equally valid fp32 orders)"""
    c, f_s, want, want_grid, allow = fixture_case(ci)
    scale = want["t1"] + 2 * want["t2"]
    l0, d0 = run_op(c["f_s"], c["f_t"])
    ok = True
    for cl_s, cl_t in ((True, False), (False, True), (True, True)):
        loss, dF = run_op(c["f_s"], c["f_t"], cl_s, cl_t)
        tag = f"case {ci} cl_s={int(cl_s)} cl_t={int(cl_t)}"
        ok &= check(tag, {"loss": float(loss), "dF_s": _np(dF)}, want, allow, full=False)
        ok &= _report(tag + " loss vs NCHW", abs(float(loss) - float(l0)) / scale, 2 * allow["loss"])
        ok &= _report(tag + " dF_s vs NCHW", rel(_np(dF), _np(d0)), 2 * allow["grad"])
        ok &= check(tag + " abi", run_abi(f_s, c["f_t"], cl_s, cl_t), want_grid, allow)
    assert ok


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("ci", range(N_CASES))
def test_bf16_storage(ci, cl):
    """inputs rounded to bf16: the run on bf16 tensors does the arithmetic of the run on the fp32 copy of the same values (fp32
    products and sums either way) -- G, norms, row sums, terms and loss are the same bits, and dF in bf16 is that run's fp32 dF
    rounded once, bit for bit; either side alone in bf16 likewise"""
    c, f_s, _want, _wg, _allow = fixture_case(ci)
    r = lambda f: _np(torch.from_numpy(np.ascontiguousarray(f)).to(BF16))          # noqa: E731
    f_s, f_t = r(f_s), r(c["f_t"])
    f = run_abi(f_s, f_t, cl, cl, F32, F32)
    for dt_s, dt_t in ((BF16, BF16), (BF16, F32), (F32, BF16)):
        b = run_abi(f_s, f_t, cl, cl, dt_s, dt_t)
        for k in ("G", "norms", "rows", "partials", "terms", "loss"):
            assert torch.equal(b["raw"][k], f["raw"][k]), (k, dt_s, dt_t)
        assert b["raw"]["dF_s"].dtype == dt_s and torch.equal(b["raw"]["dF_s"], f["raw"]["dF_s"].to(dt_s)), (dt_s, dt_t)
    # the op on bf16 tensors: the same bits as the C ABI sequence
    lb, db = run_op(f_s, f_t, cl, cl, BF16, BF16)
    b = run_abi(f_s, f_t, cl, cl, BF16, BF16)
    assert db.dtype == BF16 and float(lb) == b["loss"] and torch.equal(db, b["raw"]["dF_s"])


EDGES = [  # name, f_s shape, f_t shape, offset pointer
    ("B=1", (1, 5, 6, 6), (1, 7, 6, 6), False),
    ("C=1", (2, 1, 5, 5), (2, 1, 5, 5), False),
    ("P=1", (3, 8, 1, 1), (3, 4, 1, 1), False),
    ("Cs=256 (the cap)", (2, 256, 4, 4), (2, 8, 4, 4), False),
    ("Ct=256 with Cs=8", (2, 8, 4, 4), (2, 256, 4, 4), False),
    ("both at the cap, ragged P", (1, 256, 3, 3), (1, 256, 3, 3), False),
    ("P=49 offset pointer", (2, 6, 7, 7), (2, 6, 7, 7), True),
    ("P=64 offset pointer", (2, 8, 8, 8), (2, 12, 8, 8), True),
    ("P=31 (below two K-tiles)", (2, 5, 1, 31), (2, 9, 1, 31), False),
    ("P=33 (above two K-tiles)", (2, 5, 3, 11), (2, 9, 3, 11), False),
    ("P=65 (a second pixel tile of one pixel)", (2, 6, 5, 13), (2, 7, 5, 13), False),
    ("Cs=33 (just above one row block)", (2, 33, 4, 4), (2, 16, 4, 4), False),
    ("Cs=17, Ct=15 (slabs of 16 channels, ragged)", (2, 17, 6, 6), (2, 15, 6, 6), False),
    ("P=144: two fp32 chains", (2, 12, 12, 12), (2, 20, 12, 12), False),
    ("Cs + Ct = 160: more slabs than one fp32 chain", (1, 96, 6, 6), (1, 64, 6, 6), False),
    # 224 padded rows leave slabs of 32 pixels: P = 63 is two slabs, and neither P nor C allows a 16-byte load in either layout
    ("P=63 in two slabs, element loads", (2, 101, 7, 9), (2, 99, 7, 9), False),
    ("P=63 in two slabs, offset pointer", (2, 100, 7, 9), (2, 100, 7, 9), True),
]


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_edges_against_the_restatement(edge, cl):
    """the smallest shapes at which the kernels take another path, with an upstream gradient of 3"""
    name, ss, st, offset = edge
    _cases, allow = nst_fixture.load()
    rng = np.random.default_rng(ss[1] * 1000 + st[1] * 10 + ss[3])
    f_s = (np.round(rng.standard_normal(ss) * 32) / 32).astype(np.float32)
    f_t = (np.round(rng.standard_normal(st) * 32) / 32 + 0.5).astype(np.float32)
    want = N.pair(f_s, f_t, g_loss=3.0)
    got = run_abi(f_s, f_t, cl, cl, F32, F32, offset, g_loss=3.0)
    grad_scale = None
    if ss[2] * ss[3] == 1:
        # one pixel: every entry of G is +-1 whatever the inputs, the loss is constant and dX_i = (a Cs - c Ct - r_i) X_i / n_i^2 is
        # a total cancellation -- in float64 it leaves 1e-17, in any fp32 order its rounding.  Measured against the terms that cancel
        n = want["norms"][:, :ss[1]]
        grad_scale = 3.0 * ((4.0 / (ss[0] * ss[1])) * 2 / n).max()
        assert np.abs(want["dF_s"]).max() < 1e-12 * grad_scale
    assert check(f"{name} {'channels_last' if cl else 'NCHW'}", got, want, allow, grad_scale=grad_scale)


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("shapes", [((2, 6, 7, 7), (2, 6, 7, 7)), ((2, 100, 7, 9), (2, 100, 7, 9))], ids=["one slab", "two slabs"])
def test_bf16_behind_an_offset_pointer(shapes, cl):
    """bf16 maps that start one element (2 bytes) behind an aligned address, extents that would otherwise allow 16-byte loads
    (C = 100 in channels_last) included: element loads and stores of 2 bytes.  Values exact in bf16, so the fp32 run from the same
    offset is the same arithmetic: equal bits, dF rounded once; and that run is within the allowance of the restatement"""
    ss, st = shapes
    _cases, allow = nst_fixture.load()
    rng = np.random.default_rng(ss[1] + 17)
    f_s = (np.round(rng.standard_normal(ss) * 32) / 32).astype(np.float32)
    f_t = (np.round(rng.standard_normal(st) * 32) / 32 + 0.5).astype(np.float32)
    f = run_abi(f_s, f_t, cl, cl, F32, F32, offset=True)
    assert check(f"fp32 {ss} {'channels_last' if cl else 'NCHW'}", f, N.pair(f_s, f_t), allow)
    for dt_s, dt_t in ((BF16, BF16), (BF16, F32), (F32, BF16)):
        b = run_abi(f_s, f_t, cl, cl, dt_s, dt_t, offset=True)
        for k in ("G", "norms", "rows", "partials", "terms", "loss"):
            assert torch.equal(b["raw"][k], f["raw"][k]), (k, dt_s, dt_t)
        assert b["raw"]["dF_s"].dtype == dt_s and torch.equal(b["raw"]["dF_s"], f["raw"]["dF_s"].to(dt_s)), (dt_s, dt_t)


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.nst_loss with every buffer it allocates (G, norms, row sums, partials, terms, loss, dF) between NaN margins, at ragged
    shapes and both dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (ss, st, cl, dtype) in [((3, 5, 7, 7), (3, 9, 7, 7), False, F32), ((2, 24, 9, 9), (2, 40, 9, 9), True, BF16),
                                ((2, 200, 5, 5), (2, 24, 5, 5), False, BF16), ((5, 3, 10, 10), (5, 6, 5, 5), True, F32)]:
        rng = np.random.default_rng(ss[1] * 7 + st[1])
        mf = torch.channels_last if cl else torch.contiguous_format
        a = torch.from_numpy(rng.standard_normal(ss).astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf)
        b = torch.from_numpy(rng.standard_normal(st).astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf)

        def run(wrap):
            x, y = wrap(a).requires_grad_(True), wrap(b)
            loss = ops.nst_loss(x, y)
            (loss * 2.5).backward()
            return loss.detach().clone(), x.grad.clone()

        plain = run(lambda t: t.clone(memory_format=torch.preserve_format))
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda t: t.clone(memory_format=torch.preserve_format) if cl else _in(guard, t))
            assert guard.check(f"nst_loss {ss} {st}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_two_calls_give_the_same_bits():
    for (ss, st, cl, dtype) in [((4, 112, 14, 14), (4, 112, 14, 14), False, F32), ((4, 40, 28, 28), (4, 40, 28, 28), True, BF16),
                                ((3, 24, 56, 56), (3, 24, 56, 56), False, F32), ((2, 200, 4, 4), (2, 136, 4, 4), True, F32)]:
        rng = np.random.default_rng(ss[1])
        f_s, f_t = rng.standard_normal(ss).astype(np.float32), rng.standard_normal(st).astype(np.float32)
        l1, d1 = run_op(f_s, f_t, cl, cl, dtype, dtype)
        l2, d2 = run_op(f_s, f_t, cl, cl, dtype, dtype)
        assert torch.equal(l1, l2) and torch.equal(d1, d2)


def test_upstream_gradient_and_gradient_scope(monkeypatch):
    """the upstream gradient is a device scalar: (3 loss).backward() gives the restatement's dF at g_loss = 3; no gradient where none
    is wanted; mixed dtypes and layouts per side; a layout that is neither contiguous nor channels_last is copied first; float16 is
    refused by the op; a teacher map that wants a gradient is refused by the op and routed to the composite by the criterion"""
    from moma_amd import ops
    from moma_amd.distiller_zoo import NSTLoss
    _cases, allow = nst_fixture.load()
    rng = np.random.default_rng(11)
    f_s = (np.round(rng.standard_normal((3, 12, 8, 8)) * 32) / 32).astype(np.float32)
    f_t = (np.round(rng.standard_normal((3, 20, 8, 8)) * 32) / 32).astype(np.float32)
    want1, want3 = N.pair(f_s, f_t), N.pair(f_s, f_t, g_loss=3.0)
    scale = want1["t1"] + 2 * want1["t2"]
    l1, d1 = run_op(f_s, f_t)
    l3, d3 = run_op(f_s, f_t, g_loss=3.0)
    ok = check("g = 1", {"loss": float(l1), "dF_s": _np(d1)}, want1, allow, full=False)
    ok &= check("g = 3", {"loss": float(l3), "dF_s": _np(d3)}, want3, allow, full=False)
    ok &= _report("dF(3) vs 3 dF(1)", rel(_np(d3), 3 * _np(d1)), 2 * allow["grad"])
    # student bf16 channels_last against a teacher in fp32 NCHW (values exact in bf16: multiples of 1/32)
    lm, dm = run_op(f_s, f_t, cl_s=True, cl_t=False, dt_s=BF16, dt_t=F32)
    ok &= _report("mixed dtypes loss", abs(float(lm) - want1["loss"]) / scale, allow["loss"])
    assert ok and torch.equal(dm, d1.to(BF16).contiguous(memory_format=torch.channels_last))
    ts, tt = torch.from_numpy(f_s).cuda(), torch.from_numpy(f_t).cuda()
    with torch.no_grad():
        assert float(ops.nst_loss(ts, tt)) == float(l1)
    assert not ops.nst_loss(ts, tt).requires_grad                              # nobody wants a gradient: nothing is saved
    odd = ts.permute(0, 1, 3, 2)                                               # dense, neither layout
    assert not odd.is_contiguous() and not odd.is_contiguous(memory_format=torch.channels_last)
    w2 = N.pair(np.ascontiguousarray(f_s.transpose(0, 1, 3, 2)), np.ascontiguousarray(f_t.transpose(0, 1, 3, 2)))
    assert _report("permuted input", abs(float(ops.nst_loss(odd, tt.permute(0, 1, 3, 2))) - w2["loss"]) / scale, allow["loss"])
    with pytest.raises(TypeError):
        ops.nst_loss(tt.half(), tt.half())
    with pytest.raises(ValueError):
        ops.nst_loss(tt, torch.zeros(3, 4, 8, 6, device="cuda"))
    # a teacher that wants a gradient
    tg = tt.clone().requires_grad_(True)
    with pytest.raises(ValueError):
        ops.nst_loss(ts, tg)
    calls = []
    real = ops.nst_loss
    monkeypatch.setattr(ops, "nst_loss", lambda a, b: (calls.append(1), real(a, b))[1])
    sg = ts.clone().requires_grad_(True)
    (loss,) = NSTLoss()([sg], [tg])
    loss.backward()
    assert not calls and tg.grad is not None and bool(torch.isfinite(tg.grad).all()) and bool(tg.grad.abs().sum() > 0)
    ok = _report("composite loss", abs(float(loss) - want1["loss"]) / scale, allow["loss"])
    ok &= _report("composite dF_s", rel(_np(sg.grad), want1["dF_s"]), allow["grad"])
    s64, t64 = ts.double().cpu().requires_grad_(True), tt.double().cpu().requires_grad_(True)
    NSTLoss().composite(s64, t64).backward()
    ok &= _report("composite dF_t", rel(_np(tg.grad), t64.grad.numpy()), allow["grad"])
    assert ok


def test_criterion_takes_the_kernels_on_gpu_tensors(monkeypatch):
    from moma_amd import ops
    from moma_amd.distiller_zoo import NSTLoss
    calls = []
    real = ops.nst_loss
    monkeypatch.setattr(ops, "nst_loss", lambda a, b: (calls.append(1), real(a, b))[1])
    x, y = torch.randn(2, 8, 6, 6, device="cuda"), torch.randn(2, 4, 3, 3, device="cuda")
    crit = NSTLoss()
    out = crit([x, x.to(BF16)], [y, y])
    assert len(out) == 2 and len(calls) == 2 and all(o.dtype == F32 and o.dim() == 0 for o in out)
    ref = float(crit.composite(x, y))
    assert abs(float(out[0]) - ref) < 1e-5 * max(abs(ref), 1e-2)
    crit([x.half()], [y.half()])                                             # float16 storage: the stock-torch composite
    wide = torch.randn(2, 257, 3, 3, device="cuda")
    o1, o2 = crit([wide], [y])[0], crit([y], [wide])[0]                      # more than 256 channels on either side: likewise
    assert len(calls) == 2 and bool(torch.isfinite(o1)) and bool(torch.isfinite(o2))
    crit([torch.randn(2, 256, 3, 3, device="cuda")], [y])                    # the cap itself is served
    assert len(calls) == 3
    with pytest.raises(ValueError):
        crit([torch.randn(2, 17, 32, device="cuda")], [y])


def _loop(extra, steps=5):
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    argv = ["--distill", "nst", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
            "--batch_size", "8", "--steps_per_epoch", str(steps), "-c", "1", "-d", "1", "-b", "50", "--learning_rate", "0.01",
            "--no_graph_teacher", *extra]
    opt = parse_option(argv)
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
    dev = torch.device("cuda", 0)
    opt.device = dev
    torch.manual_seed(31)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
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
    return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace], feats


def test_five_eager_steps_of_the_loop(monkeypatch):
    """train_distill_moma with distill='nst', beta 50, resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: the pairs run on
    the kernels; loss_kd of step 1 is the restatement's value on the feature maps the two models produced in that step (stock
    torch on the device, moved to numpy); every loss is finite and the KD term does not grow; the same run in channels_last under
    bf16 autocast completes with finite losses"""
    from moma_amd import ops
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    calls = []
    real = ops.nst_loss
    monkeypatch.setattr(ops, "nst_loss", lambda a, b: (calls.append(1), real(a, b))[1])
    _cases, allow = nst_fixture.load()
    losses, kds, feats = _loop([])
    assert len(kds) == 5 and np.isfinite(kds).all() and np.isfinite(losses).all()
    mid_s, mid_t = feats["s"][1:-2], feats["t"][1:-2]
    assert len(mid_s) >= 2 and len(calls) == 5 * len(mid_s) and all(f.dim() == 4 and f.dtype == F32 for f in mid_s)
    pairs = [N.pair(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(mid_s, mid_t)]
    want, scale = sum(w["loss"] for w in pairs), sum(w["t1"] + 2 * w["t2"] for w in pairs)
    print("loss_kd per step:", " ".join(f"{v:.6e}" for v in kds), " restatement of step 1: %.6e" % want)
    assert _report("loss_kd of step 1", abs(kds[0] - want) / scale, allow["loss"])
    assert kds[-1] <= kds[0] + 0.05 * scale                                  # decreasing, or stable within 5 % of the terms
    losses, kds, feats = _loop(["--channels_last", "--amp", "bf16"])
    assert len(kds) == 5 and np.isfinite(kds).all() and np.isfinite(losses).all()
    mid = feats["s"][1:-2]
    print("bf16 / channels_last run: feature dtypes", [f.dtype for f in mid], "loss_kd", " ".join(f"{v:.6e}" for v in kds))
    assert all(f.dtype == BF16 for f in mid)                                 # the maps reach the kernels at 2 bytes

"""GPU tests of `--distill semckd`: the grouped weighted-MSE kernels (csrc/semckd.hip) and moma_sp_gram_sum through the C ABI, through
ops.semckd_weighted_mse / ops.batch_gram, SelfA.loss and the training loop.

Yardstick: the float64 evaluation of the formulas (tests/semckd_ref.py).  Allowance for a floating-point result of a recorded case:
TWICE the largest distance of that kind (`ref_vs_f64_<kind>`) that the reference's own fp32 results keep from float64 over the cases
of the golden fixture, never below one fp32 ulp (2^-23, relative); metric crd_ref.rel (units of the yardstick's largest element), the
loss relative to its own value (a sum of squares).  The edge cases use inputs that are multiples of 1/32 up to 4: there x - t and its
square are exact in fp32, so ind, loss and dx are ONE rounding of a double away from the restatement -- one fp32 ulp is the bound.  A
gradient stored in bf16 adds that rounding: half a bf16 ulp (8 significant bits), at most 2^-8 of the element.
Every call through the C ABI runs on buffers between guard margins (tests/test_gpu_guard.py): the margins must be untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from moma_amd.distiller_zoo import SelfA, SemCKDLoss  # noqa: F401  (the modules under test)
from tests import semckd_fixture, semckd_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded, _in

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8
N_CASES = semckd_fixture.N_CASES


def _L():
    from moma_amd import _lib as L
    return L


def _lib():
    return _L().load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(name, got, allowed):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e}, ratio {got / allowed:.2f})")
    return got <= allowed


def _np(t):
    return t.float().cpu().numpy().astype(np.float64) if t.dtype != torch.float64 else t.cpu().numpy()


def _r(a, dtype):
    """numpy -> the same values rounded to `dtype`, as float64"""
    return _np(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype))


def _draw(rng, shape):
    return np.clip(np.round(rng.standard_normal(shape) * 32) / 32, -4, 4)


def _weights(rng, shape):
    """attention-like weights in [0, 1) that are exact in fp32 (the restatement reads the very values the kernels do)"""
    return rng.random(shape).astype(np.float32).astype(np.float64)


def _place(guard, a, dtype, offset=False):
    """the rows of a [B, n] (or [B, ...]) array in storage order between guard margins, optionally one element behind an aligned address"""
    flat = guard.empty(a.size + int(offset), device="cuda", dtype=dtype)
    flat = flat[1:] if offset else flat
    flat.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(dtype))
    return flat


def run_abi(xs, ts, w, S, g=1.0, dt_x=None, dt_t=None, offset=False, no_dx=(), canary=None):
    """moma_semckd_fwd + moma_semckd_bwd on guarded buffers.  xs[p], ts[p]: [B, n_p] arrays; dt_x / dt_t: dtype per pair (default
    fp32) -> dict(ind, loss, dx (list; None where not asked), raw (the device tensors, for bit comparisons))"""
    L, lib, guard = _L(), _lib(), _Guarded()
    P, B = len(xs), len(xs[0])
    dt_x, dt_t = dt_x or [F32] * P, dt_t or [F32] * P
    X = [_place(guard, x, d, offset) for x, d in zip(xs, dt_x)]
    T_ = [_place(guard, t, d, offset) for t, d in zip(ts, dt_t)]
    DX = [None if p in no_dx else guard.empty(xs[p].size + int(offset), device="cuda", dtype=dt_x[p])[int(offset):] for p in range(P)]
    for d in DX:
        if d is not None and canary is not None:
            d.fill_(canary)
    code = lambda d: L.DT_BF16 if d == BF16 else L.DT_F32          # noqa: E731
    tab = (L.SemckdPair * P)()
    for p in range(P):
        tab[p] = L.SemckdPair(X[p].data_ptr(), T_[p].data_ptr(), 0 if DX[p] is None else DX[p].data_ptr(), xs[p].size // B,
                              code(dt_x[p]), code(dt_t[p]))
    wd = _place(guard, w, F32)
    gd = _place(guard, np.array([g]), F32)
    n = lib.moma_semckd_workspace_bytes(tab, P, B)
    assert n == 8 * B * sum(-(-(x.size // B) // L.SEMCKD_CHUNK) for x in xs)
    ws = guard.empty(n // 8, device="cuda", dtype=torch.float64)
    ind, loss = guard.empty(B * P, device="cuda", dtype=F32), guard.empty(1, device="cuda", dtype=F32)
    assert lib.moma_semckd_fwd(tab, P, S, B, _p(wd), _p(ws), n, _p(ind), _p(loss), _st()) == 0
    assert lib.moma_semckd_bwd(tab, P, S, B, _p(wd), _p(gd), _st()) == 0
    assert guard.check("moma_semckd_fwd / _bwd") > 0
    return {"ind": _np(ind).reshape(B, S, P // S), "loss": float(loss.item()),
            "dx": [None if d is None else _np(d).reshape(xs[p].shape) for p, d in enumerate(DX)],
            "raw": [ind.clone(), loss.clone()] + [d.clone() for d in DX if d is not None]}


def _dev_lists(xs, ts, S, dt_x, dt_t, cl=False):
    P = len(xs)
    T = P // S
    mf = torch.channels_last if cl else torch.contiguous_format
    X = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(d).cuda().contiguous(memory_format=mf).requires_grad_(True)
         for x, d in zip(xs, dt_x)]
    T_ = [torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(d).cuda().contiguous(memory_format=mf) for t, d in zip(ts, dt_t)]
    return X, T_, [X[i * T:(i + 1) * T] for i in range(S)], [T_[i * T:(i + 1) * T] for i in range(S)]


def run_op(xs, ts, w, S, g=1.0, dt_x=None, dt_t=None, cl=False):
    """ops.semckd_weighted_mse on [B,C,h,w] maps (contiguous or channels_last) + backward of g * loss"""
    from moma_amd import ops
    P = len(xs)
    dt_x, dt_t = dt_x or [F32] * P, dt_t or [F32] * P
    X, _T, s_values, targets = _dev_lists(xs, ts, S, dt_x, dt_t, cl)
    wd = torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda().requires_grad_(True)
    loss, ind = ops.semckd_weighted_mse(s_values, targets, wd)
    assert loss.dtype == F32 and loss.dim() == 0 and ind.dtype == F32 and tuple(ind.shape) == tuple(w.shape) and not ind.requires_grad
    (loss * g).backward()
    assert all(x.grad.dtype == x.dtype and x.grad.stride() == x.stride() for x in X)
    return {"ind": _np(ind), "loss": float(loss.item()), "dx": [_np(x.grad) for x in X], "dw": _np(wd.grad),
            "raw": [ind.detach().clone(), loss.detach().clone()] + [x.grad.clone() for x in X] + [wd.grad.clone()]}


def check(tag, got, want, allow, bf16_dx=()):
    """ind, loss, dx (and dw where the op gave it) against the restatement `want`, each within its allowance"""
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / max(want["loss"], 1e-300), allow["loss"]) if want["loss"] > 0 \
        else got["loss"] == 0.0
    ok &= _report(f"{tag} ind", rel(got["ind"], want["ind"]), allow["ind"]) if want["ind"].max() > 0 else not got["ind"].any()
    if "dw" in got:
        ok &= _report(f"{tag} dw", rel(got["dw"], want["dw"]), allow["dw"]) if np.abs(want["dw"]).max() > 0 else not got["dw"].any()
    for p, (a, b) in enumerate(zip(got["dx"], want["dx"])):
        if a is None:
            continue
        assert np.isfinite(a).all(), (tag, p)
        scale = np.abs(b).max()
        bound = allow["dsv"] * scale + (HALF_ULP_BF16 * np.abs(b) if p in bf16_dx else 0.0)
        worst = float((np.abs(a - b) / np.maximum(bound, 1e-300)).max()) if scale > 0 else float(np.abs(a).max() > 0)
        if worst > 1.0:
            print(f"  {tag} dx[{p}]: {worst:.2f} x the allowance")
            ok = False
    return bool(ok)


ONE_ULP = {"loss": ULP32, "ind": ULP32, "dsv": ULP32, "dw": 2 * ULP32}      # (dw = ind * (g / (B S)): two fp32 roundings)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """the recorded s_value, target and weight of every pair: ABI and op against the float64 restatement AND against the reference's
    own fp32 results, each side within its allowance"""
    cases, allow = semckd_fixture.load()
    c = cases[ci]
    S = len(c["stu"])
    want = V.tail(c["s_value"], c["target"], c["weight"])
    ref = {"loss": c["loss"], "ind": c["ind"].astype(np.float64), "dx": [d.astype(np.float64) for d in c["dsv"]],
           "dw": c["dw"].astype(np.float64)}
    flat = lambda a: [v.reshape(len(v), -1) for v in a]          # noqa: E731
    abi = run_abi(flat(c["s_value"]), flat(c["target"]), c["weight"], S)
    abi["dx"] = [d.reshape(s.shape) for d, s in zip(abi["dx"], c["s_value"])]
    op = run_op(c["s_value"], c["target"], c["weight"], S)
    ok = check("abi vs float64", abi, want, allow) & check("abi vs reference", abi, ref, allow)
    ok &= check("op vs float64", op, want, allow) & check("op vs reference", op, ref, allow)
    assert ok
    assert op["loss"] == abi["loss"] and np.array_equal(op["ind"], abi["ind"])
    assert all(np.array_equal(a, b) for a, b in zip(op["dx"], abi["dx"]))


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("dts", [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)], ids=["f32_f32", "bf16_bf16", "bf16_f32", "f32_bf16"])
@pytest.mark.parametrize("ci", [0, 2])
def test_bf16_per_side_and_both_memory_formats(ci, dts, cl):
    """the recorded pairs with either side stored in bf16, in both memory formats, through the op: against the restatement of the
    rounded values (the sums do not depend on the order of the columns, so one restatement serves both memory formats)"""
    cases, allow = semckd_fixture.load()
    c = cases[ci]
    S, P = len(c["stu"]), len(c["s_value"])
    xs, ts = [_r(x, dts[0]) for x in c["s_value"]], [_r(t, dts[1]) for t in c["target"]]
    want = V.tail(xs, ts, c["weight"], g=0.5)
    got = run_op(xs, ts, c["weight"], S, g=0.5, dt_x=[dts[0]] * P, dt_t=[dts[1]] * P, cl=cl)
    assert check(f"case {ci} {dts} cl={cl}", got, want, allow, bf16_dx=range(P) if dts[0] == BF16 else ())


def _edge_group(B, seed=11):
    """8 pairs (S = 2, T = 4) with every n_p the issue lists: 1 next to 3 CHUNK + 5, 7, CHUNK - 1, CHUNK, CHUNK + 1, 1003 (a multiple
    of neither 4 nor 8), 1; dtypes mixed per pair and side"""
    K = _L().SEMCKD_CHUNK
    rng = np.random.default_rng(seed)
    ns = [1, 3 * K + 5, 7, K - 1, K, K + 1, 1003, 1]
    dt_x = [F32, BF16, F32, BF16, F32, F32, BF16, BF16]
    dt_t = [F32, BF16, BF16, F32, F32, BF16, F32, BF16]
    xs = [_draw(rng, (B, n)) for n in ns]
    ts = [_draw(rng, (B, n)) for n in ns]
    w = _weights(rng, (B, 2, 4))
    return xs, ts, w, dt_x, dt_t


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset_by_one"])
@pytest.mark.parametrize("B", [1, 3])
def test_edges_against_the_restatement(B, offset):
    """every size at which the walk takes another path (element, 4- and 8-element accesses; one chunk, a chunk boundary, several
    chunks; n_p = 1 next to 3 CHUNK + 5 in one group), B = 1, base pointers one element behind an aligned address, a null dx among
    non-null ones, w = 0 for one pair (exact zeros in its dx), x == t for one pair (ind and dx exactly 0)"""
    xs, ts, w, dt_x, dt_t = _edge_group(B)
    w = w.copy()
    w[:, 1, 0] = 0.0                                                     # pair 4
    ts[6] = xs[6].copy()                                                 # pair 6: x == t
    want = V.tail(xs, ts, w)
    got = run_abi(xs, ts, w, 2, dt_x=dt_x, dt_t=dt_t, offset=offset, no_dx=(2,), canary=7.0)
    assert got["dx"][2] is None
    assert check(f"edges B={B}", got, want, ONE_ULP, bf16_dx=[p for p, d in enumerate(dt_x) if d == BF16])
    assert not got["dx"][4].any() and not got["dx"][6].any() and not got["ind"].reshape(B, 8)[:, 6].any()
    assert all(np.abs(d).max() > 0 for p, d in enumerate(got["dx"]) if p not in (2, 4, 6))


@pytest.mark.parametrize("P,S", [(1, 1), (64, 8)])
def test_one_pair_and_sixty_four_pairs(P, S):
    rng = np.random.default_rng(P)
    B = 2
    xs, ts = [_draw(rng, (B, 5 + p % 3)) for p in range(P)], [_draw(rng, (B, 5 + p % 3)) for p in range(P)]
    w = _weights(rng, (B, S, P // S))
    assert check(f"{P} pairs", run_abi(xs, ts, w, S), V.tail(xs, ts, w), ONE_ULP)
    maps = lambda a: [v.reshape(B, -1, 1, 1) for v in a]                 # noqa: E731
    assert check(f"{P} pairs, op", run_op(maps(xs), maps(ts), w, S), {**V.tail(maps(xs), maps(ts), w)}, ONE_ULP)


def test_equal_maps_give_exact_zeros():
    xs, ts, w, dt_x, dt_t = _edge_group(2, seed=5)
    xs = [_r(x, d) for x, d in zip(xs, dt_x)]
    got = run_abi(xs, [x.copy() for x in xs], w, 2, dt_x=dt_x, dt_t=dt_x, canary=7.0)
    assert got["loss"] == 0.0 and not got["ind"].any() and all(not d.any() for d in got["dx"])


def test_upstream_gradient_scales_dx_and_dw():
    """an upstream gradient of 3 against g = 1: dx and dw are the restatement's at g = 3 (one rounding each), and three times the
    g = 1 results up to that rounding (fp32: one ulp each side; bf16: half a bf16 ulp each side)"""
    xs, ts, w, dt_x, dt_t = _edge_group(2, seed=9)
    bf = [p for p, d in enumerate(dt_x) if d == BF16]
    one, three = run_abi(xs, ts, w, 2, dt_x=dt_x, dt_t=dt_t), run_abi(xs, ts, w, 2, g=3.0, dt_x=dt_x, dt_t=dt_t)
    assert check("g = 3", three, V.tail(xs, ts, w, g=3.0), ONE_ULP, bf16_dx=bf)
    assert three["loss"] == one["loss"] and np.array_equal(three["ind"], one["ind"])
    for p, (a, b) in enumerate(zip(three["dx"], one["dx"])):
        tol = (2 * HALF_ULP_BF16 if p in bf else 2 * ULP32) * np.abs(a)
        assert (np.abs(a - 3.0 * b) <= tol).all(), p
    maps = lambda a: [v.reshape(len(v), -1, 1, 1) for v in a]            # noqa: E731
    o1, o3 = run_op(maps(xs), maps(ts), w, 2, dt_x=dt_x, dt_t=dt_t), run_op(maps(xs), maps(ts), w, 2, g=3.0, dt_x=dt_x, dt_t=dt_t)
    assert check("op, g = 3", o3, V.tail(maps(xs), maps(ts), w, g=3.0), ONE_ULP, bf16_dx=bf)
    assert (np.abs(o3["dw"] - 3.0 * o1["dw"]) <= 4 * ULP32 * np.abs(o3["dw"])).all()


def test_shape_errors_are_returned_codes_with_nothing_written():
    """65 pairs, n_pairs % S != 0, B < 1, n_p < 1 and an unknown dtype: the code comes back, nothing is launched, nothing written"""
    L, lib, guard = _L(), _lib(), _Guarded()
    e = lambda n, dt=F32: guard.empty(n, device="cuda", dtype=dt)        # noqa: E731
    x, t, dx, w, ind, loss, g, ws = e(64), e(64), e(64), e(256), e(256), e(1), e(1), e(1024, torch.float64)
    bufs = (x, t, dx, w, ind, loss, g, ws)
    for z in bufs:
        z.fill_(1.5)

    def table(ns, dt=L.DT_F32):
        tab = (L.SemckdPair * len(ns))()
        for i, n in enumerate(ns):
            tab[i] = L.SemckdPair(x.data_ptr(), t.data_ptr(), dx.data_ptr(), n, dt, L.DT_F32)
        return tab

    for tab, P, S, B, rc in ((table([2] * 65), 65, 1, 2, -2), (table([2] * 6), 6, 4, 2, -2), (table([2]), 1, 1, 0, -2),
                             (table([2, 0]), 2, 1, 2, -2), (table([2]), 1, 0, 2, -2), (table([2], dt=3), 1, 1, 2, -6)):
        assert lib.moma_semckd_fwd(tab, P, S, B, _p(w), _p(ws), 8192, _p(ind), _p(loss), _st()) == rc
        assert lib.moma_semckd_bwd(tab, P, S, B, _p(w), _p(g), _st()) == rc
    assert lib.moma_semckd_workspace_bytes(table([2] * 65), 65, 2) == 0
    assert guard.check("refused calls") > 0
    assert all(bool((z == 1.5).all()) for z in bufs)                     # nothing written


# ---- moma_sp_gram_sum, ops.batch_gram -------------------------------------------------------------------------------------------------
def _gram_abi(x, dtype, offset=False):
    lib, guard = _lib(), _Guarded()
    B, K = x.shape
    f = _place(guard, x, dtype, offset)
    n = lib.moma_sp_workspace_bytes(B, K)
    ws, G = guard.empty(n // 4, device="cuda", dtype=F32), guard.empty(B * B, device="cuda", dtype=F32)
    assert lib.moma_sp_gram(_p(f), B, K, _L().DT_BF16 if dtype == BF16 else _L().DT_F32, _p(ws), n, _st()) == 0
    assert lib.moma_sp_gram_sum(_p(ws), n, K, B, _p(G), _st()) == 0
    assert guard.check("moma_sp_gram / _gram_sum") > 0
    return _np(G).reshape(B, B), n // (4 * B * B)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,K,offset", [(1, 1, False), (5, 7, False), (9, 130 * 9, True), (65, 1000, False), (12, 1024, True)])
def test_gram_sum_is_exact_where_every_partial_sum_is(B, K, offset, dtype):
    """inputs that are multiples of 1/32 up to 4: every product is a multiple of 2^-10 below 16, so for 16 K <= 2^14 every partial sum
    has at most 24 significant bits and the fp32 G must EQUAL the float64 value; G == G^T bit for bit"""
    assert 16 * K <= 2 ** 14 or K == 130 * 9
    x = _draw(np.random.default_rng(B * 1000 + K), (B, K))
    if K > 1024:
        x = np.clip(x, -3, 3)                                            # 9 K <= 2^14 keeps the argument for the 130-channel map
    G, _splits = _gram_abi(x, dtype, offset)
    assert np.array_equal(G, V.gram(x)) and np.array_equal(G, G.T)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gram_sum_above_the_exact_range_keeps_the_header_s_bound(dtype):
    """K = 5000, B = 65 (two row tiles): (splits + 1) 2^-24 of |X| |X|^T, entry by entry"""
    x = _draw(np.random.default_rng(77), (65, 5000))
    G, splits = _gram_abi(x, dtype)
    bound = (splits + 1) * 2.0 ** -24 * V.gram_abs(x)
    worst = float((np.abs(G - V.gram(x)) / bound).max())
    print(f"  G at K = 5000, {splits} splits: {worst:.3f} of the bound")
    assert worst <= 1.0 and np.array_equal(G, G.T)


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_batch_gram_and_its_gradient(dtype, cl):
    """ops.batch_gram of a [B,C,H,W] map in either memory format: G exact (above), dX against (dG + dG^T) X in float64.  dG holds
    multiples of 1/8 up to 4, so M is exact in fp32, every product M X has 15 significant bits and every sum below 2^24 ulps: dX is
    ONE rounding away (fp32 ulp; bf16: half a bf16 ulp more)"""
    from moma_amd import ops
    rng = np.random.default_rng(4)
    B, shape = 65, (65, 6, 5, 5)
    x = _draw(rng, shape)
    dG = np.clip(np.round(rng.standard_normal((B, B)) * 8) / 8, -4, 4)
    mf = torch.channels_last if cl else torch.contiguous_format
    f = torch.from_numpy(x.astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf).requires_grad_(True)
    G = ops.batch_gram(f)
    assert G.dtype == F32 and tuple(G.shape) == (B, B) and np.array_equal(_np(G.detach()), V.gram(x))
    G.backward(torch.from_numpy(dG.astype(np.float32)).cuda())
    assert f.grad.dtype == dtype and f.grad.stride() == f.stride()
    want = V.gram_bwd(x, dG)
    tol = (ULP32 + (HALF_ULP_BF16 if dtype == BF16 else 0.0)) * np.abs(want)
    assert (np.abs(_np(f.grad) - want) <= tol).all()


def test_two_calls_give_the_same_bits():
    xs, ts, w, dt_x, dt_t = _edge_group(3, seed=21)
    a, b = (run_abi(xs, ts, w, 2, g=1.7, dt_x=dt_x, dt_t=dt_t) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a["raw"], b["raw"]))
    maps = lambda z: [v.reshape(len(v), -1, 1, 1) for v in z]            # noqa: E731
    o1, o2 = (run_op(maps(xs), maps(ts), w, 2, g=1.7, dt_x=dt_x, dt_t=dt_t) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(o1["raw"], o2["raw"])) and o1["loss"] == a["loss"]
    x = _draw(np.random.default_rng(8), (65, 5000))
    assert np.array_equal(_gram_abi(x, F32)[0], _gram_abi(x, F32)[0])


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.semckd_weighted_mse and ops.batch_gram with every buffer they allocate (workspace, ind, loss, every dx, the Gram
    partials, G) between guard margins: margins untouched, results bit-equal to the same calls on ordinary allocations"""
    from moma_amd import ops
    xs, ts, w, dt_x, dt_t = _edge_group(3, seed=2)
    maps = lambda z: [v.reshape(len(v), -1, 1, 1) for v in z]            # noqa: E731
    X, T_, _sv, _tg = _dev_lists(maps(xs), maps(ts), 2, dt_x, dt_t)
    wd = torch.from_numpy(w.astype(np.float32)).cuda()
    fmap = torch.from_numpy(_draw(np.random.default_rng(1), (7, 5, 3, 3)).astype(np.float32)).cuda()

    def run(wrap):
        xx = [wrap(x.detach()).requires_grad_(True) for x in X]
        tt = [wrap(t) for t in T_]
        ww = wrap(wd).requires_grad_(True)
        loss, ind = ops.semckd_weighted_mse([xx[:4], xx[4:]], [tt[:4], tt[4:]], ww)
        (loss * 2.5).backward()
        f = wrap(fmap).requires_grad_(True)
        G = ops.batch_gram(f)
        G.sum().backward()
        return [loss.detach().clone(), ind.clone(), ww.grad.clone(), G.detach().clone(), f.grad.clone()] + [x.grad.clone() for x in xx]

    plain = run(lambda z: z.clone())
    guard = _Guarded()
    monkeypatch.setattr(ops, "torch", guard)
    try:
        guarded = run(lambda z: _in(guard, z))
        assert guard.check("semckd_weighted_mse / batch_gram") > 0
    finally:
        monkeypatch.setattr(ops, "torch", torch)
    for u, v in zip(plain, guarded):
        assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


# ---- SelfA.loss --------------------------------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch):
    from moma_amd import ops
    calls = {"tail": [], "gram": 0}
    real_tail, real_gram = ops.semckd_weighted_mse, ops.batch_gram

    def tail(s_values, targets, weight):
        calls["tail"].append((len(s_values) * len(s_values[0]), s_values[0][0].dtype, targets[0][0].dtype))
        return real_tail(s_values, targets, weight)

    def gram(f):
        calls["gram"] += 1
        return real_gram(f)
    monkeypatch.setattr(ops, "semckd_weighted_mse", tail)
    monkeypatch.setattr(ops, "batch_gram", gram)
    return calls


def _step(c, route, amp=None, cl=False):
    """one forward + backward of the recorded module on the GPU by `route` (loss: kernels where they apply; composite) ->
    (loss, student-map gradients, d regressor00's first weight, d query_0.linear1.weight)"""
    mod = semckd_fixture.module_of(c).cuda()
    mf = torch.channels_last if cl else torch.contiguous_format
    fs = [torch.from_numpy(f).cuda().contiguous(memory_format=mf).requires_grad_(True) for f in c["fs"]]
    ft = [torch.from_numpy(f).cuda().contiguous(memory_format=mf) for f in c["ft"]]
    with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
        loss = getattr(mod, route)(fs, ft)
    assert loss.dtype == F32
    loss.backward()
    dhead = mod.query_0.linear1.weight.grad
    return (float(loss.item()), [_np(f.grad) for f in fs], _np(mod.regressor00.regressor[0].weight.grad),
            None if dhead is None else _np(dhead), mod)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_self_attention_loss_on_the_kernels_against_the_fixture_and_the_composite_fp32(ci, monkeypatch):
    """fp32: SelfA.loss takes the kernels (S + T Gram calls, ONE grouped tail call) and agrees with the reference's recorded fp32
    results and with the composite on the same device, each within twice the chain allowances (either side may be that far from
    float64); the head's gradient in absolute terms where it is analytically 0"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    cases, allow = semckd_fixture.load()
    c = cases[ci]
    S, T = len(c["stu"]), len(c["tea"])
    calls = _count_calls(monkeypatch)
    loss, dxs, dproj, dhead, mod = _step(c, "loss")
    assert calls["gram"] == S + T and calls["tail"] == [(S * T, F32, F32)]
    assert all(p.grad is None for n, p in mod.named_parameters() if ".regressor." in n and n.startswith(("query_", "key_")))
    closs, cdxs, cdproj, cdhead, _m = _step(c, "composite")
    assert calls["gram"] == S + T and len(calls["tail"]) == 1          # the composite called neither
    ok = True
    for tag, (l2, x2, p2, h2) in (("reference", (c["loss"], c["dxs"], c["dproj"], c["dhead"])), ("composite", (closs, cdxs, cdproj, cdhead))):
        ok &= _report(f"loss vs {tag}", abs(loss - l2) / abs(l2), 2 * allow["chain_loss"])
        ok &= _report(f"dxs vs {tag}", max(rel(a, b) for a, b in zip(dxs, x2)), 2 * allow["dxs"])
        ok &= _report(f"dproj vs {tag}", rel(dproj, p2), 2 * allow["dproj"])
        if semckd_fixture.head_is_zero(c):
            ok &= dhead is None or float(np.abs(dhead).max()) <= 1e-6 * np.abs(c["dproj"]).max()
        else:
            ok &= _report(f"dhead vs {tag}", rel(dhead, h2), 2 * allow["dhead"])
    assert ok


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("ci", [0, 2])
def test_self_attention_loss_under_bf16_autocast(ci, cl, monkeypatch):
    """bf16 autocast: the projections hand the kernels bf16 maps, the targets stay fp32 (pooled once per (teacher map, grid)); kernels
    and composite see the same projections, so the losses differ by fp32 effects of the head and the tail -- bounded here by one bf16
    ulp (2^-8), the resolution of the maps they share -- and the gradients, which pass a bf16 dx through the projections' backward,
    by 2^-6 of their largest element"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    cases, _allow = semckd_fixture.load()
    c = cases[ci]
    S, T = len(c["stu"]), len(c["tea"])
    calls = _count_calls(monkeypatch)
    loss, dxs, dproj, dhead, _m = _step(c, "loss", amp=BF16, cl=cl)
    assert calls["gram"] == S + T and calls["tail"] == [(S * T, BF16, F32)]
    closs, cdxs, cdproj, cdhead, _m = _step(c, "composite", amp=BF16, cl=cl)
    ok = _report("loss vs composite", abs(loss - closs) / closs, 2.0 ** -8)
    ok &= _report("dxs vs composite", max(rel(a, b) for a, b in zip(dxs, cdxs)), 2.0 ** -6)
    ok &= _report("dproj vs composite", rel(dproj, cdproj), 2.0 ** -6)
    assert ok and np.isfinite(dhead).all()


def test_self_attention_routes(monkeypatch):
    """the composite for float16 / float64 storage, more than 64 pairs and a teacher map that records a gradient"""
    calls = _count_calls(monkeypatch)
    mod = SelfA(4, [3], [2], 1.0).cuda()
    fs, ft = [torch.randn(4, 3, 4, 4, device="cuda")], [torch.randn(4, 2, 4, 4, device="cuda")]
    assert np.isfinite(mod.loss(fs, ft).item()) and len(calls["tail"]) == 1
    with torch.autocast("cuda", dtype=torch.float16):                   # the projections hand on float16 maps
        assert np.isfinite(mod.loss(fs, ft).item()) and len(calls["tail"]) == 1
    mod64 = SelfA(4, [3], [2], 1.0).cuda().double()
    out = mod64.loss([f.double() for f in fs], [f.double() for f in ft])
    assert out.dtype == torch.float64 and len(calls["tail"]) == 1
    assert np.isfinite(mod.loss(fs, [f.clone().requires_grad_(True) for f in ft]).item()) and len(calls["tail"]) == 1
    wide = SelfA(4, [2] * 5, [2] * 13, 1.0).cuda()                      # 65 pairs
    out = wide.loss([torch.randn(4, 2, 2, 2, device="cuda")] * 5, [torch.randn(4, 2, 2, 2, device="cuda")] * 13)
    assert np.isfinite(out.item()) and len(calls["tail"]) == 1
    with pytest.raises(ValueError, match="batches of 4"):
        mod.loss([torch.randn(3, 3, 4, 4, device="cuda")], [torch.randn(3, 2, 4, 4, device="cuda")])


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
ARGV = ["--distill", "semckd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
        "--n_cls", "4", "--batch_size", "8", "-c", "1", "-d", "1", "-b", "400"]


def _loop(extra, steps=1):
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(ARGV + ["--steps_per_epoch", str(steps), "--learning_rate", "0.01", "--no_graph_teacher", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
    dev = torch.device("cuda", 0)
    opt.device = dev
    torch.manual_seed(31)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
    sa = module_list[1]
    before = {n: p.detach().clone() for n, p in sa.state_dict().items()}
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
    return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace], feats, before, sa


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='semckd', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: the pairs run on the kernels
    in one grouped call; loss_kd is SemCKDLoss(*forward(...)) in float64 on the feature maps the two models produced in that step with
    the module as it was before it; the step moves the projections and the heads; the same step in channels_last under bf16 autocast
    hands the kernels bf16 maps and stays finite"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    calls = _count_calls(monkeypatch)
    _cases, allow = semckd_fixture.load()
    losses, kds, feats, before, sa = _loop([])
    n_pairs = sa.s_len * sa.t_len
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all() and calls["tail"] == [(n_pairs, F32, F32)]
    assert calls["gram"] == sa.s_len + sa.t_len
    twin = SelfA(sa.feat_dim, [f.shape[1] for f in feats["s"][1:-1]], [f.shape[1] for f in feats["t"][1:-1]], sa.soft)
    twin.load_state_dict({k: v.cpu() for k, v in before.items()})
    import copy
    twin.train()
    twin64 = copy.deepcopy(twin).double()
    maps = [f.cpu() for f in feats["s"][1:-1]], [f.cpu() for f in feats["t"][1:-1]]
    stock = float(SemCKDLoss()(*twin(*maps)).detach())
    want = float(SemCKDLoss()(*twin64([f.double() for f in maps[0]], [f.double() for f in maps[1]])).detach())
    print("loss_kd: %.6e  float64 modules: %.6e  fp32 modules: %.6e" % (kds[0], want, stock))
    # the fixture's allowance, or twice what the same modules in fp32 stock ops keep from float64 on these very maps (Gram entries of
    # 1e4 and more in front of the heads: these maps are not the fixture's)
    assert _report("loss_kd of the step", abs(kds[0] - want) / want, max(2 * allow["chain_loss"], 2 * abs(stock - want) / want))
    after = sa.state_dict()
    for k in ("regressor00.regressor.0.weight", "regressor00.regressor.1.running_mean", "query_0.linear1.weight", "key_0.linear2.bias"):
        assert not torch.equal(before[k], after[k]), k
    assert torch.equal(before["query_0.regressor.0.weight"], after["query_0.regressor.0.weight"])
    del calls["tail"][:]
    losses, kds, feats, _before, sa = _loop(["--channels_last", "--amp", "bf16"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all()
    print("bf16 / channels_last step: loss_kd %.6e, kernel calls %s" % (kds[0], calls["tail"]))
    assert calls["tail"] == [(n_pairs, BF16, F32)] or calls["tail"] == [(n_pairs, BF16, BF16)]


def test_cli_runs_with_distill_semckd(tmp_path):
    """`python train_student_moma.py --distill semckd` on the smallest synthetic configuration: parses, builds, trains and validates"""
    from tests.test_gpu_cli import _run_cli
    r = _run_cli(tmp_path, ARGV + ["--epochs", "1", "--steps_per_epoch", "2"], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout and "nan" not in r.stdout.lower()

"""GPU tests of the Correlation Congruence kernels (csrc/cc.hip) through the C ABI, ops.cc_embed_neighbour, Correlation.loss and the
training loop.

Yardstick: the float64 evaluation of the formulas (tests/cc_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_d / _loss / _dxs / _dws / _dbs / _dwt / _dbt`) that the reference's own fp32 results keep from
float64 over the cases of the golden fixture, never below one fp32 ulp (2^-23, relative).  Metric: crd_ref.rel (units of the
yardstick's largest element); the loss relative to its own value.  A dx_s stored in bf16 adds that rounding: half a bf16 ulp (8
significant bits), at most 2^-8 of the element.  Every input is clear of the kink of |d| (cc_ref.clear, TAU = 2^-10); no element is left
out of a comparison, and the sign of every d is exact.
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result."""
import ctypes as C

import numpy as np
import pytest
import torch

from moma_amd.distiller_zoo import Correlation, LinearEmbed  # noqa: F401  (the modules under test)
from tests import cc_fixture, cc_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8
N_CASES = cc_fixture.N_CASES
GRADS = (("dx_s", "dxs"), ("dW_s", "dws"), ("db_s", "dbs"), ("dW_t", "dwt"), ("db_t", "dbt"))
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


def _np(t):
    return t.float().cpu().numpy().astype(np.float64) if t.dtype != torch.float64 else t.cpu().numpy()


def _code(dtype):
    from moma_amd import _lib as L
    return L.DT_BF16 if dtype == BF16 else L.DT_F32


def _carve(guard, shape, dtype, offset):
    """an uninitialised dense [B, C] device tensor between NaN margins, optionally starting one element behind an aligned address"""
    flat = guard.empty(shape[0] * shape[1] + int(offset), device="cuda", dtype=dtype)
    return (flat[1:] if offset else flat).view(*shape)


def _place(guard, f, dtype=F32, offset=False):
    out = _carve(guard, f.shape, dtype, offset)
    src = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dtype)
    assert np.array_equal(src.float().numpy(), np.asarray(f, np.float32))     # (the inputs are exact in the storage type)
    out.copy_(src)
    return out


ALL = ("dx_s", "dW_s", "db_s", "dW_t", "db_t")


def run_abi(x_s, x_t, W_s, b_s, W_t, b_t, dt_s=F32, dt_t=F32, off_s=False, off_t=False, g_loss=1.0, outputs=ALL, inputs=True):
    """moma_cc_fwd -> moma_cc_bwd on fresh guarded buffers; numpy inputs.  `outputs`: the gradients asked for (the others are NULL);
    inputs=False: every input the asked outputs do not need is NULL too.  -> dict of numpy float64 arrays and the raw device tensors
    under `raw`"""
    lib, guard = _lib(), _Guarded()
    B, Cs = x_s.shape
    Ct, D = x_t.shape[1], W_s.shape[0]
    ts, tt = _place(guard, x_s, dt_s, off_s), _place(guard, x_t, dt_t, off_t)

    def arr(a):
        a = np.asarray(a, np.float32)
        v = guard.empty(a.size, device="cuda", dtype=F32)
        v.copy_(torch.from_numpy(a.reshape(-1)))
        return v

    e = lambda n: guard.empty(n, device="cuda", dtype=F32)                    # noqa: E731
    tWs, tbs, tWt, tbt = arr(W_s), arr(b_s), arr(W_t), arr(b_t)
    nws = lib.moma_cc_workspace_bytes(B, Cs, Ct, D)
    assert nws > 0 and nws % 4 == 0
    ws = guard.empty((nws + 7) // 8, device="cuda", dtype=torch.float64)
    loss, gu, d_out = e(1), e(B * D), e(B * D)
    rc = lib.moma_cc_fwd(_p(ts), _p(tt), _p(tWs), _p(tbs), _p(tWt), _p(tbt), B, Cs, Ct, D, _code(dt_s), _code(dt_t), _p(ws), nws, _p(gu),
                         _p(loss), _p(d_out), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    raw = {"loss": loss, "gu": gu, "d": d_out}
    if "dx_s" in outputs:
        raw["dx_s"] = _carve(guard, x_s.shape, dt_s, off_s)
    for k, n in (("dW_s", D * Cs), ("db_s", D), ("dW_t", D * Ct), ("db_t", D)):
        if k in outputs:
            raw[k] = e(n)
    need = lambda t, k: t if inputs or k in outputs else None                 # noqa: E731
    rc = lib.moma_cc_bwd(_p(gu), _p(need(ts, "dW_s")), _p(need(tt, "dW_t")), _p(need(tWs, "dx_s")), _p(gl), _p(raw.get("dx_s")),
                         _p(raw.get("dW_s")), _p(raw.get("db_s")), _p(raw.get("dW_t")), _p(raw.get("db_t")), B, Cs, Ct, D, _code(dt_s),
                         _code(dt_t), _st())
    assert rc == 0, rc
    assert guard.check("cc C ABI") > 0                                        # every margin untouched
    out = {k: _np(v) for k, v in raw.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out["loss"] = float(loss.item())
    out["d"], out["gu"] = out["d"].reshape(B, D), out["gu"].reshape(B, D)
    for k, shape in (("dW_s", (D, Cs)), ("dW_t", (D, Ct))):
        if k in out:
            out[k] = out[k].reshape(shape)
    out["raw"] = raw
    return out


def run_op(x_s, x_t, W_s, b_s, W_t, b_t, dt_s=F32, dt_t=F32, g_loss=1.0):
    from moma_amd import ops
    mk = lambda f, dt=F32: torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dt).cuda()      # noqa: E731
    ts, tt = mk(x_s, dt_s).requires_grad_(True), mk(x_t, dt_t)
    ps = [mk(v).requires_grad_(True) for v in (W_s, b_s, W_t, b_t)]
    loss = ops.cc_embed_neighbour(ts, tt, *ps)
    (loss * g_loss).backward()
    assert ts.grad.shape == ts.shape and ts.grad.dtype == dt_s and tt.grad is None
    assert all(p.grad.dtype == F32 and p.grad.shape == p.shape for p in ps)
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    raw = {"loss": loss.detach(), "dx_s": ts.grad, "dW_s": ps[0].grad, "db_s": ps[1].grad, "dW_t": ps[2].grad, "db_t": ps[3].grad}
    out = {k: _np(v) for k, v in raw.items()}
    out["loss"] = float(loss.detach())
    out["raw"] = raw
    return out


def check(tag, got, want, allow, g_loss=1.0, bf16_out=False):
    """want: V.cc at g_loss = 1"""
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / max(want["loss"], 1e-300), allow["loss"], "loss")
    if "d" in got:
        ok &= _report(f"{tag} d", rel(got["d"], want["d"]), allow["d"], "d")
        assert np.array_equal(np.sign(got["d"]), np.sign(want["d"])), tag     # exact: the inputs are clear of the kink
    for key, kind in GRADS:
        if key not in got:
            continue
        w = g_loss * want[key]
        err = np.abs(got[key] - w)
        if key == "dx_s" and bf16_out:
            err = np.maximum(err - HALF_ULP_BF16 * np.abs(w), 0)              # the rounding of the stored gradient
        ok &= _report(f"{tag} {key}", float(err.max() / max(np.abs(w).max(), 1e-300)), allow[kind], kind)
    if "db_s" in got and "db_t" in got:
        assert torch.equal(got["raw"]["db_t"], -got["raw"]["db_s"]), tag      # bitwise
    return ok


def _draw(B, Cs, Ct, D, seed):
    """(x_s, x_t, W_s, b_s, W_t, b_t): normal draws rounded to multiples of 1/32 (exact in bf16), clipped to 4, x_s cleared; the heads
    scaled like nn.Linear's"""
    rng = np.random.default_rng(seed)
    q = lambda *s: np.clip(np.round(rng.standard_normal(s) * 32) / 32, -4, 4).astype(np.float32)          # noqa: E731
    u = lambda n, *s: (rng.uniform(-1, 1, s) / np.sqrt(n)).astype(np.float32)                             # noqa: E731
    x_s, x_t = q(B, Cs), q(B, Ct)
    W_s, b_s, W_t, b_t = u(Cs, D, Cs), u(Cs, D), u(Ct, D, Ct), u(Ct, D)
    x64, _n = V.clear(x_s, x_t, W_s, b_s, W_t, b_t)
    return x64.astype(np.float32), x_t, W_s, b_s, W_t, b_t


def teardown_module(_m):
    print("largest share of an allowance used, per kind:", {k: round(v, 3) for k, v in sorted(USED.items())})


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """every fixture case against float64, through the C ABI with both dtypes chosen per side, with and without a one-element offset of
    the base addresses, and through the op; the inputs are exact in bf16, so one yardstick serves every storage"""
    cases, allow = cc_fixture.load()
    c = cases[ci]
    args = cc_fixture.args(c)
    want = V.cc(*args)
    print(f"case {ci} B {c['B']} Cs {c['Cs']} Ct {c['Ct']} D {c['D']}")
    ok = True
    first = None
    for dt_s, dt_t in ((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)):
        for off in (False, True):
            got = run_abi(*args, dt_s=dt_s, dt_t=dt_t, off_s=off, off_t=off, g_loss=3.0)
            assert got["raw"]["dx_s"].dtype == dt_s
            ok &= check(f"abi {dt_s} {dt_t} off {int(off)}", got, want, allow, g_loss=3.0, bf16_out=dt_s == BF16)
            if first is None:
                first = got
            # the storage type and the base address change nothing but dx_s's rounding: the inputs are the same numbers
            assert all(torch.equal(got["raw"][k], first["raw"][k]) for k in ("loss", "d", "gu", "dW_s", "db_s", "dW_t", "db_t"))
    op = run_op(*args)
    ok &= check("op", op, want, allow)
    op16 = run_op(*args, dt_s=BF16, dt_t=BF16, g_loss=2.0)
    ok &= check("op bf16", op16, want, allow, g_loss=2.0, bf16_out=True)
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / c["loss"], allow["loss"] + c["ref_vs_f64_loss"])
    for key, kind in GRADS:
        ok &= _report(f"op {key} vs reference", rel(op[key], c[key]), allow[kind] + c["ref_vs_f64_" + kind])
    assert ok


EDGES = [  # (B, Cs, Ct, D): sizes at which the kernels take another path
    (2, 32, 64, 16),        # whole segments, one workgroup of columns
    (17, 31, 97, 17),       # segment tails on both sides, a second workgroup of columns, two passes of the row lanes
    (70, 65, 3, 65),        # a second tile on every side of every product
    (3, 2100, 40, 2),       # 66 + 2 segments over one tile: one segment per split, 68 splits
    (260, 200, 130, 330),   # 5 x 6 tiles, 7 + 5 segments at 2 per split: 4 + 3 splits, the last of each side one short segment; a second
                            # bias item
]


@pytest.mark.parametrize("ei", range(len(EDGES)))
def test_edges_against_the_restatement(ei):
    _cases, allow = cc_fixture.load()
    args = _draw(*EDGES[ei], 300 + ei)
    want = V.cc(*args)
    dt = (F32, BF16)[ei % 2]
    got = run_abi(*args, dt_s=dt, dt_t=F32, g_loss=3.0)
    assert check(f"{EDGES[ei]}", got, want, allow, g_loss=3.0, bf16_out=dt == BF16)


def test_identical_sides_give_exact_zeros():
    """the same x, W and b on both sides, Cs = Ct: both totals are the same bits, so d_out, the loss and every gradient are exactly 0"""
    for (B, Cc, D, dt) in [(5, 33, 17, F32), (66, 200, 70, BF16), (4, 1280, 16, F32)]:
        x_s, _xt, W_s, b_s, _Wt, _bt = _draw(B, Cc, Cc, D, B + Cc)
        got = run_abi(x_s, x_s, W_s, b_s, W_s, b_s, dt_s=dt, dt_t=dt, g_loss=7.0)
        assert got["loss"] == 0 and not got["d"].any() and not got["gu"].any()
        assert all(not got[k].any() for k in ALL), (B, Cc, D)


def test_upstream_gradient_scales_exactly():
    """g_loss is a device scalar folded in before the one rounding: 2^k against 1 scales every gradient's bits exactly, 0 gives exact
    zeros; through autograd likewise; the guards of the op"""
    from moma_amd import ops
    args = _draw(7, 40, 24, 10, 8)
    for dt in (F32, BF16):
        one = run_abi(*args, dt_s=dt, dt_t=dt)
        for g in (2.0, 0.5, 1024.0):
            got = run_abi(*args, dt_s=dt, dt_t=dt, g_loss=g)
            for k in ALL:
                assert torch.equal(got["raw"][k].float(), one["raw"][k].float() * g), (dt, g, k)
            assert all(torch.equal(got["raw"][k], one["raw"][k]) for k in ("loss", "gu", "d"))
        zero = run_abi(*args, dt_s=dt, dt_t=dt, g_loss=0.0)
        assert all(not zero[k].any() for k in ALL)
    a, b2 = run_op(*args), run_op(*args, g_loss=2.0)
    assert all(torch.equal(b2["raw"][k], a["raw"][k] * 2.0) for k in ALL)
    x_s, x_t, W_s, b_s, W_t, b_t = (torch.from_numpy(v).cuda() for v in args)
    call = lambda **kw: ops.cc_embed_neighbour(**{**dict(x_s=x_s, x_t=x_t, w_s=W_s, b_s=b_s, w_t=W_t, b_t=b_t), **kw})     # noqa: E731
    with torch.no_grad():
        assert float(call()) == a["loss"]
    assert not call().requires_grad and call(w_t=W_t.clone().requires_grad_(True)).requires_grad
    with pytest.raises(TypeError):
        call(x_s=x_s.half())
    with pytest.raises(ValueError):
        call(x_t=x_t[:, :20].contiguous())                                                            # the head's width
    with pytest.raises(ValueError):
        call(x_s=x_s.t().contiguous().t())                                                            # not contiguous
    with pytest.raises(ValueError):
        call(x_t=x_t.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        call(x_t=x_t[:5].contiguous())                                                                # the batch
    with pytest.raises(ValueError, match="no pair of neighbouring rows"):
        call(x_s=x_s[:1].contiguous(), x_t=x_t[:1].contiguous())


def test_null_outputs_are_skipped():
    """every subset of one output, with the inputs only that output needs: the same bits as the full call, nothing else written"""
    args = _draw(9, 70, 33, 66, 4)
    full = run_abi(*args, g_loss=3.0)
    for k in ALL:
        got = run_abi(*args, g_loss=3.0, outputs=(k,), inputs=False)
        assert torch.equal(got["raw"][k], full["raw"][k]), k
    pair = run_abi(*args, g_loss=3.0, outputs=("db_t", "dW_t"), inputs=False)
    assert torch.equal(pair["raw"]["db_t"], full["raw"]["db_t"]) and torch.equal(pair["raw"]["dW_t"], full["raw"]["dW_t"])


def test_one_row_and_shapes_past_the_caps_are_returned_errors():
    """B = 1: MOMA_E_SHAPE; B, Cs, Ct or D past the caps: MOMA_E_UNSUPPORTED; from both entry points, nothing launched, nothing written"""
    lib, guard = _lib(), _Guarded()
    e = lambda n, dt=F32: guard.empty(n, device="cuda", dtype=dt)             # noqa: E731
    x, t, v, d = e(8), e(8), e(8), e(16, torch.float64)
    for z in (x, t, v, d):
        z.fill_(1.5)
    big = 1 << 30

    def fwd(B, Cs, Ct, D):
        return lib.moma_cc_fwd(_p(x), _p(t), _p(v), _p(v), _p(v), _p(v), B, Cs, Ct, D, 0, 0, _p(d), big, _p(v), _p(v), _p(v), _st())

    def bwd(B, Cs, Ct, D):
        return lib.moma_cc_bwd(_p(v), _p(x), _p(t), _p(v), _p(v), _p(x), _p(v), _p(v), _p(v), _p(v), B, Cs, Ct, D, 0, 0, _st())

    assert lib.moma_cc_workspace_bytes(1, 8, 8, 1) == 0 and fwd(1, 8, 8, 1) == -2 and bwd(1, 8, 8, 1) == -2
    for shape in ((1025, 2, 2, 2), (2, 4097, 2, 2), (2, 2, 4097, 2), (2, 2, 2, 4097)):
        assert lib.moma_cc_workspace_bytes(*shape) == 0 and fwd(*shape) == -6 and bwd(*shape) == -6
    assert guard.check("refused shapes") > 0
    torch.cuda.synchronize()
    assert all(bool((z == 1.5).all()) for z in (x, t, v, d))                  # nothing written


def test_two_calls_give_the_same_bits():
    for (B, Cs, Ct, D, dtype) in [(16, 1280, 640, 40, F32), (8, 200, 100, 130, BF16), (33, 72, 33, 5, F32)]:
        args = _draw(B, Cs, Ct, D, Cs)
        a, b = (run_abi(*args, dt_s=dtype, dt_t=dtype) for _ in range(2))
        for k in a["raw"]:
            assert torch.equal(a["raw"][k], b["raw"][k]), ((B, Cs, Ct, D), k)
        o1, o2 = (run_op(*args, dtype, dtype) for _ in range(2))
        assert all(torch.equal(o1["raw"][k], o2["raw"][k]) for k in o1["raw"]) and o1["loss"] == a["loss"]
        assert all(torch.equal(o1["raw"][k].reshape(-1), a["raw"][k].reshape(-1)) for k in ALL)


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.cc_embed_neighbour with every buffer it allocates (the workspace, G, the loss, the five gradients) between NaN margins, at
    ragged shapes and both dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (B, Cs, Ct, D, dtype) in [(3, 5, 7, 3, F32), (5, 33, 9, 70, BF16), (2, 200, 5, 1, BF16), (9, 3, 70, 65, F32)]:
        args = _draw(B, Cs, Ct, D, Cs * 7 + B)
        ts = [torch.from_numpy(v).cuda() for v in args]
        ts[0], ts[1] = ts[0].to(dtype), ts[1].to(dtype)

        def run(wrap):
            xx = wrap(ts[0]).requires_grad_(True)
            ps = [wrap(v).requires_grad_(True) for v in ts[2:]]
            loss = ops.cc_embed_neighbour(xx, wrap(ts[1]), *ps)
            (loss * 2.5).backward()
            return [loss.detach().clone(), xx.grad.clone()] + [p.grad.clone() for p in ps]

        plain = run(lambda z: z.clone())
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda z: _in(guard, z))
            assert guard.check(f"cc_embed_neighbour {(B, Cs, Ct, D)}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_full_shape_once():
    """the reference's launch shape (B = 64, 1280-wide feat[-1] on both sides, --feat_dim 512), drawn and cleared here, against the
    restatement at the same allowances; bf16 on the student's side, fp32 on the teacher's"""
    _cases, allow = cc_fixture.load()
    args = _draw(64, 1280, 1280, 512, 11)
    want = V.cc(*args)
    assert not (np.abs(want["d"]) < V.TAU).any()
    got = run_abi(*args, dt_s=BF16, dt_t=F32, g_loss=4.0)
    assert check("full shape", got, want, allow, g_loss=4.0, bf16_out=True)


def _heads_of(c):
    es, et = LinearEmbed(c["Cs"], c["D"]), LinearEmbed(c["Ct"], c["D"])
    with torch.no_grad():
        es.linear.weight.copy_(torch.from_numpy(c["W_s"])); es.linear.bias.copy_(torch.from_numpy(c["b_s"]))
        et.linear.weight.copy_(torch.from_numpy(c["W_t"])); et.linear.bias.copy_(torch.from_numpy(c["b_t"]))
    return es.cuda(), et.cuda()


def _count_calls(monkeypatch):
    from moma_amd import ops
    calls = []
    real = ops.cc_embed_neighbour

    def spy(x_s, x_t, *a, **kw):
        calls.append((x_s.dtype, x_t.dtype))
        return real(x_s, x_t, *a, **kw)
    monkeypatch.setattr(ops, "cc_embed_neighbour", spy)
    return calls


@pytest.mark.parametrize("ci", [3, 5, 6])
def test_module_loss_on_the_kernels_against_the_composite(ci, monkeypatch):
    """Correlation.loss (the kernels) against float64 and against the composite fed the same tensors, in fp32 and -- under bf16 autocast
    with bf16 features -- reading the heads' fp32 master weights; [B, C, 1, 1] features give the same bits"""
    calls = _count_calls(monkeypatch)
    cases, allow = cc_fixture.load()
    c = cases[ci]
    want = V.cc(*cc_fixture.args(c))
    crit = Correlation()

    def run(mode, dtype=F32):
        es, et = _heads_of(c)
        x = torch.from_numpy(c["x_s"]).cuda().to(dtype).requires_grad_(True)
        t = torch.from_numpy(c["x_t"]).cuda().to(dtype)
        if mode == "composite":
            loss = crit.composite(es, et, x, t)
        elif mode == "4d":
            loss = crit.loss(es, et, x[:, :, None, None], t[:, :, None, None])
        elif mode == "autocast":
            with torch.autocast("cuda", dtype=BF16):
                loss = crit.loss(es, et, x, t)
        else:
            loss = crit.loss(es, et, x, t)
        assert loss.dtype == F32 and loss.dim() == 0
        loss.backward()
        raw = {"loss": loss.detach(), "dx_s": x.grad, "dW_s": es.linear.weight.grad, "db_s": es.linear.bias.grad,
               "dW_t": et.linear.weight.grad, "db_t": et.linear.bias.grad}
        out = {k: _np(v) for k, v in raw.items()}
        out["loss"], out["raw"] = float(loss.detach()), raw
        return out

    got, flat, comp, amp = run("kernels"), run("4d"), run("composite"), run("autocast", BF16)
    assert calls == [(F32, F32), (F32, F32), (BF16, BF16)]
    assert all(torch.equal(got["raw"][k], flat["raw"][k]) for k in got["raw"])
    ok = check("kernels vs float64", got, want, allow)
    ok &= check("kernels under bf16 autocast vs float64", amp, want, allow, bf16_out=True)
    ok &= _report("loss vs the composite", abs(got["loss"] - comp["loss"]) / comp["loss"], allow["loss"] + ULP32 / 2)
    for key, kind in GRADS:                                                   # (the composite's results are stored in fp32: half an ulp more)
        ok &= _report(f"{key} vs the composite", rel(got[key], comp[key]), allow[kind] + ULP32 / 2)
    assert ok


def test_module_takes_the_kernels_or_the_composite(monkeypatch):
    from moma_amd import ops
    calls = _count_calls(monkeypatch)
    c = cc_fixture.load()[0][3]
    crit = Correlation()
    es, et = _heads_of(c)
    x, t = torch.from_numpy(c["x_s"]).cuda(), torch.from_numpy(c["x_t"]).cuda()
    ref = c["loss"]
    out = crit.loss(es, et, x, t)
    assert calls == [(F32, F32)] and out.dtype == F32 and out.dim() == 0 and abs(float(out) - ref) < 1e-5 * ref
    assert abs(float(crit.loss(es, et, x.half(), t.half())) - ref) < 1e-5 * ref and len(calls) == 1   # float16: the composite
    assert crit.loss(es.double(), et.double(), x.double(), t.double()).dtype == torch.float64 and len(calls) == 1
    es, et = _heads_of(c)
    tg = t.clone().requires_grad_(True)
    crit.loss(es, et, x, tg).backward()
    assert len(calls) == 1 and tg.grad is not None                                                    # a teacher feature with a gradient
    assert bool(torch.isnan(crit.loss(es, et, x[:1], t[:1]))) and len(calls) == 1                     # B = 1: the reference's NaN
    monkeypatch.setattr(ops, "cc_native", lambda *a, **kw: False)
    assert abs(float(crit.loss(es, et, x, t)) - ref) < 1e-5 * ref and len(calls) == 1                 # routed away by the table


ARGV = ["--distill", "correlation", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
        "--n_cls", "4", "--batch_size", "8", "--feat_dim", "128", "-c", "1", "-d", "1", "-b", "0.02"]


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='correlation', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: both heads and the
    criterion run on the kernels; loss_kd is the restatement's value on the features the two models produced in that step with the
    heads as they were before it; the step moves both heads and leaves the teacher alone; the same step under bf16 autocast with the
    graphed teacher stays finite"""
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    calls = _count_calls(monkeypatch)
    _cases, allow = cc_fixture.load()

    def loop(extra):
        opt = parse_option(ARGV + ["--steps_per_epoch", "1", "--learning_rate", "0.01", *extra])
        opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
        dev = torch.device("cuda", 0)
        opt.device = dev
        torch.manual_seed(31)
        model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
        heads = (module_list[1], module_list[2])
        before = [{n: p.detach().clone() for n, p in m.state_dict().items()} for m in heads]
        teacher_before = [p.detach().clone() for p in model_t.parameters()]
        feats = {}

        def keep(k):
            def hook(_m, _i, out):
                if k not in feats:
                    feats[k] = [f.detach().clone() for f in out[0]]
            return hook
        hooks = [mod.register_forward_hook(keep(k)) for k, mod in (("s", model_s), ("t", model_t))]
        opt.trace, opt.print_freq = [], 1000
        train_distill_moma(1, SyntheticLoader(1, 8, 32, 4, 5, dev), module_list, criterion_list, None, contrast, optimizer, opt)
        for h in hooks:
            h.remove()
        assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
        assert all(p.grad is None for p in model_t.parameters())
        return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace], feats, before, heads

    losses, kds, feats, before, heads = loop(["--no_graph_teacher"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all() and calls == [(F32, F32)]
    b = [{k: v.cpu().numpy() for k, v in s.items()} for s in before]
    want = V.cc(feats["s"][-1].reshape(8, -1).cpu().numpy(), feats["t"][-1].reshape(8, -1).cpu().numpy(), b[0]["linear.weight"],
                b[0]["linear.bias"], b[1]["linear.weight"], b[1]["linear.bias"])
    print("loss_kd: %.6e  restatement: %.6e" % (kds[0], want["loss"]))
    assert _report("loss_kd of the step", abs(kds[0] - want["loss"]) / want["loss"], allow["loss"])
    for m, s in zip(heads, before):
        assert all(not torch.equal(s[k], m.state_dict()[k]) for k in ("linear.weight", "linear.bias"))
    del calls[:]
    losses, kds, _f, _b, _h = loop(["--amp", "bf16"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all()
    print("bf16 step: loss_kd %.6e, kernel calls %s" % (kds[0], calls))
    assert len(calls) == 1 and calls[0][0] in (BF16, F32)                     # (feat[-1] as autocast left it)

"""GPU tests of the SRRL kernels (csrc/srrl.hip) through the C ABI, ops.srrl_bn_relu_dual_mse, the connector and the training loop.

Yardstick: the float64 evaluation of the formulas (tests/srrl_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_loss / _dx / _dgamma / _dbeta / _rmean / _rvar`, and `_chain_loss / _dxs / _dw` for the whole
connector) that the reference's own fp32 results keep from float64 over the cases of the golden fixture, never below one fp32 ulp
(2^-23, relative).  Metric: crd_ref.rel (units of the yardstick's largest element); the loss relative to its own value (a sum of
squares).  A gradient stored in bf16 adds that rounding: half a bf16 ulp (8 significant bits), at most 2^-8 of the element.  Every
input is clear of the ReLU's kink (srrl_ref.clear); no element is left out of a comparison.
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from moma_amd.distiller_zoo import SRRL  # noqa: F401  (the module under test: without it nothing here has a subject)
from tests import srrl_fixture, srrl_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8
EPS, MOM = 1e-5, 0.1
N_CASES = srrl_fixture.N_CASES


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
    return t.float().cpu().numpy().astype(np.float64) if t.dtype != torch.float64 else t.cpu().numpy()


def _r16(a):
    """numpy -> the same values rounded to bf16, as float64"""
    return _np(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF16))


def _code(dtype):
    from moma_amd import _lib as L
    return L.DT_BF16 if dtype == BF16 else L.DT_F32


def _carve(guard, shape, dtype, offset):
    """an uninitialised dense [B, C] device tensor between NaN margins, optionally starting one element behind an aligned address"""
    flat = guard.empty(shape[0] * shape[1] + int(offset), device="cuda", dtype=dtype)
    return (flat[1:] if offset else flat).view(*shape)


def _place(guard, f, dtype=F32, offset=False):
    out = _carve(guard, f.shape, dtype, offset)
    out.copy_(torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dtype))
    return out


def run_abi(x, t, W, b, l, gamma, beta, eps=EPS, dt_x=F32, dt_t=F32, off_x=False, off_t=False, g_loss=1.0, momentum=MOM):
    """moma_srrl_fwd -> moma_srrl_bwd on fresh guarded buffers.  x, t: numpy [B, C]; b may be None.  -> dict of numpy float64 arrays
    (gradients times g_loss) and the raw device tensors under `raw`; the running statistics start from 0 / 1"""
    lib, guard = _lib(), _Guarded()
    B, Cc = x.shape
    K = W.shape[0]
    tx, tt = _place(guard, x, dt_x, off_x), _place(guard, t, dt_t, off_t)

    def arr(a):
        a = np.asarray(a, np.float32)
        v = guard.empty(a.size, device="cuda", dtype=F32)
        v.copy_(torch.from_numpy(a.reshape(-1)))
        return v

    e = lambda n: guard.empty(n, device="cuda", dtype=F32)                    # noqa: E731
    ga, be, rm, rv = arr(gamma), arr(beta), arr(np.zeros(Cc)), arr(np.ones(Cc))
    tW, tl = arr(W), arr(l)
    tb = arr(b) if b is not None else None
    nws = lib.moma_srrl_workspace_bytes(B, Cc, K)
    assert nws > 0 and nws % 4 == 0
    ws = guard.empty((nws + 7) // 8, device="cuda", dtype=torch.float64)
    loss, sums, dxu = e(1), guard.empty(2 * Cc, device="cuda", dtype=torch.float64), e(B * Cc)
    y_out, p_out = e(B * Cc), e(B * K)
    rc = lib.moma_srrl_fwd(_p(tx), _p(tt), _p(tW), _p(tb), _p(tl), _p(ga), _p(be), _p(rm), _p(rv), momentum, eps, B, Cc, K, _code(dt_x),
                           _code(dt_t), _p(ws), nws, _p(sums), _p(dxu), _p(loss), _p(y_out), _p(p_out), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    dx = _carve(guard, x.shape, dt_x, off_x)
    dga, dbe = e(Cc), e(Cc)
    rc = lib.moma_srrl_bwd(_p(dxu), _p(sums), _p(gl), _p(dx), _p(dga), _p(dbe), B, Cc, _code(dt_x), _st())
    assert rc == 0, rc
    assert guard.check("srrl C ABI") > 0                                      # every margin untouched
    raw = {"loss": loss, "sums": sums, "dxu": dxu, "dx": dx, "d_gamma": dga, "d_beta": dbe, "running_mean": rm, "running_var": rv,
           "y": y_out, "p": p_out}
    out = {k: _np(v) for k, v in raw.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out["loss"] = float(loss.item())
    out["A"], out["B"] = out["sums"][:Cc], out["sums"][Cc:]
    out["y"], out["p"] = out["y"].reshape(B, Cc), out["p"].reshape(B, K)
    out["raw"] = raw
    return out


def run_op(x, t, W, b, l, gamma, beta, eps=EPS, dt_x=F32, dt_t=F32, g_loss=1.0, momentum=MOM):
    from moma_amd import ops
    mk = lambda f, dt=F32: torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dt).cuda()      # noqa: E731
    Cc = x.shape[1]
    tx, tt = mk(x, dt_x).requires_grad_(True), mk(t, dt_t)
    ga, be = mk(gamma).requires_grad_(True), mk(beta).requires_grad_(True)
    tW, tb = mk(W).requires_grad_(True), (mk(b).requires_grad_(True) if b is not None else None)     # (a teacher's parameters do)
    rm, rv = torch.zeros(Cc, device="cuda"), torch.ones(Cc, device="cuda")
    loss = ops.srrl_bn_relu_dual_mse(tx, tt, tW, tb, mk(l), ga, be, rm, rv, momentum, eps)
    (loss * g_loss).backward()
    assert tx.grad.shape == tx.shape and tx.grad.dtype == dt_x and tt.grad is None and tW.grad is None and (tb is None or tb.grad is None)
    assert ga.grad.dtype == F32 and ga.grad.shape == ga.shape and be.grad.shape == be.shape
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    return {"loss": float(loss), "dx": _np(tx.grad), "d_gamma": _np(ga.grad), "d_beta": _np(be.grad), "running_mean": _np(rm),
            "running_var": _np(rv), "raw": {"dx": tx.grad, "loss": loss.detach(), "d_gamma": ga.grad, "d_beta": be.grad}}


def check(tag, got, want, allow, g_loss=1.0, bf16_out=False):
    """want: V.tail at g_loss = 1 with running statistics"""
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / max(want["loss"], 1e-300), allow["loss"])
    wd = g_loss * want["dx"]
    err = np.abs(got["dx"] - wd)
    if bf16_out:
        err = np.maximum(err - HALF_ULP_BF16 * np.abs(wd), 0)                 # the rounding of the stored gradient
    ok &= _report(f"{tag} dx", float(err.max() / max(np.abs(wd).max(), 1e-300)), allow["dx"])
    ok &= _report(f"{tag} d_gamma", rel(got["d_gamma"], g_loss * want["d_gamma"]), allow["dgamma"])
    ok &= _report(f"{tag} d_beta", rel(got["d_beta"], g_loss * want["d_beta"]), allow["dbeta"])
    ok &= _report(f"{tag} running_mean", rel(got["running_mean"], want["running_mean"]), allow["rmean"])
    ok &= _report(f"{tag} running_var", rel(got["running_var"], want["running_var"]), allow["rvar"])
    if "y" in got and "y_bound" in want:
        # y and p as the loss saw them, element by element against what fp32 arithmetic allows: y = fma(gamma, xh, beta) from a
        # correctly rounded xh is 2^-24 (|gamma xh| + |y|) <= 2^-23 (y + 2 |beta|) away where y > 0 and exactly 0 elsewhere (the
        # inputs are clear of the kink); p adds 32 fp32 FMAs per segment (32 2^-24 of the sum of |y W|) and its own rounding
        ok &= _report(f"{tag} y", float((np.abs(got["y"] - want["y"]) / want["y_bound"]).max()), 1.0)
        ok &= _report(f"{tag} p", float((np.abs(got["p"] - want["p"]) / want["p_bound"]).max()), 1.0)
    return ok


def _want(x, t, W, b, l, gamma, beta, eps=EPS, momentum=MOM):
    Cc = x.shape[1]
    w = V.tail(x, t, W, b, l, gamma, beta, eps, 1.0, np.zeros(Cc), np.ones(Cc), momentum)
    bmax = np.abs(np.asarray(beta, np.float64))
    w["y_bound"] = 2.0 ** -23 * (w["y"] + 2 * bmax) + 1e-300
    absW = np.abs(np.asarray(W, np.float64))
    w["p_bound"] = 34 * 2.0 ** -24 * ((w["y"] + w["y_bound"]) @ absW.T + (0 if b is None else np.abs(np.asarray(b, np.float64)))) \
        + w["y_bound"] @ absW.T + 1e-300
    return w


def _affine(Cc):
    c = np.arange(Cc)
    gamma = 0.5 + ((c * 7) % 5) * 0.25
    gamma[c % 3 == 1] *= -1.0
    return gamma.astype(np.float32), (((c * 3) % 4 - 1.5) * 0.2).astype(np.float32)


def _draw(B, Cc, K, seed, off=0.0):
    """(x, t, W, b, l, gamma, beta): normal draws rounded to multiples of 1/32 (exact in bf16), clipped to 4, x clear of the kink; the
    classifier scaled like nn.Linear's"""
    rng = np.random.default_rng(seed)
    gamma, beta = _affine(Cc)
    q = lambda *s: np.clip(np.round(rng.standard_normal(s) * 32) / 32, -4, 4)          # noqa: E731
    x = V.clear(q(B, Cc) + off, gamma, beta, EPS).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, Cc)) / np.sqrt(Cc)).astype(np.float32)
    b = (rng.uniform(-1, 1, K) / np.sqrt(Cc)).astype(np.float32)
    return x, (q(B, Cc) + off).astype(np.float32), W, b, q(B, K).astype(np.float32), gamma, beta


def _case(c):
    return c["conv_out"], c["t"], c["W"], c["b"], c["l"], c["gamma"], c["beta"]


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """the reference's own convolution output, the teacher's feature and logits and the classifier, as the connector hands them over"""
    cases, allow = srrl_fixture.load()
    c = cases[ci]
    want = _want(*_case(c), c["eps"], c["momentum"])
    print(f"case {ci} B {c['B']} t_n {c['t_n']} n_cls {c['n_cls']}")
    abi = run_abi(*_case(c), c["eps"], momentum=c["momentum"])
    ok = check("abi", abi, want, allow)
    abi3 = run_abi(*_case(c), c["eps"], momentum=c["momentum"], g_loss=3.0)
    ok &= check("abi g=3", abi3, want, allow, g_loss=3.0)
    op = run_op(*_case(c), c["eps"], momentum=c["momentum"])
    ok &= check("op", op, want, allow)
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / c["loss"], allow["loss"] + c["ref_vs_f64_loss"])
    ok &= _report("op dx vs reference", rel(op["dx"], c["d_conv_out"]), allow["dx"] + c["ref_vs_f64_dx"])
    ok &= _report("op d_gamma vs reference", rel(op["d_gamma"], c["d_gamma"]), allow["dgamma"] + c["ref_vs_f64_dgamma"])
    ok &= _report("op d_beta vs reference", rel(op["d_beta"], c["d_beta"]), allow["dbeta"] + c["ref_vs_f64_dbeta"])
    ok &= _report("op running_mean vs reference", rel(op["running_mean"], c["running_mean"]), allow["rmean"] + c["ref_vs_f64_rmean"])
    ok &= _report("op running_var vs reference", rel(op["running_var"], c["running_var"]), allow["rvar"] + c["ref_vs_f64_rvar"])
    assert ok


@pytest.mark.parametrize("ci", range(N_CASES))
def test_bf16_storage(ci):
    """inputs rounded to bf16 (the yardstick takes the rounded values, moved clear of the kink again in steps of 1/8, which bf16 holds):
    both sides in bf16 and either side alone; dx is stored in x's dtype; no bias"""
    cases, allow = srrl_fixture.load()
    c = cases[ci]
    x = _r16(V.clear(_r16(c["conv_out"]), c["gamma"], c["beta"], c["eps"]))
    assert not (np.abs(V.pre_activation(x, c["gamma"], c["beta"], c["eps"])) < V.TAU / 2).any()
    t = _r16(c["t"])
    want = _want(x, t, c["W"], None, c["l"], c["gamma"], c["beta"], c["eps"])
    ok = True
    for dt_x, dt_t in ((BF16, BF16), (BF16, F32), (F32, BF16)):
        got = run_abi(x, t, c["W"], None, c["l"], c["gamma"], c["beta"], c["eps"], dt_x, dt_t, g_loss=2.0)
        assert got["raw"]["dx"].dtype == dt_x
        ok &= check(f"case {ci} {dt_x} {dt_t}", got, want, allow, g_loss=2.0, bf16_out=dt_x == BF16)
    op = run_op(x, t, c["W"], None, c["l"], c["gamma"], c["beta"], c["eps"], BF16, BF16)
    ok &= check(f"case {ci} op bf16", op, want, allow, bf16_out=True)
    assert ok


EDGES = [  # (B, C, K): sizes at which the kernels take another path
    (3, 16, 64),        # exactly one workgroup of channels, one tile of classes
    (17, 17, 65),       # one element into the second workgroup / tile on every side; 17 rows: two passes of the row lanes
    (70, 65, 3),        # a second row tile; a reduction of 65 channels: three segments, split three ways
    (2, 2100, 2),       # 66 segments over one tile: 66 splits
    (130, 40, 600),     # 3 x 10 tiles for p (two segments, whole), 3 x 1 tiles for q (19 segments of classes, split)
    (257, 7, 5),        # the loss kernel's rows past one pass of 256 threads
]


@pytest.mark.parametrize("ei", range(len(EDGES)))
def test_edges_against_the_restatement(ei):
    B, Cc, K = EDGES[ei]
    _cases, allow = srrl_fixture.load()
    args = _draw(B, Cc, K, 100 + ei)
    want = _want(*args)
    got = run_abi(*args, g_loss=3.0)
    assert check(f"B {B} C {Cc} K {K}", got, want, allow, g_loss=3.0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_offset_base_pointers(dtype):
    """each side in turn starts one element behind an aligned address, C a multiple of 8; then both sides"""
    _cases, allow = srrl_fixture.load()
    args = _draw(4, 16, 6, 23)
    want = _want(*args)
    ok = True
    for off_x, off_t in ((True, False), (False, True), (True, True)):
        got = run_abi(*args, dt_x=dtype, dt_t=dtype, off_x=off_x, off_t=off_t, g_loss=3.0)
        ok &= check(f"offset x={int(off_x)} t={int(off_t)}", got, want, allow, g_loss=3.0, bf16_out=dtype == BF16)
    assert ok


def test_special_channels():
    """channel 0 constant (var = 0) with beta = 0.5; channel 1 with gamma = 0 and beta = 0 (mask all zero: every gradient of that channel
    exactly 0); channel 2 with every y below 0 (likewise); channel 3 ordinary"""
    _cases, allow = srrl_fixture.load()
    x, t, W, b, l, gamma, beta = _draw(5, 4, 3, 77)
    x[:, 0] = 1.25
    gamma[:], beta[:] = (1.5, 0.0, 0.5, -0.75), (0.5, 0.0, -40.0, 0.25)
    x = V.clear(x, gamma, beta, EPS).astype(np.float32)
    assert np.all(x[:, 0] == 1.25)
    want = _want(x, t, W, b, l, gamma, beta)
    assert want["var"][0] == 0 and np.all(want["y"][:, 0] == 0.5) and not want["y"][:, 1].any() and not want["y"][:, 2].any()
    for dt in (F32, BF16):
        xr, tr = (_r16(x), _r16(t)) if dt == BF16 else (x, t)
        w = _want(xr, tr, W, b, l, gamma, beta)
        got = run_abi(xr, tr, W, b, l, gamma, beta, dt_x=dt, dt_t=dt, g_loss=5.0)
        assert check(f"special {dt}", got, w, allow, g_loss=5.0, bf16_out=dt == BF16)
        for ch in (1, 2):
            assert not got["dx"][:, ch].any() and got["d_gamma"][ch] == 0 and got["d_beta"][ch] == 0
            assert got["A"][ch] == 0 and got["B"][ch] == 0
        # the constant channel: xh = 0, so d_gamma = 0 exactly
        assert got["d_gamma"][0] == 0 and got["B"][0] == 0


def test_target_equal_to_the_output_and_logits_equal_to_the_prediction():
    """t = y and l = p as a first call reports them (fp32, what the loss saw): loss 0, A = B = 0 and every gradient exactly 0"""
    x, t, W, b, l, gamma, beta = _draw(6, 40, 9, 5)
    first = run_abi(x, t, W, b, l, gamma, beta)
    y, p = first["y"].astype(np.float32), first["p"].astype(np.float32)
    assert (y > 0).any() and (y == 0).any()
    got = run_abi(x, y, W, b, p, gamma, beta, g_loss=7.0)
    assert got["loss"] == 0 and not got["dx"].any() and not got["d_gamma"].any() and not got["d_beta"].any() and not got["sums"].any()
    only_t = run_abi(x, y, W, b, l, gamma, beta)
    want = _want(x, y.astype(np.float64), W, b, l, gamma, beta)
    _cases, allow = srrl_fixture.load()
    assert _report("t = y alone: the loss is the prediction's", abs(only_t["loss"] - want["loss_pred"]) / want["loss_pred"], allow["loss"])


def test_upstream_gradient_scales_exactly():
    """g_loss is a device scalar: 2 against 1 gives the same bits times 2 in dx, d_gamma and d_beta, 0 gives exact zeros; through
    autograd likewise; the guards of the op"""
    from moma_amd import ops
    args = _draw(7, 24, 10, 8)
    for dt in (F32, BF16):
        one = run_abi(*args, dt_x=dt, dt_t=dt)
        for g in (2.0, 0.5, 1024.0):
            got = run_abi(*args, dt_x=dt, dt_t=dt, g_loss=g)
            for k in ("dx", "d_gamma", "d_beta"):
                assert torch.equal(got["raw"][k].float(), one["raw"][k].float() * g), (dt, g, k)
            assert all(torch.equal(got["raw"][k], one["raw"][k]) for k in ("loss", "sums", "dxu"))
        zero = run_abi(*args, dt_x=dt, dt_t=dt, g_loss=0.0)
        assert not zero["dx"].any() and not zero["d_gamma"].any() and not zero["d_beta"].any()
    a, b2 = run_op(*args), run_op(*args, g_loss=2.0)
    assert all(torch.equal(b2["raw"][k], a["raw"][k] * 2.0) for k in ("dx", "d_gamma", "d_beta"))
    x, t, W, b, l, gamma, beta = (torch.from_numpy(v).cuda() for v in args)
    rm, rv = torch.zeros(24, device="cuda"), torch.ones(24, device="cuda")
    call = lambda **kw: ops.srrl_bn_relu_dual_mse(**{**dict(x=x, target=t, cls_weight=W, cls_bias=b, logits=l, weight=gamma, bias=beta,    # noqa: E731
                                                          running_mean=rm, running_var=rv, momentum=MOM, eps=EPS), **kw})
    with torch.no_grad():
        assert float(call()) == a["loss"]
    assert not call(running_mean=None, running_var=None).requires_grad
    assert call(weight=gamma.clone().requires_grad_(True)).requires_grad
    with pytest.raises(TypeError):
        call(x=x.half(), target=t.half())
    with pytest.raises(ValueError):
        call(target=t[:, :20].contiguous())
    with pytest.raises(ValueError):
        call(x=x.t().contiguous().t())                                                                # not contiguous
    with pytest.raises(ValueError):
        call(target=t.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        call(logits=l.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        call(momentum=None)                                                                           # cumulative average
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        call(x=x[:1].contiguous(), target=t[:1].contiguous(), logits=l[:1].contiguous())
    with pytest.raises(ValueError):
        call(x=x[:, :20].contiguous(), target=t[:, :20].contiguous())                                 # the classifier's width


def test_one_row_and_shapes_past_the_caps_are_returned_errors():
    """B = 1: MOMA_E_SHAPE; B, C or K past the caps: MOMA_E_UNSUPPORTED; from both entry points, nothing launched, nothing written"""
    lib, guard = _lib(), _Guarded()
    e = lambda n, dt=F32: guard.empty(n, device="cuda", dtype=dt)             # noqa: E731
    x, t, v, d = e(8), e(8), e(8), e(16, torch.float64)
    for z in (x, t, v, d):
        z.fill_(1.5)
    big = 1 << 30

    def fwd(B, Cc, K):
        return lib.moma_srrl_fwd(_p(x), _p(t), _p(v), _p(v), _p(v), _p(v), _p(v), _p(v), _p(v), MOM, EPS, B, Cc, K, 0, 0, _p(d), big,
                                 _p(d), _p(v), _p(v), _p(v), _p(v), _st())

    def bwd(B, Cc):
        return lib.moma_srrl_bwd(_p(v), _p(d), _p(v), _p(x), _p(v), _p(v), B, Cc, 0, _st())

    assert lib.moma_srrl_workspace_bytes(1, 8, 1) == 0 and fwd(1, 8, 1) == -2 and bwd(1, 8) == -2
    for shape in ((1025, 2, 2), (2, 4097, 2), (2, 2, 1025)):
        assert lib.moma_srrl_workspace_bytes(*shape) == 0 and fwd(*shape) == -6
    assert bwd(1025, 2) == -6 and bwd(2, 4097) == -6
    assert guard.check("refused shapes") > 0
    assert all(bool((z == 1.5).all()) for z in (x, t, v, d))                  # nothing written


def test_two_calls_give_the_same_bits():
    for (B, Cc, K, dtype) in [(16, 1280, 4, F32), (8, 200, 100, BF16), (33, 72, 33, F32)]:
        args = _draw(B, Cc, K, Cc)
        a, b = (run_abi(*args, dt_x=dtype, dt_t=dtype) for _ in range(2))
        for k in a["raw"]:
            assert torch.equal(a["raw"][k], b["raw"][k]), ((B, Cc, K), k)
        o1, o2 = (run_op(*args, EPS, dtype, dtype) for _ in range(2))
        assert all(torch.equal(o1["raw"][k], o2["raw"][k]) for k in o1["raw"]) and o1["loss"] == a["loss"]
        assert torch.equal(o1["raw"]["dx"], a["raw"]["dx"])


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.srrl_bn_relu_dual_mse with every buffer it allocates (A and B, dx for g = 1, the workspace, loss, dx, d weight, d bias)
    between NaN margins, at ragged shapes and both dtypes: margins untouched, results bit-equal to the same call on ordinary
    allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (B, Cc, K, dtype) in [(3, 5, 7, F32), (5, 33, 9, BF16), (2, 200, 5, BF16), (9, 3, 70, F32)]:
        x, t, W, b, l, gamma, beta = _draw(B, Cc, K, Cc * 7 + B)
        a, tt = torch.from_numpy(x).to(dtype).cuda(), torch.from_numpy(t).to(dtype).cuda()
        tW, tb, tl = torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(l).cuda()
        ga, be = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()

        def run(wrap):
            xx = wrap(a).requires_grad_(True)
            g, bb = ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
            rm, rv = torch.zeros(Cc, device="cuda"), torch.ones(Cc, device="cuda")
            loss = ops.srrl_bn_relu_dual_mse(xx, wrap(tt), wrap(tW), wrap(tb), wrap(tl), g, bb, rm, rv, MOM, EPS)
            (loss * 2.5).backward()
            return loss.detach().clone(), xx.grad.clone(), g.grad.clone(), bb.grad.clone(), rm, rv

        plain = run(lambda z: z.clone())
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda z: _in(guard, z))
            assert guard.check(f"srrl_bn_relu_dual_mse {(B, Cc, K)}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_op_agrees_with_autograd_through_the_stock_chain_in_float64():
    """the op's gradients (fp32 storage) against torch.autograd through batch_norm -> relu -> mse_loss, linear -> mse_loss in float64
    on the device"""
    _cases, allow = srrl_fixture.load()
    x, t, W, b, l, gamma, beta = _draw(6, 12, 5, 41)
    op = run_op(x, t, W, b, l, gamma, beta, g_loss=3.0)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64)).cuda()          # noqa: E731
    tx, tg, tb = d(x).requires_grad_(True), d(gamma).requires_grad_(True), d(beta).requires_grad_(True)
    rm, rv = torch.zeros(12, device="cuda", dtype=torch.float64), torch.ones(12, device="cuda", dtype=torch.float64)
    y = F.relu(F.batch_norm(tx, rm, rv, tg, tb, True, MOM, EPS))
    loss = F.mse_loss(y, d(t)) + F.mse_loss(F.linear(y, d(W), d(b)), d(l))
    (3.0 * loss).backward()
    want = {"loss": float(loss), "dx": _np(tx.grad) / 3.0, "d_gamma": _np(tg.grad) / 3.0, "d_beta": _np(tb.grad) / 3.0,
            "running_mean": _np(rm), "running_var": _np(rv)}
    assert check("op vs float64 autograd", op, want, allow, g_loss=3.0)


def _connector_of(c):
    m = SRRL(s_n=c["s_n"], t_n=c["t_n"])
    lin = nn.Linear(c["t_n"], c["n_cls"])
    with torch.no_grad():
        m.transfer[0].weight.copy_(torch.from_numpy(c["w"]))
        m.transfer[1].weight.copy_(torch.from_numpy(c["gamma"]))
        m.transfer[1].bias.copy_(torch.from_numpy(c["beta"]))
        lin.weight.copy_(torch.from_numpy(c["W"]))
        lin.bias.copy_(torch.from_numpy(c["b"]))
    return m.cuda().train(), lin.cuda().eval()


def _count_calls(monkeypatch):
    from moma_amd import ops
    calls = []
    real = ops.srrl_bn_relu_dual_mse

    def spy(x, t, *a, **kw):
        calls.append((x.dtype, t.dtype))
        return real(x, t, *a, **kw)
    monkeypatch.setattr(ops, "srrl_bn_relu_dual_mse", spy)
    return calls


CHAIN = [i for i in range(N_CASES) if i in (0, 1, 2, 3, 4, 8)]


@pytest.mark.parametrize("ci", CHAIN)
def test_connector_loss_kernels_against_the_composite_fp32(ci, monkeypatch):
    """SRRL.loss (F.linear + the kernels) against float64 (the restatement of the chain) within the fixture's allowances, and against
    the composite fed the same convolution output; [B, C, 1, 1] features give the same bits; an EfficientNet-style classifier
    (inactive Dropout + Linear) takes the kernels too"""
    calls = _count_calls(monkeypatch)
    cases, allow = srrl_fixture.load()
    c = cases[ci]
    w = V.chain(c["f_s"], c["t"], c["w"], c["W"], c["b"], c["l"], c["gamma"], c["beta"], c["eps"], 1.0, np.zeros(c["t_n"]),
                np.ones(c["t_n"]), c["momentum"])

    def run(mode):
        m, lin = _connector_of(c)
        f = torch.from_numpy(c["f_s"]).cuda().requires_grad_(True)
        t, l = torch.from_numpy(c["t"]).cuda(), torch.from_numpy(c["l"]).cuda()
        if mode == "composite":
            x = F.linear(f, m.transfer[0].weight.view(c["t_n"], c["s_n"]))
            loss = m.composite(x, t, l, lin)
        elif mode == "4d":
            loss = m.loss(f[:, :, None, None], t[:, :, None, None], l, nn.Sequential(nn.Dropout(0.2), lin).eval())
        else:
            loss = m.loss(f, t, l, lin)
        loss.backward()
        bn = m.transfer[1]
        assert lin.weight.grad is None
        return {"loss": float(loss), "dxs": _np(f.grad), "dw": _np(m.transfer[0].weight.grad).reshape(c["t_n"], c["s_n"]),
                "d_gamma": _np(bn.weight.grad), "d_beta": _np(bn.bias.grad), "running_mean": _np(bn.running_mean),
                "running_var": _np(bn.running_var), "n": int(bn.num_batches_tracked)}

    got, flat, comp = run("kernels"), run("4d"), run("composite")
    assert calls == [(F32, F32), (F32, F32)] and got["n"] == flat["n"] == comp["n"] == 1
    assert all(np.array_equal(got[k], flat[k]) for k in got)
    ok = True
    for k, kind, key in (("loss", "chain_loss", "loss"), ("dxs", "dxs", "dx_s"), ("dw", "dw", "dw"), ("d_gamma", "dgamma", "d_gamma"),
                         ("d_beta", "dbeta", "d_beta"), ("running_mean", "rmean", "running_mean"), ("running_var", "rvar", "running_var")):
        dist = (lambda a, b: abs(a - b) / abs(b)) if k == "loss" else rel
        own = dist(comp[k], w[key])
        if kind in srrl_fixture.CHAIN_KINDS:
            # what the fixture recorded for the whole chain: against float64, and against the composite with its own distance added
            ok &= _report(f"{k} vs float64", dist(got[k], w[key]), allow[kind])
            ok &= _report(f"{k} vs the composite (itself {own:.1e} from float64)", dist(got[k], comp[k]), allow[kind] + own)
        else:
            # the tail's own results: the allowances were recorded for the tail on ONE convolution output, and the composite is the
            # float64 evaluation of the tail on the very output the kernels read (the library's fp32 GEMM is some 1e-7 away from
            # the float64 chain by itself, which is not the tail's to answer for); its results are stored in fp32: half an ulp more
            print(f"  {k}: the composite is {own:.1e} from the float64 chain")
            ok &= _report(f"{k} vs the composite", dist(got[k], comp[k]), allow[kind] + ULP32 / 2)
    assert ok


@pytest.mark.parametrize("ci", [2, 4])
def test_connector_loss_kernels_against_the_composite_bf16_autocast(ci, monkeypatch):
    """under bf16 autocast F.linear hands the kernels a bf16 [B, t_n] map; the comparison is made against the composite (float64) fed the
    SAME bf16-rounded convolution output and bf16 target, so only the tail differs: the fp32 allowances, dx (stored in bf16) plus
    half a bf16 ulp"""
    calls = _count_calls(monkeypatch)
    cases, allow = srrl_fixture.load()
    c = cases[ci]
    m, lin = _connector_of(c)
    f = torch.from_numpy(c["f_s"]).cuda()
    t, l = torch.from_numpy(c["t"]).cuda().to(BF16), torch.from_numpy(c["l"]).cuda()
    with torch.autocast("cuda", dtype=BF16):
        x16 = F.linear(f, m.transfer[0].weight.view(c["t_n"], c["s_n"])).detach()
    assert x16.dtype == BF16
    xq = V.clear(_np(x16), c["gamma"], c["beta"], c["eps"])
    if not np.array_equal(xq, _np(x16)):                       # a rounded output on the kink: compare at the moved map through the op
        x16 = torch.from_numpy(xq.astype(np.float32)).cuda().to(BF16)
    want = _want(_np(x16), _np(t), c["W"], c["b"], c["l"], c["gamma"], c["beta"], c["eps"], c["momentum"])
    from moma_amd import ops
    xk = x16.clone().requires_grad_(True)
    bn = m.transfer[1]
    loss = ops.srrl_bn_relu_dual_mse(xk, t, lin.weight.detach(), lin.bias.detach(), l, bn.weight, bn.bias, bn.running_mean,
                                     bn.running_var, bn.momentum, bn.eps)
    loss.backward()
    got = {"loss": float(loss), "dx": _np(xk.grad), "d_gamma": _np(bn.weight.grad), "d_beta": _np(bn.bias.grad),
           "running_mean": _np(bn.running_mean), "running_var": _np(bn.running_var)}
    m2, lin2 = _connector_of(c)
    xc = x16.clone().requires_grad_(True)
    lc = m2.composite(xc, t, l, lin2)
    lc.backward()
    bn2 = m2.transfer[1]
    comp = {"loss": float(lc), "dx": _np(xc.grad), "d_gamma": _np(bn2.weight.grad), "d_beta": _np(bn2.bias.grad),
            "running_mean": _np(bn2.running_mean), "running_var": _np(bn2.running_var)}
    assert xk.grad.dtype == BF16
    ok = check("kernels vs float64", got, want, allow, bf16_out=True)
    ok &= check("composite vs float64 (its dx is rounded to bf16 too)", comp, want, allow, bf16_out=True)
    # and the module's own route under autocast reaches the kernels with bf16 operands
    m3, lin3 = _connector_of(c)
    with torch.autocast("cuda", dtype=BF16):
        out = m3.loss(f.clone().requires_grad_(True), t, l, lin3)
    out.backward()
    assert calls[-1] == (BF16, BF16) and out.dtype == F32 and bool(torch.isfinite(out)) and int(m3.transfer[1].num_batches_tracked) == 1
    assert ok


def test_connector_takes_the_kernels_or_the_composite(monkeypatch):
    from moma_amd import ops
    calls = _count_calls(monkeypatch)
    c = srrl_fixture.load()[0][3]
    m, lin = _connector_of(c)
    f, t, l = torch.from_numpy(c["f_s"]).cuda(), torch.from_numpy(c["t"]).cuda(), torch.from_numpy(c["l"]).cuda()
    ref = c["loss"]
    out = m.loss(f, t, l, lin)
    assert calls == [(F32, F32)] and out.dtype == F32 and out.dim() == 0 and abs(float(out) - ref) < 1e-5 * ref
    assert int(m.transfer[1].num_batches_tracked) == 1 and bool(m.transfer[1].running_mean.abs().sum() > 0)
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.loss(f, t.half(), l, lin)
    assert len(calls) == 1 and out.dtype == F32 and abs(float(out) - ref) < 3e-2 * ref                # float16: the composite
    assert len(calls) == 1 and np.isfinite(float(m.loss(f, t, l, nn.Sequential(nn.Dropout(0.5), lin).train())))   # an active Dropout
    assert len(calls) == 1 and np.isfinite(float(m.loss(f, t, l, nn.Sequential(lin, nn.Tanh()))))    # another classifier module
    tg = t.clone().requires_grad_(True)
    m.loss(f, tg, l, lin).backward()
    assert len(calls) == 1 and tg.grad is not None                                                    # a target with a gradient
    monkeypatch.setattr(ops, "srrl_native", lambda *a, **kw: False)
    assert abs(float(m.loss(f, t, l, lin)) - ref) < 1e-5 * ref and len(calls) == 1                    # routed away by the table
    monkeypatch.undo()
    calls = _count_calls(monkeypatch)
    m.transfer[1].momentum = None
    assert abs(float(m.loss(f, t, l, lin)) - ref) < 1e-5 * ref and not calls                          # cumulative average
    m.transfer[1].momentum = 0.1
    n = int(m.transfer[1].num_batches_tracked)
    m.eval()
    out = m.loss(f, t, l, lin)
    trans, pred = m(f, lin)
    assert not calls and abs(float(out) - float(F.mse_loss(trans, t) + F.mse_loss(pred, l))) < 1e-5 * float(out)   # eval mode
    assert int(m.transfer[1].num_batches_tracked) == n


ARGV = ["--distill", "srrl", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
        "--n_cls", "4", "--batch_size", "8", "-c", "1", "-d", "0", "-b", "1"]


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='srrl', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: the tail runs on the kernels;
    loss_kd is the restatement's value on the features and logits the two models produced in that step with the connector as it was
    before it; the step moves the convolution, gamma, beta and the running statistics and leaves the teacher alone; the same step
    under bf16 autocast with the graphed teacher hands the kernels bf16 maps and stays finite"""
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    calls = _count_calls(monkeypatch)
    _cases, allow = srrl_fixture.load()

    def loop(extra):
        opt = parse_option(ARGV + ["--steps_per_epoch", "1", "--learning_rate", "0.01", *extra])
        opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
        dev = torch.device("cuda", 0)
        opt.device = dev
        torch.manual_seed(31)
        model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
        con = module_list[1]
        before = {n: p.detach().clone() for n, p in con.state_dict().items()}
        teacher_before = [p.detach().clone() for p in model_t.parameters()]
        feats = {}

        def keep(k):
            def hook(_m, _i, out):
                if k not in feats:
                    feats[k] = ([f.detach().clone() for f in out[0]], out[1].detach().clone())
            return hook
        hooks = [mod.register_forward_hook(keep(k)) for k, mod in (("s", model_s), ("t", model_t))]
        opt.trace, opt.print_freq = [], 1000
        train_distill_moma(1, SyntheticLoader(1, 8, 32, 4, 5, dev), module_list, criterion_list, None, contrast, optimizer, opt)
        for h in hooks:
            h.remove()
        assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
        assert all(p.grad is None for p in model_t.parameters())
        return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace], feats, before, con, model_t

    losses, kds, feats, before, con, model_t = loop(["--no_graph_teacher"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all() and calls == [(F32, F32)]
    b = {k: v.cpu().numpy() for k, v in before.items()}
    fc = model_t.get_feat_modules()[-1]
    want = V.chain(feats["s"][0][-1].reshape(8, -1).cpu().numpy(), feats["t"][0][-1].reshape(8, -1).cpu().numpy(), b["transfer.0.weight"],
                   fc.weight.detach().cpu().numpy(), fc.bias.detach().cpu().numpy(), feats["t"][1].float().cpu().numpy(),
                   b["transfer.1.weight"], b["transfer.1.bias"], con.transfer[1].eps)
    print("loss_kd: %.6e  restatement: %.6e" % (kds[0], want["loss"]))
    assert _report("loss_kd of the step", abs(kds[0] - want["loss"]) / want["loss"], allow["chain_loss"])
    after = con.state_dict()
    for k in ("transfer.0.weight", "transfer.1.weight", "transfer.1.bias", "transfer.1.running_mean", "transfer.1.running_var"):
        assert not torch.equal(before[k], after[k]), k
    assert int(after["transfer.1.num_batches_tracked"]) == 1
    del calls[:]
    losses, kds, _f, _b, _c, _t = loop(["--amp", "bf16"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all()
    print("bf16 step: loss_kd %.6e, kernel calls %s" % (kds[0], calls))
    assert len(calls) == 1 and calls[0][0] == BF16


def test_cli_trains_checkpoints_and_resumes_with_distill_srrl(tmp_path):
    """`python train_student_moma.py --distill srrl` on the smallest synthetic configuration for two steps, then a second run that
    resumes from its checkpoint (key `model_fmsr`) for one more epoch"""
    from tests.test_gpu_cli import _run_cli
    r = _run_cli(tmp_path, ARGV + ["--epochs", "1", "--steps_per_epoch", "2"], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout and "nan" not in r.stdout.lower()
    cks = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == "ckpt_last.pth"]
    assert len(cks) == 1
    ck = torch.load(cks[0], map_location="cpu", weights_only=False)
    assert int(ck["model_fmsr"]["transfer.1.num_batches_tracked"]) == 2 and ck["epoch"] == 1
    r = _run_cli(tmp_path, ARGV + ["--epochs", "2", "--steps_per_epoch", "2", "--resume", cks[0]], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "resumed from" in r.stdout and "images/sec" in r.stdout and "nan" not in r.stdout.lower()
    cks = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == "ckpt_last.pth"]
    ck2 = max((torch.load(p, map_location="cpu", weights_only=False) for p in cks), key=lambda k: k["epoch"])
    assert int(ck2["model_fmsr"]["transfer.1.num_batches_tracked"]) == 4 and ck2["epoch"] == 2

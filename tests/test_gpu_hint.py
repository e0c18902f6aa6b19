"""GPU tests of the FitNets hint kernels (csrc/hint.hip) through the C ABI, ops.hint_bn_relu_mse, the regressor and the training loop.

Yardstick: the float64 evaluation of the formulas (tests/hint_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_loss / _dx / _dgamma / _dbeta / _rmean / _rvar`, and `_chain_loss / _dxs / _dw` for the whole
regressor) that the reference's own fp32 results keep from float64 over the cases of the golden fixture, never below one fp32 ulp
(2^-23, relative).  Metric: crd_ref.rel (units of the yardstick's largest element); the loss relative to its own value (a sum of
squares).  mean and invstd are doubles: 1e-10 of the largest |x| and 2^-24 (the fp32 eps).  A gradient stored in bf16 adds that rounding: half a bf16 ulp
(8 significant bits), at most 2^-8 of the element.  Every input is clear of the ReLU's kink (hint_ref.clear_of_kink); no element is
left out of a comparison.
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result."""
import ctypes as C

import numpy as np
import pytest
import torch

from moma_amd.distiller_zoo import ConvReg, HintLoss  # noqa: F401  (the modules under test: without them nothing here has a subject)
from tests import hint_fixture, hint_ref as V
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ULP32, HALF_ULP_BF16 = 2.0 ** -23, 2.0 ** -8
EPS, MOM = 1e-5, 0.1


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


def _chunk():
    from moma_amd import _lib as L
    return L.HINT_CHUNK


def run_abi(x, t, gamma, beta, eps=EPS, cl_x=False, cl_t=False, dt_x=F32, dt_t=F32, off_x=False, off_t=False, g_loss=1.0,
            conv_bias=None, momentum=MOM):
    """moma_hint_fwd -> moma_hint_bwd on fresh guarded buffers.  x, t: numpy [B,C,H,W].  -> dict of numpy float64 arrays (gradients
    times g_loss) and the raw device tensors under `raw`; the running statistics start from 0 / 1"""
    from moma_amd import _lib as L
    lib, guard = _lib(), _Guarded()
    B, Cc, H, W = x.shape
    P = H * W
    tx, tt = _place(guard, x, dt_x, cl_x, off_x), _place(guard, t, dt_t, cl_t, off_t)

    def vec(a, dtype=F32):
        v = guard.empty(len(a), device="cuda", dtype=dtype)
        v.copy_(torch.from_numpy(np.asarray(a, np.float64)).to(dtype))
        return v

    e = lambda *shape: guard.empty(*shape, device="cuda", dtype=F32)          # noqa: E731
    ga, be, rm, rv = vec(gamma), vec(beta), vec(np.zeros(Cc)), vec(np.ones(Cc))
    cb = vec(conv_bias) if conv_bias is not None else None
    codes = (*_codes(dt_x, cl_x), *_codes(dt_t, cl_t))
    nws = lib.moma_hint_workspace_bytes(B, Cc, P, *codes)
    bi = max(1, min(B, L.HINT_CHUNK // P))
    assert nws == 3 * -(-B // bi) * -(-P // L.HINT_CHUNK) * Cc * 8
    ws = guard.empty(nws // 8, device="cuda", dtype=torch.float64)
    loss = e(1)
    mean, invstd, sums = (guard.empty(n, device="cuda", dtype=torch.float64) for n in (Cc, Cc, 2 * Cc))
    rc = lib.moma_hint_fwd(_p(tx), _p(tt), _p(ga), _p(be), _p(cb), _p(rm), _p(rv), momentum, eps, B, Cc, P, *codes, _p(ws), nws,
                           _p(mean), _p(invstd), _p(sums), _p(loss), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    dx = _carve(guard, x.shape, dt_x, cl_x, off_x)                           # dtype and layout of x
    dga, dbe = e(Cc), e(Cc)
    rc = lib.moma_hint_bwd(_p(tx), _p(tt), _p(ga), _p(be), _p(mean), _p(invstd), _p(sums), _p(gl), _p(dx), _p(dga), _p(dbe), B, Cc, P,
                           *codes, _st())
    assert rc == 0, rc
    assert guard.check("hint C ABI") > 0                                      # every margin untouched
    raw = {"loss": loss, "mean": mean, "invstd": invstd, "sums": sums, "dx": dx, "d_gamma": dga, "d_beta": dbe, "running_mean": rm,
           "running_var": rv, "partials": ws}
    out = {k: _np(v) for k, v in raw.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out["loss"] = float(loss.item())
    out["A"], out["B"] = out["sums"][:Cc], out["sums"][Cc:]
    out["raw"] = raw
    return out


def run_op(x, t, gamma, beta, eps=EPS, cl_x=False, cl_t=False, dt_x=F32, dt_t=F32, g_loss=1.0, conv_bias=None, momentum=MOM):
    from moma_amd import ops
    mk = lambda f, cl, dt: torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dt).cuda().contiguous(    # noqa: E731
        memory_format=torch.channels_last if cl else torch.contiguous_format)
    vec = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()        # noqa: E731
    Cc = x.shape[1]
    tx, tt = mk(x, cl_x, dt_x).requires_grad_(True), mk(t, cl_t, dt_t)
    ga, be = vec(gamma).requires_grad_(True), vec(beta).requires_grad_(True)
    cb = vec(conv_bias).requires_grad_(True) if conv_bias is not None else None
    rm, rv = torch.zeros(Cc, device="cuda"), torch.ones(Cc, device="cuda")
    loss = ops.hint_bn_relu_mse(tx, tt, ga, be, rm, rv, momentum, eps, conv_bias=cb)
    (loss * g_loss).backward()
    assert tx.grad.stride() == tx.stride() and tx.grad.dtype == dt_x and tt.grad is None
    assert ga.grad.dtype == F32 and ga.grad.shape == ga.shape and be.grad.shape == be.shape
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    if cb is not None:
        assert cb.grad is not None and cb.grad.shape == cb.shape and not cb.grad.any()       # exact zeros
    return {"loss": float(loss), "dx": _np(tx.grad), "d_gamma": _np(ga.grad), "d_beta": _np(be.grad), "running_mean": _np(rm),
            "running_var": _np(rv), "raw": {"dx": tx.grad, "loss": loss.detach(), "d_gamma": ga.grad, "d_beta": be.grad}}


def check(tag, got, want, allow, g_loss=1.0, bf16_out=False, full=True, x_scale=1.0):
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
    if full:
        # kept in double: sums of at most 2^21 exact terms (1e-10 of the largest |x|, far below what fp32 results can show); eps
        # reaches the kernels as an fp32 number (2^-24 relative, seen by invstd only where the variance is no larger than eps)
        ok &= _report(f"{tag} mean", float(np.abs(got["mean"] - want["mean"]).max() / x_scale), 1e-10)
        ok &= _report(f"{tag} invstd", float((np.abs(got["invstd"] - want["invstd"]) / want["invstd"]).max()), 2.0 ** -24)
    return ok


def _want(x, t, gamma, beta, eps=EPS, conv_bias=None, momentum=MOM):
    Cc = x.shape[1]
    return V.tail(x, t, gamma, beta, eps, 1.0, np.zeros(Cc), np.ones(Cc), momentum, conv_bias)


def _affine(Cc):
    c = np.arange(Cc)
    gamma = 0.5 + ((c * 7) % 5) * 0.25
    gamma[c % 3 == 1] *= -1.0
    return gamma.astype(np.float32), (((c * 3) % 4 - 1.5) * 0.2).astype(np.float32)


def _draw(shape, seed, off=0.0):
    """(x, t, gamma, beta): normal draws rounded to multiples of 1/32 (exact in bf16), clipped to 4, x clear of the kink"""
    rng = np.random.default_rng(seed)
    gamma, beta = _affine(shape[1])
    q = lambda: np.clip(np.round(rng.standard_normal(shape) * 32) / 32, -4, 4) + off          # noqa: E731
    x = V.clear_of_kink(q(), gamma, beta, EPS).astype(np.float32)
    return x, q().astype(np.float32), gamma, beta


def _two_values(shape, seed):
    """inputs for M = 2 (B = 2, P = 1).  There xh = +-sqrt(var / (var + eps)) whatever the two values are: the output barely depends
    on x, and dx is the fraction eps / (var + eps) of the terms it is the difference of, so fp32 rounding of those terms (2^-24) shows
    in dx magnified by (var + eps) / eps -- for values a unit apart 1e5 times, in the reference's kernels as in any other.  The two
    values of a channel lie 1/32 apart here (var = 2^-12, eps / (var + eps) = 0.04): dx keeps 4 % of its terms and the comparison
    keeps its meaning.  The pre-activation is +-0.98 gamma + beta, clear of the kink for every (gamma, beta) of _affine"""
    x, t, gamma, beta = _draw(shape, seed)
    x[1] = x[0] + 1.0 / 32
    assert not (np.abs(V.pre_activation(x, gamma, beta, EPS)) < V.TAU).any()
    return x, t, gamma, beta


N_CASES = hint_fixture.N_CASES


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    """the reference's own convolution output and the teacher's map on the regressor's grid, as the regressor hands them to the kernels
    (the reference's output carries the convolution's bias: here it is part of x, and conv_bias is not given)"""
    cases, allow = hint_fixture.load()
    c = cases[ci]
    x, t = c["conv_out"], c["t_grid"]
    want = _want(x, t, c["gamma"], c["beta"], c["eps"], momentum=c["momentum"])
    print(f"case {ci} {c['s_shape']} -> {c['t_shape']}")
    abi = run_abi(x, t, c["gamma"], c["beta"], c["eps"], momentum=c["momentum"])
    ok = check("abi", abi, want, allow, x_scale=np.abs(x).max())
    op = run_op(x, t, c["gamma"], c["beta"], c["eps"], momentum=c["momentum"])
    ok &= check("op", op, want, allow, full=False)
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / c["loss"], allow["loss"] + c["ref_vs_f64_loss"])
    ok &= _report("op dx vs reference", rel(op["dx"], c["d_conv_out"]), allow["dx"] + c["ref_vs_f64_dx"])
    ok &= _report("op d_gamma vs reference", rel(op["d_gamma"], c["d_gamma"]), allow["dgamma"] + c["ref_vs_f64_dgamma"])
    ok &= _report("op d_beta vs reference", rel(op["d_beta"], c["d_beta"]), allow["dbeta"] + c["ref_vs_f64_dbeta"])
    ok &= _report("op running_mean vs reference", rel(op["running_mean"], c["running_mean"]), allow["rmean"] + c["ref_vs_f64_rmean"])
    ok &= _report("op running_var vs reference", rel(op["running_var"], c["running_var"]), allow["rvar"] + c["ref_vs_f64_rvar"])
    assert ok


@pytest.mark.parametrize("ci", range(N_CASES))
def test_layouts_agree(ci):
    """all four layout combinations of the two sides, upstream gradient 3: within the allowance of the float64 value"""
    cases, allow = hint_fixture.load()
    c = cases[ci]
    x, t = c["conv_out"], c["t_grid"]
    want = _want(x, t, c["gamma"], c["beta"], c["eps"])
    ok = True
    for cl_x, cl_t in ((False, False), (True, False), (False, True), (True, True)):
        got = run_abi(x, t, c["gamma"], c["beta"], c["eps"], cl_x, cl_t, g_loss=3.0)
        tag = f"case {ci} cl_x={int(cl_x)} cl_t={int(cl_t)}"
        ok &= check(tag, got, want, allow, g_loss=3.0, x_scale=np.abs(x).max())
        ok &= check(tag + " op", run_op(x, t, c["gamma"], c["beta"], c["eps"], cl_x, cl_t), want, allow, full=False)
    assert ok


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("ci", range(N_CASES))
def test_bf16_storage(ci, cl):
    """inputs rounded to bf16 (the yardstick takes the rounded values, moved clear of the kink again in steps of 1/8, which bf16 holds):
    both sides in bf16, either side alone, in both layouts, and a bf16 NCHW x against an fp32 channels_last t; dx is stored in x's dtype"""
    cases, allow = hint_fixture.load()
    c = cases[ci]
    x = _r16(V.clear_of_kink(_r16(c["conv_out"]), c["gamma"], c["beta"], c["eps"]))
    assert not (np.abs(V.pre_activation(x, c["gamma"], c["beta"], c["eps"])) < V.TAU / 2).any()
    t = _r16(c["t_grid"])
    want = _want(x, t, c["gamma"], c["beta"], c["eps"])
    ok = True
    for dt_x, dt_t, cl_x, cl_t in ((BF16, BF16, cl, cl), (BF16, F32, cl, cl), (F32, BF16, cl, cl), (BF16, F32, False, True)):
        got = run_abi(x, t, c["gamma"], c["beta"], c["eps"], cl_x, cl_t, dt_x, dt_t, g_loss=2.0)
        assert got["raw"]["dx"].dtype == dt_x
        ok &= check(f"case {ci} {dt_x} {dt_t} cl {int(cl_x)}{int(cl_t)}", got, want, allow, g_loss=2.0, bf16_out=dt_x == BF16,
                    x_scale=np.abs(x).max())
    op = run_op(x, t, c["gamma"], c["beta"], c["eps"], cl, cl, BF16, BF16)
    ok &= check(f"case {ci} op bf16", op, want, allow, bf16_out=True, full=False)
    assert ok


def _edges():
    K = _chunk()
    return [  # name, shape, layouts
        ("C=1", (2, 1, 6, 6), (False, True)),
        ("P=1 with B=2", (2, 5, 1, 1), (False, True)),          # (inputs: see _two_values)
        ("P=1, C=1283", (2, 1283, 1, 1), (False, True)),
        ("P=1023", (1, 3, 1, K - 1), (False, True)),
        ("P=1024: exactly one chunk", (1, 3, 1, K), (False, True)),
        ("P=1025: one element into the second chunk", (1, 3, 1, K + 1), (False, True)),
        ("a plane of three chunks, the last ragged, 8 channels", (2, 8, 1, 2 * K + 40), (False, True)),
        ("P=49: no vector width divides it", (2, 6, 7, 7), (False, True)),
        ("P=36: vectors of 4", (2, 7, 6, 6), (False,)),
        ("C=12 channels_last: vectors of 4", (2, 12, 3, 3), (True,)),
        ("C=72 channels_last: two tiles of channel vectors", (2, 72, 5, 5), (True,)),
        ("C=257 channels_last", (2, 257, 3, 3), (True,)),
        ("C=520: one lane per channel in the finalize kernels", (2, 520, 2, 2), (False, True)),
        ("B=65 with two channels", (65, 2, 2, 2), (False, True)),
    ]


@pytest.mark.parametrize("ei", range(14))
def test_edges_against_the_restatement(ei):
    """the smallest shapes at which the kernels take another path, with an upstream gradient of 3 and a convolution bias"""
    name, shape, layouts = _edges()[ei]
    _cases, allow = hint_fixture.load()
    x, t, gamma, beta = (_two_values if shape[0] * shape[2] * shape[3] == 2 and shape[1] < 100 else _draw)(
        shape, shape[1] * 1000 + shape[2] * 10 + shape[3])
    cb = np.linspace(-1, 1, shape[1]).astype(np.float32)
    want = _want(x, t, gamma, beta, conv_bias=cb)
    ok = True
    for cl in layouts:
        got = run_abi(x, t, gamma, beta, cl_x=cl, cl_t=cl, g_loss=3.0, conv_bias=cb)
        ok &= check(f"{name} {'channels_last' if cl else 'NCHW'}", got, want, allow, g_loss=3.0, x_scale=np.abs(x).max())
    assert ok


def test_special_channels():
    """channel 0 constant (var = 0) with beta = 0.5; channel 1 with gamma = 0 and beta = 0 (mask all zero: every gradient of that channel
    exactly 0); channel 2 with every y below 0 (likewise); channel 3 ordinary"""
    _cases, allow = hint_fixture.load()
    x, t, gamma, beta = _draw((3, 4, 5, 5), 77)
    x[:, 0] = 1.25
    gamma[:], beta[:] = (1.5, 0.0, 0.5, -0.75), (0.5, 0.0, -40.0, 0.25)
    x = V.clear_of_kink(x, gamma, beta, EPS).astype(np.float32)
    assert np.all(x[:, 0] == 1.25)
    want = _want(x, t, gamma, beta)
    assert want["var"][0] == 0 and np.all(want["y"][:, 0] == 0.5) and not want["y"][:, 1].any() and not want["y"][:, 2].any()
    for cl in (False, True):
        for dt in (F32, BF16):
            xr, tr = (_r16(x), _r16(t)) if dt == BF16 else (x, t)
            w = _want(xr, tr, gamma, beta)
            got = run_abi(xr, tr, gamma, beta, cl_x=cl, cl_t=cl, dt_x=dt, dt_t=dt, g_loss=5.0)
            assert check(f"special cl={int(cl)} {dt}", got, w, allow, g_loss=5.0, bf16_out=dt == BF16, x_scale=4.0)
            assert abs(got["invstd"][0] * np.sqrt(np.float64(np.float32(EPS))) - 1) < 1e-15
            for ch in (1, 2):
                assert not got["dx"][:, ch].any() and got["d_gamma"][ch] == 0 and got["d_beta"][ch] == 0
                assert got["A"][ch] == 0 and got["B"][ch] == 0
            # the constant channel: xh = 0, so d_gamma = 0 exactly and dx = k gamma invstd (g - A / M) sums to nothing over the channel
            assert got["d_gamma"][0] == 0 and got["B"][0] == 0


def test_target_equal_to_the_output():
    """x = +-a_c in equal halves with gamma a power of two: mean, variance and y are exact in fp32 and known in advance; t = y gives
    loss 0, A = B = 0 and every gradient exactly 0"""
    B, Cc, H, W = 2, 3, 4, 4
    a = np.array([0.75, 1.5, 3.0], np.float32)
    gamma, beta = np.array([1.0, 2.0, -0.5], np.float32), np.array([0.3125, -0.1, 0.7], np.float32)
    sign = np.where((np.arange(B * H * W) % 2) == 0, 1.0, -1.0).reshape(B, 1, H, W).astype(np.float32)
    x = sign * a.reshape(1, Cc, 1, 1)
    inv = 1.0 / np.sqrt(a.astype(np.float64) ** 2 + np.float64(np.float32(EPS)))
    xh = (x.astype(np.float64) * inv.reshape(1, Cc, 1, 1)).astype(np.float32)
    y = np.maximum((gamma.reshape(1, Cc, 1, 1).astype(np.float64) * xh + beta.reshape(1, Cc, 1, 1)).astype(np.float32), 0)
    assert (y > 0).any() and (y == 0).any()
    for cl in (False, True):
        got = run_abi(x, y, gamma, beta, cl_x=cl, cl_t=cl, g_loss=7.0)
        assert not got["mean"].any() and np.abs(got["invstd"] / inv - 1).max() < 1e-15
        assert got["loss"] == 0 and not got["dx"].any() and not got["d_gamma"].any() and not got["d_beta"].any()
        assert not got["sums"].any()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cl", [False, True])
def test_offset_base_pointers(cl, dtype):
    """each side in turn starts one element behind an aligned address, C and P both multiples of 8: no 16-byte access is possible on
    that side, so the pair is walked element by element; then both sides"""
    _cases, allow = hint_fixture.load()
    x, t, gamma, beta = _draw((2, 8, 4, 4), 23 + int(cl))
    want = _want(x, t, gamma, beta)
    ok = True
    for off_x, off_t in ((True, False), (False, True), (True, True)):
        got = run_abi(x, t, gamma, beta, cl_x=cl, cl_t=cl, dt_x=dtype, dt_t=dtype, off_x=off_x, off_t=off_t, g_loss=3.0)
        ok &= check(f"offset x={int(off_x)} t={int(off_t)}", got, want, allow, g_loss=3.0, bf16_out=dtype == BF16, x_scale=4.0)
    assert ok


def test_upstream_gradient_scales_exactly():
    """g_loss is a device scalar: 2 against 1 gives the same bits times 2 in dx, d_gamma and d_beta, 0 gives exact zeros; through
    autograd likewise; the guards of the op"""
    from moma_amd import ops
    x, t, gamma, beta = _draw((3, 12, 7, 7), 8)
    for cl, dt in ((False, F32), (True, F32), (False, BF16), (True, BF16)):
        one = run_abi(x, t, gamma, beta, cl_x=cl, cl_t=cl, dt_x=dt, dt_t=dt)
        for g in (2.0, 0.5, 1024.0):
            got = run_abi(x, t, gamma, beta, cl_x=cl, cl_t=cl, dt_x=dt, dt_t=dt, g_loss=g)
            for k in ("dx", "d_gamma", "d_beta"):
                assert torch.equal(got["raw"][k].float(), one["raw"][k].float() * g), (cl, dt, g, k)
            assert torch.equal(got["raw"]["loss"], one["raw"]["loss"]) and torch.equal(got["raw"]["sums"], one["raw"]["sums"])
        zero = run_abi(x, t, gamma, beta, cl_x=cl, cl_t=cl, dt_x=dt, dt_t=dt, g_loss=0.0)
        assert not zero["dx"].any() and not zero["d_gamma"].any() and not zero["d_beta"].any()
    a, b = run_op(x, t, gamma, beta), run_op(x, t, gamma, beta, g_loss=2.0)
    assert all(torch.equal(b["raw"][k], a["raw"][k] * 2.0) for k in ("dx", "d_gamma", "d_beta"))
    tx, tt = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    ga, be = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    rm, rv = torch.zeros(12, device="cuda"), torch.ones(12, device="cuda")
    with torch.no_grad():
        assert float(ops.hint_bn_relu_mse(tx, tt, ga, be, rm, rv, MOM, EPS)) == a["loss"]
    assert not ops.hint_bn_relu_mse(tx, tt, ga, be, None, None, MOM, EPS).requires_grad
    assert ops.hint_bn_relu_mse(tx, tt, ga.clone().requires_grad_(True), be, None, None, MOM, EPS).requires_grad
    with pytest.raises(TypeError):
        ops.hint_bn_relu_mse(tx.half(), tt.half(), ga, be, rm, rv, MOM, EPS)
    with pytest.raises(ValueError):
        ops.hint_bn_relu_mse(tx, tt[:, :, :, :6], ga, be, rm, rv, MOM, EPS)
    with pytest.raises(ValueError):
        ops.hint_bn_relu_mse(tx.permute(0, 1, 3, 2), tt.permute(0, 1, 3, 2), ga, be, rm, rv, MOM, EPS)     # dense, neither layout
    with pytest.raises(ValueError):
        ops.hint_bn_relu_mse(tx, tt.clone().requires_grad_(True), ga, be, rm, rv, MOM, EPS)
    with pytest.raises(ValueError):
        ops.hint_bn_relu_mse(tx, tt, ga, be, rm, rv, None, EPS)                                           # cumulative average
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.hint_bn_relu_mse(tx[:1, :, :1, :1].contiguous(), tt[:1, :, :1, :1].contiguous(), ga, be, rm, rv, MOM, EPS)


def test_one_value_per_channel_is_a_returned_error():
    """M = 1: MOMA_E_SHAPE from both entry points, nothing launched, nothing written"""
    lib, guard = _lib(), _Guarded()
    e = lambda n, dt=F32: guard.empty(n, device="cuda", dtype=dt)             # noqa: E731
    x, t, v, d = e(8), e(8), e(8), e(16, torch.float64)
    for z in (x, t, v, d):
        z.fill_(1.5)
    assert lib.moma_hint_workspace_bytes(1, 8, 1, 0, 0, 0, 0) == 0
    rc = lib.moma_hint_fwd(_p(x), _p(t), _p(v), _p(v), None, None, None, MOM, EPS, 1, 8, 1, 0, 0, 0, 0, _p(d), 1 << 20, _p(v), _p(v), _p(d),
                           _p(v), _st())
    assert rc == -2
    assert lib.moma_hint_bwd(_p(x), _p(t), _p(v), _p(v), _p(v), _p(v), _p(d), _p(v), _p(x), _p(v), _p(v), 1, 8, 1, 0, 0, 0, 0, _st()) == -2
    assert guard.check("M = 1") > 0
    assert all(bool((z == 1.5).all()) for z in (x, t, v, d))                  # nothing written


def test_two_calls_give_the_same_bits():
    for (shape, cl, dtype) in [((4, 112, 14, 14), False, F32), ((4, 40, 28, 28), True, BF16), ((3, 24, 56, 56), False, BF16),
                               ((2, 1280, 4, 4), True, F32), ((2, 200, 5, 5), False, F32)]:
        x, t, gamma, beta = _draw(shape, shape[1])
        a, b = (run_abi(x, t, gamma, beta, cl_x=cl, cl_t=cl, dt_x=dtype, dt_t=dtype) for _ in range(2))
        for k in a["raw"]:
            assert torch.equal(a["raw"][k], b["raw"][k]), (shape, k)
        o1, o2 = (run_op(x, t, gamma, beta, EPS, cl, cl, dtype, dtype) for _ in range(2))
        assert all(torch.equal(o1["raw"][k], o2["raw"][k]) for k in o1["raw"]) and o1["loss"] == a["loss"]


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.hint_bn_relu_mse with every buffer it allocates (partials, mean, invstd, A and B, loss, dx, d weight, d bias, the zeros of
    conv_bias) between NaN margins, at ragged shapes and both dtypes: margins untouched, results bit-equal to the same call on ordinary
    allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (shape, cl, dtype) in [((3, 5, 7, 7), False, F32), ((2, 24, 9, 9), True, BF16), ((2, 200, 5, 5), False, BF16),
                               ((5, 3, 10, 10), True, F32), ((1, 3, 1, _chunk() + 7), False, F32)]:
        x, t, gamma, beta = _draw(shape, shape[1] * 7 + shape[2])
        mf = torch.channels_last if cl else torch.contiguous_format
        a = torch.from_numpy(x).to(dtype).cuda().contiguous(memory_format=mf)
        b = torch.from_numpy(t).to(dtype).cuda().contiguous(memory_format=mf)
        ga, be = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        cb = torch.linspace(-1, 1, shape[1], device="cuda")

        def run(wrap):
            xx, tt = wrap(a).requires_grad_(True), wrap(b)
            g, bb, c = ga.clone().requires_grad_(True), be.clone().requires_grad_(True), cb.clone().requires_grad_(True)
            rm, rv = torch.zeros(shape[1], device="cuda"), torch.ones(shape[1], device="cuda")
            loss = ops.hint_bn_relu_mse(xx, tt, g, bb, rm, rv, MOM, EPS, conv_bias=c)
            (loss * 2.5).backward()
            return loss.detach().clone(), xx.grad.clone(), g.grad.clone(), bb.grad.clone(), c.grad.clone(), rm, rv

        plain = run(lambda z: z.clone(memory_format=torch.preserve_format))
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda z: z.clone(memory_format=torch.preserve_format) if cl else _in(guard, z))
            assert guard.check(f"hint_bn_relu_mse {shape}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def _regressor_of(c):
    reg = ConvReg(c["s_shape"], c["t_shape"])
    with torch.no_grad():
        reg.conv.weight.copy_(torch.from_numpy(c["w"]))
        reg.conv.bias.copy_(torch.from_numpy(c["b"]))
        reg.bn.weight.copy_(torch.from_numpy(c["gamma"]))
        reg.bn.bias.copy_(torch.from_numpy(c["beta"]))
    return reg.cuda().train()


def _count_calls(monkeypatch):
    from moma_amd import ops
    calls = []
    real = ops.hint_bn_relu_mse

    def spy(x, t, *a, **kw):
        calls.append((x.dtype, t.dtype))
        return real(x, t, *a, **kw)
    monkeypatch.setattr(ops, "hint_bn_relu_mse", spy)
    return calls


def test_regressor_takes_the_kernels_or_the_composite(monkeypatch):
    """on GPU tensors in training mode: the kernels in fp32 and under bf16 autocast (the convolution's output arrives in bf16), in
    channels_last too; the composite for eval mode, float16 storage, momentum=None, a shape ops.hint_native refuses and a target that
    records a gradient; both routes advance num_batches_tracked; token lists are refused"""
    from moma_amd import ops
    calls = _count_calls(monkeypatch)
    c4 = hint_fixture.load()[0][4]                      # 9 x 9 planes in fp32 NCHW: the class the routing table keeps off the kernels
    _regressor_of(c4).loss(torch.from_numpy(c4["x"]).cuda(), torch.from_numpy(c4["t"]).cuda())
    assert not calls
    c = hint_fixture.load()[0][5]
    reg = _regressor_of(c)
    x, t = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["t"]).cuda()
    ref = c["loss"]
    out = reg.loss(x, t)
    assert calls == [(F32, F32)] and out.dtype == F32 and out.dim() == 0 and abs(float(out) - ref) < 1e-5 * ref
    assert int(reg.bn.num_batches_tracked) == 1 and bool(reg.bn.running_mean.abs().sum() > 0)
    with torch.autocast("cuda", dtype=BF16):
        out = reg.loss(x, t.to(BF16))
    assert calls[1:] == [(BF16, BF16)] and out.dtype == F32 and abs(float(out) - ref) < 3e-2 * ref
    out = reg.loss(x.contiguous(memory_format=torch.channels_last), t.contiguous(memory_format=torch.channels_last))
    assert len(calls) == 3 and abs(float(out) - ref) < 1e-5 * ref and int(reg.bn.num_batches_tracked) == 3
    with torch.autocast("cuda", dtype=torch.float16):
        out = reg.loss(x, t.half())
    assert len(calls) == 3 and out.dtype == F32 and abs(float(out) - ref) < 3e-2 * ref            # float16: the composite
    assert int(reg.bn.num_batches_tracked) == 4
    tg = t.clone().requires_grad_(True)
    reg.loss(x, tg).backward()
    assert len(calls) == 3 and tg.grad is not None and bool(tg.grad.abs().sum() > 0)              # a target with a gradient: likewise
    monkeypatch.setattr(ops, "hint_native", lambda B, Cc, P, **kw: False)
    assert abs(float(reg.loss(x, t)) - ref) < 1e-5 * ref and len(calls) == 3                      # routed away by the table
    monkeypatch.undo()
    calls = _count_calls(monkeypatch)
    reg.bn.momentum = None
    assert abs(float(reg.loss(x, t)) - ref) < 1e-5 * ref and not calls                            # cumulative average
    reg.bn.momentum = 0.1
    n = int(reg.bn.num_batches_tracked)
    rm = reg.bn.running_mean.clone()
    reg.eval()
    out = reg.loss(x, t)
    f_s, f_t = reg(x, t)
    assert not calls and abs(float(out) - float(HintLoss()(f_s, f_t))) < 1e-5 * float(out)        # eval mode: the running statistics
    assert int(reg.bn.num_batches_tracked) == n and torch.equal(rm, reg.bn.running_mean)
    with pytest.raises(ValueError, match="feature maps"):
        reg.loss(torch.randn(2, 17, 24, device="cuda"), torch.randn(2, 17, 24, device="cuda"))


@pytest.mark.parametrize("ci", [i for i in range(N_CASES) if i != 8])
def test_regressor_loss_agrees_with_the_stock_chain_fp32(ci, monkeypatch):
    """ConvReg.loss (convolution without its bias + the kernels) against float64 where the restatement covers the chain (1 x 1 branch)
    and against the reference's fp32 results in every branch, within the fixture's allowances; and against
    HintLoss(*ConvReg.forward(...)) in stock ops on the same device: no further from it than the allowance plus the distance the
    stock evaluation itself keeps from the same anchor (float64 on the 1 x 1 branch, the reference's results, with their own distance
    from float64, elsewhere) -- the stock kernels of the device are another fp32 evaluation, and at M = 2 a poorly conditioned one.
    The bias gradient is exact zeros; the running mean carries the bias"""
    from moma_amd import ops
    monkeypatch.setattr(ops, "hint_native", lambda *a, **kw: True)      # (the routing table is not the subject: every case on the kernels)
    calls = _count_calls(monkeypatch)
    cases, allow = hint_fixture.load()
    c = cases[ci]
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False

    def run(fused):
        reg = _regressor_of(c)
        x, t = torch.from_numpy(c["x"]).cuda().requires_grad_(True), torch.from_numpy(c["t"]).cuda()
        loss = reg.loss(x, t) if fused else HintLoss()(*reg(x, t))
        loss.backward()
        return {"loss": float(loss), "dxs": _np(x.grad), "dw": _np(reg.conv.weight.grad), "db": _np(reg.conv.bias.grad),
                "d_gamma": _np(reg.bn.weight.grad), "d_beta": _np(reg.bn.bias.grad), "running_mean": _np(reg.bn.running_mean),
                "running_var": _np(reg.bn.running_var), "n": int(reg.bn.num_batches_tracked)}

    got, stock = run(True), run(False)
    assert calls == [(F32, F32)] and got["n"] == stock["n"] == 1 and not got["db"].any()
    print(f"case {ci} {c['s_shape']} -> {c['t_shape']}")
    ok = True
    pairs = (("loss", "chain_loss"), ("dxs", "dxs"), ("dw", "dw"), ("d_gamma", "dgamma"), ("d_beta", "dbeta"),
             ("running_mean", "rmean"), ("running_var", "rvar"))
    refs = {"loss": c["loss"], "dxs": c["dx_s"], "dw": c["dw"], "d_gamma": c["d_gamma"], "d_beta": c["d_beta"],
            "running_mean": c["running_mean"], "running_var": c["running_var"]}
    anchors, slack = refs, {kind: c["ref_vs_f64_" + kind] for _k, kind in pairs}
    if ci <= 7:
        w = V.chain(c["x"], c["t"], c["w"], c["b"], c["gamma"], c["beta"], c["eps"], 1.0, np.zeros(c["t_shape"][1]),
                    np.ones(c["t_shape"][1]), c["momentum"])
        anchors = {"loss": w["loss"], "dxs": w["dx_s"], "dw": w["dw"].reshape(c["dw"].shape), "d_gamma": w["d_gamma"],
                   "d_beta": w["d_beta"], "running_mean": w["running_mean"], "running_var": w["running_var"]}
        slack = {kind: 0.0 for _k, kind in pairs}
    for k, kind in pairs:
        dist = (lambda a, b: abs(a - b) / abs(b)) if k == "loss" else rel
        ok &= _report(f"{k} vs reference", dist(got[k], refs[k]), allow[kind] + c["ref_vs_f64_" + kind])
        # (all three distances in units of the anchor's largest element, so that the triangle inequality holds to the last digit)
        unit = float(np.abs(np.asarray(anchors[k], np.float64)).max())
        away = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / unit      # noqa: E731
        own, mine = away(stock[k], anchors[k]), away(got[k], anchors[k])
        print(f"  {k}: stock ops from the anchor {own:.3e}")
        ok &= _report(f"{k} vs the anchor", mine, allow[kind] + slack[kind])
        ok &= _report(f"{k} vs stock ops", away(got[k], stock[k]), allow[kind] + slack[kind] + own)
    if ci <= 7:
        ok &= _report("loss vs float64", abs(got["loss"] - w["loss"]) / w["loss"], allow["chain_loss"])
        ok &= _report("dxs vs float64", rel(got["dxs"], w["dx_s"]), allow["dxs"])
        ok &= _report("dw vs float64", rel(got["dw"].reshape(w["dw"].shape), w["dw"]), allow["dw"])
        ok &= _report("running_mean vs float64", rel(got["running_mean"], w["running_mean"]), allow["rmean"])
    assert ok


@pytest.mark.parametrize("ci", [1, 4, 5, 7])
def test_regressor_loss_agrees_with_the_stock_chain_bf16_autocast(ci, monkeypatch):
    """under bf16 autocast the 1 x 1 convolution runs on the streaming kernel where ops.pwconv_fwd_native admits the shape (case 7) and
    the kernels read bf16 maps.  Yardstick: the float64 chain over the bf16-rounded operands (input, target, weight).  Allowance: twice
    the distance HintLoss(*ConvReg.forward(...)) in stock ops shows under the same autocast, measured here"""
    calls = _count_calls(monkeypatch)
    c = hint_fixture.load()[0][ci]
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    xr, tr, wr = _r16(c["x"]), _r16(c["t"]), _r16(c["w"])
    w = V.chain(xr, tr, wr, c["b"], c["gamma"], c["beta"], c["eps"])

    def run(fused):
        reg = _regressor_of(c)
        x = torch.from_numpy(xr.astype(np.float32)).cuda().requires_grad_(True)
        t = torch.from_numpy(tr.astype(np.float32)).cuda().to(BF16)
        with torch.autocast("cuda", dtype=BF16):
            loss = reg.loss(x, t) if fused else HintLoss()(*reg(x, t))
        loss.backward()
        return {"loss": abs(float(loss) - w["loss"]) / w["loss"], "dxs": rel(_np(x.grad), w["dx_s"]),
                "dw": rel(_np(reg.conv.weight.grad).reshape(w["dw"].shape), w["dw"]),
                "d_gamma": rel(_np(reg.bn.weight.grad), w["d_gamma"]), "d_beta": rel(_np(reg.bn.bias.grad), w["d_beta"])}

    fused, stock = run(True), run(False)
    assert calls == [(BF16, BF16)]
    ok = True
    for k in fused:
        print(f"  {k}: stock ops {stock[k]:.3e}")
        ok &= _report(k, fused[k], 2 * max(stock[k], ULP32))
    assert ok


ARGV = ["--distill", "hint", "--hint_layer", "1", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
        "--n_cls", "4", "--batch_size", "8", "-c", "1", "-d", "1", "-b", "100"]


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
    reg = module_list[1]
    before = {n: p.detach().clone() for n, p in reg.state_dict().items()}
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
    return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace], feats, before, reg


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='hint', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: the pair runs on the kernels;
    loss_kd is the restatement's value on the feature maps the two models produced in that step with the regressor as it was before
    it; the step moves the convolution, gamma, beta and the running statistics; the same step in channels_last under bf16 autocast
    hands the kernels bf16 maps and stays finite"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    calls = _count_calls(monkeypatch)
    _cases, allow = hint_fixture.load()
    losses, kds, feats, before, reg = _loop([])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all() and calls == [(F32, F32)]
    b = {k: v.cpu().numpy() for k, v in before.items()}
    want = V.chain(feats["s"][1].cpu().numpy(), feats["t"][1].cpu().numpy(), b["conv.weight"], b["conv.bias"], b["bn.weight"], b["bn.bias"],
                   reg.bn.eps)
    print("loss_kd: %.6e  restatement: %.6e" % (kds[0], want["loss"]))
    assert _report("loss_kd of the step", abs(kds[0] - want["loss"]) / want["loss"], allow["chain_loss"])
    after = reg.state_dict()
    for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
        assert not torch.equal(before[k], after[k]), k
    assert int(after["bn.num_batches_tracked"]) == 1
    del calls[:]
    losses, kds, feats, _before, reg = _loop(["--channels_last", "--amp", "bf16"])
    assert len(kds) == 1 and np.isfinite(kds).all() and np.isfinite(losses).all()
    print("bf16 / channels_last step: loss_kd %.6e, kernel calls %s" % (kds[0], calls))
    assert calls == [(BF16, BF16)]


def test_cli_runs_with_distill_hint(tmp_path):
    """`python train_student_moma.py --distill hint --hint_layer 1` on the smallest synthetic configuration: parses, builds, trains and
    validates"""
    from tests.test_gpu_cli import _run_cli
    r = _run_cli(tmp_path, ARGV + ["--epochs", "1", "--steps_per_epoch", "2"], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout and "nan" not in r.stdout.lower()

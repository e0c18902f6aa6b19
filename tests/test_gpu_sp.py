"""GPU tests of the Similarity-Preserving distillation kernels (csrc/sp.hip) through the C ABI, ops.sp_loss, the criterion, the
training loop and the CLI.

Conventions as in tests/test_gpu_nst.py's header.  Yardstick: the float64 evaluation of the formulas (tests/sp_ref.py).  Allowance
for every floating-point result: TWICE the largest distance of that kind (`ref_vs_f64_loss / _grad / _G / _H`) that the reference's
own fp32 results keep from that evaluation over the cases of the golden fixture, never below one fp32 ulp (2^-23, relative).
Metric: crd_ref.rel (units of the yardstick's largest element); the loss in units of the loss (one sample: the loss is 0, absolute).
G takes the `G` allowance, H `H`, M and dF_s `grad`.  Every comparison prints the share of its allowance it used (`_report`).
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result.

bf16 storage: the Gram of a bf16 side runs on the bf16-input MFMA (exact products, fp32 sums in another order than the fp32 side's
chain), so its bits differ from the fp32 run's: each is held to the allowance.  A bf16 dF_s carries bf16's own rounding on top: one
rounding to nearest at 8 significand bits (the implicit one included), i.e. at most half a spacing of 2^-7 of the binade = 2^-8 of
the element (the unit roundoff 2^-p, p = 8; fp32: 2^-24), which the comparison adds per element and nothing more."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sp_fixture, sp_ref as R
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
RAW = ("ws_s", "ws_t", "G", "H", "rows", "M", "loss", "dF_s")
N_CASES = len(sp_fixture.CASES)


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


def _bf16_exact(a):
    return torch.from_numpy(np.asarray(a, np.float32)).bfloat16().float().numpy()


def _place(guard, f, dtype=F32, offset=False):
    """numpy [B, ...] -> a device tensor [B, K] between NaN margins, optionally starting one element behind an aligned address"""
    t = torch.from_numpy(np.ascontiguousarray(f)).to(dtype).reshape(len(f), -1)
    flat = guard.empty(t.numel() + int(offset), device="cuda", dtype=dtype)
    if offset:
        flat[0] = float("nan")
        flat = flat[1:]
    out = flat.view(t.shape)
    out.copy_(t)
    return out


def _code(dtype):
    from moma_amd import _lib as L
    return L.DT_BF16 if dtype == BF16 else L.DT_F32


def _np(t):
    return t.double().cpu().numpy()


def _splits(B, K):
    nt = -(-B // 64)
    return min(-(-K // 128), -(-512 // (nt * (nt + 1) // 2)))


def run_abi(f_s, f_t, dt_s=F32, dt_t=F32, off_s=False, off_t=False, g_loss=1.0):
    """moma_sp_gram x 2 -> moma_sp_terms -> moma_sp_bwd on fresh guarded buffers, the maps in the storage order they are given in.
    -> dict of numpy float64 arrays G_s, G_t, H_s, H_t, M, dF_s [B, Ks], the loss, and the raw device tensors under `raw`"""
    lib, guard = _lib(), _Guarded()
    B = len(f_s)
    ts, tt = _place(guard, f_s, dt_s, off_s), _place(guard, f_t, dt_t, off_t)
    Ks, Kt = ts.shape[1], tt.shape[1]
    e = lambda *shape, dtype=F32: guard.empty(*shape, device="cuda", dtype=dtype)          # noqa: E731
    n_s, n_t = lib.moma_sp_workspace_bytes(B, Ks), lib.moma_sp_workspace_bytes(B, Kt)
    assert n_s == _splits(B, Ks) * B * B * 4 and n_t == _splits(B, Kt) * B * B * 4
    ws_s, ws_t = e(n_s // 4), e(n_t // 4)
    G, H, rows, M, loss = e(2, B, B, dtype=F64), e(2, B, B, dtype=F64), e(4, B, dtype=F64), e(B, B, dtype=F64), e(1)
    rc = lib.moma_sp_gram(_p(ts), B, Ks, _code(dt_s), _p(ws_s), n_s, _st())
    assert rc == 0, rc
    rc = lib.moma_sp_gram(_p(tt), B, Kt, _code(dt_t), _p(ws_t), n_t, _st())
    assert rc == 0, rc
    rc = lib.moma_sp_terms(_p(ws_s), n_s, Ks, _p(ws_t), n_t, Kt, B, _p(G), _p(H), _p(rows), _p(M), _p(loss), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    flat = guard.empty(ts.numel() + int(off_s), device="cuda", dtype=dt_s)
    dF = (flat[1:] if off_s else flat).view(ts.shape)
    rc = lib.moma_sp_bwd(_p(ts), _p(M), _p(gl), _p(dF), B, Ks, _code(dt_s), _st())
    assert rc == 0, rc
    assert guard.check("sp C ABI") > 0                                         # every margin untouched
    raw = {"ws_s": ws_s, "ws_t": ws_t, "G": G, "H": H, "rows": rows, "M": M, "loss": loss, "dF_s": dF}
    for k, v in raw.items():
        assert bool(torch.isfinite(v.float() if v.dtype == BF16 else v).all()), k
    out = {"G_s": _np(G[0]), "G_t": _np(G[1]), "H_s": _np(H[0]), "H_t": _np(H[1]), "M": _np(M), "dF_s": _np(dF),
           "n_s": _np(rows[0]), "n_t": _np(rows[1]), "loss": float(loss.item()), "raw": raw, "bf16_grad": dt_s == BF16}
    return out


def run_op(f_s, f_t, dt_s=F32, dt_t=F32, g_loss=1.0, crit=None, cl=False):
    """f_s, f_t: numpy [B, ...] (logical shape); cl: both maps in channels_last"""
    from moma_amd import ops
    mf = torch.channels_last if cl else torch.contiguous_format
    ts = torch.from_numpy(np.ascontiguousarray(f_s)).to(dt_s).cuda().contiguous(memory_format=mf).requires_grad_(True)
    tt = torch.from_numpy(np.ascontiguousarray(f_t)).to(dt_t).cuda().contiguous(memory_format=mf)
    loss = ops.sp_loss(ts, tt) if crit is None else crit([ts], [tt])[0]
    (loss * g_loss).backward()
    assert ts.grad.stride() == ts.stride() and ts.grad.dtype == dt_s and ts.grad.shape == ts.shape and tt.grad is None
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    return loss.detach(), ts.grad


def _grad_ok(tag, got, want, allow, bf16):
    """fp32: crd_ref.rel within the grad allowance.  bf16: the same plus one rounding to bf16 per element (2^-8 of the element)"""
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    if not want.any():
        return _report(f"{tag} dF_s (yardstick 0, absolute)", float(np.abs(got).max()), allow)
    if not bf16:
        return _report(f"{tag} dF_s", rel(got, want), allow)
    room = allow * np.abs(want).max() + 2.0 ** -8 * np.abs(want)
    return _report(f"{tag} dF_s (bf16: allowance + 2^-8 of the element)", float((np.abs(got - want) / room).max()), 1.0)


def check(tag, got, want, allow, full=True, grad=True):
    """got: G, H, M (full) and loss, dF_s against the restatement's"""
    B = want["G_s"].shape[0]
    scale = want["loss"] if B > 1 and want["loss"] > 0 else 1.0
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / scale, allow["loss"])
    if grad:
        ok &= _grad_ok(tag, got["dF_s"], want["dF_s"].reshape(B, -1), allow["grad"], got.get("bf16_grad", False))
    if full:
        for k in ("G_s", "G_t"):
            assert np.array_equal(got[k], got[k].T), k                         # one computation per pair
            ok &= _report(f"{tag} {k}", rel(got[k], want[k]) if want[k].any() else float(np.abs(got[k]).max()), allow["G"])
        for k in ("H_s", "H_t"):
            ok &= _report(f"{tag} {k}", rel(got[k], want[k]) if want[k].any() else float(np.abs(got[k]).max()), allow["H"])
        assert np.array_equal(got["M"], got["M"].T)
        ok &= _report(f"{tag} M", rel(got["M"], want["M"]) if want["M"].any() else float(np.abs(got["M"]).max()), allow["grad"])
    return ok


_WANT = {}


def fixture_case(ci):
    """(case, float64 results) -- evaluated once, shared by the tests"""
    cases, allow = sp_fixture.load()
    if ci not in _WANT:
        _WANT[ci] = R.pair(cases[ci]["f_s"], cases[ci]["f_t"])
    return cases[ci], _WANT[ci], allow


def _ref_grad(c, got):
    """distance of the reference's recorded gradient (the long case: its stored columns) from `got`, in units of got's largest"""
    got = np.asarray(got, np.float64).reshape(c["shape"][0], -1)
    d = np.abs(c["dF_s"].reshape(got.shape) - got).max() if "dF_s" in c else np.abs(c["dF_s_cols"] - got[:, ::sp_fixture.LONG_STRIDE]).max()
    return float(d / max(np.abs(got).max(), 1e-300))


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    c, want, allow = fixture_case(ci)
    B = c["shape"][0]
    print(f"case {ci} {c['shape']} {c['note']}")
    abi = run_abi(c["f_s"], c["f_t"])
    ok = check("abi", abi, want, allow)
    if c["note"] == "zero":                                                    # the clamp: H = 0 on the all-zero rows, Q = E / 1e-12
        assert abi["n_s"][sp_fixture.ZERO_S] == 0 and not abi["H_s"][sp_fixture.ZERO_S].any() and not abi["H_t"][sp_fixture.ZERO_T].any()
    if B == 1:
        assert abi["loss"] == 0 and not abi["dF_s"].any() and abs(abi["H_s"][0, 0]) == 1
    loss, dF_s = run_op(c["f_s"], c["f_t"])
    op = {"loss": float(loss), "dF_s": _np(dF_s)}
    ok &= check("op", op, want, allow, full=False)
    assert np.isfinite(op["dF_s"]).all()
    assert float(loss) == abi["loss"] and np.array_equal(op["dF_s"].reshape(B, -1), abi["dF_s"])      # the op is the C ABI sequence
    if B > 1:
        # against the reference's own fp32 results: each side is within its allowance of the float64 value
        ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / want["loss"], allow["loss"] + c["ref_vs_f64_loss"])
        ok &= _report("op dF_s vs reference", _ref_grad(c, op["dF_s"]), allow["grad"] + c["ref_vs_f64_grad"])
    assert ok


@pytest.mark.parametrize("ci", range(N_CASES))
def test_bf16_storage_per_side(ci):
    """the fixture's inputs are exact in bf16: either side alone and both in bf16 meet the same allowance (a bf16 side's Gram runs on
    the bf16-input MFMA); the op on bf16 tensors is the C ABI sequence"""
    c, want, allow = fixture_case(ci)
    ok = True
    for dt_s, dt_t in ((BF16, BF16), (BF16, F32), (F32, BF16)):                 # (fp32, fp32): the test above
        b = run_abi(c["f_s"], c["f_t"], dt_s, dt_t)
        assert b["raw"]["dF_s"].dtype == dt_s
        ok &= check(f"s={dt_s} t={dt_t}", b, want, allow)
    lb, db = run_op(c["f_s"], c["f_t"], BF16, BF16)
    assert db.dtype == BF16
    both = run_abi(c["f_s"], c["f_t"], BF16, BF16)
    assert float(lb) == both["loss"] and torch.equal(db.reshape(both["raw"]["dF_s"].shape), both["raw"]["dF_s"])
    assert ok


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_channels_last_against_nchw(dtype):
    """the same values as NCHW-contiguous and as channels_last maps: both within the allowance of the restatement (no bit equality:
    the columns are summed in storage order), the gradient in the strides of its input"""
    _cases, allow = sp_fixture.load()
    rng = np.random.default_rng(44)
    f_s, f_t = _bf16_exact(rng.standard_normal((6, 24, 5, 5))), _bf16_exact(rng.standard_normal((6, 40, 3, 3)) + 0.5)
    want = R.pair(f_s, f_t, g_loss=2.0)
    ok = True
    for cl in (False, True):
        loss, dF = run_op(f_s, f_t, dtype, dtype, g_loss=2.0, cl=cl)
        assert dF.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        got = {"loss": float(loss), "dF_s": _np(dF), "bf16_grad": dtype == BF16}
        ok &= check(f"{'channels_last' if cl else 'NCHW'} {dtype}", got, want, allow, full=False)
    # through the C ABI: the channels_last map is handed over as it lies in memory, the gradient comes back in that order
    perm = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))              # noqa: E731
    abi = run_abi(perm(f_s), perm(f_t), dtype, dtype, g_loss=2.0)
    want_cl = dict(want, dF_s=perm(want["dF_s"]))
    ok &= check(f"abi, storage order of channels_last {dtype}", abi, want_cl, allow)
    assert ok


EDGES = [  # name, B, Ks, Kt, student pointer one element past an aligned address, teacher likewise
    ("K=1", 5, 1, 1, False, False),
    ("B=1", 1, 70, 9, False, False),
    ("K=63: below the fp32 slab", 5, 63, 127, False, False),
    ("K=64 / 128: one slab exactly, 16-byte loads", 5, 64, 128, False, False),
    ("K=65 / 129: a second slab of one column", 5, 65, 129, False, False),
    ("K=127 / 255, odd: element loads of bf16", 5, 127, 255, False, False),
    ("K=136 / 264: two slabs, 16-byte loads, a ragged tail", 5, 136, 264, False, False),
    ("student behind an offset pointer", 9, 128, 64, True, False),
    ("teacher behind an offset pointer", 9, 64, 128, False, True),
    ("B=17: one past a tile of M", 17, 12, 20, False, False),
    ("B=33: one past an MFMA subtile", 33, 72, 16, False, False),
    ("B=65: one past a tile of G, three tile pairs", 65, 40, 24, False, False),
    ("B=129: one past the backward's row block", 129, 65, 8, False, False),
    ("B=130, K=11131: last split ragged, empty splits, element loads", 130, 11131, 300, False, False),
    ("B=130, K=11128: last split ragged, empty splits, 16-byte loads", 130, 11128, 304, False, False),
]


@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_edges_against_the_restatement(edge):
    """the smallest shapes at which the kernels take another path, with an upstream gradient of 3, in fp32 and in bf16"""
    name, B, Ks, Kt, off_s, off_t = edge
    _cases, allow = sp_fixture.load()
    rng = np.random.default_rng(B * 1000 + Ks * 10 + Kt)
    f_s, f_t = _bf16_exact(rng.standard_normal((B, Ks))), _bf16_exact(rng.standard_normal((B, Kt)) + 0.5)
    want = R.pair(f_s, f_t, g_loss=3.0)
    if B == 130:                                                               # the plan the case is about
        per_bf, per_f = -(-(-(-Ks // 128)) // _splits(B, Ks)), -(-(-(-Ks // 64)) // _splits(B, Ks))
        assert per_bf * (_splits(B, Ks) - 1) >= -(-Ks // 128) and per_f * (_splits(B, Ks) - 1) >= -(-Ks // 64)      # empty splits
        assert -(-Ks // 128) % per_bf and Ks % 128                             # a last split short of slabs, a last slab short of columns
    ok = check(f"{name} fp32", run_abi(f_s, f_t, F32, F32, off_s, off_t, g_loss=3.0), want, allow)
    ok &= check(f"{name} bf16", run_abi(f_s, f_t, BF16, BF16, off_s, off_t, g_loss=3.0), want, allow)
    assert ok


def test_the_largest_batch():
    """B = MOMA_SP_MAX_B = 1024 with K = 8: 136 tile pairs, one split, grids and workspace at the limit"""
    from moma_amd import _lib as L
    _cases, allow = sp_fixture.load()
    B = L.SP_MAX_B
    rng = np.random.default_rng(1024)
    f_s, f_t = _bf16_exact(rng.standard_normal((B, 8))), _bf16_exact(rng.standard_normal((B, 5)))
    want = R.pair(f_s, f_t)
    ok = check("B = 1024 fp32", run_abi(f_s, f_t), want, allow)
    ok &= check("B = 1024 bf16", run_abi(f_s, f_t, BF16, BF16), want, allow)
    assert ok


def test_upstream_gradient():
    """g_loss is a device scalar folded in before the one rounding: 0.5 scales every bit pattern exactly, 0 gives zeros, 3 gives the
    restatement's gradient at g_loss = 3"""
    c, want, allow = fixture_case(6)
    one = run_abi(c["f_s"], c["f_t"])
    half = run_abi(c["f_s"], c["f_t"], g_loss=0.5)
    assert torch.equal(half["raw"]["dF_s"], one["raw"]["dF_s"] * 0.5) and torch.equal(half["raw"]["M"], one["raw"]["M"])
    zero = run_abi(c["f_s"], c["f_t"], g_loss=0.0)
    assert not zero["raw"]["dF_s"].any()
    b1, bh = run_abi(c["f_s"], c["f_t"], BF16, F32), run_abi(c["f_s"], c["f_t"], BF16, F32, g_loss=0.5)
    assert torch.equal(bh["raw"]["dF_s"], b1["raw"]["dF_s"] * 0.5)
    three = run_abi(c["f_s"], c["f_t"], g_loss=3.0)
    assert _report("dF_s at g = 3", rel(three["dF_s"], 3.0 * want["dF_s"]), allow["grad"])
    # through autograd: a scaled loss reaches the kernel as that scalar
    l1, d1 = run_op(c["f_s"], c["f_t"])
    l2, d2 = run_op(c["f_s"], c["f_t"], g_loss=0.5)
    assert torch.equal(l1, l2) and torch.equal(d2, d1 * 0.5)


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(77)
    for B, Ks, Kt, dt in ((64, 6272, 1280, F32), (130, 1000, 24, BF16), (33, 515, 2048, F32), (70, 4096, 4100, BF16)):
        f_s, f_t = rng.standard_normal((B, Ks)).astype(np.float32), rng.standard_normal((B, Kt)).astype(np.float32)
        a, b = run_abi(f_s, f_t, dt, dt), run_abi(f_s, f_t, dt, dt)
        for k in RAW:
            assert torch.equal(a["raw"][k], b["raw"][k]), (k, B)


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.sp_loss with every buffer it allocates (workspaces, G, H, rows, M, loss, dF) between NaN margins, at ragged shapes and
    both dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    for (B, Ks, Kt, dtype) in [(5, 7, 9, F32), (19, 129, 40, BF16), (67, 200, 3, F32), (3, 1037, 520, BF16)]:
        rng = np.random.default_rng(B * 7 + Ks)
        a = torch.from_numpy(rng.standard_normal((B, Ks)).astype(np.float32)).to(dtype).cuda()
        b = torch.from_numpy(rng.standard_normal((B, Kt)).astype(np.float32)).to(dtype).cuda()

        def run():
            x = a.clone().requires_grad_(True)
            loss = ops.sp_loss(x, b)
            (loss * 2.5).backward()
            return loss.detach().clone(), x.grad.clone()

        plain = run()
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run()
            assert guard.check(f"sp_loss {B} {Ks} {Kt}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_op_and_criterion(monkeypatch):
    """the criterion hands dense fp32 / bf16 device maps to the op and returns a list of 0-dim fp32 scalars; float16, a batch above
    the limit, a teacher that wants a gradient and a map that is not dense go to the composite and agree with the kernels; the
    error paths of the op"""
    from moma_amd import _lib as L, ops
    from moma_amd.distiller_zoo import Similarity
    c, want, allow = fixture_case(4)
    crit = Similarity()
    calls = []
    real = ops.sp_loss
    monkeypatch.setattr(ops, "sp_loss", lambda *a: (calls.append(1), real(*a))[1])
    l0, d0 = run_op(c["f_s"], c["f_t"], crit=crit)
    assert len(calls) == 1
    ok = check("criterion", {"loss": float(l0), "dF_s": _np(d0)}, want, allow, full=False)
    lr, dr = run_op(c["f_s"], c["f_t"])                                        # (the op called directly: counted too)
    assert torch.equal(l0, lr) and torch.equal(d0, dr) and len(calls) == 2     # the op and the criterion agree bit for bit
    l4, d4 = run_op(c["f_s"][:, :, None, None], c["f_t"][:, :, None, None], crit=crit)     # [B, C, 1, 1]: the same bits, 4-D gradient
    assert d4.dim() == 4 and torch.equal(l4, l0) and torch.equal(d4.flatten(1), d0) and len(calls) == 3
    ts, tt = torch.from_numpy(c["f_s"]).cuda(), torch.from_numpy(c["f_t"]).cuda()
    with torch.no_grad():
        assert float(real(ts, tt)) == float(l0)
    assert not real(ts, tt).requires_grad                                      # nobody wants a gradient: nothing is saved
    n = len(calls)
    # float16 storage: the composite (the fixture's values are exact in bf16, not in fp16: its yardstick is the fp16 values')
    sh = ts.half().requires_grad_(True)
    lh = crit([sh], [tt.half()])[0]
    lh.backward()
    wh = R.pair(sh.detach().float().cpu().numpy(), tt.half().float().cpu().numpy())
    ok &= _report("fp16 composite loss", abs(float(lh.detach()) - wh["loss"]) / wh["loss"], allow["loss"])
    ok &= _report("fp16 composite dF_s (+ fp16 rounding 2^-11)", rel(_np(sh.grad), wh["dF_s"]), allow["grad"] + 2.0 ** -11)
    # a teacher that wants a gradient: the composite, and it gets one
    sg, tg = ts.clone().requires_grad_(True), tt.clone().requires_grad_(True)
    lg = crit([sg], [tg])[0]
    lg.backward()
    assert len(calls) == n and tg.grad is not None and bool(torch.isfinite(tg.grad).all()) and bool(tg.grad.abs().sum() > 0)
    ok &= check("composite (teacher gradient)", {"loss": float(lg.detach()), "dF_s": _np(sg.grad)}, want, allow, full=False)
    ok &= _report("composite vs kernels, loss", abs(float(lg.detach()) - float(l0)) / want["loss"], 2 * allow["loss"])
    ok &= _report("composite vs kernels, dF_s", rel(_np(sg.grad), _np(d0)), 2 * allow["grad"])
    # a batch above the limit (the limit itself is served by the kernels: test_the_largest_batch)
    monkeypatch.setattr(L, "SP_MAX_B", 4)
    s5 = ts.clone().requires_grad_(True)
    l5 = crit([s5], [tt])[0]
    l5.backward()
    assert len(calls) == n
    ok &= check("composite (B above the limit)", {"loss": float(l5.detach()), "dF_s": _np(s5.grad)}, want, allow, full=False)
    with pytest.raises(ValueError):
        real(ts, tt)                                                           # the op itself refuses it
    monkeypatch.setattr(L, "SP_MAX_B", 1024)
    # a map that is not dense: the composite; the op names the strides
    wide = torch.randn(8, 140, device="cuda")
    assert bool(torch.isfinite(crit([wide[:, :131]], [tt])[0])) and len(calls) == n
    with pytest.raises(ValueError, match="strides"):
        real(wide[:, :131], tt)
    with pytest.raises(ValueError):
        real(ts, tg)                                                           # a teacher that wants a gradient
    with pytest.raises(ValueError):
        real(ts, tt[:-1])                                                      # batch sizes differ
    with pytest.raises(TypeError):
        real(ts.half(), tt.half())
    assert ok


def _loop(extra, steps=1):
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    argv = ["--distill", "similarity", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
            "--batch_size", "8", "--steps_per_epoch", str(steps), "-c", "1", "-d", "1", "-b", "1", "--learning_rate", "0.01",
            "--no_graph_teacher", *extra]
    opt = parse_option(argv)
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
    dev = torch.device("cuda", 0)
    opt.device = dev
    torch.manual_seed(31)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
    feats = {}

    def keep(k):                                                               # feat[-2] of the first step
        def hook(_m, _i, out):
            feats.setdefault(k, out[0][-2].detach().clone())
        return hook
    hooks = [m.register_forward_hook(keep(k)) for k, m in (("s", model_s), ("t", model_t))]
    before = [p.detach().clone() for p in model_s.parameters()]
    opt.trace, opt.print_freq = [], 1000
    train_distill_moma(1, SyntheticLoader(steps, 8, 32, 4, 5, dev), module_list, criterion_list, None, contrast, optimizer, opt)
    for h in hooks:
        h.remove()
    moved = any(not torch.equal(a, b) for a, b in zip(before, model_s.parameters()))
    return opt.trace, feats, moved


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='similarity', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, `--amp bf16 --channels_last`:
    the pair reaches the kernels as bf16 channels_last maps, loss_kd is the restatement's value on feat[-2] of that step, the loss
    is finite and the student's weights change"""
    from moma_amd import ops
    _cases, allow = sp_fixture.load()
    calls = []
    real = ops.sp_loss

    def spy(f_s, f_t):
        calls.append((f_s.dtype, f_t.dtype, f_s.dim() == 4 and f_s.is_contiguous(memory_format=torch.channels_last)))
        return real(f_s, f_t)
    monkeypatch.setattr(ops, "sp_loss", spy)
    trace, feats, moved = _loop(["--amp", "bf16", "--channels_last"])
    (loss, _idx, loss_kd), = trace
    assert calls == [(BF16, BF16, True)] and moved
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd))
    want = R.pair(feats["s"].float().cpu().numpy(), feats["t"].float().cpu().numpy())["loss"]
    assert _report("loss_kd of the step", abs(float(loss_kd) - want) / want, allow["loss"])


def test_cli_runs_with_distill_similarity(tmp_path):
    """`python train_student_moma.py --distill similarity` on the smallest synthetic configuration: parses, builds, trains and
    validates"""
    from tests.test_gpu_cli import _run_cli
    r = _run_cli(tmp_path, ["--distill", "similarity", "--dataset", "cifar100", "--model_s", "resnet8x4", "--model_t", "resnet32x4",
                            "--n_cls", "4", "--batch_size", "8",
                            "--epochs", "1", "--steps_per_epoch", "2"], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout and "nan" not in r.stdout.lower()

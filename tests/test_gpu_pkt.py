"""GPU tests of the Probabilistic Knowledge Transfer kernels (csrc/pkt.hip) through the C ABI, ops.pkt_loss, the criterion, the
training loop and the CLI.

Conventions as in tests/test_gpu_rkd.py's header.  Yardstick: the float64 evaluation of the formulas (tests/pkt_ref.py).  Allowance
for every floating-point result: TWICE the largest distance of that kind (`ref_vs_f64_loss / _grad / _G`) that the reference's own
fp32 results keep from that evaluation over the cases of the golden fixture, never below one fp32 ulp (2^-23, relative).  Metric:
crd_ref.rel (units of the yardstick's largest element); the loss in units of abs_terms = mean_ij |T_ij log((T_ij + eps) / (P_ij +
eps))| -- the loss is a nearly cancelling sum of these -- and the single-row case, where everything vanishes identically, exactly.
G takes the `G` allowance, M and dF_s the `grad` allowance; where a student row is all zero (its gradient is 1 / eps times the
others') dF_s is compared once over all rows and once over the other rows in their own scale.  Every comparison prints the share
of its allowance it used (`_report`).  Every call through the C ABI runs on buffers between NaN-filled margins
(tests/test_gpu_guard.py): the margins must be untouched and no NaN may reach a result.

bf16 storage: the kernels widen every input to double, so a run on bf16 tensors does the arithmetic of the run on the fp32 copy of
the same values: G, M and loss are the same bits, and dF_s in bf16 is that run's fp32 dF_s rounded once, bit for bit (the kernel
rounds double -> fp32 -> bf16 in two steps for this reason)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pkt_fixture, pkt_ref as R
from tests.crd_ref import rel
from tests.test_gpu_guard import _Guarded

pytestmark = pytest.mark.gpu
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
RAW = ("G_s", "G_t", "M", "loss", "dF_s")
USED = {}                                                                      # kind -> largest share of its allowance seen


def _lib():
    from moma_amd import _lib as L
    return L.load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _report(name, got, allowed, kind=None):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e}, ratio {got / allowed:.2f})")
    if kind:
        USED[kind] = max(USED.get(kind, 0.0), got / allowed)
        print(f"  largest share so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(USED.items())))
    return got <= allowed


def _place(guard, f, dtype=F32, offset=False):
    """numpy [B, D] -> a device tensor between NaN margins, optionally starting one element behind an aligned address"""
    t = torch.from_numpy(np.ascontiguousarray(f)).to(dtype)
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


def run_abi(f_s, f_t, dt_s=F32, dt_t=F32, off_s=False, off_t=False, g_loss=1.0):
    """moma_pkt_gram x 2 (and moma_pkt_gram_pair next to them) -> moma_pkt_terms -> moma_pkt_bwd on fresh guarded buffers.  -> dict of numpy float64 arrays G_s, G_t, M,
    dF_s, the loss, and the raw device tensors under `raw`"""
    lib, guard = _lib(), _Guarded()
    B, Ds = f_s.shape
    Dt = f_t.shape[1]
    ts, tt = _place(guard, f_s, dt_s, off_s), _place(guard, f_t, dt_t, off_t)
    e = lambda *shape, dtype=F32: guard.empty(*shape, device="cuda", dtype=dtype)          # noqa: E731
    nws = lib.moma_pkt_workspace_bytes(B)
    assert nws == (B * B + 2 * B) * 8
    G_s, G_t, M, ws = e(B, B, dtype=F64), e(B, B, dtype=F64), e(B, B, dtype=F64), e(nws // 8, dtype=F64)
    loss = e(1)
    rc = lib.moma_pkt_gram(_p(ts), B, Ds, _code(dt_s), _p(G_s), _st())
    assert rc == 0, rc
    rc = lib.moma_pkt_gram(_p(tt), B, Dt, _code(dt_t), _p(G_t), _st())
    assert rc == 0, rc
    P_s, P_t = e(B, B, dtype=F64), e(B, B, dtype=F64)                          # both sides in one launch: the same bits
    rc = lib.moma_pkt_gram_pair(_p(ts), Ds, _code(dt_s), _p(tt), Dt, _code(dt_t), B, _p(P_s), _p(P_t), _st())
    assert rc == 0, rc
    assert torch.equal(P_s, G_s) and torch.equal(P_t, G_t)
    rc = lib.moma_pkt_terms(_p(G_s), _p(G_t), B, _p(ws), nws, _p(M), _p(loss), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    flat = guard.empty(ts.numel() + int(off_s), device="cuda", dtype=dt_s)
    dF = (flat[1:] if off_s else flat).view(ts.shape)
    rc = lib.moma_pkt_bwd(_p(ts), _p(M), _p(gl), _p(dF), B, Ds, _code(dt_s), _st())
    assert rc == 0, rc
    assert guard.check("pkt C ABI") > 0                                        # every margin untouched
    raw = {"G_s": G_s, "G_t": G_t, "M": M, "loss": loss, "dF_s": dF, "ws": ws}
    out = {k: _np(v) for k, v in raw.items()}
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    out["loss"] = float(loss.item())
    out["raw"] = raw
    return out


def run_op(f_s, f_t, dt_s=F32, dt_t=F32, g_loss=1.0, crit=None):
    from moma_amd import ops
    ts = torch.from_numpy(np.ascontiguousarray(f_s)).to(dt_s).cuda().requires_grad_(True)
    tt = torch.from_numpy(np.ascontiguousarray(f_t)).to(dt_t).cuda()
    loss = ops.pkt_loss(ts, tt) if crit is None else crit(ts, tt)
    (loss * g_loss).backward()
    assert ts.grad.stride() == ts.stride() and ts.grad.dtype == dt_s and ts.grad.shape == ts.shape and tt.grad is None
    assert loss.dtype == F32 and loss.dim() == 0 and loss.is_cuda
    return loss.detach(), ts.grad


def check(tag, got, want, allow, full=True, grad=True, rows=None, kernels=True):
    """got: G_s, G_t, M (full) and loss, dF_s against the restatement's.  A single row: exact zeros.  kernels=False: a result of the
    composite, kept out of the kernels' largest shares"""
    B = want["G_s"].shape[0]
    if B == 1:
        assert got["loss"] == 0 and not np.asarray(got["dF_s"]).any() and (not full or not got["M"].any())
        return True
    k_loss, k_grad = ("loss", "dF_s") if kernels else (None, None)
    ok = _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / want["abs_terms"], allow["loss"], k_loss)
    if grad:
        ok &= _report(f"{tag} dF_s", rel(got["dF_s"], want["dF_s"]), allow["grad"], k_grad)
        if rows is not None:
            ok &= _report(f"{tag} dF_s, the other rows", rel(got["dF_s"][rows], want["dF_s"][rows]), allow["grad"], k_grad)
    if full:
        for k in ("G_s", "G_t"):
            assert np.array_equal(got[k], got[k].T), k                        # one computation per pair
            ok &= _report(f"{tag} {k}", rel(got[k], want[k]), allow["G"], "G")
        assert np.array_equal(got["M"], got["M"].T)                           # the same two operands in both positions
        ok &= _report(f"{tag} M", rel(got["M"], want["M"]), allow["grad"], "M")
        if rows is not None:
            ok &= _report(f"{tag} M, the other rows", rel(got["M"][rows][:, rows], want["M"][rows][:, rows]), allow["grad"], "M")
    return ok


_WANT = {}


def fixture_case(ci):
    """(case, float64 results) -- evaluated once, shared by the tests"""
    cases, allow = pkt_fixture.load()
    if ci not in _WANT:
        _WANT[ci] = R.pair(cases[ci]["f_s"], cases[ci]["f_t"])
    return cases[ci], _WANT[ci], allow


def _other_rows(c):
    return ~c["nan_rows"] if "nan_rows" in c else None


N_CASES = 13


@pytest.mark.parametrize("ci", range(N_CASES))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    c, want, allow = fixture_case(ci)
    print(f"case {ci} {c['shape']}")
    rows = _other_rows(c)
    abi = run_abi(c["f_s"], c["f_t"])
    ok = check("abi", abi, want, allow, rows=rows)
    if ci == pkt_fixture.DUP_CASE:                                             # equal rows: equal rows of G
        (a, b), (ta, tb) = pkt_fixture.DUP_S, pkt_fixture.DUP_T
        assert np.array_equal(abi["G_s"][a], abi["G_s"][b]) and np.array_equal(abi["G_t"][ta], abi["G_t"][tb])
    if ci == pkt_fixture.ZERO_CASE:                                            # a zero row: zero Gram row, finite gradient
        assert not abi["G_s"][pkt_fixture.ZERO_S].any() and not abi["G_t"][pkt_fixture.ZERO_T].any()
        assert np.isnan(c["dF_s"][pkt_fixture.ZERO_S]).all() and np.isfinite(abi["dF_s"][pkt_fixture.ZERO_S]).all()
    loss, dF_s = run_op(c["f_s"], c["f_t"])
    op = {"loss": float(loss), "dF_s": _np(dF_s)}
    ok &= check("op", op, want, allow, full=False, rows=rows)
    assert np.isfinite(op["dF_s"]).all()
    assert float(loss) == abi["loss"] and np.array_equal(op["dF_s"], abi["dF_s"])          # the op is the C ABI sequence
    if c["shape"][0] > 1:
        # against the reference's own fp32 results: each side is within its allowance of the float64 value
        r = np.ones(c["shape"][0], bool) if rows is None else rows
        ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / want["abs_terms"], allow["loss"] + c["ref_vs_f64_loss"])
        scale = np.abs(want["dF_s"][r]).max()
        ok &= _report("op dF_s vs reference", np.abs(op["dF_s"][r] - c["dF_s"][r]).max() / scale, allow["grad"] + c["ref_vs_f64_grad"])
    assert ok


def _same_bits(b, f, dt_s, what):
    for k in ("G_s", "G_t", "M", "loss"):
        assert torch.equal(b["raw"][k], f["raw"][k]), (k, what)
    assert b["raw"]["dF_s"].dtype == dt_s and torch.equal(b["raw"]["dF_s"], f["raw"]["dF_s"].to(dt_s)), what


@pytest.mark.parametrize("ci", range(N_CASES))
def test_bf16_storage(ci):
    """the fixture's inputs are exact in bf16: either side alone and both in bf16 give the fp32 run's bits in every forward result
    (hence the same allowance is met), and a bf16 dF_s that is the fp32 dF_s rounded to bf16 bit for bit"""
    c, want, allow = fixture_case(ci)
    f = run_abi(c["f_s"], c["f_t"])
    for dt_s, dt_t in ((BF16, BF16), (BF16, F32), (F32, BF16)):
        b = run_abi(c["f_s"], c["f_t"], dt_s, dt_t)
        _same_bits(b, f, dt_s, (dt_s, dt_t))
        assert check(f"{dt_s} {dt_t}", b, want, allow, grad=dt_s != BF16, rows=_other_rows(c))    # (a bf16 dF_s carries bf16's own rounding)
    lb, db = run_op(c["f_s"], c["f_t"], BF16, BF16)
    b = run_abi(c["f_s"], c["f_t"], BF16, BF16)
    assert db.dtype == BF16 and float(lb) == b["loss"] and torch.equal(db, b["raw"]["dF_s"])


# The kernels' constants: 16 x 16 tiles of G and M' (pkt_gram, pkt_m), 128-column slabs of D (pkt_gram), 256 columns per pass of a
# pkt_rows thread, 32 rows x 64 columns and 16-row slabs of the summation index (pkt_bwd).  They are RKD's, plus the 256 of pkt_rows.
EDGES = [  # name, B, Ds, Dt, student pointer one element past an aligned address, teacher likewise
    ("B=1: a single row", 1, 5, 3, False, False),
    ("B=2", 2, 2, 3, False, False),
    ("B=3 D=1", 3, 1, 1, False, False),
    ("B=16: one full tile", 16, 8, 8, False, False),
    ("B=17: a second tile of one row", 17, 12, 20, False, False),
    ("B=31 D=63: below the backward's tiles", 31, 63, 16, False, False),
    ("B=32 D=64: the backward's tiles exactly", 32, 64, 16, False, False),
    ("B=33 D=65: one past both", 33, 65, 16, False, False),
    ("D=127: below one slab, element loads", 6, 127, 127, False, False),
    ("D=128: one slab, 16-byte loads", 6, 128, 128, False, False),
    ("D=129: a second slab of one column", 6, 129, 129, False, False),
    ("D=136: two slabs, 16-byte loads", 6, 136, 264, False, False),
    ("student behind an offset pointer", 9, 128, 64, True, False),
    ("teacher behind an offset pointer", 9, 64, 128, False, True),
    ("B=130: nine tiles a side", 130, 8, 5, False, False),
    ("B=256: one column per pkt_rows thread", 256, 6, 4, False, False),
    ("B=257: one thread owns a second column", 257, 4, 6, False, False),
]


@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_edges_against_the_restatement(edge):
    """the smallest shapes at which the kernels take another path, with an upstream gradient of 3, in fp32 and in bf16"""
    name, B, Ds, Dt, off_s, off_t = edge
    _cases, allow = pkt_fixture.load()
    rng = np.random.default_rng(B * 1000 + Ds * 10 + Dt)
    f_s = (np.round(rng.standard_normal((B, Ds)) * 32) / 32 + 0.25).astype(np.float32)
    f_t = (np.round(rng.standard_normal((B, Dt)) * 32) / 32 + 0.5).astype(np.float32)
    want = R.pair(f_s, f_t, g_loss=3.0)
    f = run_abi(f_s, f_t, F32, F32, off_s, off_t, g_loss=3.0)
    assert check(name, f, want, allow)
    b = run_abi(f_s, f_t, BF16, BF16, off_s, off_t, g_loss=3.0)
    _same_bits(b, f, BF16, name)


def test_upstream_gradient_scales_exactly():
    """g_loss is a device scalar folded in before the one rounding: a power of two (a GradScaler factor) scales every bit pattern
    exactly and leaves M unchanged, and 3 gives the restatement's gradient at g_loss = 3"""
    c, want, allow = fixture_case(6)
    one = run_abi(c["f_s"], c["f_t"])
    big = run_abi(c["f_s"], c["f_t"], g_loss=65536.0)
    assert torch.equal(big["raw"]["dF_s"], one["raw"]["dF_s"] * 65536.0) and torch.equal(big["raw"]["M"], one["raw"]["M"])
    b16 = run_abi(c["f_s"], c["f_t"], BF16, F32, g_loss=65536.0)
    assert torch.equal(b16["raw"]["dF_s"], (one["raw"]["dF_s"] * 65536.0).to(BF16))
    three = run_abi(c["f_s"], c["f_t"], g_loss=3.0)
    assert _report("dF_s at g = 3", rel(three["dF_s"], 3.0 * want["dF_s"]), allow["grad"], "dF_s")


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(77)
    for B, Ds, Dt, dt in ((64, 1280, 1280, F32), (130, 40, 24, BF16), (33, 512, 2048, F32)):
        f_s, f_t = rng.standard_normal((B, Ds)).astype(np.float32), rng.standard_normal((B, Dt)).astype(np.float32)
        a, b = run_abi(f_s, f_t, dt, dt), run_abi(f_s, f_t, dt, dt)
        for k in RAW + ("ws",):
            assert torch.equal(a["raw"][k], b["raw"][k]), (k, B)


def _torch_yardstick(x, y, eps=1e-7):
    """the formulas in float64 torch ops on the device, autograd for the gradient: -> loss, abs_terms, dF_s, G_s"""
    def prob(f):
        n = f.pow(2).sum(1, keepdim=True).sqrt()
        z = f / (n + eps)
        k = (z @ z.t() + 1.0) / 2.0
        return k / k.sum(1, keepdim=True)
    x = x.double().requires_grad_(True)
    p, t = prob(x), prob(y.double())
    terms = t * torch.log((t + eps) / (p + eps))
    loss = terms.mean()
    loss.backward()
    with torch.no_grad():
        G = x @ x.t()
    return float(loss.detach()), float(terms.detach().abs().mean()), x.grad, G


def test_the_largest_batch():
    """B = MOMA_PKT_MAX_B = 1024 (64 x 64 tiles, four columns per pkt_rows thread): against float64 torch ops on the device"""
    from moma_amd import _lib as L
    _cases, allow = pkt_fixture.load()
    B = L.PKT_MAX_B
    rng = np.random.default_rng(1024)
    f_s = (np.round(rng.standard_normal((B, 5)) * 32) / 32 + 0.125).astype(np.float32)
    f_t = (np.round(rng.standard_normal((B, 3)) * 32) / 32 + 0.125).astype(np.float32)
    assert (np.abs(f_s).sum(1) > 0).all()
    got = run_abi(f_s, f_t)
    loss, abs_terms, grad, G_s = _torch_yardstick(torch.from_numpy(f_s).cuda(), torch.from_numpy(f_t).cuda())
    assert np.array_equal(got["G_s"], got["G_s"].T) and np.array_equal(got["M"], got["M"].T)
    ok = _report("B = 1024 G_s", rel(got["G_s"], _np(G_s)), allow["G"], "G")
    ok &= _report("B = 1024 loss", abs(got["loss"] - loss) / abs_terms, allow["loss"], "loss")
    ok &= _report("B = 1024 dF_s", rel(got["dF_s"], _np(grad)), allow["grad"], "dF_s")
    assert ok


def test_antiparallel_rows():
    """f_s[7] = -f_s[3], f_t[5] = -2 f_t[2]: K = 0 up to eps there and the log's argument is eps; every product is exact in
    double, so the kernels stay within the allowance of the float64 evaluation (the reference's own fp32 loss does not: 1e-3)"""
    _cases, allow = pkt_fixture.load()
    rng = np.random.default_rng(1207)
    f_s = (np.round(rng.standard_normal((12, 32)) * 32) / 32).astype(np.float32)
    f_t = (np.round(rng.standard_normal((12, 32)) * 32) / 32).astype(np.float32)
    f_s[7], f_t[5] = -f_s[3], -2 * f_t[2]
    want = R.pair(f_s, f_t)
    assert want["C_s"][7, 3] < -1 + 1e-6 and want["C_t"][5, 2] < -1 + 1e-6
    got = run_abi(f_s, f_t)
    assert check("antiparallel", got, want, allow)
    loss, dF_s = run_op(f_s, f_t)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dF_s).all()) and float(loss) == got["loss"]


def test_op_and_criterion(monkeypatch):
    """gradient dtype, shape and strides follow the input; [B, C, 1, 1] maps; no gradient where none is wanted; float16 and a teacher
    that wants a gradient go to the composite and agree with the kernels; the error paths"""
    from moma_amd import _lib as L, ops
    from moma_amd.distiller_zoo import PKT
    c, want, allow = fixture_case(4)
    crit = PKT()
    calls = []
    real = ops.pkt_loss
    monkeypatch.setattr(ops, "pkt_loss", lambda *a: (calls.append(1), real(*a))[1])
    l0, d0 = run_op(c["f_s"], c["f_t"], crit=crit)
    assert len(calls) == 1
    ok = check("criterion", {"loss": float(l0), "dF_s": _np(d0)}, want, allow, full=False)
    l4, d4 = run_op(c["f_s"][:, :, None, None], c["f_t"][:, :, None, None], crit=crit)     # [B, C, 1, 1]: the same bits, 4-D gradient
    assert d4.dim() == 4 and torch.equal(l4, l0) and torch.equal(d4.flatten(1), d0) and len(calls) == 2
    ts, tt = torch.from_numpy(c["f_s"]).cuda(), torch.from_numpy(c["f_t"]).cuda()
    with torch.no_grad():
        assert float(real(ts, tt)) == float(l0)
    assert not real(ts, tt).requires_grad                                      # nobody wants a gradient: nothing is saved
    # float16 storage and a teacher that wants a gradient: the stock-torch composite (values exact in fp16 too)
    n = len(calls)
    sh = ts.half().requires_grad_(True)
    lh = crit(sh, tt.half())
    lh.backward()
    ok &= check("fp16 composite", {"loss": float(lh.detach()), "dF_s": _np(sh.grad)}, want, {"loss": allow["loss"], "grad": 2.0 ** -10}, full=False,
                kernels=False)
    sg, tg = ts.clone().requires_grad_(True), tt.clone().requires_grad_(True)
    lg = crit(sg, tg)
    lg.backward()
    assert len(calls) == n and tg.grad is not None and bool(torch.isfinite(tg.grad).all()) and bool(tg.grad.abs().sum() > 0)
    ok &= check("composite (teacher gradient)", {"loss": float(lg.detach()), "dF_s": _np(sg.grad)}, want, allow, full=False, kernels=False)
    ok &= _report("composite vs kernels, loss", abs(float(lg.detach()) - float(l0)) / want["abs_terms"], 2 * allow["loss"])
    ok &= _report("composite vs kernels, dF_s", rel(_np(sg.grad), _np(d0)), 2 * allow["grad"])
    assert ok
    # a batch above the limit: the composite; the limit itself is served by the kernels (test_the_largest_batch)
    wide = torch.randn(L.PKT_MAX_B + 1, 2, device="cuda")
    assert bool(torch.isfinite(crit(wide, wide * 2 + 1))) and len(calls) == n
    with pytest.raises(ValueError):
        real(ts, tg)                                                           # a teacher that wants a gradient
    with pytest.raises(ValueError):
        real(ts, tt[:-1])                                                      # batch sizes differ
    with pytest.raises(ValueError):
        real(wide, wide)                                                       # B above the limit
    with pytest.raises(ValueError):
        real(ts.t(), tt)                                                       # not contiguous
    with pytest.raises(TypeError):
        real(ts.half(), tt.half())


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.pkt_loss with every buffer it allocates (G, M, workspace, loss, dF) between NaN margins, at ragged shapes and both
    dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    for (B, Ds, Dt, dtype) in [(5, 7, 9, F32), (19, 129, 40, BF16), (35, 66, 3, F32)]:
        rng = np.random.default_rng(B * 7 + Ds)
        a = torch.from_numpy(rng.standard_normal((B, Ds)).astype(np.float32)).to(dtype).cuda()
        b = torch.from_numpy(rng.standard_normal((B, Dt)).astype(np.float32)).to(dtype).cuda()

        def run():
            x = a.clone().requires_grad_(True)
            loss = ops.pkt_loss(x, b)
            (loss * 2.5).backward()
            return loss.detach().clone(), x.grad.clone()

        plain = run()
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run()
            assert guard.check(f"pkt_loss {B} {Ds} {Dt}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_one_eager_step_of_the_loop(monkeypatch):
    """train_distill_moma with distill='pkt', resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8: the pair runs on the kernels, loss_kd
    is the restatement's value on feat[-1] of that step, the loss is finite and the student's weights change"""
    from moma_amd import ops
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    _cases, allow = pkt_fixture.load()
    calls = []
    real = ops.pkt_loss
    monkeypatch.setattr(ops, "pkt_loss", lambda *a: (calls.append(1), real(*a))[1])
    opt = parse_option(["--distill", "pkt", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
                        "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "1", "--learning_rate", "0.01",
                        "--no_graph_teacher"])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
    dev = torch.device("cuda", 0)
    opt.device = dev
    torch.manual_seed(31)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
    feats = {}

    def keep(k):
        def hook(_m, _i, out):
            feats.setdefault(k, out[0][-1].detach().clone())
        return hook
    hooks = [m.register_forward_hook(keep(k)) for k, m in (("s", model_s), ("t", model_t))]
    before = [p.detach().clone() for p in model_s.parameters()]
    opt.trace, opt.print_freq = [], 1000
    train_distill_moma(1, SyntheticLoader(1, 8, 32, 4, 5, dev), module_list, criterion_list, None, contrast, optimizer, opt)
    for h in hooks:
        h.remove()
    (loss, _idx, loss_kd), = opt.trace
    assert len(calls) == 1 and np.isfinite(float(loss)) and np.isfinite(float(loss_kd))
    assert any(not torch.equal(a, b) for a, b in zip(before, model_s.parameters()))
    want = R.pair(feats["s"].float().cpu().numpy(), feats["t"].float().cpu().numpy())
    assert _report("loss_kd of the step", abs(float(loss_kd) - want["loss"]) / want["abs_terms"], allow["loss"], "loss")


def test_cli_runs_with_distill_pkt(tmp_path):
    """`python train_student_moma.py --distill pkt` on the smallest synthetic configuration: parses, builds, trains and validates"""
    from tests.test_gpu_cli import _run_cli
    r = _run_cli(tmp_path, ["--distill", "pkt", "--dataset", "cifar100", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--n_cls", "4",
                            "--batch_size", "8",
                            "--epochs", "1", "--steps_per_epoch", "2"], timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "images/sec" in r.stdout and "nan" not in r.stdout.lower()

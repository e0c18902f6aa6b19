"""GPU tests of the Attention Transfer kernels (csrc/attention.hip) through the C ABI, ops.attention_loss, the criterion and the
training loop.

Yardstick: the float64 evaluation of the formulas (tests/at_ref.py).  Allowance for every floating-point result: TWICE the largest
distance of that kind (`ref_vs_f64_loss / _grad / _map`) that the reference's own fp32 results keep from that evaluation over the
cases of the golden fixture, never below one fp32 ulp (2^-23, relative): a different but equally valid fp32 summation order can land
on the other side of the float64 value.  Metric: crd_ref.rel (units of the yardstick's largest element), relative for the scalar.
Every call through the C ABI runs on buffers between NaN-filled margins (tests/test_gpu_guard.py): the margins must be untouched
and no NaN may reach a result."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import at_fixture, at_ref as A
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
    if cl:
        out = flat.view(B, H, W, Cc).permute(0, 3, 1, 2)
        assert out.is_contiguous(memory_format=torch.channels_last)
    else:
        out = flat.view(B, Cc, H, W)
    out.copy_(t)
    return out


def _layout(t):
    from moma_amd import _lib as L
    return L.LAYOUT_NCHW if t.is_contiguous() else L.LAYOUT_NHWC


def _dt(t):
    from moma_amd import _lib as L
    return L.DT_BF16 if t.dtype == BF16 else L.DT_F32


def run_abi(f_s, f_t, cl_s=False, cl_t=False, dtype=F32, offset=False, g_loss=1.0, want_t=False):
    """moma_at_map x 2 -> moma_at_pair -> moma_at_bwd on fresh guarded buffers.  f_s, f_t: numpy, already on a common-grid-able shape
    (integer ratios).  -> dict of numpy float64 arrays: a_s, a_t, ah_s, ah_t, norms, loss, dF_s (, dF_t) and the raw dF tensors"""
    lib, guard = _lib(), _Guarded()
    oh, ow = A.grid(f_s.shape, f_t.shape)
    B, n = f_s.shape[0], oh * ow
    ts, tt = _place(guard, f_s, dtype, cl_s, offset), _place(guard, f_t, dtype, cl_t, offset)
    e = lambda *shape: guard.empty(*shape, device="cuda", dtype=F32)          # noqa: E731
    maps = []
    for t in (ts, tt):
        Bc, Cc, H, W = t.shape
        a = e(B, n)
        nws = lib.moma_at_workspace_bytes(Bc, Cc, H, W, oh, ow, _dt(t), _layout(t))
        ws = guard.empty(nws, device="cuda", dtype=torch.uint8) if nws else None
        rc = lib.moma_at_map(_p(t), _p(a), Bc, Cc, H, W, oh, ow, _dt(t), _layout(t), _p(ws), nws, _st())
        assert rc == 0, rc
        maps.append(a)
    norms, partials, loss, g_s, ah_s, ah_t = e(B, 2), e(B), e(1), e(B, n), e(B, n), e(B, n)
    g_t = e(B, n) if want_t else None
    rc = lib.moma_at_pair(_p(maps[0]), _p(maps[1]), B, n, _p(norms), _p(partials), _p(loss), _p(g_s), _p(g_t), _p(ah_s), _p(ah_t), _st())
    assert rc == 0, rc
    gl = torch.full((1,), float(g_loss), device="cuda")
    out = {}
    for side, t, g in (("s", ts, g_s), ("t", tt, g_t)):
        if g is None:
            continue
        Bc, Cc, H, W = t.shape
        flat = guard.empty(t.numel() + int(offset), device="cuda", dtype=dtype)
        flat = flat[1:] if offset else flat
        dF = flat.as_strided(t.shape, t.stride())                          # dtype and layout of f
        rc = lib.moma_at_bwd(_p(t), _p(g), _p(gl), _p(dF), Bc, Cc, H, W, oh, ow, _dt(t), _layout(t), _st())
        assert rc == 0, rc
        out["dF_" + side + "_raw"] = dF
        out["dF_" + side] = dF.float().cpu().numpy().astype(np.float64)
    assert guard.check("attention C ABI") > 0                              # every margin untouched
    for k, v in (("a_s", maps[0]), ("a_t", maps[1]), ("ah_s", ah_s), ("ah_t", ah_t), ("norms", norms), ("partials", partials),
                 ("g_s", g_s), ("g_t", g_t)):
        if v is not None:
            out[k] = v.cpu().numpy().astype(np.float64)
            assert np.isfinite(out[k]).all(), k
    out["loss"] = float(loss.item())
    assert np.isfinite(out["loss"]) and all(np.isfinite(out[k]).all() for k in out if k in ("dF_s", "dF_t"))
    return out


def run_op(f_s, f_t, cl_s=False, cl_t=False, dtype=F32, grad_t=False, g_loss=1.0):
    from moma_amd import ops
    mk = lambda f, cl: torch.from_numpy(np.ascontiguousarray(f)).to(dtype).cuda().contiguous(    # noqa: E731
        memory_format=torch.channels_last if cl else torch.contiguous_format)
    ts, tt = mk(f_s, cl_s).requires_grad_(True), mk(f_t, cl_t).requires_grad_(grad_t)
    loss = ops.attention_loss(ts, tt)
    (loss * g_loss).backward()
    assert ts.grad.stride() == ts.stride() and ts.grad.dtype == dtype
    return loss.detach(), ts.grad, tt.grad


def check(tag, got, want, allow, sides=("s",), maps=True):
    ok = True
    if maps:
        for s in ("s", "t"):
            ok &= _report(f"{tag} ah_{s}", rel(got["ah_" + s], want["ah_" + s]), allow["map"])
    # (a 1 x 1 map normalises to exactly 1 on both sides: the loss is exactly 0 and must come out as 0)
    ok &= _report(f"{tag} loss", abs(got["loss"] - want["loss"]) / abs(want["loss"]) if want["loss"] else abs(got["loss"]), allow["loss"])
    for s in sides:
        ok &= _report(f"{tag} dF_{s}", rel(got["dF_" + s], want["dF_" + s]), allow["grad"])
    return ok


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


_WANT = {}


def fixture_case(ci):
    """(case, float64 results) -- evaluated once, shared by the tests"""
    cases, allow = at_fixture.load()
    if ci not in _WANT:
        _WANT[ci] = A.pair(cases[ci]["f_s"], cases[ci]["f_t"])
    return cases[ci], _WANT[ci], allow


@pytest.mark.parametrize("ci", range(8))
def test_fixture_cases_through_the_abi_and_the_op(ci):
    c, want, allow = fixture_case(ci)
    B, Cs, Ct, Hs, Ht = c["shape"]
    print(f"case {ci} {c['shape']}")
    ok = True
    f_s, f_t = c["f_s"], c["f_t"]
    h = min(Hs, Ht)
    if max(Hs, Ht) % h:         # a non-integer ratio: the wrapper's route -- stock pooling first, then the kernels at ratio 1
        pooled = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(f_s if Hs > Ht else f_t).cuda(), (h, h)).cpu().numpy()
        f_s, f_t = (pooled, f_t) if Hs > Ht else (f_s, pooled)
        abi = run_abi(f_s, f_t)
        ok &= check("abi", abi, dict(want, dF_s=A.pair(f_s, f_t)["dF_s"]), allow)
    else:
        abi = run_abi(f_s, f_t)
        ok &= check("abi", abi, want, allow)
    if B > 1:
        assert not abi["dF_s"][0].any() and not abi["ah_s"][0].any()        # the all-zero image: exactly zero, nothing undefined
    loss, dF_s, _ = run_op(c["f_s"], c["f_t"])
    op = {"loss": float(loss), "dF_s": _np(dF_s)}
    ok &= check("op", op, want, allow, maps=False)
    assert np.isfinite(op["dF_s"]).all() and (B == 1 or not op["dF_s"][0].any())
    # against the reference's own fp32 results: each side is within its allowance of the float64 value
    ok &= _report("op loss vs reference", abs(op["loss"] - c["loss"]) / abs(c["loss"]), allow["loss"] + c["ref_vs_f64_loss"])
    ok &= _report("op dF_s vs reference", rel(op["dF_s"], c["dF_s"]), allow["grad"] + c["ref_vs_f64_grad"])
    assert ok


@pytest.mark.parametrize("ci", range(8))
def test_layouts_agree(ci):
    """f_s and / or f_t in channels_last: the same results as the NCHW run, within the allowance (of the float64 value, and of
    each other: two equally valid fp32 orders)"""
    c, want, allow = fixture_case(ci)
    l0, d0, _ = run_op(c["f_s"], c["f_t"])
    ok = True
    for cl_s, cl_t in ((True, False), (False, True), (True, True)):
        loss, dF, _ = run_op(c["f_s"], c["f_t"], cl_s, cl_t)
        tag = f"case {ci} cl_s={int(cl_s)} cl_t={int(cl_t)}"
        ok &= check(tag, {"loss": float(loss), "dF_s": _np(dF)}, want, allow, maps=False)
        ok &= _report(tag + " loss vs NCHW", abs(float(loss) - float(l0)) / abs(float(l0)), 2 * allow["loss"])
        ok &= _report(tag + " dF_s vs NCHW", rel(_np(dF), _np(d0)), 2 * allow["grad"])
    if min(c["shape"][3:]) == max(c["shape"][3:]) or max(c["shape"][3:]) % min(c["shape"][3:]) == 0:
        abi = run_abi(c["f_s"], c["f_t"], cl_s=True, cl_t=True)
        ok &= check(f"case {ci} abi channels_last", abi, want, allow)
    assert ok


def _bf16_ordered(t):
    """bf16 tensor -> int32 whose differences count representable values (+0 and -0 coincide)"""
    bits = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where(bits >= 0x8000, -mag, mag)


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("ci", range(8))
def test_bf16_storage(ci, cl):
    """inputs rounded to bf16: the run on bf16 tensors gives maps and loss within the fp32 allowance of the run on the fp32 copy of
    the same values (fp32 accumulation either way), and dF is that run's dF rounded once: within one bf16 ulp per element"""
    c, _want, allow = fixture_case(ci)
    Hs, Ht = c["shape"][3:]
    if max(Hs, Ht) % min(Hs, Ht):
        # the non-integer ratio goes through stock pooling in the storage dtype: compared at the op level, loss only, in bf16 terms
        lb, db, _ = run_op(c["f_s"], c["f_t"], cl, cl, BF16)
        lf, df, _ = run_op(_np(torch.from_numpy(c["f_s"]).to(BF16)), _np(torch.from_numpy(c["f_t"]).to(BF16)), cl, cl, F32)
        assert bool(torch.isfinite(db.float()).all()) and abs(float(lb) - float(lf)) <= 2.0 ** -7 * abs(float(lf))
        return
    r = lambda f: _np(torch.from_numpy(f).to(BF16))                            # noqa: E731
    f_s, f_t = r(c["f_s"]), r(c["f_t"])
    b = run_abi(f_s, f_t, cl, cl, BF16)
    f = run_abi(f_s, f_t, cl, cl, F32)
    ok = True
    for s in ("s", "t"):
        ok &= _report(f"a_{s} bf16 vs fp32 storage", rel(b["a_" + s], f["a_" + s]), allow["map"])
        ok &= _report(f"ah_{s} bf16 vs fp32 storage", rel(b["ah_" + s], f["ah_" + s]), allow["map"])
    ok &= _report("loss bf16 vs fp32 storage", abs(b["loss"] - f["loss"]) / abs(f["loss"]), allow["loss"])
    got, want = _bf16_ordered(b["dF_s_raw"]), _bf16_ordered(f["dF_s_raw"].to(BF16))
    worst = int((got - want).abs().max())
    print(f"  dF_s: {worst} bf16 ulp at worst, {int((got != want).sum())} of {got.numel()} elements differ")
    assert ok and worst <= 1
    # the op on bf16 tensors: the same bits as the C ABI sequence
    lb, db, _ = run_op(f_s, f_t, cl, cl, BF16)
    assert db.dtype == BF16 and float(lb) == b["loss"] and torch.equal(db, b["dF_s_raw"])


EDGES = [  # name, f_s shape, f_t shape, offset pointer
    ("B=1", (1, 5, 6, 6), (1, 7, 6, 6), False),
    ("C=1", (2, 1, 5, 5), (2, 1, 5, 5), False),
    ("HW=1", (3, 8, 1, 1), (3, 4, 1, 1), False),
    ("HW=49 offset pointer", (2, 6, 7, 7), (2, 6, 7, 7), True),
    ("HW=64 offset pointer", (2, 8, 8, 8), (2, 8, 8, 8), True),
    ("C=24 / C=1280", (2, 24, 7, 7), (2, 1280, 7, 7), False),
    ("C=3 vs C=1280, 49 pixels", (3, 3, 7, 7), (3, 1280, 7, 7), False),
    ("rectangular, no pooling", (2, 6, 6, 10), (2, 4, 6, 10), False),
    ("ratio 2 on the student", (2, 6, 8, 8), (2, 10, 4, 4), False),
    ("ratio 4 on the student", (2, 6, 16, 16), (2, 10, 4, 4), False),
    ("ratio 2 on the teacher", (2, 6, 4, 4), (2, 10, 8, 8), False),
    ("ratio 4 on the teacher", (2, 8, 4, 4), (2, 12, 16, 16), False),
    ("ratio 2 x 3 window", (2, 8, 8, 12), (2, 4, 4, 4), False),
    ("ratio 2, offset pointer", (2, 8, 12, 12), (2, 8, 6, 6), True),
    ("channel splits (small NCHW map, many channels)", (2, 1280, 7, 7), (2, 320, 7, 7), False),
    ("more rows than one pass of a workgroup", (2, 4, 40, 40), (2, 4, 40, 40), False),
    ("grid-stride loop, 128 x 128", (2, 4, 128, 128), (2, 4, 128, 128), False),
    # 9 * 16384 pixels at one pixel per lane (offset pointer) / 8 lanes per pixel (C = 5): more work items than the 2048 workgroups
    ("grid-stride loop wraps", (9, 5, 128, 128), (9, 5, 128, 128), True),
]


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_edges_against_the_restatement(edge, cl):
    """the smallest shapes at which the kernels take another path, both sides' gradients, with an upstream gradient of 3"""
    name, ss, st, offset = edge
    _cases, allow = at_fixture.load()
    rng = np.random.default_rng(abs(hash((ss, st))) % (1 << 31))
    f_s = (np.round(rng.standard_normal(ss) * 32) / 32).astype(np.float32)
    f_t = (np.round(rng.standard_normal(st) * 32) / 32 + 0.5).astype(np.float32)
    want = A.pair(f_s, f_t, g_loss=3.0)
    got = run_abi(f_s, f_t, cl, cl, F32, offset, g_loss=3.0, want_t=True)
    ok = check(f"{name} {'channels_last' if cl else 'NCHW'}", got, want, allow, sides=("s", "t"))
    ok &= _report("norms", rel(got["norms"], want["norms"]), allow["map"])
    ok &= _report("g_s", rel(got["g_s"], want["g_s"]), allow["grad"])
    assert ok


def test_op_writes_stay_inside_and_results_do_not_depend_on_the_allocation(monkeypatch):
    """ops.attention_loss with every buffer it allocates (maps, norms, partials, loss, g_a, workspace, dF) between NaN margins, at
    ragged shapes and both dtypes: margins untouched, results bit-equal to the same call on ordinary allocations"""
    from moma_amd import ops
    from tests.test_gpu_guard import _in
    for (ss, st, cl, dtype) in [((3, 5, 7, 7), (3, 9, 7, 7), False, F32), ((2, 24, 9, 9), (2, 40, 3, 3), True, BF16),
                                ((2, 1280, 7, 7), (2, 24, 7, 7), False, BF16), ((5, 3, 10, 10), (5, 6, 5, 5), True, F32)]:
        rng = np.random.default_rng(ss[1] * 7 + st[1])
        mf = torch.channels_last if cl else torch.contiguous_format
        a = torch.from_numpy(rng.standard_normal(ss).astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf)
        b = torch.from_numpy(rng.standard_normal(st).astype(np.float32)).to(dtype).cuda().contiguous(memory_format=mf)

        def run(wrap):
            x, y = wrap(a).requires_grad_(True), wrap(b).requires_grad_(True)
            loss = ops.attention_loss(x, y)
            (loss * 2.5).backward()
            return loss.detach().clone(), x.grad.clone(), y.grad.clone()

        plain = run(lambda t: t.clone(memory_format=torch.preserve_format))
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda t: t.clone(memory_format=torch.preserve_format) if cl else _in(guard, t))
            assert guard.check(f"attention_loss {ss} {st}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for u, v in zip(plain, guarded):
            assert torch.equal(u, v) and bool(torch.isfinite(u.float()).all())


def test_two_calls_give_the_same_bits():
    for (ss, st, cl, dtype) in [((4, 1280, 7, 7), (4, 1280, 7, 7), False, F32), ((4, 112, 14, 14), (4, 112, 14, 14), True, BF16),
                                ((3, 24, 56, 56), (3, 40, 28, 28), False, F32)]:
        rng = np.random.default_rng(ss[1])
        f_s, f_t = rng.standard_normal(ss).astype(np.float32), rng.standard_normal(st).astype(np.float32)
        l1, d1, t1 = run_op(f_s, f_t, cl, cl, dtype, grad_t=True)
        l2, d2, t2 = run_op(f_s, f_t, cl, cl, dtype, grad_t=True)
        assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(t1, t2)


def test_gradient_to_both_sides_and_mixed_sides():
    """f_t.requires_grad: dF_t matches the restatement; the two sides may differ in layout AND dtype; a no-grad call allocates no
    gradient; a layout that is neither contiguous nor channels_last is copied first; float16 is refused by the op"""
    from moma_amd import ops
    _cases, allow = at_fixture.load()
    rng = np.random.default_rng(11)
    f_s = (np.round(rng.standard_normal((3, 12, 8, 8)) * 32) / 32).astype(np.float32)
    f_t = (np.round(rng.standard_normal((3, 20, 4, 4)) * 32) / 32).astype(np.float32)
    want = A.pair(f_s, f_t, g_loss=0.5)
    loss, dF_s, dF_t = run_op(f_s, f_t, cl_s=True, cl_t=False, grad_t=True, g_loss=0.5)
    assert check("both sides", {"loss": float(loss), "dF_s": _np(dF_s), "dF_t": _np(dF_t)}, want, allow, sides=("s", "t"), maps=False)
    # student bf16 channels_last against a teacher in fp32 NCHW (values exact in bf16: multiples of 1/32)
    ts = torch.from_numpy(f_s).to(BF16).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tt = torch.from_numpy(f_t).cuda()
    mixed = ops.attention_loss(ts, tt)
    assert _report("mixed dtypes loss", abs(mixed.item() - want["loss"]) / want["loss"], allow["loss"])
    with torch.no_grad():
        assert float(ops.attention_loss(ts, tt)) == float(mixed)
    odd = torch.from_numpy(f_s).cuda().permute(0, 1, 3, 2)                    # dense, neither layout
    assert not odd.is_contiguous() and not odd.is_contiguous(memory_format=torch.channels_last)
    w2 = A.pair(np.ascontiguousarray(f_s.transpose(0, 1, 3, 2)), f_t)
    assert _report("permuted input", abs(float(ops.attention_loss(odd, tt)) - w2["loss"]) / w2["loss"], allow["loss"])
    with pytest.raises(TypeError):
        ops.attention_loss(tt.half(), tt.half())
    with pytest.raises(ValueError):
        ops.attention_loss(tt, torch.zeros(3, 4, 4, 6, device="cuda"))


def test_criterion_takes_the_kernels_on_gpu_tensors(monkeypatch):
    from moma_amd import ops
    from moma_amd.distiller_zoo import Attention
    calls = []
    real = ops.attention_loss
    monkeypatch.setattr(ops, "attention_loss", lambda a, b: (calls.append(1), real(a, b))[1])
    x, y = torch.randn(2, 8, 6, 6, device="cuda"), torch.randn(2, 4, 3, 3, device="cuda")
    crit = Attention()
    out = crit([x, x.to(BF16)], [y, y])
    assert len(out) == 2 and len(calls) == 2 and all(o.dtype == F32 and o.dim() == 0 for o in out)
    crit([x.half()], [y.half()])                                             # float16 storage: the stock-torch composite
    Attention(p=3)([x], [y])
    assert len(calls) == 2
    assert abs(float(out[0]) - float(crit.composite(x, y))) < 1e-6 * float(out[0])
    with pytest.raises(ValueError):
        crit([torch.randn(2, 17, 32, device="cuda")], [y])


def _loop(extra, steps=5):
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.train_student_moma import build_training, parse_option
    argv = ["--distill", "attention", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
            "--batch_size", "8", "--steps_per_epoch", str(steps), "-c", "1", "-d", "1", "-b", "1000", "--learning_rate", "0.01",
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


def test_five_eager_steps_of_the_loop():
    """train_distill_moma with distill='attention', beta 1000, resnet8x4 <- resnet32x4, synthetic 32 x 32, B = 8, fp32: loss_kd of
    step 1 is the restatement's value on the feature maps the two models produced in that step (stock torch on the device, moved to
    numpy); every loss is finite; the same run in channels_last under bf16 autocast completes with finite losses"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    _cases, allow = at_fixture.load()
    losses, kds, feats = _loop([])
    assert len(kds) == 5 and np.isfinite(kds).all() and np.isfinite(losses).all()
    assert len(feats["s"]) == 5 and all(f.dim() == 4 and f.dtype == F32 for f in feats["s"][1:-1])
    want = A.loss_of([f.cpu().numpy() for f in feats["s"][1:-1]], [f.cpu().numpy() for f in feats["t"][1:-1]])
    print("loss_kd per step:", " ".join(f"{v:.6e}" for v in kds), " restatement of step 1: %.6e" % want)
    assert _report("loss_kd of step 1", abs(kds[0] - want) / want, allow["loss"])
    losses, kds, feats = _loop(["--channels_last", "--amp", "bf16"])
    assert len(kds) == 5 and np.isfinite(kds).all() and np.isfinite(losses).all()
    mid = feats["s"][1:-1]
    print("bf16 / channels_last run: feature dtypes", [f.dtype for f in mid], "loss_kd", " ".join(f"{v:.6e}" for v in kds))
    assert all(f.dtype == BF16 for f in mid)                                 # the maps reach the kernels at 2 bytes

"""GPU tests of the CRD kernels (csrc/crd.hip) through the C ABI, the torch wrappers, the modules and the training loop.

Yardstick: the float64 evaluation of the formulas (tests/crd_ref.py).  Allowance for every floating-point result: TWICE the distance
the reference's own fp32 result keeps from that evaluation, as recorded in the golden fixture (`ref_vs_f64_*` of the case; for the
sweeps, which have no case of their own, the largest over the fixture's cases): a different but equally valid fp32 summation order
can land on the other side of the float64 value.  Indices, params[0:2] and untouched bank rows: exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import crd_ref as R, golden_npz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g11():
    return golden_npz.load(os.path.join(ROOT, "tests", "golden", "g11_crd.npz"))


def _lib():
    from moma_amd import _lib as L
    return L.load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


class Call:
    """one moma_crd_fused / moma_crd_scores(+bwd) call through the C ABI on fresh buffers"""

    def __init__(self, v1, v2, m1, m2, idx, T, Z=None):
        self.v1, self.v2, self.m1, self.m2, self.idx, self.T = v1, v2, m1, m2, idx, float(T)
        self.B, self.d = v1.shape
        self.K1, self.n_data = idx.shape[1], m1.shape[0]
        self.Z = torch.full((2,), -1.0, device="cuda") if Z is None else Z
        self.bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ws_bytes = _lib().moma_crd_workspace_bytes(self.B, self.d, self.K1)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")

    def fused(self, set_z, want_dv=True):
        loss = torch.empty(2, device="cuda")
        dv1 = torch.empty(self.B, self.d, device="cuda") if want_dv else None
        dv2 = torch.empty(self.B, self.d, device="cuda") if want_dv else None
        rc = _lib().moma_crd_fused(_p(self.v1), _p(self.v2), _p(self.m1), _p(self.m2), _p(self.idx), self.B, self.d, self.K1,
                                   self.n_data, self.T, _p(self.Z), int(set_z), _p(loss), _p(dv1), _p(dv2), _p(self.bad),
                                   _p(self.ws), self.ws_bytes, _st())
        assert rc == 0, rc
        return loss, dv1, dv2

    def scores(self, set_z):
        o1, o2 = torch.empty(self.B, self.K1, device="cuda"), torch.empty(self.B, self.K1, device="cuda")
        rc = _lib().moma_crd_scores(_p(self.v1), _p(self.v2), _p(self.m1), _p(self.m2), _p(self.idx), self.B, self.d, self.K1,
                                    self.n_data, self.T, _p(self.Z), int(set_z), _p(o1), _p(o2), _p(self.bad), _p(self.ws),
                                    self.ws_bytes, _st())
        assert rc == 0, rc
        return o1, o2

    def scores_bwd(self, do1, do2, o1, o2):
        dv1, dv2 = torch.empty(self.B, self.d, device="cuda"), torch.empty(self.B, self.d, device="cuda")
        rc = _lib().moma_crd_scores_bwd(_p(do1), _p(do2), _p(o1), _p(o2), _p(self.m1), _p(self.m2), _p(self.idx), self.B, self.d,
                                        self.K1, self.n_data, self.T, _p(dv1), _p(dv2), _p(self.bad), _p(self.ws), self.ws_bytes, _st())
        assert rc == 0, rc
        return dv1, dv2


def _update(m1, m2, v1, v2, y, momentum, bad):
    rc = _lib().moma_crd_update(_p(m1), _p(m2), _p(v1), _p(v2), _p(y), v1.shape[0], v1.shape[1], m1.shape[0], float(momentum),
                                _p(bad), _st())
    assert rc == 0, rc


def _contrast_loss_grad(x, n_data):
    """ContrastLoss over materialised scores and its gradient w.r.t. them, in torch on the device (the reference sequence)"""
    from moma_amd.crd import ContrastLoss
    x = x.detach().clone().requires_grad_(True)
    loss = ContrastLoss(n_data)(x.unsqueeze(2)).sum()
    loss.backward()
    return loss.detach(), x.grad


def _report(name, got, allowed):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e})")
    return got <= allowed


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_fused_and_materialised_against_the_fixture_step_by_step(g11, ci):
    """(B, d, nce_k, n_data) = (8, 64, 256, 600) and (6, 128, 1000, 900), three steps, and the repeated-y case: every output of both
    paths, Z on step 1 only, the banks after the update"""
    p = f"c{ci}_"
    B, d, K, n_data, s_dim, t_dim, steps, rep = (int(v) for v in g11[p + "shape"])
    tol = {k: 2 * float(g11[p + "ref_vs_f64_" + k]) for k in ("loss", "dv", "out", "rows", "z")}
    m1, m2 = _cu(g11[p + "memory_v1"]), _cu(g11[p + "memory_v2"])
    Z = torch.full((2,), -1.0, device="cuda")
    ok = True
    for st in range(steps):
        q = f"{p}s{st}_"
        print(f"case {ci} step {st}")
        params = g11[q + "params"]
        T, mom = float(params[1]), float(params[4])
        idx_np = g11[q + "idx"].astype(np.int64)
        y_np = idx_np[:, 0]
        m1_np, m2_np = m1.cpu().numpy(), m2.cpu().numpy()
        v1_64, _ = R.embed(g11[q + "f_s"], g11[p + "ws"], g11[p + "bs"])
        v2_64, _ = R.embed(g11[q + "f_t"], g11[p + "wt"], g11[p + "bt"])
        v1, v2 = _cu(v1_64, torch.float32), _cu(v2_64, torch.float32)
        w1 = R.side(v1.cpu().numpy(), m2_np, idx_np, T, float(params[2]))
        w2 = R.side(v2.cpu().numpy(), m1_np, idx_np, T, float(params[3]))
        call = Call(v1, v2, m1, m2, _cu(idx_np), T, Z)
        loss, dv1, dv2 = call.fused(set_z=(st == 0))
        if st == 0:
            z_got = Z.cpu().numpy().astype(np.float64)
            for s_, w_ in ((0, w1), (1, w2)):
                zf = R.z_of(w_["e"], n_data)
                ok &= _report(f"Z side {s_ + 1}", abs(z_got[s_] - zf) / zf, tol["z"])
            z_first = Z.clone()
        else:
            assert torch.equal(Z, z_first)                                   # Z is written by the first step only
        o1, o2 = call.scores(set_z=False)
        assert int(call.bad.item()) == 0
        ok &= _report("out_v1", R.rel(o1.cpu().numpy(), w1["x"]), tol["out"])
        ok &= _report("out_v2", R.rel(o2.cpu().numpy(), w2["x"]), tol["out"])
        l = loss.cpu().numpy().astype(np.float64)
        ok &= _report("loss side 1", abs(l[0] - w1["loss"]) / abs(w1["loss"]), tol["loss"])
        ok &= _report("loss side 2", abs(l[1] - w2["loss"]) / abs(w2["loss"]), tol["loss"])
        ok &= _report("dv1", R.rel(dv1.cpu().numpy(), w1["dv"]), tol["dv"])
        ok &= _report("dv2", R.rel(dv2.cpu().numpy(), w2["dv"]), tol["dv"])
        # fused == materialised + ContrastLoss on the same inputs
        ls1, g1 = _contrast_loss_grad(o1, n_data)
        ls2, g2 = _contrast_loss_grad(o2, n_data)
        mv1, mv2 = call.scores_bwd(g1, g2, o1, o2)
        ok &= _report("materialised loss 1", abs(float(ls1) - w1["loss"]) / abs(w1["loss"]), tol["loss"])
        ok &= _report("materialised loss 2", abs(float(ls2) - w2["loss"]) / abs(w2["loss"]), tol["loss"])
        ok &= _report("materialised dv1", R.rel(mv1.cpu().numpy(), w1["dv"]), tol["dv"])
        ok &= _report("materialised dv2", R.rel(mv2.cpu().numpy(), w2["dv"]), tol["dv"])
        # bitwise repeatability of two calls
        loss_b, dv1_b, dv2_b = call.fused(set_z=False)
        assert torch.equal(loss, loss_b) and torch.equal(dv1, dv1_b) and torch.equal(dv2, dv2_b)
        o1_b, _ = call.scores(set_z=False)
        assert torch.equal(o1, o1_b)
        # the update of the banks, behind the gathers
        _update(m1, m2, v1, v2, _cu(y_np), mom, call.bad)
        n1, n2 = m1.cpu().numpy(), m2.cpu().numpy()
        untouched = np.ones(n_data, bool)
        untouched[y_np] = False
        assert np.array_equal(n1[untouched], m1_np[untouched]) and np.array_equal(n2[untouched], m2_np[untouched])    # bit-equal
        want1, want2 = R.update(m1_np, v1.cpu().numpy(), y_np, mom), R.update(m2_np, v2.cpu().numpy(), y_np, mom)      # last writer wins
        ok &= _report("rows_v1", R.rel(n1[y_np], want1[y_np]), tol["rows"])
        ok &= _report("rows_v2", R.rel(n2[y_np], want2[y_np]), tol["rows"])
        if rep:
            assert len(set(y_np.tolist())) < B
        assert int(call.bad.item()) == 0
    assert ok


@pytest.mark.parametrize("d", [64, 128, 512, 1280])
@pytest.mark.parametrize("B", [1, 7, 64])
@pytest.mark.parametrize("nce_k", [1, 255, 16384])
def test_sweep_against_the_restatement(g11, d, B, nce_k):
    n_data, T = 2048, 0.07
    tol = {k: 2 * max(float(g11[f"c{c}_ref_vs_f64_{k}"]) for c in range(3)) for k in ("loss", "dv", "out", "z")}
    rng = np.random.default_rng(d * 131 + B * 17 + nce_k)
    stdv = 1 / np.sqrt(d / 3)
    m1_np = rng.uniform(-stdv, stdv, (n_data, d)).astype(np.float32)
    m2_np = rng.uniform(-stdv, stdv, (n_data, d)).astype(np.float32)
    m1_np[: n_data // 2] /= np.linalg.norm(m1_np[: n_data // 2], axis=1, keepdims=True)       # half of the rows already updated
    m2_np[: n_data // 2] /= np.linalg.norm(m2_np[: n_data // 2], axis=1, keepdims=True)
    v = rng.standard_normal((2, B, d))
    v = (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)
    idx_np = rng.integers(0, n_data, (B, nce_k + 1))
    idx_np[:, 0] = rng.permutation(n_data)[:B]
    call = Call(_cu(v[0]), _cu(v[1]), _cu(m1_np), _cu(m2_np), _cu(idx_np), T)
    loss, dv1, dv2 = call.fused(set_z=True)
    o1, o2 = call.scores(set_z=False)
    Z = call.Z.cpu().numpy().astype(np.float64)
    assert int(call.bad.item()) == 0
    w1, w2 = R.side_dense(v[0], m2_np, idx_np, T, Z[0]), R.side_dense(v[1], m1_np, idx_np, T, Z[1])
    l = loss.cpu().numpy().astype(np.float64)
    ok = True
    for s_, w_ in ((0, w1), (1, w2)):
        zf = R.z_of(w_["e"], n_data)
        ok &= _report(f"Z {s_ + 1}", abs(Z[s_] - zf) / zf, tol["z"])
        ok &= _report(f"loss {s_ + 1}", abs(l[s_] - w_["loss"]) / abs(w_["loss"]), tol["loss"])
    ok &= _report("out_v1", R.rel(o1.cpu().numpy(), w1["x"]), tol["out"])
    ok &= _report("out_v2", R.rel(o2.cpu().numpy(), w2["x"]), tol["out"])
    ok &= _report("dv1", R.rel(dv1.cpu().numpy(), w1["dv"]), tol["dv"])
    ok &= _report("dv2", R.rel(dv2.cpu().numpy(), w2["dv"]), tol["dv"])
    # forward only (dv NULL, NULL): the same loss bits
    loss_f, _, _ = call.fused(set_z=False, want_dv=False)
    assert torch.equal(loss_f, loss)
    assert ok


def test_guards_around_every_operand_output_and_workspace(monkeypatch):
    """NaN canaries (tests/test_gpu_guard.py) in front of and behind every operand, every output and the workspace, at ragged shapes:
    no write outside a buffer, and results bit-equal to the same calls on ordinary allocations (a read past an operand's end would
    bring a NaN in)"""
    from moma_amd import ops
    from tests.test_gpu_guard import _Guarded, _in
    for (B, d, K, n_data) in [(3, 68, 37, 50), (5, 132, 130, 77), (2, 1284, 9, 40), (7, 64, 1, 64), (4, 12, 66, 30)]:
        rng = np.random.default_rng(B * d + K)
        v1, v2 = _cu(rng.standard_normal((B, d)) / np.sqrt(d), torch.float32), _cu(rng.standard_normal((B, d)) / np.sqrt(d), torch.float32)
        m1, m2 = _cu(rng.standard_normal((n_data, d)) / np.sqrt(d), torch.float32), _cu(rng.standard_normal((n_data, d)) / np.sqrt(d), torch.float32)
        idx = _cu(rng.integers(0, n_data, (B, K + 1)))
        y = idx[:, 0].contiguous()
        g0 = _cu(rng.standard_normal(2), torch.float32)

        def run(wrap, alloc):
            a1, a2, b1, b2, ii, yy = (wrap(t) for t in (v1, v2, m1, m2, idx, y))
            a1.requires_grad_(True); a2.requires_grad_(True)
            Z, bad = alloc.zeros(2, device="cuda", dtype=torch.float32), alloc.zeros(1, device="cuda", dtype=torch.int32)
            loss = ops.crd_fused(a1, a2, b1, b2, ii, 0.07, n_data, Z, True, bad)
            (loss * g0).sum().backward()
            f = (loss.detach().clone(), a1.grad.clone(), a2.grad.clone(), Z.clone())
            a1.grad = a2.grad = None
            o1, o2 = ops.crd_scores(a1, a2, b1, b2, ii, 0.07, n_data, Z, False, bad, update_y=yy)
            ops.crd_update_(b1, b2, a1.detach(), a2.detach(), yy, 0.5, bad)
            (o1.sum() * 0.5 + (o2 * o2).sum()).backward()
            return f + (o1.detach().clone(), o2.detach().clone(), a1.grad.clone(), a2.grad.clone(), b1.clone(), b2.clone(), bad.clone())

        plain = run(lambda t: t.clone(), torch)
        guard = _Guarded()
        monkeypatch.setattr(ops, "torch", guard)
        try:
            guarded = run(lambda t: _in(guard, t), guard)
            assert guard.check(f"crd B={B} d={d} K={K}") > 0
        finally:
            monkeypatch.setattr(ops, "torch", torch)
        for a, b in zip(plain, guarded):
            assert torch.equal(a, b) and (not a.is_floating_point() or bool(torch.isfinite(a).all()))


def test_an_index_that_is_no_row_is_skipped_and_flagged(g11):
    """One entry of idx set to n_data and one to -1: nothing comes from them, the flag is set, everything else equals the call on
    the index matrix without those two columns.  (The kernel's check -- `id < 0 || id >= n_data` in front of every address that is
    formed from an index, csrc/crd.hip -- was read before this test was written; it tests the guard.)"""
    B, d, K, n_data, T = 4, 128, 300, 500, 0.07
    tol = {k: 2 * max(float(g11[f"c{c}_ref_vs_f64_{k}"]) for c in range(3)) for k in ("loss", "dv", "rows")}
    rng = np.random.default_rng(5)
    v = rng.standard_normal((2, B, d))
    v = (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)
    m1, m2 = _cu(rng.uniform(-.15, .15, (n_data, d)), torch.float32), _cu(rng.uniform(-.15, .15, (n_data, d)), torch.float32)
    idx_np = rng.integers(0, n_data, (B, K + 1))
    Z = torch.tensor([700.0, 650.0], device="cuda")
    good = Call(_cu(v[0]), _cu(v[1]), m1, m2, _cu(idx_np), T, Z)
    bad_np = idx_np.copy()
    bad_np[1, 17] = n_data
    bad_np[2, 255] = -1
    bad = Call(_cu(v[0]), _cu(v[1]), m1, m2, _cu(bad_np), T, Z)
    ob1, ob2 = bad.scores(set_z=False)
    og1, og2 = good.scores(set_z=False)
    assert int(bad.bad.item()) == 1 and int(good.bad.item()) == 0
    assert float(ob1[1, 17]) == 0 and float(ob2[2, 255]) == 0 and float(ob1[2, 255]) == 0
    mask = torch.ones(B, K + 1, dtype=torch.bool, device="cuda")
    mask[1, 17] = mask[2, 255] = False
    assert torch.equal(ob1[mask], og1[mask]) and torch.equal(ob2[mask], og2[mask])
    # the fused pass: equal to the float64 evaluation that leaves the two entries out
    bad.bad.zero_()
    loss, dv1, dv2 = bad.fused(set_z=False)
    assert int(bad.bad.item()) == 1
    w1 = R.side(v[0], m2.cpu().numpy(), bad_np, T, 700.0)
    lg, dg1, _ = good.fused(set_z=False)
    assert _report("loss", abs(float(loss[0]) - w1["loss"]) / abs(w1["loss"]), tol["loss"])
    assert _report("dv1", R.rel(dv1.cpu().numpy(), w1["dv"]), tol["dv"])
    assert torch.equal(dv1[0], dg1[0]) and torch.equal(dv1[3], dg1[3])         # rows of the batch without such an entry: same bits
    # the update: a y that is no row is skipped and flagged, the other rows are updated as without it
    y_np = np.array([3, n_data, 9, -1])
    ma, mb = m1.clone(), m2.clone()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _update(ma, mb, _cu(v[0]), _cu(v[1]), _cu(y_np), 0.5, flag)
    assert int(flag.item()) == 1
    changed = (ma != m1).any(1).nonzero().flatten().tolist()
    assert changed == [3, 9]
    want = R.update(m1.cpu().numpy(), v[0], y_np, 0.5)
    assert _report("rows", R.rel(ma.cpu().numpy()[[3, 9]], want[[3, 9]]), tol["rows"])


def _crd_training(steps_per_epoch, n_data=None, fused=True):
    from moma_amd.train_student_moma import build_training, parse_option
    from moma_amd.dataset.synthetic import SyntheticSampleLoader
    argv = ["--distill", "crd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
            "--batch_size", "16", "--steps_per_epoch", str(steps_per_epoch), "--nce_k", "128", "--feat_dim", "64", "-b", "0.8",
            "--learning_rate", "0.02", "--no_graph_teacher"] + ([] if fused else ["--no_fused"]) + ([] if n_data is None else ["--n_data", str(n_data)])
    opt = parse_option(argv)
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size = 0, False, 0, 1
    dev = torch.device("cuda", 0)
    opt.device = dev
    torch.manual_seed(77)
    built = build_training(opt, dev)
    loader = SyntheticSampleLoader(steps_per_epoch, 16, 32, 4, opt.nce_k, opt.mode, 5, dev, n_data=opt.n_data)
    return opt, built, loader


def _epoch(opt, built, loader, epoch):
    from moma_amd.helper.loops_moma import train_distill_moma
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = built
    opt.trace = []
    opt.print_freq = 1000
    train_distill_moma(epoch, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    return [float(t[0]) for t in opt.trace], [float(t[2]) for t in opt.trace]


@pytest.mark.parametrize("fused", [True, False])
def test_twenty_training_steps(fused):
    """train_distill_moma with --distill crd on the resnet8x4 / resnet32x4 pair, 20 steps = two epochs of ten over the same 160 of
    400 samples (in the second the positive row of the bank is the sample's own earlier embedding): the KD term is finite and
    falls, the banks change at the visited rows only, Z is set once, the teacher-side head trains, the teacher does not"""
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    opt, built, loader = _crd_training(10, n_data=400, fused=fused)
    kd = built[3][2]
    b1, b2 = kd.contrast.memory_v1.clone(), kd.contrast.memory_v2.clone()
    wt, wteacher = kd.embed_t.linear.weight.detach().clone(), [p.detach().clone() for p in built[1].parameters()]
    losses, kds = _epoch(opt, built, loader, 1)
    l2, k2 = _epoch(opt, built, loader, 2)
    losses, kds = losses + l2, kds + k2
    assert len(kds) == 20 and np.isfinite(kds).all() and np.isfinite(losses).all()
    print("loss_kd per step:", " ".join(f"{v:.4f}" for v in kds))
    assert np.mean(kds[-5:]) < np.mean(kds[:5])
    visited = torch.zeros(opt.n_data, dtype=torch.bool, device="cuda")
    for _, _, index, _ in loader:
        visited[index] = True
    assert int(visited.sum()) == 160
    ch1, ch2 = (kd.contrast.memory_v1 != b1).any(1), (kd.contrast.memory_v2 != b2).any(1)
    assert torch.equal(ch1, visited) and torch.equal(ch2, visited)
    n1 = kd.contrast.memory_v1[visited].norm(dim=1)
    assert float((n1 - 1).abs().max()) < 1e-5
    p = kd.contrast.params.tolist()
    assert p[0] == 128 and p[2] > 0 and p[3] > 0
    assert not torch.equal(kd.embed_t.linear.weight, wt)
    assert all(torch.equal(a, b) for a, b in zip(built[1].parameters(), wteacher))
    kd.contrast.check_indices()


def test_fused_and_materialised_modules_agree_and_idx_none_draws(g11):
    # each path is allowed twice the reference's distance from the float64 value: the two may differ by four times it
    tol = {k: 4 * max(float(g11[f"c{c}_ref_vs_f64_{k}"]) for c in range(3)) for k in ("loss", "dv")}
    from moma_amd.crd import ContrastMemory
    torch.manual_seed(3)
    a, b = ContrastMemory(128, 700, 200).cuda(), ContrastMemory(128, 700, 200).cuda()
    b.load_state_dict(a.state_dict())
    from moma_amd.crd import ContrastLoss
    crit = ContrastLoss(700)
    for step in range(3):
        v1 = torch.nn.functional.normalize(torch.randn(9, 128, device="cuda")).requires_grad_(True)
        v2 = torch.nn.functional.normalize(torch.randn(9, 128, device="cuda")).requires_grad_(True)
        y = torch.randperm(700, device="cuda")[:9]
        idx = torch.randint(0, 700, (9, 201), device="cuda")
        idx[:, 0] = y
        la = a.forward_fused(v1, v2, y, idx)
        la.backward()
        ga = (v1.grad.clone(), v2.grad.clone())
        v1.grad = v2.grad = None
        o1, o2 = b(v1, v2, y, idx)
        assert o1.shape == (9, 201, 1)
        lb = (crit(o1) + crit(o2)).sum()
        lb.backward()                                   # (behind the update of b's banks: the pre-update rows stand in)
        assert _report("loss", abs(float(la) - float(lb)) / abs(float(lb)), tol["loss"])
        assert _report("dv1", R.rel(v1.grad.cpu().numpy(), ga[0].cpu().numpy()), tol["dv"])
        assert _report("dv2", R.rel(v2.grad.cpu().numpy(), ga[1].cpu().numpy()), tol["dv"])
        assert torch.equal(a.memory_v1, b.memory_v1) and torch.equal(a.memory_v2, b.memory_v2) and torch.equal(a.params, b.params)
    assert a._state()[3] is False and float(a.params[2]) > 0
    loss = a.forward_fused(v1.detach(), v2.detach(), y)             # idx=None: drawn from the alias tables on the device
    assert bool(torch.isfinite(loss))
    a.check_indices()


def test_checkpoint_resume_round_trip_continues_with_identical_losses(tmp_path):
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    opt, built, loader = _crd_training(6)
    _epoch(opt, built, loader, 1)
    model_s, model_t, module_list, criterion_list, _tr, _c, optimizer = built
    path = str(tmp_path / "ck.pth")
    torch.save({"model": model_s.state_dict(), "model_t": model_t.state_dict(), "criterion_kd": criterion_list[2].state_dict(),
                "optimizer": optimizer.state_dict(), "loader_gen": loader.gen.get_state(), "rng": torch.cuda.get_rng_state()}, path)
    straight = _epoch(opt, built, loader, 2)
    opt2, built2, loader2 = _crd_training(6)
    ck = torch.load(path, map_location="cuda", weights_only=False)
    built2[0].load_state_dict(ck["model"]); built2[1].load_state_dict(ck["model_t"])
    built2[3][2].load_state_dict(ck["criterion_kd"]); built2[6].load_state_dict(ck["optimizer"])
    loader2.gen.set_state(ck["loader_gen"].cpu()); torch.cuda.set_rng_state(ck["rng"].cpu())
    assert {"contrast.memory_v1", "contrast.memory_v2", "contrast.params"} <= set(ck["criterion_kd"])
    assert float(ck["criterion_kd"]["contrast.params"][2]) > 0
    resumed = _epoch(opt2, built2, loader2, 2)
    assert resumed == straight                                       # identical losses, step by step
    assert torch.equal(built2[3][2].contrast.params, built[3][2].contrast.params)          # Z carried over, not set again


def test_cli_trains_checkpoints_and_resumes(tmp_path):
    import glob
    import subprocess
    import sys
    base = [sys.executable, os.path.join(ROOT, "train_student_moma.py"), "--distill", "crd", "--model_s", "resnet8x4", "--model_t",
            "resnet32x4", "--dataset", "cifar100", "-b", "0.8", "--n_cls", "4", "--batch_size", "16", "--steps_per_epoch", "6",
            "--nce_k", "256", "--feat_dim", "128", "--print_freq", "2", "--miopen_find", "off", "--save_root", str(tmp_path)]
    r = subprocess.run(base + ["--epochs", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "images/sec" in r.stdout
    ck = glob.glob(str(tmp_path / "**" / "ckpt_last.pth"), recursive=True)
    assert len(ck) == 1
    state = torch.load(ck[0], map_location="cpu", weights_only=False)
    z = state["criterion_kd"]["contrast.params"][2:4]
    assert state["epoch"] == 1 and bool((z > 0).all()) and state["criterion_kd"]["contrast.memory_v1"].shape == (96, 128)
    r = subprocess.run(base + ["--epochs", "2", "--resume", ck[0]], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "resumed from" in r.stdout
    state2 = torch.load(ck[0], map_location="cpu", weights_only=False)
    assert state2["epoch"] == 2 and torch.equal(state2["criterion_kd"]["contrast.params"][2:4], z)      # Z is not set a second time
    assert not torch.equal(state2["criterion_kd"]["contrast.memory_v1"], state["criterion_kd"]["contrast.memory_v1"])

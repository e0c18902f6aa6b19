"""CPU checks of the `--distill pkt` path: the numpy restatement of the Probabilistic Knowledge Transfer formulas (tests/pkt_ref.py)
against the golden fixture recorded from the reference and against torch autograd over the published formula in float64, the
documented deviation on an all-zero student row, the criterion's stock-torch composite on CPU tensors, the workspace query and the
argument checks of the C ABI, the construction of the training objects and one CPU step of the loop.  (The C ABI's table-driven
argument test in tests/test_abi_cpu.py picks the new entry points up by itself.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import golden_npz, pkt_fixture, pkt_ref as R
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 4, 4), (2, 3, 5), (3, 8, 8), (5, 3, 1), (5, 17, 33), (8, 64, 40), (33, 100, 60), (65, 24, 24), (16, 128, 256),
          (12, 32, 32), (12, 32, 32), (16, 1283, 1280), (64, 1280, 1280)]
ZERO = pkt_fixture.ZERO_CASE
EPS = 1e-7


def _defined_rows(c):
    """the rows on which the reference's autograd is defined (all but an all-zero student row)"""
    return ~c["nan_rows"] if "nan_rows" in c else np.ones(c["shape"][0], bool)


def _published(f_s, f_t, eps=EPS):
    """the published form of the loss, typed again in torch ops (float64 in, float64 out): rows / (norm + eps) -> mm -> (. + 1) / 2
    -> rows / row sums -> mean of T log((T + eps) / (P + eps))"""
    def prob(f):
        x = f.reshape(f.shape[0], -1)
        x = x / (x.pow(2).sum(1, keepdim=True).sqrt() + eps)
        k = (x @ x.t() + 1.0) / 2.0
        return k / k.sum(1, keepdim=True)
    p, t = prob(f_s), prob(f_t)
    return (t * torch.log((t + eps) / (p + eps))).mean()


def test_fixture_files_stay_below_the_size_limit():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "g16_pkt*.npz"))
    assert files and all(os.path.getsize(f) < golden_npz.LIMIT for f in files)


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation): the generator printed at most 2.5e-6 of abs_terms
    for the loss (the +3 case), 1.9e-5 for the gradient (the same case) and 0 for G (sums of multiples of 1/1024 this small are
    exact in fp32), so the allowances are 4.9e-6, 3.8e-5 and the floor of one fp32 ulp.  G is exactly symmetric"""
    cases, allow = pkt_fixture.load()
    assert [c["shape"] for c in cases] == SHAPES
    assert allow["loss"] < 1e-5 and allow["grad"] < 1e-4 and allow["G"] == pkt_fixture.ULP32
    for ci, c in enumerate(cases):
        w = R.pair(c["f_s"], c["f_t"])
        for G in (w["G_s"], w["G_t"], w["M"]):
            assert np.array_equal(G, G.T)
        assert np.isfinite(w["dF_s"]).all() and np.isfinite(w["M"]).all() and np.isfinite(w["loss"])
        rows = _defined_rows(c)
        assert np.isfinite(c["dF_s"][rows]).all()
        if c["shape"][0] == 1:
            assert c["loss"] == 0 and w["loss"] == 0 and not c["dF_s"].any() and not w["dF_s"].any()
            continue
        assert abs(c["loss"] - w["loss"]) <= c["ref_vs_f64_loss"] * w["abs_terms"] * (1 + 1e-9)
        assert rel(c["dF_s"][rows], w["dF_s"][rows]) <= c["ref_vs_f64_grad"] * (1 + 1e-9)
    w = R.pair(cases[pkt_fixture.DUP_CASE]["f_s"], cases[pkt_fixture.DUP_CASE]["f_t"])
    (a, b), (ta, tb) = pkt_fixture.DUP_S, pkt_fixture.DUP_T
    assert np.array_equal(w["P"][a], w["P"][b]) and np.array_equal(w["T"][ta], w["T"][tb])


def test_restatement_agrees_with_autograd_over_the_published_formula():
    """every fixture case in float64: torch autograd over the published formula vs the restatement's closed form, on the rows
    autograd defines.  Both are float64 evaluations of the same function in different orders: the bound 1e-9 (of abs_terms for the
    loss, of the largest gradient element for the gradient) is 2^-53 times a generous 1e7 for the length of the longest chain of
    roundings (B^2 terms behind a D-term dot product), and four orders of magnitude below the fp32 distances the fixture records"""
    cases, _allow = pkt_fixture.load()
    for ci, c in enumerate(cases):
        f_s = torch.from_numpy(c["f_s"]).double().requires_grad_(True)
        loss = _published(f_s, torch.from_numpy(c["f_t"]).double())
        loss.backward()
        w = R.pair(c["f_s"], c["f_t"])
        rows = _defined_rows(c)
        got = f_s.grad.numpy()
        assert np.isfinite(got[rows]).all() and (ci == ZERO) == bool(np.isnan(got[~rows]).any() if (~rows).any() else False)
        if c["shape"][0] == 1:                                           # (loss and gradient vanish identically: absolute)
            assert abs(float(loss.detach())) <= 1e-9 and np.abs(got).max() <= 1e-9 and not w["dF_s"].any()
            continue
        d_loss = abs(float(loss.detach()) - w["loss"]) / w["abs_terms"]
        d_grad = rel(got[rows], w["dF_s"][rows])
        print(f"case {ci} {c['shape']}: loss {d_loss:.2e} grad {d_grad:.2e}")
        assert d_loss <= 1e-9 and d_grad <= 1e-9


def test_restatement_gradient_is_the_derivative_of_its_loss():
    """central differences of the float64 loss at (B, Ds, Dt) = (4, 3, 2)"""
    rng = np.random.default_rng(5)
    f_s, f_t = rng.standard_normal((4, 3)), rng.standard_normal((4, 2))
    g = R.pair(f_s, f_t, g_loss=1.5)["dF_s"]
    num = np.zeros_like(f_s)
    for idx in np.ndindex(*f_s.shape):
        d = np.zeros_like(f_s)
        d[idx] = 1e-6
        num[idx] = 1.5 * (R.pair(f_s + d, f_t)["loss"] - R.pair(f_s - d, f_t)["loss"]) / 2e-6
    assert np.abs(num - g).max() < 1e-7 * max(1.0, np.abs(g).max())


def test_zero_row_the_documented_deviation():
    """an all-zero student row: the reference's autograd returns NaN for that row alone (sqrt's backward at 0); the restatement's
    gradient there is finite, equal to sum_j M'_ij x_j, and the derivative of the loss at that point (central differences).  It is
    NOT small: x / (|x| + eps) has slope 1 / eps = 1e7 at 0, so the row's gradient is about 1e7 times the other rows' (here 1.9e3
    against 1e-4) -- the true derivative, bounded by 1 / eps times an ordinary row's"""
    cases, _allow = pkt_fixture.load()
    c = cases[ZERO]
    z = pkt_fixture.ZERO_S
    assert list(np.flatnonzero(c["nan_rows"])) == [z] and np.isnan(c["dF_s"][z]).all()
    assert np.isfinite(c["dF_s"][~c["nan_rows"]]).all() and not c["f_s"][z].any() and not c["f_t"][pkt_fixture.ZERO_T].any()
    w = R.pair(c["f_s"], c["f_t"])
    assert np.isfinite(w["dF_s"]).all() and np.abs(w["dF_s"][z]).max() > 0
    X = c["f_s"].astype(np.float64)
    assert np.allclose(w["dF_s"][z], w["M"][z] @ X, rtol=1e-12, atol=0)
    others = np.abs(np.delete(w["dF_s"], z, 0)).max()
    # |sum_j M'_zj x_j| <= (1 / eps) sum_j |M_zj| |x_j| / (n_j + eps) <= (1 / eps) sum_j |W_zj + W_jz|
    assert 0 < others < 1e-3 and np.abs(w["dF_s"][z]).max() <= np.abs(w["W"][z] + w["W"][:, z]).sum() / EPS
    # x |x| is odd, so the central difference keeps an error of h / eps relative: h = 1e-11 for 1e-4
    for k in range(3):
        d = np.zeros_like(X)
        d[z, k] = 1e-11
        num = (R.pair(X + d, c["f_t"])["loss"] - R.pair(X - d, c["f_t"])["loss"]) / 2e-11
        assert abs(num - w["dF_s"][z, k]) <= 1e-3 * np.abs(w["dF_s"][z]).max()
    assert np.array_equal(w["C_s"][z], np.zeros(len(X))) and np.array_equal(w["C_t"][pkt_fixture.ZERO_T], np.zeros(len(X)))


def test_composite_on_cpu_tensors_matches_the_restatement():
    from moma_amd.distiller_zoo import PKT
    cases, allow = pkt_fixture.load()
    crit = PKT()
    for ci, c in enumerate(cases):
        f_s, f_t = torch.from_numpy(c["f_s"]).requires_grad_(True), torch.from_numpy(c["f_t"])
        loss = crit(f_s, f_t)
        loss.backward()
        w = R.pair(c["f_s"], c["f_t"])
        assert loss.dtype == torch.float32 and loss.dim() == 0 and np.isfinite(loss.item())
        assert abs(loss.item() - w["loss"]) <= allow["loss"] * w["abs_terms"]
        assert bool(torch.isfinite(f_s.grad).all())                       # (the zero row too: a CPU step never produces NaN)
        if c["shape"][0] == 1:                                            # (vanishes identically; autograd leaves float64 noise)
            assert float(f_s.grad.abs().max()) <= 1e-12
            continue
        assert rel(f_s.grad.numpy(), w["dF_s"]) <= allow["grad"]          # (every row: the composite follows the same zero-row rule)
        rows = _defined_rows(c)                                           # (and the rows next to a zero row in their own scale)
        assert rel(f_s.grad.numpy()[rows], w["dF_s"][rows]) <= allow["grad"]
    # [B, C, 1, 1] maps; bfloat16 and float16 storage (evaluated in float64, returned in float32)
    f = torch.randn(6, 10, 1, 1)
    t = torch.randn(6, 7, 1, 1)
    w = R.pair(f.numpy(), t.numpy())
    assert abs(float(crit(f, t)) - w["loss"]) <= allow["loss"] * w["abs_terms"]
    for dt in (torch.bfloat16, torch.float16):
        fh, th = f.to(dt).requires_grad_(True), t.to(dt)
        lh = crit(fh, th)
        lh.backward()
        wh = R.pair(fh.detach().float().numpy(), th.float().numpy())
        assert lh.dtype == torch.float32 and abs(lh.item() - wh["loss"]) <= allow["loss"] * wh["abs_terms"]
        assert fh.grad.dtype == dt and fh.grad.shape == fh.shape and bool(torch.isfinite(fh.grad).all())
    # a teacher that wants a gradient gets one
    tg = torch.randn(6, 7, requires_grad=True)
    crit(f, tg).backward()
    assert tg.grad is not None and bool(tg.grad.abs().sum() > 0)
    with pytest.raises(ValueError):
        crit(torch.randn(4, 3), torch.randn(5, 3))


def test_a_single_row_gives_zero():
    """B = 1: P = T = 1, loss 0 and gradient 0 -- legal (the composite's autograd leaves float64 rounding noise of 1e-24 in the
    gradient of O(1) inputs; the closed form gives exact zeros)"""
    from moma_amd.distiller_zoo import PKT
    f_s = torch.randn(1, 5, requires_grad=True)
    loss = PKT()(f_s, torch.randn(1, 3))
    loss.backward()
    assert float(loss.detach()) == 0 and float(f_s.grad.abs().max()) <= 1e-12
    w = R.pair(f_s.detach().numpy(), np.ones((1, 3)))
    assert w["loss"] == 0 and not w["dF_s"].any()


def test_ops_pkt_loss_refuses_cpu_tensors():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    with pytest.raises(_lib.MomaHipError):
        ops.pkt_loss(torch.zeros(3, 4), torch.zeros(3, 4))


def test_workspace_query_and_argument_checks():
    """host arithmetic only: the workspace is (B^2 + 2 B) doubles; fewer than 1 or more than MOMA_PKT_MAX_B rows, an empty row, a
    null pointer, an unknown dtype, a misaligned buffer and a workspace that is too small are refused before anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.moma_pkt_workspace_bytes
    assert _lib.PKT_MAX_B == 1024 and lib.moma_version() == 4
    assert f(1) == 3 * 8 and f(2) == 8 * 8 and f(17) == (289 + 34) * 8 and f(1024) == (1024 * 1024 + 2048) * 8
    assert f(0) == 0 and f(-3) == 0 and f(1025) == 0
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    odd = lambda n: C.c_void_p(p.value + n)                                                           # noqa: E731
    f32, bf16, big = _lib.DT_F32, _lib.DT_BF16, 1 << 30
    gram = lambda B, D=8, dt=f32, ptr=p, G=p: lib.moma_pkt_gram(ptr, B, D, dt, G, None)               # noqa: E731
    bwd = lambda B, D=8, dt=f32, ptr=p, G=p: lib.moma_pkt_bwd(ptr, G, p, p, B, D, dt, None)           # noqa: E731
    terms = lambda B, ws=big, ptr=p, M=p: lib.moma_pkt_terms(ptr, p, B, p, ws, M, p, None)            # noqa: E731
    for call in (gram, bwd):
        assert call(4, ptr=None) == -1                                                                # MOMA_E_NULL
        assert call(0) == -2 and call(-1) == -2 and call(4, D=0) == -2                                # MOMA_E_SHAPE
        assert call(4, dt=7) == -3                                                                    # MOMA_E_DTYPE
        assert call(1025) == -6                                                                       # MOMA_E_UNSUPPORTED
        assert call(4, dt=bf16, ptr=odd(1)) == -4 and call(4, ptr=odd(2)) == -4 and call(4, G=odd(4)) == -4      # MOMA_E_ALIGN
    pair = lambda B, Ds=8, Dt=8, ds=f32, dt=f32, fs=p, ft=p, Gt=p: lib.moma_pkt_gram_pair(fs, Ds, ds, ft, Dt, dt, B, p, Gt, None)      # noqa: E731
    assert pair(4, fs=None) == -1 and pair(4, ft=None) == -1 and pair(0) == -2 and pair(4, Ds=0) == -2 and pair(4, Dt=0) == -2
    assert pair(4, ds=7) == -3 and pair(4, dt=7) == -3 and pair(1025) == -6
    assert pair(4, dt=bf16, ft=odd(1)) == -4 and pair(4, fs=odd(2)) == -4 and pair(4, Gt=odd(4)) == -4
    assert terms(4, ptr=None) == -1 and terms(0) == -2 and terms(1025) == -6
    assert terms(4, ws=f(4) - 1) == -5 and terms(4, M=odd(4)) == -4


def _pkt_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "pkt", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "1",
                        "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_with_distill_pkt():
    """(the parent commit has no PKT criterion and its build_training raises NotImplementedError("pkt"))"""
    from moma_amd.distiller_zoo import PKT
    _opt, built = _pkt_training(torch.device("cpu"))
    model_s, _model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    assert isinstance(criterion_list[2], PKT) and contrast is None
    assert len(list(criterion_list[2].parameters())) == 0 and len(trainable_list) == 1 and len(module_list) == 2
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()}


def test_one_cpu_step_of_the_loop():
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _pkt_training(dev)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = built
    before = [p.detach().clone() for p in model_s.parameters()]
    teacher_before = [p.detach().clone() for p in model_t.parameters()]
    opt.trace, opt.print_freq = [], 1000
    loader = SyntheticLoader(1, 8, 32, 4, 3, dev)
    train_distill_moma(1, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    (loss, _idx, loss_kd), = opt.trace
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd)) and float(loss_kd) > 0
    grads = [p.grad for p in model_s.parameters()]
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads) and any(g is not None and bool(g.abs().sum() > 0) for g in grads)
    assert any(not torch.equal(a, b) for a, b in zip(before, model_s.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
    # the KD term is the restatement's value on feat[-1] of the same (pre-step) models: the composite evaluates in float64 and
    # returns float32 -- one rounding of the loss, 2^-24 of it, and the loss is at most abs_terms
    _opt2, built2 = _pkt_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    want = R.pair(fs[-1].numpy(), ft[-1].numpy())
    assert abs(float(loss_kd) - want["loss"]) <= 1e-6 * want["abs_terms"]

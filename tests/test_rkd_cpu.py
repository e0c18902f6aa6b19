"""CPU checks of the `--distill rkd` path: the numpy restatement of the Relational Knowledge Distillation formulas
(tests/rkd_ref.py) against the golden fixture recorded from the reference, the documented deviation on duplicated rows, the
criterion's stock-torch composite on CPU tensors, the workspace query and the argument checks of the C ABI, the construction of the
training objects and one CPU step of the loop.  (The C ABI's table-driven argument test in tests/test_abi_cpu.py picks the new entry
points up by itself.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import golden_npz, rkd_fixture, rkd_ref as R
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 3, 5), (3, 8, 8), (5, 3, 1), (5, 17, 33), (8, 64, 40), (33, 100, 60), (65, 24, 24), (16, 128, 256), (12, 32, 32),
          (12, 32, 32), (16, 1283, 1280)]
DUP = rkd_fixture.DUP_CASE
W_D, W_A = 25.0, 50.0


def _other_rows(ci, B):
    rows = np.ones(B, bool)
    if ci == DUP:
        rows[list(rkd_fixture.DUP_S)] = False
    return rows


def test_fixture_files_stay_below_the_size_limit():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "g14_rkd*.npz"))
    assert files and all(os.path.getsize(f) < golden_npz.LIMIT for f in files)


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation); S is exactly symmetric with an exactly zero diagonal"""
    cases, allow = rkd_fixture.load()
    assert [c["shape"] for c in cases] == SHAPES
    assert allow["loss"] < 2e-6 and allow["grad"] < 1e-5 and allow["S"] < 1e-6
    for ci, c in enumerate(cases):
        B = c["shape"][0]
        w = R.pair(c["f_s"], c["f_t"])
        for S in (w["S_s"], w["S_t"]):
            assert np.array_equal(S, S.T) and not np.diag(S).any()
        assert np.isfinite(w["dF_s"]).all() and np.isfinite(w["Q"]).all() and np.isfinite(c["dF_s"]).all()
        if B == 2:
            continue                                                      # (both terms vanish identically: below)
        assert abs(c["loss"] - w["loss"]) <= c["ref_vs_f64_loss"] * w["loss"] * (1 + 1e-9)
        rows = _other_rows(ci, B)
        assert rel(c["dF_s"][rows], w["dF_s"][rows]) <= c["ref_vs_f64_grad"] * (1 + 1e-9)
    w = R.pair(cases[DUP]["f_s"], cases[DUP]["f_t"])
    (a, b), (ta, tb) = rkd_fixture.DUP_S, rkd_fixture.DUP_T
    assert w["S_s"][a, b] == 0 and w["S_t"][ta, tb] == 0


def test_duplicated_rows_the_documented_deviation():
    """two exactly equal student rows: the reference's autograd divides by F.normalize's clamp and returns gradients more than 1e6
    times anything the formulas give; the restatement's gradient is finite and of ordinary size on every row"""
    cases, _allow = rkd_fixture.load()
    c = cases[DUP]
    w = R.pair(c["f_s"], c["f_t"])
    biggest = np.abs(w["dF_s"]).max()
    assert np.isfinite(biggest) and 0 < biggest < 10
    for r in rkd_fixture.DUP_S:
        assert c["row_max"][r] > 1e6 * biggest
    assert c["row_max"][_other_rows(DUP, c["shape"][0])].max() < 10


def test_restatement_gradient_is_the_derivative_of_its_loss():
    """central differences of the float64 loss at (B, Ds, Dt) = (4, 3, 2), no duplicates"""
    rng = np.random.default_rng(5)
    f_s, f_t = rng.standard_normal((4, 3)), rng.standard_normal((4, 2))
    g = R.pair(f_s, f_t, g_loss=1.5)["dF_s"]
    num = np.zeros_like(f_s)
    for idx in np.ndindex(*f_s.shape):
        d = np.zeros_like(f_s)
        d[idx] = 1e-6
        num[idx] = 1.5 * (R.pair(f_s + d, f_t)["loss"] - R.pair(f_s - d, f_t)["loss"]) / 2e-6
    assert np.abs(num - g).max() < 1e-7 * max(1.0, np.abs(g).max())


def test_composite_on_cpu_tensors_matches_the_restatement():
    from moma_amd.distiller_zoo import RKDLoss
    cases, allow = rkd_fixture.load()
    crit = RKDLoss()
    for ci, c in enumerate(cases):
        if c["shape"][0] == 2:
            continue
        f_s, f_t = torch.from_numpy(c["f_s"]).requires_grad_(True), torch.from_numpy(c["f_t"])
        loss = crit(f_s, f_t)
        loss.backward()
        w = R.pair(c["f_s"], c["f_t"])
        assert loss.dtype == torch.float32 and loss.dim() == 0 and abs(loss.item() - w["loss"]) <= allow["loss"] * w["loss"]
        assert rel(f_s.grad.numpy(), w["dF_s"]) <= allow["grad"]          # (every row: the composite follows the same duplicate rule)
    # [B, C, 1, 1] maps; bfloat16 and float16 storage (evaluated in float64, returned in float32); other weights
    f = torch.randn(6, 10, 1, 1)
    t = torch.randn(6, 7, 1, 1)
    assert abs(float(crit(f, t)) - R.pair(f.numpy(), t.numpy())["loss"]) <= allow["loss"] * float(crit(f, t))
    assert crit(f.bfloat16(), t.bfloat16()).dtype == torch.float32 and crit(f.half(), t.half()).dtype == torch.float32
    want = R.pair(f.numpy(), t.numpy(), w_d=2.0, w_a=3.0)["loss"]
    assert abs(float(RKDLoss(2, 3)(f, t)) - want) <= allow["loss"] * want
    # a teacher that wants a gradient gets one
    tg = torch.randn(6, 7, requires_grad=True)
    crit(f, tg).backward()
    assert tg.grad is not None and bool(tg.grad.abs().sum() > 0)
    with pytest.raises(ValueError):
        crit(torch.randn(4, 3), torch.randn(5, 3))
    with pytest.raises(ValueError):
        crit(torch.randn(1, 3), torch.randn(1, 3))


def test_two_points_carry_no_relation():
    """B = 2: one distance (its normalised value is 1 on both sides) and no angle -- both terms vanish identically"""
    from moma_amd.distiller_zoo import RKDLoss
    cases, allow = rkd_fixture.load()
    c = cases[0]
    assert c["shape"][0] == 2
    w = R.pair(c["f_s"], c["f_t"])
    bound = allow["loss"] * (W_D + W_A)
    f_s = torch.from_numpy(c["f_s"]).requires_grad_(True)
    loss = RKDLoss()(f_s, torch.from_numpy(c["f_t"]))
    loss.backward()
    for v in (c["loss"], w["loss"], float(loss.detach())):
        assert np.isfinite(v) and abs(v) <= bound
    assert np.isfinite(c["dF_s"]).all() and np.isfinite(w["dF_s"]).all() and bool(torch.isfinite(f_s.grad).all())


def test_ops_rkd_loss_refuses_cpu_tensors():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    with pytest.raises(_lib.MomaHipError):
        ops.rkd_loss(torch.zeros(3, 4), torch.zeros(3, 4))


def test_workspace_query_and_argument_checks():
    """host arithmetic only: the workspace is (2 B^2 + 4 B + ceil(B / 16)^2) doubles; fewer than 2 or more than MOMA_RKD_MAX_B rows,
    an empty row, a null pointer, an unknown dtype, a misaligned buffer and a workspace that is too small are refused before
    anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.moma_rkd_workspace_bytes
    assert _lib.RKD_MAX_B == 1024
    assert f(2) == (8 + 8 + 1) * 8 and f(16) == (512 + 64 + 1) * 8 and f(17) == (578 + 68 + 4) * 8
    assert f(256) == (2 * 65536 + 1024 + 256) * 8 and f(1024) == (2 * 1024 * 1024 + 4096 + 4096) * 8
    assert f(1) == 0 and f(0) == 0 and f(-3) == 0 and f(1025) == 0
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    odd = lambda n: C.c_void_p(p.value + n)                                                           # noqa: E731
    f32, bf16, big = _lib.DT_F32, _lib.DT_BF16, 1 << 30
    dist = lambda B, D=8, dt=f32, ptr=p, S=p: lib.moma_rkd_dist(ptr, B, D, dt, S, None)               # noqa: E731
    bwd = lambda B, D=8, dt=f32, ptr=p, S=p: lib.moma_rkd_bwd(ptr, S, p, p, B, D, dt, None)           # noqa: E731
    terms = lambda B, ws=big, ptr=p, Q=p: lib.moma_rkd_terms(ptr, p, B, 25.0, 50.0, p, ws, Q, p, p, None)     # noqa: E731
    for call in (dist, bwd):
        assert call(4, ptr=None) == -1                                                                # MOMA_E_NULL
        assert call(0) == -2 and call(-1) == -2 and call(4, D=0) == -2                                # MOMA_E_SHAPE
        assert call(4, dt=7) == -3                                                                    # MOMA_E_DTYPE
        assert call(1) == -6 and call(1025) == -6                                                     # MOMA_E_UNSUPPORTED
        assert call(4, dt=bf16, ptr=odd(1)) == -4 and call(4, ptr=odd(2)) == -4 and call(4, S=odd(4)) == -4      # MOMA_E_ALIGN
    assert terms(4, ptr=None) == -1 and terms(0) == -2 and terms(1) == -6 and terms(1025) == -6
    assert terms(4, ws=f(4) - 1) == -5 and terms(4, Q=odd(4)) == -4


def _rkd_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "rkd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "1",
                        "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_with_distill_rkd():
    """(the parent commit has no RKDLoss criterion and its build_training raises NotImplementedError("rkd"))"""
    from moma_amd.distiller_zoo import RKDLoss
    _opt, built = _rkd_training(torch.device("cpu"))
    model_s, _model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    assert isinstance(criterion_list[2], RKDLoss) and contrast is None
    assert (criterion_list[2].w_d, criterion_list[2].w_a) == (25, 50)
    assert len(list(criterion_list[2].parameters())) == 0 and len(trainable_list) == 1 and len(module_list) == 2
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()}


def test_one_cpu_step_of_the_loop():
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _rkd_training(dev)
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
    # the KD term is the restatement's value on feat[-1] of the same (pre-step) models
    _opt2, built2 = _rkd_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    want = R.pair(fs[-1].numpy(), ft[-1].numpy())["loss"]
    assert abs(float(loss_kd) - want) <= 1e-5 * want

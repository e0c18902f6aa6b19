"""CPU checks of the `--distill nst` path: the numpy restatement of the Neuron Selectivity Transfer formulas (tests/nst_ref.py)
against the golden fixture recorded from the reference, the criterion's stock-torch composite on CPU tensors, the workspace query
and the argument checks of the C ABI, the construction of the training objects and one CPU step of the loop, and the refusal of
token lists.  (The C ABI's table-driven argument test in tests/test_abi_cpu.py picks the new entry points up by itself.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import nst_fixture, nst_ref as N
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 3, 5, 4, 4, 4, 4), (3, 24, 40, 7, 7, 7, 7), (2, 33, 65, 5, 3, 5, 3), (2, 112, 112, 14, 14, 14, 14),
         (2, 24, 24, 56, 56, 56, 56), (2, 64, 128, 8, 8, 8, 8), (2, 40, 40, 28, 28, 28, 28), (2, 200, 136, 4, 4, 4, 4),
         (2, 8, 12, 8, 8, 4, 4), (2, 8, 12, 7, 7, 4, 4)]


def _scale(w):
    """what a loss distance is relative to: t1 + 2 t2 (the loss is their difference and crosses zero)"""
    return w["t1"] + 2 * w["t2"]


def test_fixture_files_stay_below_the_size_limit():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "g13_nst*.npz"))
    assert files and all(os.path.getsize(f) < (1 << 20) for f in files)


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation); the all-zero row gets an exactly zero gradient"""
    cases, allow = nst_fixture.load()
    assert [c["shape"] for c in cases] == CASES
    assert allow["loss"] < 1e-6 and allow["grad"] < 1e-5 and allow["gram"] < 1e-5
    assert any(c["loss"] < 0 for c in cases) and any(c["loss"] > 0 for c in cases)
    for c in cases:
        w = N.pair(c["f_s"], c["f_t"])
        assert abs(c["loss"] - w["loss"]) <= c["ref_vs_f64_loss"] * _scale(w) * (1 + 1e-9)
        assert rel(c["dF_s"], w["dF_s"]) <= c["ref_vs_f64_grad"] * (1 + 1e-9)
        assert np.isfinite(c["dF_s"]).all() and np.isfinite(w["dF_s"]).all() and np.isfinite(w["G"]).all()
        assert not c["f_s"][0, 1].any() and not c["dF_s"][0, 1].any() and not w["dF_s"][0, 1].any()
        if c["shape"][3] == c["shape"][5]:
            assert w["norms"][0, 1] == N.EPS and not w["G"][0, 1].any() and not w["G"][0, :, 1].any()


def test_restatement_gradient_is_the_derivative_of_its_loss():
    """central differences of the float64 loss at a ragged shape, the clamped row left out"""
    rng = np.random.default_rng(3)
    f_s, f_t = rng.standard_normal((2, 3, 2, 3)), rng.standard_normal((2, 4, 2, 3))
    g = N.pair(f_s, f_t, g_loss=1.5)["dF_s"]
    num = np.zeros_like(f_s)
    for idx in np.ndindex(*f_s.shape):
        d = np.zeros_like(f_s)
        d[idx] = 1e-6
        num[idx] = 1.5 * (N.pair(f_s + d, f_t)["loss"] - N.pair(f_s - d, f_t)["loss"]) / 2e-6
    assert np.abs(num - g).max() < 1e-8


def test_composite_on_cpu_tensors_matches_the_fixture():
    from moma_amd.distiller_zoo import NSTLoss
    cases, allow = nst_fixture.load()
    crit = NSTLoss()
    for c in cases:
        f_s, f_t = torch.from_numpy(c["f_s"]).requires_grad_(True), torch.from_numpy(c["f_t"])
        (loss,) = crit([f_s], [f_t])
        loss.backward()
        w = N.pair(c["f_s"], c["f_t"])
        assert loss.dtype == torch.float32 and abs(loss.item() - w["loss"]) <= allow["loss"] * _scale(w)
        assert rel(f_s.grad.numpy(), w["dF_s"]) <= allow["grad"]
        assert abs(loss.item() - c["loss"]) <= (allow["loss"] + c["ref_vs_f64_loss"]) * _scale(w)
        assert not f_s.grad[0, 1].any()
    # float16 storage stays on the composite (evaluated in float64, returned in float32); the list form pairs up to the shorter list
    f = torch.randn(2, 4, 6, 6)
    assert len(crit([f, f], [f + 1])) == 1
    assert crit.nst_loss(f.half(), f.half()).dtype == torch.float32
    # a teacher that wants a gradient gets one
    t = torch.randn(2, 5, 6, 6, requires_grad=True)
    crit.nst_loss(f, t).backward()
    assert t.grad is not None and bool(t.grad.abs().sum() > 0)


def test_token_lists_are_refused():
    from moma_amd.distiller_zoo import NSTLoss
    tokens = [torch.randn(2, 17, 32), torch.randn(2, 17, 32)]
    with pytest.raises(ValueError, match="feature maps"):
        NSTLoss()(tokens, tokens)
    with pytest.raises(ValueError):
        NSTLoss().nst_loss(torch.randn(2, 8, 4, 4), torch.randn(2, 17, 32))


def test_ops_nst_loss_refuses_cpu_tensors():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    with pytest.raises(_lib.MomaHipError):
        ops.nst_loss(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4))


def test_workspace_query_and_argument_checks():
    """host arithmetic only: the workspace is the Gram, B Cs (Cs + Ct) 4 bytes; more than 256 channels on a side, an empty batch or
    map, a null pointer, an unknown layout or dtype and a workspace that is too small are refused before anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.moma_nst_workspace_bytes
    nchw, nhwc, f32, bf16 = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC, _lib.DT_F32, _lib.DT_BF16
    assert f(256, 112, 112) == 256 * 112 * 224 * 4 and f(2, 3, 5) == 2 * 3 * 8 * 4 and f(1, 256, 256) == 256 * 512 * 4
    assert f(2, 257, 8) == 0 and f(2, 8, 257) == 0 and f(0, 8, 8) == 0 and f(2, 0, 8) == 0
    assert _lib.NST_MAX_C == 256 and _lib.NST_ROW_BLOCK == 32
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30
    gram = lambda B, Cs, Ct, P, ds=f32, ls=nchw, dt=f32, lt=nchw, ws=big, ptr=p: lib.moma_nst_gram(    # noqa: E731
        ptr, p, B, Cs, Ct, P, ds, ls, dt, lt, p, ws, p, p, p, p, p, None)
    bwd = lambda B, Cs, Ct, P, ds=f32, ls=nchw, dt=f32, lt=nchw, ws=big, ptr=p: lib.moma_nst_bwd(     # noqa: E731
        ptr, p, p, ws, p, p, p, p, B, Cs, Ct, P, ds, ls, dt, lt, None)
    for call in (gram, bwd):
        assert call(2, 8, 8, 16, ptr=None) == -1                                                     # MOMA_E_NULL
        assert call(0, 8, 8, 16) == -2 and call(2, 8, 8, 0) == -2 and call(2, -1, 8, 16) == -2       # MOMA_E_SHAPE
        assert call(2, 8, 8, 16, ds=7) == -3 and call(2, 8, 8, 16, dt=2) == -3                       # MOMA_E_DTYPE
        assert call(2, 8, 8, 16, ws=2 * 8 * 16 * 4 - 1) == -5                                        # MOMA_E_WORKSPACE
        assert call(2, 257, 8, 16) == -6 and call(2, 8, 257, 16) == -6                               # MOMA_E_UNSUPPORTED
        assert call(2, 8, 8, 16, ls=2) == -6 and call(2, 8, 8, 16, lt=-1) == -6
        assert call(2, 8, 8, 16, ds=bf16, ls=nhwc, ptr=C.c_void_p(p.value + 1)) == -4                # MOMA_E_ALIGN


def _nst_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "nst", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "50",
                        "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_with_distill_nst_and_one_cpu_step():
    """(the parent commit has no NSTLoss criterion and its build_training raises NotImplementedError("nst"))"""
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.distiller_zoo import NSTLoss
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _nst_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    assert isinstance(criterion_list[2], NSTLoss) and contrast is None
    assert len(list(criterion_list[2].parameters())) == 0 and len(trainable_list) == 1 and len(module_list) == 2
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()}
    before = [p.detach().clone() for p in model_s.parameters()]
    teacher_before = [p.detach().clone() for p in model_t.parameters()]
    opt.trace, opt.print_freq = [], 1000
    loader = SyntheticLoader(1, 8, 32, 4, 3, dev)
    train_distill_moma(1, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    (loss, _idx, loss_kd), = opt.trace
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd))
    grads = [p.grad for p in model_s.parameters()]
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads) and any(g is not None and bool(g.abs().sum() > 0) for g in grads)
    assert any(not torch.equal(a, b) for a, b in zip(before, model_s.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
    # the KD term is the restatement's sum over feat[1:-2] of the same (pre-step) models
    opt2, built2 = _nst_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    pairs = [N.pair(a.numpy(), b.numpy()) for a, b in zip(fs[1:-2], ft[1:-2])]
    assert len(pairs) >= 2
    want, scale = sum(w["loss"] for w in pairs), sum(_scale(w) for w in pairs)
    assert abs(float(loss_kd) - want) <= 1e-5 * scale

"""CPU checks of the `--distill similarity` path: the numpy restatement of the Similarity-Preserving formulas (tests/sp_ref.py)
against the golden fixture recorded from the reference and against torch autograd in float64, the criterion's stock-torch composite
on CPU tensors (fp32 and bf16 storage, channels_last), who gets a gradient, the workspace query and the argument checks of the C ABI,
the construction of the training objects and one CPU step of the loop.  (The C ABI's table-driven argument test in
tests/test_abi_cpu.py picks the new entry points up by itself.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import golden_npz, sp_fixture, sp_ref as R
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref_grad_ok(c, got, bound):
    """the reference's recorded gradient (the long case: its stored columns) against `got` (full gradient, any shape), in units of
    got's largest element -- the generator's metric"""
    got = np.asarray(got, np.float64).reshape(c["shape"][0], -1)
    if "dF_s" in c:
        d = np.abs(c["dF_s"].reshape(got.shape) - got).max()
    else:
        d = np.abs(c["dF_s_cols"] - got[:, ::sp_fixture.LONG_STRIDE]).max()
    return d <= bound * np.abs(got).max()


def test_fixture_files_stay_below_the_size_limit():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "g15_sp*.npz"))
    assert files and all(os.path.getsize(f) < golden_npz.LIMIT for f in files)
    g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g15_sp.npz"))
    assert all(np.asarray(g[k]).nbytes < (600 << 10) for k in g.files)


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation)"""
    cases, allow = sp_fixture.load()
    assert len(cases) == len(sp_fixture.CASES)
    assert allow["loss"] < 1e-5 and allow["grad"] < 3e-5 and allow["G"] < 1e-5 and allow["H"] < 2e-6
    assert max(c["ref_vs_f64_G"] for c in cases) > 0                      # (the G allowance is not its floor)
    for c in cases:
        B = c["shape"][0]
        for f in (c["f_s"], c["f_t"]):                                    # exact in bfloat16: both storages hold these values
            assert np.array_equal(torch.from_numpy(f).bfloat16().float().numpy(), f)
        w = R.pair(c["f_s"], c["f_t"])
        assert np.isfinite(w["dF_s"]).all() and np.isfinite(w["M"]).all()
        scale = w["loss"] if B > 1 else 1.0
        assert abs(c["loss"] - w["loss"]) <= c["ref_vs_f64_loss"] * scale * (1 + 1e-9) + 1e-300
        assert _ref_grad_ok(c, w["dF_s"], c["ref_vs_f64_grad"] * (1 + 1e-9))
    one = R.pair(cases[0]["f_s"], cases[0]["f_t"])
    assert one["loss"] == 0 and not one["dF_s"].any() and abs(one["H_s"][0, 0]) == 1              # B = 1: H is +-1


def test_the_special_rows_of_the_fixture():
    cases, _allow = sp_fixture.load()
    notes = [c["note"] for c in cases]
    dup, zero, silu = cases[notes.index("dup")], cases[notes.index("zero")], cases[notes.index("silu")]
    a, b = sp_fixture.DUP
    assert np.array_equal(dup["f_s"][a], dup["f_s"][b]) and np.array_equal(dup["f_t"][a], dup["f_t"][b])
    assert not zero["f_s"][sp_fixture.ZERO_S].any() and not zero["f_t"][sp_fixture.ZERO_T].any()
    w = R.pair(zero["f_s"], zero["f_t"])
    assert w["n_s"][sp_fixture.ZERO_S] == 0 and not w["H_s"][sp_fixture.ZERO_S].any()
    # the clamp: Q_i = E_i / 1e-12 on the all-zero student row -- the reference's behaviour, kept
    assert np.abs(w["Q"][sp_fixture.ZERO_S]).max() > 1e9 and np.isfinite(w["dF_s"]).all()
    w = R.pair(silu["f_s"], silu["f_t"])
    assert (w["G_s"] > 0).all() and (w["G_t"] > 0).all() and w["loss"] < 0.05 * (w["H_s"] ** 2).mean()


def test_restatement_against_torch_autograd_in_float64():
    """the reference's formula written with stock ops in float64 and differentiated by autograd: loss and gradient agree with the
    restatement to rounding on every fixture case, the all-zero-row case and the long-K case included"""
    cases, _allow = sp_fixture.load()
    for c in cases:
        x = torch.from_numpy(c["f_s"]).double().requires_grad_(True)
        y = torch.from_numpy(c["f_t"]).double()
        B = x.shape[0]
        gs = torch.nn.functional.normalize(x.reshape(B, -1) @ x.reshape(B, -1).t(), dim=1)
        gt = torch.nn.functional.normalize(y.reshape(B, -1) @ y.reshape(B, -1).t(), dim=1)
        loss = (gt - gs).square().sum() / (B * B)
        (1.5 * loss).backward()
        w = R.pair(c["f_s"], c["f_t"], g_loss=1.5)
        assert abs(float(loss.detach()) - w["loss"]) <= 1e-14 * max(w["loss"], 1e-300) + 1e-300
        assert rel(x.grad.numpy(), w["dF_s"]) <= 1e-12 or not w["dF_s"].any()


def test_column_order_does_not_matter():
    """G is invariant under a permutation of the K columns: the restatement fed a map in channels_last storage order returns the
    same loss and the gradient in that order"""
    rng = np.random.default_rng(3)
    f_s, f_t = rng.standard_normal((5, 6, 3, 2)), rng.standard_normal((5, 4, 3, 2))
    a = R.pair(f_s, f_t)
    b = R.pair(np.ascontiguousarray(f_s.transpose(0, 2, 3, 1)), np.ascontiguousarray(f_t.transpose(0, 2, 3, 1)))
    assert abs(a["loss"] - b["loss"]) <= 1e-14 * a["loss"]
    assert rel(b["dF_s"].transpose(0, 3, 1, 2), a["dF_s"]) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_composite_on_cpu_tensors_matches_the_fixture(dtype):
    from moma_amd.distiller_zoo import Similarity
    cases, allow = sp_fixture.load()
    crit = Similarity()
    for c in cases:
        B = c["shape"][0]
        f_s, f_t = torch.from_numpy(c["f_s"]).to(dtype).requires_grad_(True), torch.from_numpy(c["f_t"]).to(dtype)
        out = crit([f_s], [f_t])
        assert isinstance(out, list) and len(out) == 1
        loss = out[0]
        loss.backward()
        w = R.pair(c["f_s"], c["f_t"])
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert abs(loss.item() - w["loss"]) <= allow["loss"] * (w["loss"] if B > 1 else 1.0)
        assert f_s.grad.dtype == dtype and f_s.grad.shape == f_s.shape
        if dtype == torch.float32:                                        # (a bf16 gradient carries bf16's own rounding)
            assert rel(f_s.grad.numpy(), w["dF_s"]) <= allow["grad"] or not w["dF_s"].any()
            assert abs(loss.item() - c["loss"]) <= (allow["loss"] + c["ref_vs_f64_loss"]) * (w["loss"] if B > 1 else 1.0)
            assert _ref_grad_ok(c, f_s.grad.numpy(), allow["grad"] + c["ref_vs_f64_grad"]) or not w["dF_s"].any()
        else:
            assert rel(f_s.grad.float().numpy(), w["dF_s"]) <= 2.0 ** -8 or not w["dF_s"].any()
    assert crit([torch.randn(4, 6).half()], [torch.randn(4, 3).half()])[0].dtype == torch.float32
    assert crit([torch.randn(4, 6).double()], [torch.randn(4, 3).double()])[0].dtype == torch.float64
    with pytest.raises(ValueError):
        crit([torch.randn(4, 3)], [torch.randn(5, 3)])


def test_channels_last_is_accepted_and_equals_the_contiguous_copy():
    """(the reference's `.view(bsz, -1)` raises on a channels_last map)"""
    from moma_amd.distiller_zoo import Similarity
    _cases, allow = sp_fixture.load()
    crit = Similarity()
    torch.manual_seed(2)
    f_s, f_t = torch.randn(6, 8, 3, 3), torch.randn(6, 5, 3, 3)
    cl_s, cl_t = f_s.contiguous(memory_format=torch.channels_last), f_t.contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        cl_s.view(6, -1)
    a, b = f_s.clone().requires_grad_(True), cl_s.clone(memory_format=torch.preserve_format).requires_grad_(True)
    la, lb = crit([a], [f_t])[0], crit([b], [cl_t])[0]
    la.backward()
    lb.backward()
    w = R.pair(f_s.numpy(), f_t.numpy())
    for loss, x in ((la, a), (lb, b)):
        assert abs(loss.item() - w["loss"]) <= allow["loss"] * w["loss"] and rel(x.grad.numpy(), w["dF_s"]) <= allow["grad"]
    assert abs(la.item() - lb.item()) <= allow["loss"] * w["loss"] and rel(b.grad.numpy(), a.grad.numpy()) <= allow["grad"]


def test_who_gets_a_gradient():
    """the kernel route gives f_t none and says so; the composite gives it one"""
    from moma_amd import _lib, build, ops
    from moma_amd.distiller_zoo import Similarity
    build.build(verbose=False)
    with pytest.raises(_lib.MomaHipError):
        ops.sp_loss(torch.zeros(3, 4), torch.zeros(3, 4))                 # CPU tensors: refused, no fallback inside ops
    f_s, f_t = torch.randn(5, 7, requires_grad=True), torch.randn(5, 4, requires_grad=True)
    Similarity()([f_s], [f_t])[0].backward()
    assert f_t.grad is not None and bool(f_t.grad.abs().sum() > 0) and bool(f_s.grad.abs().sum() > 0)
    # ops.sp_dense: what the kernels can read in storage order
    x = torch.randn(4, 6, 3, 3)
    assert ops.sp_dense(x) and ops.sp_dense(x.contiguous(memory_format=torch.channels_last)) and ops.sp_dense(x[:1].expand(1, 6, 3, 3))
    assert ops.sp_dense(torch.randn(4, 6, 1, 1)) and ops.sp_dense(torch.randn(4, 6))
    assert not ops.sp_dense(x[:, ::2]) and not ops.sp_dense(x[::2]) and not ops.sp_dense(torch.randn(6, 4).t()) and not ops.sp_dense(x[..., :2])


def test_workspace_query_and_argument_checks():
    """host arithmetic only: a side's workspace is splits(B, K) B^2 fp32, splits = min(ceil(K / 128), ceil(512 / pairs)), pairs the
    upper-triangle pairs of 64-row tiles; no rows, more than MOMA_SP_MAX_B rows, an empty row, a null pointer, an unknown dtype, a
    misaligned buffer and a workspace that is too small are refused before anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.moma_sp_workspace_bytes
    assert _lib.SP_MAX_B == 1024

    def splits(B, K):
        nt = -(-B // 64)
        return min(-(-K // 128), -(-512 // (nt * (nt + 1) // 2)))
    for B, K in ((1, 1), (1, 129), (64, 62720), (65, 62720), (256, 62720), (256, 125440), (1024, 8), (1024, 62720), (130, 87 * 128 - 5),
                 (3, 1 << 33)):
        assert f(B, K) == splits(B, K) * B * B * 4, (B, K)
    assert splits(64, 62720) == 490 and splits(256, 62720) == 52 and splits(1024, 62720) == 4 and splits(1024, 8) == 1
    assert f(0, 8) == 0 and f(-3, 8) == 0 and f(1025, 8) == 0 and f(4, 0) == 0 and f(4, -1) == 0
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    odd = lambda n: C.c_void_p(p.value + n)                                                           # noqa: E731
    f32, bf16, big = _lib.DT_F32, _lib.DT_BF16, 1 << 30
    gram = lambda B, K=8, dt=f32, ptr=p, ws=p, n=big: lib.moma_sp_gram(ptr, B, K, dt, ws, n, None)    # noqa: E731
    bwd = lambda B, K=8, dt=f32, ptr=p, M=p: lib.moma_sp_bwd(ptr, M, p, p, B, K, dt, None)            # noqa: E731
    terms = lambda B, Ks=8, Kt=8, ws=p, n=big, G=p: lib.moma_sp_terms(ws, n, Ks, p, big, Kt, B, G, p, p, p, p, None)   # noqa: E731
    for call in (gram, bwd):
        assert call(4, ptr=None) == -1                                                                # MOMA_E_NULL
        assert call(0) == -2 and call(-1) == -2 and call(4, K=0) == -2                                # MOMA_E_SHAPE
        assert call(4, dt=7) == -3                                                                    # MOMA_E_DTYPE
        assert call(1025) == -6                                                                       # MOMA_E_UNSUPPORTED
        assert call(4, dt=bf16, ptr=odd(1)) == -4 and call(4, ptr=odd(2)) == -4                       # MOMA_E_ALIGN
    assert gram(4, n=f(4, 8) - 1) == -5 and gram(4, ws=odd(2)) == -4 and bwd(4, M=odd(4)) == -4
    assert terms(4, ws=None) == -1 and terms(0) == -2 and terms(4, Kt=0) == -2 and terms(1025) == -6
    assert terms(4, n=f(4, 8) - 1) == -5 and terms(4, G=odd(4)) == -4


def _sp_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "similarity", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "1",
                        "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_with_distill_similarity():
    """(the parent commit has no Similarity criterion and its build_training raises NotImplementedError("similarity"))"""
    from moma_amd.distiller_zoo import Similarity
    _opt, built = _sp_training(torch.device("cpu"))
    model_s, _model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    assert isinstance(criterion_list[2], Similarity) and contrast is None
    assert len(list(criterion_list[2].parameters())) == 0 and len(trainable_list) == 1 and len(module_list) == 2
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()}


def test_one_cpu_step_of_the_loop():
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _sp_training(dev)
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
    # the KD term is the restatement's value on feat[-2] of the same (pre-step) models
    _opt2, built2 = _sp_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    want = R.pair(fs[-2].numpy(), ft[-2].numpy())["loss"]
    assert abs(float(loss_kd) - want) <= 1e-5 * want

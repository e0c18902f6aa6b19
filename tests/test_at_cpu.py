"""CPU checks of the `--distill attention` path: the numpy restatement of the Attention Transfer formulas (tests/at_ref.py) against
the golden fixture recorded from the reference, the criterion's stock-torch composite on CPU tensors, the construction of the
training objects and one CPU step of the loop, and the refusal of token lists.  (The C ABI's table-driven argument test in
tests/test_abi_cpu.py picks the new entry points up by itself.)"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import at_fixture, at_ref as A
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 3, 5, 7, 7), (3, 16, 64, 8, 4), (2, 8, 8, 16, 4), (2, 3, 5, 7, 4), (4, 64, 256, 4, 4), (4, 64, 256, 32, 32),
         (2, 24, 40, 56, 56), (2, 1280, 1280, 7, 7)]


def test_fixture_files_stay_below_the_size_limit():
    files = glob.glob(os.path.join(ROOT, "tests", "golden", "g12_at*.npz"))
    assert files and all(os.path.getsize(f) < (1 << 20) for f in files)


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation); the all-zero image gets an exactly zero gradient"""
    cases, allow = at_fixture.load()
    assert [c["shape"] for c in cases] == CASES
    assert allow["loss"] < 1e-6 and allow["grad"] < 1e-5 and allow["map"] < 1e-6
    for c in cases:
        w = A.pair(c["f_s"], c["f_t"])
        assert abs(c["loss"] - w["loss"]) <= c["ref_vs_f64_loss"] * abs(w["loss"]) * (1 + 1e-9)
        assert rel(c["dF_s"], w["dF_s"]) <= c["ref_vs_f64_grad"] * (1 + 1e-9)
        assert np.isfinite(c["dF_s"]).all() and np.isfinite(w["dF_s"]).all() and np.isfinite(w["dF_t"]).all()
        if c["shape"][0] > 1:
            assert not c["f_s"][0].any() and not c["dF_s"][0].any() and not w["dF_s"][0].any()
            assert not w["ah_s"][0].any() and np.isfinite(w["g_s"]).all()


def test_restatement_pooling_matches_adaptive_avg_pool2d():
    rng = np.random.default_rng(0)
    for (H, W, oh, ow) in [(7, 7, 4, 4), (8, 8, 4, 4), (16, 12, 4, 4), (5, 9, 3, 3), (4, 4, 4, 4)]:
        f = rng.standard_normal((2, 3, H, W))
        want = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(f), (oh, ow)).numpy()
        assert np.abs(A.pool(f, oh, ow) - want).max() < 1e-14
        g = rng.standard_normal((2, 3, oh, ow))
        t = torch.from_numpy(f).requires_grad_(True)
        (torch.nn.functional.adaptive_avg_pool2d(t, (oh, ow)) * torch.from_numpy(g)).sum().backward()
        assert np.abs(A.pool_bwd(g, H, W) - t.grad.numpy()).max() < 1e-14


def test_composite_on_cpu_tensors_matches_the_fixture():
    from moma_amd.distiller_zoo import Attention
    cases, allow = at_fixture.load()
    crit = Attention()
    for c in cases:
        f_s, f_t = torch.from_numpy(c["f_s"]).requires_grad_(True), torch.from_numpy(c["f_t"])
        (loss,) = crit([f_s], [f_t])
        loss.backward()
        w = A.pair(c["f_s"], c["f_t"])
        assert loss.dtype == torch.float32 and abs(loss.item() - w["loss"]) <= allow["loss"] * abs(w["loss"])
        assert rel(f_s.grad.numpy(), w["dF_s"]) <= allow["grad"]
        assert abs(loss.item() - c["loss"]) <= 2 * allow["loss"] * abs(c["loss"])
    # other exponents and float16 storage stay on the composite; the list form pairs up to the shorter list
    f = torch.randn(2, 4, 6, 6)
    assert len(Attention(p=1)([f, f], [f + 1])) == 1
    assert float(Attention(p=4).at_loss(f, f)) == 0.0
    assert Attention().at_loss(f.half(), f.half()).dtype == torch.float32


def test_token_lists_are_refused():
    from moma_amd.distiller_zoo import Attention
    tokens = [torch.randn(2, 17, 32), torch.randn(2, 17, 32)]
    with pytest.raises(ValueError, match="feature maps"):
        Attention()(tokens, tokens)
    with pytest.raises(ValueError):
        Attention().at_loss(torch.randn(2, 8, 4, 4), torch.randn(2, 17, 32))


def test_ops_attention_loss_refuses_cpu_tensors():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    with pytest.raises(_lib.MomaHipError):
        ops.attention_loss(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4))


def test_workspace_query_and_argument_checks():
    """host arithmetic only: no workspace where (b, pixel tiles) fill the chip or the layout is channels_last, one partial map per
    channel split for small NCHW maps; a grid that does not divide the map, an unknown layout and an unknown dtype are refused"""
    import ctypes as C
    from moma_amd import _lib
    lib = _lib.load()
    f = lib.moma_at_workspace_bytes
    nchw, nhwc, f32, bf16 = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC, _lib.DT_F32, _lib.DT_BF16
    assert f(256, 24, 56, 56, 56, 56, f32, nchw) == 0 and f(64, 1280, 7, 7, 7, 7, bf16, nhwc) == 0
    n = f(64, 1280, 7, 7, 7, 7, f32, nchw)
    assert n > 0 and n % (64 * 49 * 4) == 0 and n // (64 * 49 * 4) <= 64
    assert f(64, 1280, 7, 7, 7, 7, bf16, nchw) == n                    # decided on the shape alone
    assert f(2, 3, 7, 7, 4, 4, f32, nchw) == 0 and f(2, 3, 7, 7, 7, 7, 5, nchw) == 0 and f(2, 3, 7, 7, 7, 7, f32, 2) == 0
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    assert lib.moma_at_map(p, p, 2, 3, 7, 7, 4, 4, f32, nchw, p, 4096, None) == -2                  # MOMA_E_SHAPE
    assert lib.moma_at_map(p, p, 2, 3, 8, 8, 4, 4, f32, 7, p, 4096, None) == -6                     # MOMA_E_UNSUPPORTED
    assert lib.moma_at_map(p, p, 2, 3, 8, 8, 4, 4, 9, nchw, p, 4096, None) == -3                    # MOMA_E_DTYPE
    assert lib.moma_at_map(p, p, 64, 1280, 7, 7, 7, 7, f32, nchw, p, 16, None) == -5                # MOMA_E_WORKSPACE
    assert lib.moma_at_bwd(p, p, p, p, 2, 3, 7, 7, 3, 3, bf16, nhwc, None) == -2
    assert lib.moma_at_pair(p, p, 0, 5, p, p, p, p, None, None, None, None) == -2


def _attention_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "attention", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "1000",
                        "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_with_distill_attention_and_one_cpu_step():
    """(the parent commit has no Attention criterion and its build_training raises NotImplementedError("attention"))"""
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.distiller_zoo import Attention
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _attention_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    assert isinstance(criterion_list[2], Attention) and criterion_list[2].p == 2 and contrast is None
    assert len(list(criterion_list[2].parameters())) == 0 and len(trainable_list) == 1 and len(module_list) == 2
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()}
    before = [p.detach().clone() for p in model_s.parameters()]
    teacher_before = [p.detach().clone() for p in model_t.parameters()]
    opt.trace, opt.print_freq = [], 1000
    loader = SyntheticLoader(1, 8, 32, 4, 3, dev)
    train_distill_moma(1, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    (loss, _idx, loss_kd), = opt.trace
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd)) and float(loss_kd) > 0
    grads = [p.grad for p in model_s.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.abs().sum() > 0) for g in grads)
    assert any(not torch.equal(a, b) for a, b in zip(before, model_s.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
    # the KD term is the restatement's sum over feat[1:-1] of the same (pre-step) models
    opt2, built2 = _attention_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    want = A.loss_of([f.numpy() for f in fs[1:-1]], [f.numpy() for f in ft[1:-1]])
    assert abs(float(loss_kd) - want) <= 1e-5 * want

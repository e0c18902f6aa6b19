"""CPU checks of the `--distill vid` path: the numpy restatement of Variational Information Distillation (tests/vid_ref.py) against
the golden fixture recorded from the reference, the criterion's stock-torch composite on CPU tensors, its parameter names and
initial state, the workspace query and the argument checks of the C ABI, the construction of the training objects (the criterion's
parameters reach the optimizer), one CPU step of the loop, a checkpoint round trip through `--resume`, and the gradient
synchronisation of the criterion's parameters.  (The C ABI's table-driven argument test in tests/test_abi_cpu.py picks the new entry
points up by itself.)"""
import os

import numpy as np
import pytest
import torch

from moma_amd.distiller_zoo import VIDLoss  # noqa: F401  (the criterion under test: without it nothing here has a subject)
from tests import vid_fixture, vid_ref as V
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 1, 1, 1, 1), (2, 3, 5, 4, 4), (3, 8, 8, 7, 7), (2, 5, 4, 3, 5), (2, 16, 24, 9, 9), (4, 24, 24, 16, 16), (2, 40, 40, 8, 8),
         (2, 12, 12, 4, 4), (65, 3, 2, 2, 2), (2, 130, 257, 6, 6), (4, 64, 1280, 4, 4)]


def test_fixture_files_stay_below_the_size_limit():
    files = vid_fixture.files()
    assert files and all(os.path.getsize(f) < (1 << 20) for f in files)


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded, and those
    are fp32 rounding noise (so the formulas ARE the reference's computation)"""
    cases, allow = vid_fixture.load()
    assert [c["shape"] for c in cases] == CASES
    assert all(c["ref_vs_f64_" + k] < 2e-6 for c in cases for k in vid_fixture.KINDS)
    assert all(-3 <= c["log_scale"].min() and c["log_scale"].max() <= 8 for c in cases)
    assert cases[6]["x"].shape[2:] == (16, 16) and cases[7]["target"].shape[2:] == (8, 8)          # the two pooled cases
    assert cases[10]["x"].min() == 0 and cases[10]["target"].min() == 0 and cases[4]["target"].mean() > 2.5
    up = 1 + 1e-9
    for c in cases:
        w = V.criterion(c["x"], c["target"], c["w"], c["log_scale"], c["eps"])
        assert abs(c["loss"] - w["loss"]) <= c["ref_vs_f64_chain_loss"] * w["abs_terms"] * up
        assert rel(c["dx"], w["dx"]) <= c["ref_vs_f64_dx"] * up
        assert max(rel(a, b) for a, b in zip(c["dw"], w["dw"])) <= c["ref_vs_f64_dw"] * up
        assert rel(c["pred_mean"], w["pred_mean"]) < 1e-5
        a = V.nll(c["pred_mean"], w["target"], c["log_scale"], c["eps"])                          # from the reference's own pred_mean
        assert abs(c["loss"] - a["loss"]) <= c["ref_vs_f64_loss"] * a["abs_terms"] * up
        assert rel(c["d_pred_mean"], a["d_mean"]) <= c["ref_vs_f64_dmean"] * up
        assert rel(c["d_log_scale"], a["d_ls"]) <= c["ref_vs_f64_dls"] * up


@pytest.mark.parametrize("ci", [0, 1])
def test_restatement_gradient_is_the_derivative_of_its_loss(ci):
    """central differences of the float64 loss on the two smallest cases: the input, every weight, log_scale, and -- for the
    likelihood alone -- the mean; with an upstream gradient of 1.5"""
    c = vid_fixture.load()[0][ci]
    x, t, ws, ls = c["x"].astype(np.float64), c["target"], [w.astype(np.float64) for w in c["w"]], c["log_scale"].astype(np.float64)
    g = V.criterion(x, t, ws, ls, c["eps"], g_loss=1.5)
    h = 1e-6

    def num(arr, f):
        out = np.zeros_like(arr)
        for idx in np.ndindex(*arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            hi = f()
            arr[idx] = keep - h
            lo = f()
            arr[idx] = keep
            out[idx] = 1.5 * (hi - lo) / (2 * h)
        return out

    loss = lambda: V.criterion(x, t, ws, ls, c["eps"])["loss"]          # noqa: E731
    assert np.abs(num(x, loss) - g["dx"]).max() < 1e-8
    for i in range(3):
        assert np.abs(num(ws[i], loss) - g["dw"][i]).max() < 1e-8
    assert np.abs(num(ls, loss) - g["d_ls"]).max() < 1e-8
    pm = g["pred_mean"].copy()
    assert np.abs(num(pm, lambda: V.nll(pm, t, ls, c["eps"])["loss"]) - g["d_mean"]).max() < 1e-8


def _criterion_of(c, dtype=torch.float32):
    """the project's VIDLoss carrying the case's weights and log_scale"""
    from moma_amd.distiller_zoo import VIDLoss
    B, Cs, Ct, H, W = c["shape"]
    crit = VIDLoss(Cs, c["mid"], Ct)
    with torch.no_grad():
        for i, w in zip((0, 2, 4), c["w"]):
            crit.regressor[i].weight.copy_(torch.from_numpy(w).view_as(crit.regressor[i].weight))
        crit.log_scale.copy_(torch.from_numpy(c["log_scale"]))
    return crit.to(dtype)


def test_composite_on_cpu_tensors_matches_the_fixture():
    """CPU tensors take the composite: the loss and every gradient -- input, weights, log_scale -- within the allowances of the
    float64 restatement and of the reference's own fp32 results"""
    cases, allow = vid_fixture.load()
    for c in cases:
        crit = _criterion_of(c)
        x, t = torch.from_numpy(c["x"]).requires_grad_(True), torch.from_numpy(c["target"])
        loss = crit(x, t)
        loss.backward()
        w = V.criterion(c["x"], c["target"], c["w"], c["log_scale"], c["eps"])
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert abs(loss.item() - w["loss"]) <= allow["chain_loss"] * w["abs_terms"]
        assert abs(loss.item() - c["loss"]) <= (allow["chain_loss"] + c["ref_vs_f64_chain_loss"]) * w["abs_terms"]
        assert rel(x.grad.numpy(), w["dx"]) <= allow["dx"]
        for i, k in enumerate((0, 2, 4)):
            assert rel(crit.regressor[k].weight.grad.numpy().reshape(w["dw"][i].shape), w["dw"][i]) <= allow["dw"]
        assert rel(crit.log_scale.grad.numpy(), w["d_ls"]) <= allow["dls"]
    # float16 storage stays on the composite (evaluated in float64, returned in float32); float64 comes back as float64
    crit = _criterion_of(cases[1])
    pm, t = torch.randn(2, 5, 4, 4), torch.randn(2, 5, 4, 4)
    assert crit.composite(pm.half(), t.half()).dtype == torch.float32 and crit.composite(pm.double(), t.double()).dtype == torch.float64
    # a target that wants a gradient gets one
    tg = torch.randn(2, 5, 4, 4, requires_grad=True)
    crit(torch.randn(2, 3, 4, 4), tg).backward()
    assert tg.grad is not None and bool(tg.grad.abs().sum() > 0)
    # log_scale far beyond the reference's fp32 overflow stays finite
    with torch.no_grad():
        crit.log_scale.fill_(100.0)
    assert bool(torch.isfinite(crit(torch.randn(2, 3, 4, 4), t)))


def test_parameter_names_and_initial_state_are_the_reference_s():
    from moma_amd.backbones.efficientnet import SamePadConv2d
    from moma_amd.distiller_zoo import VIDLoss
    torch.manual_seed(1701)
    crit = VIDLoss(3, 5, 5)
    assert list(crit.state_dict()) == ["log_scale", "regressor.0.weight", "regressor.2.weight", "regressor.4.weight"]
    assert [n for n, _ in crit.named_parameters()] == ["log_scale", "regressor.0.weight", "regressor.2.weight", "regressor.4.weight"]
    assert all(isinstance(crit.regressor[i], SamePadConv2d) and crit.regressor[i].bias is None for i in (0, 2, 4))
    assert all(isinstance(crit.regressor[i], torch.nn.ReLU) for i in (1, 3))
    # the construction order, so the RNG draws: the weights are the ones the reference drew under the same seed (fixture case 1)
    c = vid_fixture.load()[0][1]
    for i, w in zip((0, 2, 4), c["w"]):
        assert np.array_equal(crit.regressor[i].weight.detach().numpy().reshape(w.shape), w)
    assert np.array_equal(crit.log_scale.detach().numpy(), c["log_scale"]) and crit.log_scale.dtype == torch.float32
    assert abs(crit.log_scale[0].item() - np.log(np.exp(5.0 - 1e-5) - 1.0)) < 1e-6 and crit.eps == 1e-5
    other = VIDLoss(4, 6, 7, init_pred_var=2.0, eps=1e-3)
    assert other.log_scale.shape == (7,) and abs(other.log_scale[0].item() - np.log(np.exp(2.0 - 1e-3) - 1.0)) < 1e-6
    assert other.regressor[0].weight.shape == (6, 4, 1, 1) and other.regressor[4].weight.shape == (7, 6, 1, 1)


def test_token_lists_are_refused():
    from moma_amd.distiller_zoo import VIDLoss
    crit = VIDLoss(32, 32, 32)
    with pytest.raises(ValueError, match=r"feature maps.*\(2, 17, 32\)"):
        crit(torch.randn(2, 17, 32), torch.randn(2, 17, 32))
    with pytest.raises(ValueError):
        crit(torch.randn(2, 32, 4, 4), torch.randn(2, 17, 32))


def test_ops_vid_nll_refuses_cpu_tensors():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    with pytest.raises(_lib.MomaHipError):
        ops.vid_nll(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4), torch.zeros(3))


def test_workspace_query_and_argument_checks():
    """host arithmetic only: the workspace is one double per image, chunk of MOMA_VID_CHUNK pixels and channel; an empty batch or
    map, a null pointer, an unknown layout or dtype, a misaligned pointer and a workspace that is too small are refused before
    anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.moma_vid_workspace_bytes
    nchw, nhwc, f32, bf16 = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC, _lib.DT_F32, _lib.DT_BF16
    K = _lib.VID_CHUNK
    assert K >= 64 and K % 8 == 0
    assert f(64, 24, 128 * 128, bf16, nchw, bf16, nchw) == 64 * -(-128 * 128 // K) * 24 * 8
    assert f(64, 1280, 256, f32, nhwc, bf16, nchw) == 64 * -(-256 // K) * 1280 * 8
    assert f(1, 1, 1, f32, nchw, f32, nchw) == 8 and f(3, 5, K, f32, nchw, f32, nchw) == 3 * 5 * 8
    assert f(3, 5, K + 1, f32, nchw, f32, nchw) == 3 * 2 * 5 * 8
    assert f(0, 8, 8, f32, nchw, f32, nchw) == 0 and f(2, 0, 8, f32, nchw, f32, nchw) == 0 and f(2, 8, -1, f32, nchw, f32, nchw) == 0
    assert f(2, 8, 8, 5, nchw, f32, nchw) == 0 and f(2, 8, 8, f32, nchw, f32, 2) == 0
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30
    nll = lambda B, Cc, P, dm=f32, lm=nchw, dt=f32, lt=nchw, ws=big, ptr=p: lib.moma_vid_nll(    # noqa: E731
        ptr, p, p, 1e-5, B, Cc, P, dm, lm, dt, lt, p, ws, p, p, p, p, None)
    bwd = lambda B, Cc, P, dm=f32, lm=nchw, dt=f32, lt=nchw, ws=big, ptr=p: lib.moma_vid_bwd(    # noqa: E731
        ptr, p, p, p, p, B, Cc, P, dm, lm, dt, lt, None)
    for call in (nll, bwd):
        assert call(2, 8, 16, ptr=None) == -1                                                    # MOMA_E_NULL
        assert call(0, 8, 16) == -2 and call(2, 8, 0) == -2 and call(2, -1, 16) == -2            # MOMA_E_SHAPE
        assert call(2, 8, 16, dm=7) == -6 and call(2, 8, 16, dt=2) == -6                         # MOMA_E_UNSUPPORTED
        assert call(2, 8, 16, lm=2) == -6 and call(2, 8, 16, lt=-1) == -6
        assert call(2, 8, 16, dm=bf16, lm=nhwc, ptr=C.c_void_p(p.value + 1)) == -4               # MOMA_E_ALIGN
    assert nll(2, 8, 16, ws=2 * 8 * 8 - 1) == -5                                                 # MOMA_E_WORKSPACE
    assert lib.moma_version() == 4


def _vid_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "vid", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
                        "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "1",
                        "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_puts_the_criterion_in_the_optimizer():
    """(the parent commit's build_training raises NotImplementedError("vid"))"""
    from moma_amd.distiller_zoo import VIDLoss
    dev = torch.device("cpu")
    opt, built = _vid_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    kd = criterion_list[2]
    assert isinstance(kd, torch.nn.ModuleList) and len(kd) >= 2 and all(isinstance(c, VIDLoss) for c in kd) and contrast is None
    with torch.no_grad():
        probe = torch.randn(2, 3, 32, 32)
        fs, ft = model_s(probe, is_feat=True)[0][1:-1], model_t(probe, is_feat=True)[0][1:-1]
    assert len(kd) == len(fs) == len(ft)
    for c, a, b in zip(kd, fs, ft):                         # VIDLoss(s, t, t)
        assert c.regressor[0].weight.shape == (b.shape[1], a.shape[1], 1, 1) and c.regressor[2].weight.shape == (b.shape[1], b.shape[1], 1, 1)
        assert c.regressor[4].weight.shape == (b.shape[1], b.shape[1], 1, 1) and c.log_scale.shape == (b.shape[1],)
    assert any(m is kd for m in trainable_list) and len(module_list) == 2 and module_list[-1] is model_t
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()} | {id(p) for p in kd.parameters()}
    assert len(list(kd.parameters())) == 4 * len(kd) and all(p.requires_grad for p in kd.parameters())
    assert not any(id(p) in opt_params for p in model_t.parameters())


def test_one_cpu_step_of_the_loop_trains_the_criterion():
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _vid_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    kd = criterion_list[2]
    before = {n: p.detach().clone() for n, p in kd.named_parameters()}
    student_before = [p.detach().clone() for p in model_s.parameters()]
    teacher_before = [p.detach().clone() for p in model_t.parameters()]
    opt.trace, opt.print_freq = [], 1000
    loader = SyntheticLoader(1, 8, 32, 4, 3, dev)
    train_distill_moma(1, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    (loss, _idx, loss_kd), = opt.trace
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd)) and loss_kd.dtype == torch.float32
    after = dict(kd.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in after.values())
    for i in range(len(kd)):
        assert not torch.equal(before[f"{i}.log_scale"], after[f"{i}.log_scale"])
        assert not torch.equal(before[f"{i}.regressor.0.weight"], after[f"{i}.regressor.0.weight"])
        assert not torch.equal(before[f"{i}.regressor.4.weight"], after[f"{i}.regressor.4.weight"])
    assert any(not torch.equal(a, b) for a, b in zip(student_before, model_s.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
    # the KD term is the restatement's sum over feat[1:-1] of the same (pre-step) models and criteria
    opt2, built2 = _vid_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    want = [V.criterion(a.numpy(), b.numpy(), [c.regressor[i].weight.detach().numpy() for i in (0, 2, 4)], c.log_scale.detach().numpy(), c.eps)
            for a, b, c in zip(fs[1:-1], ft[1:-1], built2[3][2])]
    assert len(want) >= 2
    assert abs(float(loss_kd) - sum(w["loss"] for w in want)) <= 1e-5 * sum(w["abs_terms"] for w in want)


def test_checkpoint_round_trip_through_resume(tmp_path, monkeypatch):
    """one epoch of the CLI's worker on the CPU writes ckpt_last.pth; a second run with --resume hands the loop a criterion whose
    log_scale and regressors are the checkpoint's (not a fresh initialisation), and an optimizer that carries their momentum"""
    from moma_amd import train_student_moma as T
    monkeypatch.setattr(T, "_REQUIRE_GPU", False)
    argv = ["--distill", "vid", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
            "--batch_size", "8", "--steps_per_epoch", "2", "-c", "1", "-d", "1", "-b", "1", "--learning_rate", "0.05", "--seed", "7",
            "--print_freq", "1000", "--save_root", str(tmp_path)]

    def worker(extra):
        opt = T.parse_option(argv + extra)
        opt.world_size, opt.ngpus_per_node = 1, 1
        T.main_worker(0, 1, opt)
        return opt

    opt = worker(["--epochs", "1"])
    path = os.path.join(opt.save_folder, "ckpt_last.pth")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    keys = list(ck["criterion_kd"])
    assert "0.log_scale" in keys and "0.regressor.0.weight" in keys and "1.regressor.4.weight" in keys
    opt0 = T.parse_option(argv)
    opt0.gpu, opt0.multiprocessing_distributed = 0, False
    torch.manual_seed(7)
    fresh = T.build_training(opt0, torch.device("cpu"))[3][2].state_dict()
    assert not torch.equal(fresh["0.log_scale"], ck["criterion_kd"]["0.log_scale"])              # the epoch trained them
    assert not torch.equal(fresh["0.regressor.0.weight"], ck["criterion_kd"]["0.regressor.0.weight"])
    seen = {}

    def stub(epoch, loader, module_list, criterion_list, trainer, contrast, optimizer, o):
        seen["epoch"] = epoch
        seen["state"] = {k: v.detach().clone() for k, v in criterion_list[2].state_dict().items()}
        ids = {id(p) for g in optimizer.param_groups for p in g["params"]}
        seen["in_optimizer"] = all(id(p) in ids for p in criterion_list[2].parameters())
        seen["momentum"] = sum(1 for p in criterion_list[2].parameters() if "momentum_buffer" in optimizer.state.get(p, {}))
        return 0.0, 0.0

    monkeypatch.setattr(T, "train_distill_moma", stub)
    worker(["--epochs", "2", "--resume", path])
    assert seen["epoch"] == 2 and seen["in_optimizer"] and seen["momentum"] == len(keys)
    assert list(seen["state"]) == keys and all(torch.equal(seen["state"][k], ck["criterion_kd"][k]) for k in keys)


def test_gradient_sync_receives_exactly_the_criterion_s_parameters():
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma

    class Trainer:
        grad_sync_single_rank = True

        def __init__(self):
            self.attached, self.finished = [], 0

        def attach_grad_sync(self, params):
            self.attached.append(list(params))

        def finish_grad_sync(self):
            self.finished += 1

    dev = torch.device("cpu")
    opt, built = _vid_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    opt.trace, opt.print_freq = [], 1000
    trainer = Trainer()
    train_distill_moma(1, SyntheticLoader(1, 8, 32, 4, 3, dev), module_list, criterion_list, trainer, contrast, optimizer, opt)
    assert len(trainer.attached) == 1 and trainer.finished == 1
    assert [id(p) for p in trainer.attached[0]] == [id(p) for p in criterion_list[2].parameters()]

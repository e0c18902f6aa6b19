"""CPU checks of the `--distill hint` path: the numpy restatement of the FitNets hint (tests/hint_ref.py) against torch autograd over
the published modules in float64 and against the golden fixture recorded from the reference, the regressor's stock-torch composite on
CPU tensors, its state-dict keys and the order of its RNG draws, the analytic zero of the convolution's bias gradient, the argument
checks of the C ABI, the construction of the training objects (the regressor rides in module_list[1] and reaches the optimizer), one
CPU step of the loop, a checkpoint that resumes to the same next loss, and the gradient synchronisation of the regressor's
parameters.  (The C ABI's table-driven argument test in tests/test_abi_cpu.py picks the new entry points up by itself.)"""
import os

import numpy as np
import pytest
import torch

from moma_amd.distiller_zoo import ConvReg, HintLoss  # noqa: F401  (the modules under test: without them nothing here has a subject)
from tests import hint_fixture, hint_ref as V
from tests.crd_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((2, 1, 1, 1), (2, 1, 1, 1)), ((2, 4, 4, 4), (2, 3, 4, 4)), ((3, 6, 7, 7), (3, 8, 7, 7)), ((2, 3, 3, 5), (2, 5, 3, 5)),
          ((2, 8, 9, 9), (2, 16, 9, 9)), ((1, 5, 33, 33), (1, 4, 33, 33)), ((65, 2, 2, 2), (65, 3, 2, 2)), ((2, 7, 6, 6), (2, 130, 6, 6)),
          ((4, 16, 2, 2), (4, 1280, 2, 2)), ((2, 3, 8, 8), (2, 4, 4, 4)), ((2, 3, 4, 4), (2, 4, 8, 8)), ((2, 3, 7, 7), (2, 4, 5, 5)),
          ((2, 3, 5, 5), (2, 4, 8, 8))]
POINTWISE = [0, 1, 2, 3, 4, 5, 6, 7]           # the cases whose whole chain the restatement covers (1 x 1 branch, convolution run)
KEYS = ["conv.weight", "conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]


def _regressor_of(c, dtype=torch.float32):
    """the project's ConvReg carrying the case's weights"""
    reg = ConvReg(c["s_shape"], c["t_shape"])
    with torch.no_grad():
        reg.conv.weight.copy_(torch.from_numpy(c["w"]))
        reg.conv.bias.copy_(torch.from_numpy(c["b"]))
        reg.bn.weight.copy_(torch.from_numpy(c["gamma"]))
        reg.bn.bias.copy_(torch.from_numpy(c["beta"]))
    return reg.to(dtype).train()


def test_fixture_files_stay_below_the_size_limit():
    files = hint_fixture.files()
    assert files and all(os.path.getsize(f) < (1 << 20) for f in files)


def test_fixture_is_what_the_issue_lists_and_clear_of_the_kink():
    cases, allow = hint_fixture.load()
    assert len(cases) == hint_fixture.N_CASES and [(c["s_shape"], c["t_shape"]) for c in cases] == SHAPES
    assert [c["tail_only"] for c in cases] == [i == 8 for i in range(13)]
    for c in cases:
        assert c["conv_out"].shape == c["t_grid"].shape and c["t_grid"].shape[:2] == c["t_shape"][:2]
        assert (c["gamma"] < 0).any() or len(c["gamma"]) == 1
        assert np.abs(c["t"]).max() <= 7 and np.array_equal(c["t"] * 32, np.round(c["t"] * 32))
        # every element of what the kernels are handed is clear of the kink (half of tau: the convolution ran in fp32)
        assert not (np.abs(V.pre_activation(c["conv_out"], c["gamma"], c["beta"], c["eps"])) < V.TAU / 2).any()
    assert cases[4]["t"].mean() > 2.5 and cases[8]["t"].min() == 0 and cases[12]["t_grid"].shape[2:] == (5, 5)
    # fp32 rounding noise everywhere but the M = 2 case, whose dx is the difference of two nearly equal numbers
    assert all(c["ref_vs_f64_" + k] < 2e-6 for c in cases[1:] for k in hint_fixture.TAIL_KINDS + hint_fixture.CHAIN_KINDS
               if "ref_vs_f64_" + k in c)
    assert all(allow[k] >= hint_fixture.ULP32 for k in allow)


def test_clear_of_kink_moves_exactly_the_near_elements():
    rng = np.random.default_rng(3)
    x = np.round(rng.standard_normal((2, 3, 4, 4)) * 32) / 32
    gamma, beta = np.array([1.0, -0.5, 0.0]), np.array([0.25, 0.1, 0.0])
    mean, _var, invstd = V.bn_stats(x, 1e-5)
    x[1, 0, 2, 2] = mean[0] - 0.25 / invstd[0]                       # pre-activation ~ 0 (the statistics move a little with it)
    for _ in range(20):
        mean, _var, invstd = V.bn_stats(x, 1e-5)
        x[1, 0, 2, 2] = mean[0] - 0.25 / invstd[0]
    assert abs(V.pre_activation(x, gamma, beta, 1e-5)[1, 0, 2, 2]) < V.TAU
    y = V.clear_of_kink(x, gamma, beta, 1e-5)
    assert not (np.abs(V.pre_activation(y, gamma, beta, 1e-5))[:, :2] < V.TAU).any()
    moved = y != x
    assert moved[1, 0, 2, 2] and moved.sum() >= 1 and not moved[:, 2].any()      # (gamma = 0: nothing to clear)
    assert np.array_equal((y - x)[moved] * 8, np.round((y - x)[moved] * 8))
    z = np.round(rng.standard_normal((2, 3, 4, 4)) * 32) / 32 + 0.5
    if not (np.abs(V.pre_activation(z, [1, 1, 1], [0.3, 0.3, 0.3], 1e-5)) < V.TAU).any():
        assert np.array_equal(V.clear_of_kink(z, [1, 1, 1], [0.3, 0.3, 0.3], 1e-5), z)


@pytest.mark.parametrize("ci", POINTWISE)
def test_restatement_against_float64_autograd_over_the_published_modules(ci):
    """ConvReg.forward + HintLoss of this package in float64 (stock conv -> BatchNorm2d -> ReLU -> MSELoss) against the numpy chain:
    loss, every gradient (upstream gradient 1.5), the running statistics after the step; the bias gradient of the autograd is below
    1e-12 of the largest weight-gradient entry -- which is what justifies the exact zeros of the fused route"""
    c = hint_fixture.load()[0][ci]
    reg = _regressor_of(c, torch.float64)
    x = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_(True)
    f_s, f_t = reg(x, torch.from_numpy(c["t"].astype(np.float64)))
    loss = HintLoss()(f_s, f_t)
    (1.5 * loss).backward()
    Ct = c["t_shape"][1]
    w = V.chain(c["x"], c["t"], c["w"], c["b"], c["gamma"], c["beta"], c["eps"], 1.5, np.zeros(Ct), np.ones(Ct), c["momentum"])
    assert abs(loss.item() - w["loss"]) <= 1e-13 * w["loss"]
    # (M = 2: dx is a difference of nearly equal numbers, the two float64 evaluations agree to fewer digits)
    tol = 1e-7 if ci == 0 else 1e-11
    assert rel(x.grad.numpy(), w["dx_s"]) < tol
    assert rel(reg.conv.weight.grad.numpy().reshape(w["dw"].shape), w["dw"]) < tol
    assert rel(reg.bn.weight.grad.numpy(), w["d_gamma"]) < tol and rel(reg.bn.bias.grad.numpy(), w["d_beta"]) < tol
    assert rel(reg.bn.running_mean.numpy(), w["running_mean"]) < 1e-13 and rel(reg.bn.running_var.numpy(), w["running_var"]) < 1e-12
    assert int(reg.bn.num_batches_tracked) == 1
    assert reg.conv.bias.grad.abs().max().item() < (1e-7 if ci == 0 else 1e-12) * reg.conv.weight.grad.abs().max().item()
    assert np.abs(w["db"]).max() < (1e-7 if ci == 0 else 1e-12) * np.abs(w["dw"]).max()


def test_restatement_reproduces_the_reference():
    """float64 evaluation of the formulas vs the reference's fp32 results: within the distances the generator recorded"""
    cases, _allow = hint_fixture.load()
    up = 1 + 1e-9
    for ci, c in enumerate(cases):
        Ct = c["t_shape"][1]
        a = V.tail(c["conv_out"], c["t_grid"], c["gamma"], c["beta"], c["eps"], 1.0, np.zeros(Ct), np.ones(Ct), c["momentum"])
        assert abs(c["loss"] - a["loss"]) <= c["ref_vs_f64_loss"] * a["loss"] * up
        assert rel(c["d_conv_out"], a["dx"]) <= c["ref_vs_f64_dx"] * up
        assert rel(c["d_gamma"], a["d_gamma"]) <= c["ref_vs_f64_dgamma"] * up and rel(c["d_beta"], a["d_beta"]) <= c["ref_vs_f64_dbeta"] * up
        assert rel(c["running_mean"], a["running_mean"]) <= c["ref_vs_f64_rmean"] * up
        assert rel(c["running_var"], a["running_var"]) <= c["ref_vs_f64_rvar"] * up
        if ci in POINTWISE:
            w = V.chain(c["x"], c["t"], c["w"], c["b"], c["gamma"], c["beta"], c["eps"])
            assert rel(c["conv_out"], w["conv_out"]) < 1e-5
            assert abs(c["loss"] - w["loss"]) <= (c["ref_vs_f64_chain_loss"] + 1e-12) * w["loss"] * up
            assert rel(c["dx_s"], w["dx_s"]) <= c["ref_vs_f64_dxs"] * up + (1e-7 if ci == 0 else 1e-11)
            assert rel(c["dw"].reshape(w["dw"].shape), w["dw"]) <= c["ref_vs_f64_dw"] * up + (1e-7 if ci == 0 else 1e-11)


@pytest.mark.parametrize("ci", [0, 1])
def test_restatement_gradient_is_the_derivative_of_its_loss(ci):
    """central differences of the float64 loss of the tail on the two smallest cases: x, gamma, beta; with an upstream gradient of 1.5"""
    c = hint_fixture.load()[0][ci]
    x, t = c["conv_out"].astype(np.float64), c["t_grid"].astype(np.float64)
    ga, be = c["gamma"].astype(np.float64), c["beta"].astype(np.float64)
    g = V.tail(x, t, ga, be, c["eps"], g_loss=1.5)
    h = 1e-6

    def num(arr):
        out = np.zeros_like(arr)
        for idx in np.ndindex(*arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            hi = V.tail(x, t, ga, be, c["eps"])["loss"]
            arr[idx] = keep - h
            lo = V.tail(x, t, ga, be, c["eps"])["loss"]
            arr[idx] = keep
            out[idx] = 1.5 * (hi - lo) / (2 * h)
        return out

    assert np.abs(num(x) - g["dx"]).max() < 2e-7
    assert np.abs(num(ga) - g["d_gamma"]).max() < 1e-8 and np.abs(num(be) - g["d_beta"]).max() < 1e-8


def test_composite_on_cpu_tensors_matches_the_fixture():
    """CPU tensors take the composite through ConvReg.loss: the loss, every gradient and the running statistics within the
    allowances, against the reference's own fp32 results (every branch) and the float64 chain (1 x 1 branch)"""
    cases, allow = hint_fixture.load()
    for ci, c in enumerate(cases):
        if c["tail_only"]:
            continue
        reg = _regressor_of(c)
        x, t = torch.from_numpy(c["x"]).requires_grad_(True), torch.from_numpy(c["t"])
        loss = reg.loss(x, t)
        loss.backward()
        assert loss.dtype == torch.float32 and loss.dim() == 0 and int(reg.bn.num_batches_tracked) == 1
        assert abs(loss.item() - c["loss"]) <= (allow["chain_loss"] + c["ref_vs_f64_chain_loss"]) * c["loss"]
        assert rel(x.grad.numpy(), c["dx_s"]) <= allow["dxs"] + c["ref_vs_f64_dxs"]
        assert rel(reg.conv.weight.grad.numpy(), c["dw"]) <= allow["dw"] + c["ref_vs_f64_dw"]
        assert rel(reg.bn.weight.grad.numpy(), c["d_gamma"]) <= allow["dgamma"] + c["ref_vs_f64_dgamma"]
        assert rel(reg.bn.bias.grad.numpy(), c["d_beta"]) <= allow["dbeta"] + c["ref_vs_f64_dbeta"]
        assert rel(reg.bn.running_mean.numpy(), c["running_mean"]) <= allow["rmean"] + c["ref_vs_f64_rmean"]
        assert rel(reg.bn.running_var.numpy(), c["running_var"]) <= allow["rvar"] + c["ref_vs_f64_rvar"]
        if ci in POINTWISE:
            w = V.chain(c["x"], c["t"], c["w"], c["b"], c["gamma"], c["beta"], c["eps"])
            assert abs(loss.item() - w["loss"]) <= allow["chain_loss"] * w["loss"]
            assert rel(x.grad.numpy(), w["dx_s"]) <= allow["dxs"] and rel(reg.conv.weight.grad.numpy().reshape(w["dw"].shape), w["dw"]) <= allow["dw"]
        # the loss is HintLoss of the reference's contract, forward(x, t) -> (f_s, f_t) in stock ops
        ref = _regressor_of(c)
        f_s, f_t = ref(torch.from_numpy(c["x"]), t)
        assert f_s.shape == f_t.shape == tuple(c["t_grid"].shape) and np.array_equal(f_t.numpy(), c["t_grid"])
        # (two fp32 evaluations, each within the allowance of the float64 value)
        assert abs(HintLoss()(f_s, f_t).item() - c["loss"]) <= 2 * allow["chain_loss"] * c["loss"]
    # eval mode: the running statistics normalise and stay put
    c = cases[1]
    reg = _regressor_of(c).eval()
    out = reg.loss(torch.from_numpy(c["x"]), torch.from_numpy(c["t"]))
    f_s, f_t = _regressor_of(c).eval()(torch.from_numpy(c["x"]), torch.from_numpy(c["t"]))
    assert abs(out.item() - HintLoss()(f_s, f_t).item()) < 1e-6 * out.item()
    assert int(reg.bn.num_batches_tracked) == 0 and not reg.bn.running_mean.any()
    # float64 comes back as float64; a target that wants a gradient gets one
    reg = _regressor_of(c, torch.float64)
    tg = torch.from_numpy(c["t"].astype(np.float64)).requires_grad_(True)
    out = reg.loss(torch.from_numpy(c["x"].astype(np.float64)), tg)
    out.backward()
    assert out.dtype == torch.float64 and tg.grad is not None and bool(tg.grad.abs().sum() > 0)


def test_state_dict_keys_and_rng_draws_are_the_reference_s():
    from moma_amd.backbones.efficientnet import SamePadConv2d
    cases, _ = hint_fixture.load()
    for ci, c in enumerate(cases):
        torch.manual_seed(1800 + ci)
        reg = ConvReg(c["s_shape"], c["t_shape"])
        assert list(reg.state_dict()) == KEYS == c["state_keys"]
        assert np.array_equal(reg.conv.weight.detach().numpy(), c["w"]) and np.array_equal(reg.conv.bias.detach().numpy(), c["b"])
        assert isinstance(reg.bn, torch.nn.BatchNorm2d) and isinstance(reg.relu, torch.nn.ReLU)
        assert isinstance(reg.conv, SamePadConv2d) == (ci <= 8) and isinstance(reg.conv, torch.nn.ConvTranspose2d) == (ci == 10)
    reg = ConvReg((2, 3, 4, 4), (2, 5, 4, 4))
    x = torch.randn(2, 3, 4, 4)
    assert torch.equal(reg.conv(x, with_bias=False) + reg.conv.bias.view(1, -1, 1, 1), reg.conv(x)) or \
        torch.allclose(reg.conv(x, with_bias=False) + reg.conv.bias.view(1, -1, 1, 1), reg.conv(x), atol=1e-6)
    assert reg.conv.bias is not None and [n for n, _ in reg.named_parameters()] == KEYS[:4]


def test_token_lists_are_refused():
    with pytest.raises(ValueError, match=r"feature maps.*\(2, 17, 32\).*ViT"):
        HintLoss()(torch.randn(2, 17, 32), torch.randn(2, 17, 32))
    with pytest.raises(ValueError, match="ViT"):
        ConvReg((2, 17, 32), (2, 17, 32))
    reg = ConvReg((2, 8, 4, 4), (2, 8, 4, 4))
    with pytest.raises(ValueError, match="ViT"):
        reg.loss(torch.randn(2, 17, 8), torch.randn(2, 8, 4, 4))
    with pytest.raises(ValueError, match="ViT"):
        reg(torch.randn(2, 8, 4, 4), torch.randn(2, 17, 8))


def test_ops_hint_refuses_cpu_tensors_and_routes_every_shape():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    z = torch.zeros(2, 3, 4, 4)
    v = torch.zeros(3)
    with pytest.raises(_lib.MomaHipError):
        ops.hint_bn_relu_mse(z, z, v, v, v, v, 0.1, 1e-5)
    assert all(ops.hint_native(64, c, p) for c, p in ((16, 65536), (24, 16384), (40, 4096), (112, 1024), (1280, 256), (1, 1)))
    # the one losing row of profiles/hint_layer_microbench.txt: 112 x 14 x 14 in fp32 NCHW; bf16 and channels_last stay
    assert not ops.hint_native(256, 112, 196, dtype=torch.float32, channels_last=False)
    assert ops.hint_native(256, 112, 196, dtype=torch.bfloat16, channels_last=False)
    assert ops.hint_native(256, 112, 196, dtype=torch.float32, channels_last=True) and ops.hint_native(256, 112, 196)
    assert ops.hint_native(256, 1280, 49, dtype=torch.float32, channels_last=False)
    assert ops.hint_native(256, 40, 784, dtype=torch.float32, channels_last=False)


def test_workspace_query_and_argument_checks():
    """host arithmetic only: the workspace is three doubles per group of images (planes shorter than a chunk share an item with as
    many images as fill one), chunk of MOMA_HINT_CHUNK pixels and channel; one value per
    channel (M < 2), an empty map, a null pointer, an unknown layout or dtype, a misaligned pointer and a workspace that is too small
    are refused before anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.moma_hint_workspace_bytes
    nchw, nhwc, f32, bf16 = _lib.LAYOUT_NCHW, _lib.LAYOUT_NHWC, _lib.DT_F32, _lib.DT_BF16
    K = _lib.HINT_CHUNK
    assert K >= 64 and K % 8 == 0
    assert f(64, 24, 128 * 128, bf16, nchw, bf16, nchw) == 3 * 64 * -(-128 * 128 // K) * 24 * 8
    assert f(64, 1280, 256, f32, nhwc, bf16, nchw) == 3 * (64 // (K // 256)) * 1280 * 8
    assert f(256, 1280, 49, f32, nchw, f32, nchw) == 3 * -(-256 // (K // 49)) * 1280 * 8
    assert f(2, 1, 1, f32, nchw, f32, nchw) == 3 * 8 and f(3, 5, K + 1, f32, nchw, f32, nchw) == 3 * 3 * 2 * 5 * 8
    assert f(3, 5, K, f32, nchw, f32, nchw) == 3 * 3 * 5 * 8 and f(3, 5, K // 2 + 1, f32, nchw, f32, nchw) == 3 * 3 * 5 * 8
    assert f(1, 1, 1, f32, nchw, f32, nchw) == 0 and f(1, 8, 2, f32, nchw, f32, nchw) == 3 * 8 * 8           # M = 1 / M = 2
    assert f(0, 8, 8, f32, nchw, f32, nchw) == 0 and f(2, 0, 8, f32, nchw, f32, nchw) == 0 and f(2, 8, -1, f32, nchw, f32, nchw) == 0
    assert f(2, 8, 8, 5, nchw, f32, nchw) == 0 and f(2, 8, 8, f32, nchw, f32, 2) == 0
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30
    fwd = lambda B, Cc, P, dm=f32, lm=nchw, dt=f32, lt=nchw, ws=big, ptr=p: lib.moma_hint_fwd(    # noqa: E731
        ptr, p, p, p, None, None, None, 0.1, 1e-5, B, Cc, P, dm, lm, dt, lt, p, ws, p, p, p, p, None)
    bwd = lambda B, Cc, P, dm=f32, lm=nchw, dt=f32, lt=nchw, ws=big, ptr=p: lib.moma_hint_bwd(    # noqa: E731
        ptr, p, p, p, p, p, p, p, p, p, p, B, Cc, P, dm, lm, dt, lt, None)
    for call in (fwd, bwd):
        assert call(2, 8, 16, ptr=None) == -1                                                    # MOMA_E_NULL
        assert call(0, 8, 16) == -2 and call(2, 8, 0) == -2 and call(2, -1, 16) == -2            # MOMA_E_SHAPE
        assert call(1, 8, 1) == -2 and call(1, 1280, 1) == -2                                    # M < 2: one value per channel
        assert call(2, 8, 16, dm=7) == -6 and call(2, 8, 16, dt=2) == -6                         # MOMA_E_UNSUPPORTED
        assert call(2, 8, 16, lm=2) == -6 and call(2, 8, 16, lt=-1) == -6
        assert call(2, 8, 16, dm=bf16, lm=nhwc, ptr=C.c_void_p(p.value + 1)) == -4               # MOMA_E_ALIGN
    assert fwd(2, 8, 16, ws=3 * 8 * 8 - 1) == -5                                                 # MOMA_E_WORKSPACE
    assert lib.moma_hint_bwd(p, p, p, p, p, p, p, p, None, None, None, 2, 8, 16, f32, nchw, f32, nchw, None) == -1   # nothing asked for


ARGV = ["--distill", "hint", "--hint_layer", "1", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
        "--n_cls", "4", "--batch_size", "8", "-c", "1", "-d", "1", "-b", "100"]


def _hint_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(ARGV + ["--steps_per_epoch", "1", "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def test_build_training_puts_the_regressor_in_module_list_and_the_optimizer():
    """(the parent commit's build_training raises NotImplementedError("hint"))"""
    dev = torch.device("cpu")
    opt, built = _hint_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    reg = module_list[1]
    assert isinstance(criterion_list[2], HintLoss) and isinstance(reg, ConvReg) and contrast is None
    assert len(module_list) == 3 and module_list[0] is model_s and module_list[-1] is model_t
    with torch.no_grad():
        probe = torch.randn(2, 3, 32, 32)
        fs, ft = model_s(probe, is_feat=True)[0][opt.hint_layer], model_t(probe, is_feat=True)[0][opt.hint_layer]
    assert reg.conv.weight.shape[:2] == (ft.shape[1], fs.shape[1]) and reg.bn.num_features == ft.shape[1]
    assert any(m is reg for m in trainable_list)
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()} | {id(p) for p in reg.parameters()}
    assert len(list(reg.parameters())) == 4 and not list(criterion_list[2].parameters())
    assert not any(id(p) in opt_params for p in model_t.parameters())
    # another layer: another pair of shapes
    opt4, built4 = _hint_training(dev, ["--hint_layer", "3"])
    assert built4[2][1].bn.num_features == model_t(probe, is_feat=True)[0][3].shape[1]


def test_one_cpu_step_of_the_loop_trains_the_regressor():
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _hint_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    reg = module_list[1]
    before = {n: v.detach().clone() for n, v in reg.state_dict().items()}
    student_before = [p.detach().clone() for p in model_s.parameters()]
    teacher_before = [p.detach().clone() for p in model_t.parameters()]
    opt.trace, opt.print_freq = [], 1000
    loader = SyntheticLoader(1, 8, 32, 4, 3, dev)
    train_distill_moma(1, loader, module_list, criterion_list, None, contrast, optimizer, opt)
    (loss, _idx, loss_kd), = opt.trace
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd)) and loss_kd.dtype == torch.float32
    after = reg.state_dict()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in reg.parameters())
    for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
        assert not torch.equal(before[k], after[k]), k
    assert int(after["bn.num_batches_tracked"]) == 1
    assert any(not torch.equal(a, b) for a, b in zip(student_before, model_s.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
    # the KD term is the restatement's value on feat[hint_layer] of the same (pre-step) models and regressor
    opt2, built2 = _hint_training(dev)
    images, _labels = next(iter(loader))
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](images, is_feat=True)
        ft, _ = built2[1](images, is_feat=True)
    r2 = built2[2][1]
    want = V.chain(fs[1].numpy(), ft[1].numpy(), r2.conv.weight.detach().numpy(), r2.conv.bias.detach().numpy(),
                   r2.bn.weight.detach().numpy(), r2.bn.bias.detach().numpy(), r2.bn.eps)
    assert abs(float(loss_kd) - want["loss"]) <= 1e-5 * want["loss"]


def test_checkpoint_after_step_one_resumes_to_the_same_step_two_loss(tmp_path, monkeypatch):
    """two epochs of one step each in one run, against one epoch, then a second run with --resume: the resumed epoch starts from the
    checkpoint's regressor (key `regress_s`, restored before the optimizer state, momentum included) and reports the same loss"""
    from moma_amd import train_student_moma as T
    monkeypatch.setattr(T, "_REQUIRE_GPU", False)
    real = T.train_distill_moma
    seen = []

    def spy(epoch, loader, module_list, criterion_list, trainer, contrast, optimizer, o):
        acc, loss = real(epoch, loader, module_list, criterion_list, trainer, contrast, optimizer, o)
        seen.append((epoch, float(loss), {k: v.detach().clone() for k, v in module_list[1].state_dict().items()}))
        return acc, loss

    monkeypatch.setattr(T, "train_distill_moma", spy)

    def worker(root, extra):
        opt = T.parse_option(ARGV + ["--steps_per_epoch", "1", "--learning_rate", "0.05", "--seed", "7", "--print_freq", "1000",
                                     "--save_root", str(root)] + extra)
        opt.world_size, opt.ngpus_per_node = 1, 1
        T.main_worker(0, 1, opt)
        return opt

    worker(tmp_path / "straight", ["--epochs", "2"])
    opt = worker(tmp_path / "split", ["--epochs", "1"])
    path = os.path.join(opt.save_folder, "ckpt_last.pth")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck["regress_s"]) == KEYS and not list(ck["criterion_kd"])
    assert all(torch.equal(ck["regress_s"][k], seen[2][2][k]) for k in KEYS) and int(ck["regress_s"]["bn.num_batches_tracked"]) == 1
    worker(tmp_path / "split", ["--epochs", "2", "--resume", path])
    assert [s[0] for s in seen] == [1, 2, 1, 2]
    assert seen[0][1] == seen[2][1]                                  # the same first step
    assert seen[3][1] == seen[1][1], (seen[3][1], seen[1][1])        # and, through the checkpoint, the same second step
    assert all(torch.equal(seen[3][2][k], seen[1][2][k]) for k in KEYS)
    assert seen[1][1] != seen[0][1]


def test_checkpoints_of_other_modes_carry_no_new_key(tmp_path, monkeypatch):
    from moma_amd import train_student_moma as T
    monkeypatch.setattr(T, "_REQUIRE_GPU", False)
    opt = T.parse_option(["--distill", "kd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
                          "--batch_size", "8", "--steps_per_epoch", "1", "--epochs", "1", "--print_freq", "1000", "--seed", "7",
                          "--save_root", str(tmp_path)])
    opt.world_size, opt.ngpus_per_node = 1, 1
    T.main_worker(0, 1, opt)
    ck = torch.load(os.path.join(opt.save_folder, "ckpt_last.pth"), map_location="cpu", weights_only=False)
    assert "regress_s" not in ck and "criterion_kd" in ck


def test_gradient_sync_receives_exactly_the_regressor_s_parameters():
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
    opt, built = _hint_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    opt.trace, opt.print_freq = [], 1000
    trainer = Trainer()
    train_distill_moma(1, SyntheticLoader(1, 8, 32, 4, 3, dev), module_list, criterion_list, trainer, contrast, optimizer, opt)
    assert len(trainer.attached) == 1 and trainer.finished == 1
    assert [id(p) for p in trainer.attached[0]] == [id(p) for p in module_list[1].parameters()] and len(trainer.attached[0]) == 4

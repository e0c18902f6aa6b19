"""`--distill semckd` without a GPU: the fixture recorded from the reference, the float64 restatement, the modules (names, keys, RNG
order, the composite route), the C ABI's argument checks, build_training, one step of the loop, checkpoint and resume, the gradient
exchanges with the never-used parameters present, the ragged-batch skip.  On the parent commit `--distill semckd` raises
NotImplementedError and moma_amd.distiller_zoo has no SelfA: everything here fails there."""
import argparse
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from moma_amd.distiller_zoo import MLPEmbed, Proj, SelfA, SemCKDLoss  # noqa: F401  (the modules under test)
from tests import semckd_fixture, semckd_ref as V
from tests.crd_ref import rel

CASES, ALLOW = semckd_fixture.load()
GENERAL = [ci for ci, c in enumerate(CASES) if not semckd_fixture.head_is_zero(c)]


def test_fixture_files_stay_below_the_size_limit():
    fs = semckd_fixture.files()
    assert fs and all(os.path.getsize(f) <= (1 << 20) for f in fs)


def test_fixture_is_what_the_issue_lists():
    assert len(CASES) == semckd_fixture.N_CASES
    assert [(c["B"], c["stu"], c["tea"]) for c in CASES] == [
        (8, [(3, 8), (5, 4)], [(4, 8), (6, 4), (7, 2)]),
        (9, [(2, 6), (3, 3)], [(3, 5), (130, 3)]),
        (12, [(3, 9), (4, 5), (6, 3), (16, 2)], [(3, 9), (4, 5), (6, 3), (20, 2)]),
        (8, [(3, 4)], [(2, 7)]),
        (4, [(3, 8), (5, 4)], [(4, 8), (6, 4), (7, 2)])]
    for ci, c in enumerate(CASES):
        for f in c["fs"] + c["ft"]:                                    # multiples of 1/32 up to 4: exact in bf16
            assert np.array_equal(f, np.round(f * 32) / 32) and np.abs(f).max() <= 4
        assert c["kink_margin"] >= 2.0 ** -18, ci                      # (make_golden_semckd.py says why not 2^-10 everywhere)
        assert c["weight"].min() > 1e-6                                # no softmax row degenerates
        assert np.allclose(c["weight"].sum(-1), 1.0, atol=1e-6)
    # what the issue measured on the first three shapes: the reference's fp32 within 7e-8 of float64 on the loss, 2e-6 elsewhere
    for ci in GENERAL:
        c = CASES[ci]
        assert c["ref_vs_f64_loss"] <= 1e-7 and c["ref_vs_f64_chain_loss"] <= 1e-7, ci
        assert all(c["ref_vs_f64_" + k] <= 2e-6 for k in ("ind", "dsv", "dw", "weight", "dxs", "dproj", "dhead")), ci
    assert CASES[3]["head_noise"] == 0.0 and CASES[4]["head_noise"] < 1e-6
    assert ALLOW["loss"] <= 2e-7 and all(ALLOW[k] <= 4e-6 for k in ALLOW)


@pytest.mark.parametrize("ci", range(semckd_fixture.N_CASES))
def test_restatement_reproduces_the_reference_s_tail(ci):
    c = CASES[ci]
    r = V.tail(c["s_value"], c["target"], c["weight"])
    assert abs(c["loss"] - r["loss"]) <= ALLOW["loss"] * r["loss"]
    assert rel(c["ind"], r["ind"]) <= ALLOW["ind"] and rel(c["dw"], r["dw"]) <= ALLOW["dw"]
    for q, (a, b) in enumerate(zip(c["dsv"], r["dx"])):
        assert rel(a, b) <= ALLOW["dsv"], q


def test_restatement_gradient_is_the_derivative_of_its_loss():
    rng = np.random.default_rng(3)
    B, S, T = 3, 2, 2
    xs = [rng.standard_normal((B, 2, 3, 3)) for _ in range(S * T)]
    ts = [rng.standard_normal((B, 2, 3, 3)) for _ in range(S * T)]
    w = rng.random((B, S, T))
    r = V.tail(xs, ts, w, g=3.0)
    h = 1e-6
    for p, idx in ((0, (1, 0, 2, 1)), (3, (2, 1, 0, 0))):
        xp = [x.copy() for x in xs]
        xp[p][idx] += h
        xm = [x.copy() for x in xs]
        xm[p][idx] -= h
        num = 3.0 * (V.tail(xp, ts, w)["loss"] - V.tail(xm, ts, w)["loss"]) / (2 * h)
        assert abs(num - r["dx"][p][idx]) <= 1e-8
    wp = w.copy()
    wp[1, 0, 1] += h
    assert abs(3.0 * (V.tail(xs, ts, wp)["loss"] - r["loss"]) / h - r["dw"][1, 0, 1]) <= 1e-8
    x = rng.standard_normal((4, 2, 3))
    dG = rng.standard_normal((4, 4))
    xq = x.copy()
    xq[2, 1, 0] += h
    assert abs(((V.gram(xq) - V.gram(x)) * dG).sum() / h - V.gram_bwd(x, dG)[2, 1, 0]) <= 1e-5


def _maps(c, dtype=torch.float32, grad=True):
    fs = [torch.from_numpy(f).to(dtype).requires_grad_(grad) for f in c["fs"]]
    return fs, [torch.from_numpy(f).to(dtype) for f in c["ft"]]


def _check_against_fixture(c, mod, loss, fs, what):
    """loss and the recorded gradients of one step against the reference's fp32 results, each within its allowance"""
    assert loss.dtype == torch.float32 and abs(float(loss.detach()) - c["loss"]) <= 2 * ALLOW["chain_loss"] * c["loss"], what
    for i, f in enumerate(fs):
        assert rel(f.grad.numpy(), c["dxs"][i]) <= 2 * ALLOW["dxs"], (what, i)
    dproj = mod.regressor00.regressor[0].weight.grad.numpy()
    assert rel(dproj, c["dproj"]) <= 2 * ALLOW["dproj"], what
    dhead = mod.query_0.linear1.weight.grad
    if semckd_fixture.head_is_zero(c):
        # analytically 0: compared in absolute terms against the largest gradient of the projection (rounding noise at most)
        assert dhead is None or float(dhead.abs().max()) <= 1e-6 * np.abs(c["dproj"]).max(), what
    else:
        assert rel(dhead.numpy(), c["dhead"]) <= 2 * ALLOW["dhead"], what


@pytest.mark.parametrize("ci", range(semckd_fixture.N_CASES))
def test_composite_on_cpu_tensors_matches_the_fixture(ci):
    """SelfA.loss on CPU tensors takes the composite (float64 head and errors around the fp32 projections): within twice the
    allowance of the reference's fp32 results (its own distance from float64 and the composite's add)"""
    c = CASES[ci]
    mod = semckd_fixture.module_of(c)
    fs, ft = _maps(c)
    loss = mod.loss(fs, ft)
    loss.backward()
    _check_against_fixture(c, mod, loss, fs, "composite")
    assert all(p.grad is None for n, p in mod.named_parameters() if ".regressor." in n and ("query_" in n or "key_" in n))


@pytest.mark.parametrize("ci", [0, 1, 3])
def test_forward_and_semckd_loss_are_the_reference_s(ci):
    """forward(feat_s, feat_t) -> (s_value, target, weight) as recorded, SemCKDLoss of them on the CPU (no .cuda())"""
    c = CASES[ci]
    mod = semckd_fixture.module_of(c)
    fs, ft = _maps(c)
    s_value, target, weight = mod(fs, ft)
    S, T = len(c["stu"]), len(c["tea"])
    assert len(s_value) == len(target) == S and all(len(r) == T for r in s_value) and tuple(weight.shape) == (c["B"], S, T)
    for q in range(S * T):
        assert rel(s_value[q // T][q % T].detach().numpy(), c["s_value"][q]) <= 1e-5, q
        assert np.array_equal(target[q // T][q % T].numpy(), c["target"][q]), q
    assert rel(weight.detach().numpy(), c["weight"]) <= 1e-5
    loss = SemCKDLoss()(s_value, target, weight)
    loss.backward()
    _check_against_fixture(c, mod, loss, fs, "forward + SemCKDLoss")


def test_state_dict_keys_and_rng_draws_are_the_reference_s():
    for c in CASES:
        mod = semckd_fixture.module_of(c)            # (asserts the key list, the recorded tensors bit for bit, the checksums)
        assert sum(1 for k in c["state_keys"] if ".regressor." in k and k.startswith(("query_", "key_"))) == 4 * (len(c["stu"]) + len(c["tea"]))
    mod = semckd_fixture.module_of(CASES[0])
    assert isinstance(mod.query_0, MLPEmbed) and isinstance(mod.key_2, MLPEmbed) and isinstance(mod.regressor12, Proj)
    assert mod.s_len == 2 and mod.t_len == 3 and mod.feat_dim == 8 and mod.soft == 1.0
    conv = mod.regressor00.regressor[0]
    assert conv.bias is None and conv.kernel_size == (1, 1) and mod.regressor00.regressor[3].kernel_size == (3, 3)


def test_token_lists_and_other_batch_sizes_are_refused():
    mod = SelfA(4, [3], [2], 1.0)
    tok = torch.zeros(4, 5, 3)
    with pytest.raises(ValueError, match="feature maps"):
        mod.loss([tok], [torch.zeros(4, 2, 2, 2)])
    with pytest.raises(ValueError, match="batches of 4"):
        mod.loss([torch.zeros(3, 3, 2, 2)], [torch.zeros(3, 2, 2, 2)])
    with pytest.raises(ValueError, match="batches of 4"):
        mod([torch.zeros(4, 3, 2, 2)], [torch.zeros(5, 2, 2, 2)])
    with pytest.raises(ValueError, match="1 student and 1 teacher"):
        mod.loss([torch.zeros(4, 3, 2, 2)] * 2, [torch.zeros(4, 2, 2, 2)])


def test_ops_refuse_cpu_tensors():
    from moma_amd import _lib, build, ops
    build.build(verbose=False)
    z = torch.zeros(2, 3, 4, 4)
    with pytest.raises(_lib.MomaHipError):
        ops.batch_gram(z)
    with pytest.raises(_lib.MomaHipError):
        ops.semckd_weighted_mse([[z]], [[z]], torch.ones(2, 1, 1))
    assert ops.semckd_native(1) and ops.semckd_native(64) and not ops.semckd_native(65) and not ops.semckd_native(0)


def test_workspace_query_and_argument_checks():
    """host arithmetic only: one double per (pair, sample, chunk); the shape errors, an unknown dtype, a null or misaligned pointer
    and a workspace that is too small are refused before anything is launched"""
    import ctypes as C
    from moma_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    K = _lib.SEMCKD_CHUNK
    assert K >= 256 and K % 8 == 0 and _lib.SEMCKD_MAX_PAIRS == 64
    buf = C.create_string_buffer(1 << 12)
    p = C.cast(buf, C.c_void_p).value
    f32, bf16 = _lib.DT_F32, _lib.DT_BF16

    def table(ns, dx=f32, dt=f32, x=p, t=p, d=p):
        tab = (_lib.SemckdPair * max(len(ns), 1))()
        for i, n in enumerate(ns):
            tab[i] = _lib.SemckdPair(x, t, d, n, dx, dt)
        return tab

    ws = lib.moma_semckd_workspace_bytes
    assert ws(table([1]), 1, 1) == 8 and ws(table([K]), 1, 3) == 3 * 8 and ws(table([K + 1]), 1, 3) == 3 * 2 * 8
    assert ws(table([1, 3 * K + 5, K - 1]), 3, 5) == 5 * (1 + 4 + 1) * 8
    assert ws(table([7] * 64), 64, 2) == 64 * 2 * 8
    assert ws(table([7] * 65), 65, 2) == 0 and ws(table([7]), 0, 2) == 0 and ws(table([7]), 1, 0) == 0 and ws(table([0]), 1, 2) == 0
    assert ws(None, 1, 2) == 0
    big = 1 << 30
    fwd = lambda tab, n, S, B, w=p, wsb=big: lib.moma_semckd_fwd(tab, n, S, B, w, p, wsb, p, p, None)      # noqa: E731
    bwd = lambda tab, n, S, B, w=p, wsb=big: lib.moma_semckd_bwd(tab, n, S, B, w, p, None)                 # noqa: E731
    for call in (fwd, bwd):
        assert call(None, 1, 1, 2) == -1 and call(table([7]), 1, 1, 2, w=None) == -1                       # MOMA_E_NULL
        assert call(table([7], x=None), 1, 1, 2) == -1
        assert call(table([7] * 65), 65, 1, 2) == -2 and call(table([7]), 0, 1, 2) == -2                   # MOMA_E_SHAPE
        assert call(table([7]), 1, 1, 0) == -2 and call(table([7, 0]), 2, 1, 2) == -2 and call(table([7, -3]), 2, 2, 2) == -2
        assert call(table([7] * 6), 6, 4, 2) == -2 and call(table([7] * 6), 6, 0, 2) == -2                 # n_pairs % S
        assert call(table([7], dx=5), 1, 1, 2) == -6 and call(table([7], dt=-1), 1, 1, 2) == -6            # MOMA_E_UNSUPPORTED
        assert call(table([7], dx=bf16, x=p + 1), 1, 1, 2) == -4 and call(table([7], t=p + 2), 1, 1, 2) == -4   # MOMA_E_ALIGN
    assert bwd(table([7], d=p + 2), 1, 1, 2) == -4
    assert fwd(table([K + 1]), 1, 1, 3, wsb=3 * 2 * 8 - 1) == -5                                           # MOMA_E_WORKSPACE
    gs = lib.moma_sp_gram_sum
    n = lib.moma_sp_workspace_bytes(4, 100)
    assert n == 4 * 4 * 4
    assert gs(None, n, 100, 4, p, None) == -1 and gs(p, n, 100, 4, None, None) == -1
    assert gs(p, n, 100, 0, p, None) == -2 and gs(p, n, 0, 4, p, None) == -2
    assert gs(p, n, 100, 1025, p, None) == -6 and gs(p, n - 1, 100, 4, p, None) == -5 and gs(p + 2, n, 100, 4, p, None) == -4


ARGV = ["--distill", "semckd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100",
        "--n_cls", "4", "--batch_size", "8", "-c", "1", "-d", "1", "-b", "400"]


def _semckd_training(dev, extra=()):
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(ARGV + ["--steps_per_epoch", "1", "--learning_rate", "0.01", *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    return opt, build_training(opt, dev)


def _unused(sa):
    return [p for n, p in sa.named_parameters() if ".regressor." in n and n.startswith(("query_", "key_"))]


def test_build_training_puts_self_attention_in_module_list_and_the_optimizer():
    """(the parent commit's build_training raises NotImplementedError("semckd"))"""
    dev = torch.device("cpu")
    opt, built = _semckd_training(dev, ["--soft", "2.5"])
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    sa = module_list[1]
    assert isinstance(criterion_list[2], SemCKDLoss) and isinstance(sa, SelfA) and contrast is None
    assert len(module_list) == 3 and module_list[0] is model_s and module_list[-1] is model_t
    with torch.no_grad():
        probe = torch.randn(2, 3, 32, 32)
        fs, ft = model_s(probe, is_feat=True)[0][1:-1], model_t(probe, is_feat=True)[0][1:-1]
    assert sa.feat_dim == 8 and sa.soft == 2.5 and sa.s_len == len(fs) and sa.t_len == len(ft)
    for i, f in enumerate(fs):
        for j, t in enumerate(ft):
            reg = getattr(sa, f"regressor{i}{j}").regressor
            assert reg[0].in_channels == f.shape[1] and reg[6].out_channels == t.shape[1]
    assert any(m is sa for m in trainable_list)
    opt_params = {id(p) for g in optimizer.param_groups for p in g["params"]}
    assert opt_params == {id(p) for p in model_s.parameters()} | {id(p) for p in sa.parameters()}
    assert not list(criterion_list[2].parameters()) and not any(id(p) in opt_params for p in model_t.parameters())


def test_one_cpu_step_of_the_loop_trains_self_attention_and_skips_a_ragged_batch():
    from moma_amd.helper.loops_moma import train_distill_moma
    dev = torch.device("cpu")
    opt, built = _semckd_training(dev)
    model_s, model_t, module_list, criterion_list, trainable_list, contrast, optimizer = built
    sa = module_list[1]
    before = {n: v.detach().clone() for n, v in sa.state_dict().items()}
    student_before = [p.detach().clone() for p in model_s.parameters()]
    teacher_before = [p.detach().clone() for p in model_t.parameters()]
    opt.trace, opt.print_freq = [], 1000
    g = torch.Generator().manual_seed(5)
    full = (torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 4, (8,), generator=g))
    ragged = (torch.randn(5, 3, 32, 32, generator=g), torch.randint(0, 4, (5,), generator=g))
    train_distill_moma(1, [ragged, full, ragged], module_list, criterion_list, None, contrast, optimizer, opt)
    (loss, _idx, loss_kd), = opt.trace                                  # one step: the two short batches were skipped before it
    assert np.isfinite(float(loss)) and np.isfinite(float(loss_kd)) and loss_kd.dtype == torch.float32 and float(loss_kd) > 0
    after = sa.state_dict()
    unused = {id(p) for p in _unused(sa)}
    assert len(unused) == 4 * (sa.s_len + sa.t_len)
    for n, p in sa.named_parameters():
        if id(p) in unused:
            assert p.grad is None and torch.equal(before[n], after[n]), n         # never used: no gradient, not moved by the optimizer
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for k in ("regressor00.regressor.0.weight", "regressor00.regressor.1.running_mean", "query_0.linear1.weight", "key_0.linear2.bias"):
        assert not torch.equal(before[k], after[k]), k
    assert int(after["regressor00.regressor.1.num_batches_tracked"]) == 1
    assert any(not torch.equal(a, b) for a, b in zip(student_before, model_s.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, model_t.parameters()))
    # the KD term is SemCKDLoss(*forward(...)) on feat[1:-1] of the same (pre-step) models and module, evaluated in float64
    opt2, built2 = _semckd_training(dev)
    built2[0].train(); built2[1].eval()
    with torch.no_grad():
        fs, _ = built2[0](full[0], is_feat=True)
        ft, _ = built2[1](full[0], is_feat=True)
    sa2 = built2[2][1].double()
    s_value, target, weight = sa2([f.double() for f in fs[1:-1]], [f.double() for f in ft[1:-1]])
    want = float(SemCKDLoss()(s_value, target, weight).detach())
    assert abs(float(loss_kd) - want) <= 1e-5 * want


KEY = "self_attention"


def test_checkpoint_after_step_one_resumes_to_the_same_step_two_loss(tmp_path, monkeypatch):
    """two epochs of one step each in one run, against one epoch, then a second run with --resume: the resumed epoch starts from the
    checkpoint's SelfA (key `self_attention`, restored before the optimizer state, momentum included) and reports the same loss"""
    from moma_amd import train_student_moma as T
    monkeypatch.setattr(T, "_REQUIRE_GPU", False)
    # host logic, checked to the bit: on the CPU also where a GPU is present (stock convolution backwards there are not repeatable
    # from process to process, and the second step inherits their last bits)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
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
    keys = list(seen[2][2])
    assert list(ck[KEY]) == keys and not list(ck["criterion_kd"]) and "regress_s" not in ck
    assert any(".regressor." in k and k.startswith("query_") for k in keys)      # the never-used heads own keys in the checkpoint
    assert all(torch.equal(ck[KEY][k], seen[2][2][k]) for k in keys)
    worker(tmp_path / "split", ["--epochs", "2", "--resume", path])
    assert [s[0] for s in seen] == [1, 2, 1, 2]
    assert seen[0][1] == seen[2][1]                                  # the same first step
    assert seen[3][1] == seen[1][1], (seen[3][1], seen[1][1])        # and, through the checkpoint, the same second step
    assert all(torch.equal(seen[3][2][k], seen[1][2][k]) for k in keys)
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
    assert KEY not in ck and "criterion_kd" in ck


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, out, dp):
    """two steps of the loop on `world` gloo ranks, SelfA outside any wrap: `flat` = FlatDataParallel.allreduce_grads over the
    student's and SelfA's parameters, `ddp` = the stock reducer on the student + trainer.attach_grad_sync on SelfA's"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from moma_amd.backbones.resnet_cifar import resnet8
    from moma_amd.distiller_zoo import DistillKL
    from moma_amd.helper.loops_moma import train_distill_moma
    from moma_amd.learning.contrast_trainer import ContrastTrainer
    from moma_amd.learning.ddp import wrap_student
    B = 4
    opt = argparse.Namespace(distill="semckd", soft=1.0, cls=1.0, div=1.0, beta=1.0, kd_T=4.0, gpu=None, device=torch.device("cpu"),
                             multiprocessing_distributed=True, print_freq=10 ** 9, batch_size=B, rank=rank, local_rank=rank,
                             node_rank=0, ngpus_per_node=world, world_size=world, trace=[], head="None", attn="self", mem="MoCo",
                             moma_prec="fp32", moma_fused=True, shuffle_bn="per_rank", alpha=0.9)
    torch.manual_seed(0)                                   # identical initial weights on every rank
    ms, mt = resnet8(num_classes=10), resnet8(num_classes=10)
    with torch.no_grad():
        probe = torch.randn(2, 3, 16, 16)
        s_n = [f.shape[1] for f in ms(probe, is_feat=True)[0][1:-1]]
        t_n = [f.shape[1] for f in mt(probe, is_feat=True)[0][1:-1]]
    sa = SelfA(B, s_n, t_n, opt.soft)
    trainer = ContrastTrainer(opt)
    optimizer = torch.optim.SGD(nn.ModuleList([ms, sa]).parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    ddp = wrap_student(ms, mode=dp)
    g = torch.Generator().manual_seed(100 + rank)          # different data shard per rank
    loader = [(torch.randn(B, 3, 16, 16, generator=g), torch.randint(0, 10, (B,), generator=g)) for _ in range(2)]
    train_distill_moma(1, loader, nn.ModuleList([ddp, sa, mt]), nn.ModuleList([nn.CrossEntropyLoss(), DistillKL(4.0), SemCKDLoss()]),
                       trainer, None, optimizer, opt)
    unused = {id(p) for p in _unused(sa)}
    used = torch.cat([p.detach().reshape(-1) for p in sa.parameters() if id(p) not in unused])
    rest = torch.cat([p.detach().reshape(-1) for p in sa.parameters() if id(p) in unused])
    torch.save(dict(student=torch.cat([p.detach().reshape(-1) for p in ms.parameters()]), used=used, rest=rest,
                    used_grad=torch.cat([p.grad.reshape(-1) for p in sa.parameters() if id(p) not in unused]),
                    unused_grad_none=all(p.grad is None for p in sa.parameters() if id(p) in unused),
                    steps=len(opt.trace), launches=getattr(trainer, "grad_sync_launches", 0)), os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("dp", ["flat", "ddp"])
def test_gradient_exchange_with_the_never_used_parameters_present(tmp_path, dp):
    world, port = 2, _free_port()
    mp.spawn(_sync_worker, args=(world, port, str(tmp_path), dp), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert r0["steps"] == r1["steps"] == 2 and r0["launches"] == r1["launches"] >= 2
    assert r0["unused_grad_none"] and r1["unused_grad_none"] and torch.equal(r0["rest"], r1["rest"])
    # different shards, one averaged gradient: SelfA stays identical across the ranks, and so does the student
    assert torch.equal(r0["used_grad"], r1["used_grad"]) and float(r0["used_grad"].abs().max()) > 0
    assert torch.equal(r0["used"], r1["used"]) and torch.equal(r0["student"], r1["student"])
    assert r0["used"].numel() > 0 and r0["rest"].numel() > 0

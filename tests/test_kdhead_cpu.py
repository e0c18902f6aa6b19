"""CPU tests of the student head (helper/kd_head.py: StudentHead, its float64 composite) against the golden fixture and the float64
restatement (tests/kdhead_ref.py), the label rule, the caps of ops.kd_head_native, the `--student_head` flag and one step of
MomaStep.run_eager per head.

Allowance for every floating-point result: TWICE the largest distance of that kind that the reference's own fp32 results keep from
float64 over the fixture's cases, never below one fp32 ulp (tests/kdhead_fixture.py computes it from the .npz).  The composite is float64
inside: its doubles are compared with the restatement at 1e-12 and its float32 results at one fp32 ulp.  acc is compared exactly."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from moma_amd.distiller_zoo import DistillKL
from moma_amd.helper.kd_head import StudentHead
from moma_amd.helper.util import accuracy
from tests import kdhead_fixture, kdhead_ref as V
from tests.crd_ref import rel

CPU = torch.device("cpu")
ULP32 = 2.0 ** -23
N_CASES = kdhead_fixture.N_CASES


def _report(name, got, allowed):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e}, ratio {got / allowed:.2f})")
    return got <= allowed


def _relerr(got, want):
    return abs(got - want) / max(abs(want), 1e-300)


def test_loader_and_allowances():
    cases, allow = kdhead_fixture.load()
    assert len(cases) == N_CASES == 13 and set(allow) == {"cls", "div", "dz"}
    assert all(ULP32 <= allow[k] < 1e-4 for k in allow), allow                 # (fp32 results: a few ulps of sums of up to 2500 terms)
    assert kdhead_fixture.ONE_WALK_K == __import__("moma_amd._lib", fromlist=["x"]).KDHEAD_ONE_WALK_K
    shapes = [(c["B"], c["K"], c["T"]) for c in cases]
    L = kdhead_fixture.ONE_WALK_K
    assert shapes == [(1, 2, 4), (2, 1, 4), (3, 5, 4), (65, 4, 4), (64, 9, 1), (7, 100, 2.5), (5, 1000, 4), (4, L, 4), (3, L + 1, 4),
                      (3, 2500, 4), (3, 5, 1), (6, 5, 4), (4, 9, 4)]
    assert np.abs(cases[10]["logit_s"]).max() > 64 and cases[1]["loss_cls"] == 0.0 and cases[1]["loss_div"] == 0.0
    assert np.array_equal(cases[12]["logit_s"], cases[12]["logit_t"])


@pytest.mark.parametrize("ci", range(N_CASES))
def test_restatement_against_the_recorded_reference(ci):
    """the float64 restatement is where the fixture says it is: within the recorded distances of the reference's fp32 results"""
    c = kdhead_fixture.load()[0][ci]
    w = V.head(c["logit_s"], c["logit_t"], c["labels"], c["T"])
    slack = 1e-12
    assert _relerr(c["loss_cls"], w["loss_cls"]) <= c["ref_vs_f64_cls"] + slack
    if c["same"]:
        assert w["loss_div"] == 0.0 and abs(c["loss_div"]) <= c["ref_vs_f64_div"] and not w["dz_div"].any()
    else:
        assert _relerr(c["loss_div"], w["loss_div"]) <= c["ref_vs_f64_div"] + slack
    assert rel(c["dz"], w["dz"]) <= c["ref_vs_f64_dz"] + slack
    assert abs(c["acc"] - w["acc"]) < 1e-4


@pytest.mark.parametrize("ci", range(N_CASES))
def test_composite_against_the_restatement(ci):
    cases, allow = kdhead_fixture.load()
    c = cases[ci]
    T = c["T"]
    w = V.head(c["logit_s"], c["logit_t"], c["labels"], T, g_cls=3.0, g_div=0.5)
    y = torch.from_numpy(c["labels"])
    # float64 in, the doubles out: 1e-12
    zs = torch.from_numpy(c["logit_s"]).double().requires_grad_(True)
    zt = torch.from_numpy(c["logit_t"]).double()
    res, full = StudentHead.composite(zs, zt, y, T, full=True)
    assert all(r.dtype == torch.float32 and r.dim() == 0 for r in res)
    (3.0 * full["loss_cls"] + 0.5 * full["loss_div"]).backward()
    assert abs(float(full["loss_cls"].detach()) - w["loss_cls"]) <= 1e-12 * max(1.0, abs(w["loss_cls"]))
    assert abs(float(full["loss_div"].detach()) - w["loss_div"]) <= 1e-12 * max(1.0, abs(w["loss_div"]))
    assert float(full["acc"]) == w["acc"] and np.array_equal(full["pred"].numpy(), w["pred"])
    for k in ("lse", "lseS", "lseT"):
        assert np.abs(full[k].detach().numpy() - w[k]).max() <= 1e-12 * max(1.0, np.abs(w[k]).max()), k
    assert np.abs(zs.grad.numpy() - w["dz"]).max() <= 1e-12 * max(1.0, np.abs(w["dz"]).max())
    # the float32 results: one fp32 ulp
    assert abs(float(res[0]) - w["loss_cls"]) <= ULP32 * abs(w["loss_cls"]) and abs(float(res[1]) - w["loss_div"]) <= ULP32 * abs(w["loss_div"])
    assert float(res[2]) == np.float32(w["acc"])
    # the module on float32 CPU tensors: the composite, gradients in float32
    head = StudentHead(T)
    assert head.T == T and not head.native(zs, zt, y)
    xs = torch.from_numpy(c["logit_s"]).requires_grad_(True)
    lc, ld, acc = head(xs, torch.from_numpy(c["logit_t"]), y)
    (3.0 * lc + 0.5 * ld).backward()
    assert torch.equal(lc, res[0]) and torch.equal(ld, res[1]) and torch.equal(acc, res[2]) and not acc.requires_grad
    assert xs.grad.dtype == torch.float32 and rel(xs.grad.numpy(), w["dz"]) <= 2 * ULP32
    if c["same"]:
        assert float(ld) == 0.0


@pytest.mark.parametrize("ci", range(N_CASES))
def test_module_against_the_stock_pair(ci):
    """StudentHead on CPU tensors against nn.CrossEntropyLoss + DistillKL + accuracy on the same tensors: each side within its
    allowance of float64 (the stock pair IS the reference's arithmetic: the recorded distance)"""
    cases, allow = kdhead_fixture.load()
    c = cases[ci]
    y = torch.from_numpy(c["labels"])
    xs, xt = torch.from_numpy(c["logit_s"]).requires_grad_(True), torch.from_numpy(c["logit_t"])
    lc, ld, acc = StudentHead(c["T"])(xs, xt, y)
    (lc + ld).backward()
    ss = torch.from_numpy(c["logit_s"]).requires_grad_(True)
    sc, sd = nn.CrossEntropyLoss()(ss, y), DistillKL(c["T"])(ss, xt)
    (sc + sd).backward()
    sacc = accuracy(ss.detach(), y, topk=(1,))[0].squeeze(0)
    ok = _report("loss_cls vs stock", _relerr(float(lc), float(sc)), allow["cls"] + ULP32 / 2 + c["ref_vs_f64_cls"])
    if c["same"]:
        ok &= _report("loss_div vs stock (absolute)", abs(float(ld) - float(sd)), max(c["ref_vs_f64_div"], ULP32 * c["T"] ** 2))
    else:
        ok &= _report("loss_div vs stock", _relerr(float(ld), float(sd)), allow["div"] + ULP32 / 2 + c["ref_vs_f64_div"])
    ok &= _report("dz vs stock", rel(xs.grad.numpy(), ss.grad.numpy()), allow["dz"] + ULP32 / 2 + c["ref_vs_f64_dz"])
    assert ok and float(acc) == float(sacc) and acc.shape == sacc.shape


def test_the_label_rule():
    cases, allow = kdhead_fixture.load()
    c = cases[11]
    zs0, zt0, y0, T = c["logit_s"], c["logit_t"], c["labels"], c["T"]
    ign = y0 == V.IGNORE
    assert ign.sum() == 2
    zs = torch.from_numpy(zs0).requires_grad_(True)
    lc, ld, acc = StudentHead(T)(zs, torch.from_numpy(zt0), torch.from_numpy(y0))
    lc.backward()                                                            # the cross-entropy alone: ignored rows get nothing
    assert not zs.grad[torch.from_numpy(ign)].any() and zs.grad[torch.from_numpy(~ign)].abs().sum() > 0
    keep = V.head(zs0[~ign], zt0[~ign], y0[~ign], T)
    whole = V.head(zs0, zt0, y0, T)
    assert _relerr(float(lc), keep["loss_cls"]) <= allow["cls"] + ULP32 / 2
    assert _relerr(float(ld), whole["loss_div"]) <= allow["div"] + ULP32 / 2          # the KL term does not look at labels
    assert float(acc) == np.float32(100.0 * keep["hits"] / 6)                         # acc divides by B
    # a bad label: NaN loss_cls, a finite loss_div, zero CE gradient on that row; the other rows keep theirs; no exception
    for bad in (5, -1, 1 << 40):
        yb = y0.copy()
        yb[0] = bad
        zs = torch.from_numpy(zs0).requires_grad_(True)
        lc, ld, acc = StudentHead(T)(zs, torch.from_numpy(zt0), torch.from_numpy(yb))
        assert torch.isnan(lc) and _relerr(float(ld), whole["loss_div"]) <= allow["div"] + ULP32 / 2
        lc.backward()
        w = V.head(zs0, zt0, yb, T)
        assert np.isnan(w["loss_cls"]) and w["n_bad"] == 1 and not w["dz_cls"][0].any()
        assert not zs.grad[0].any() and not zs.grad[torch.from_numpy(ign)].any()
        others = ~ign
        others[0] = False
        assert rel(zs.grad.numpy()[others], w["dz_cls"][others]) <= allow["dz"] + ULP32 / 2
        zs2 = torch.from_numpy(zs0).requires_grad_(True)
        StudentHead(T)(zs2, torch.from_numpy(zt0), torch.from_numpy(yb))[1].backward()      # the divergence's gradient reaches every row
        assert rel(zs2.grad.numpy(), w["dz_div"]) <= allow["dz"] + ULP32 / 2 and zs2.grad[0].abs().sum() > 0
    # an all-ignored batch: NaN as torch, no CE gradient
    zs = torch.from_numpy(zs0).requires_grad_(True)
    lc, ld, acc = StudentHead(T)(zs, torch.from_numpy(zt0), torch.full((6,), V.IGNORE, dtype=torch.int64))
    lc.backward()
    assert torch.isnan(lc) and torch.isfinite(ld) and float(acc) == 0.0 and not zs.grad.any()
    # other dtypes take the composite too
    assert StudentHead(T)(torch.from_numpy(zs0).double(), torch.from_numpy(zt0).half(), torch.from_numpy(y0).int())[1].dtype == torch.float32
    for T_bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            StudentHead(T_bad)


def test_native_caps():
    from moma_amd import _lib, ops
    F32, BF16 = torch.float32, torch.bfloat16
    assert (_lib.KDHEAD_MAX_B, _lib.KDHEAD_MAX_K) == (_lib.CE_MAX_B, _lib.CE_MAX_K) == (16384, 32768)
    assert ops.kd_head_native(64, 4) and ops.kd_head_native(64, 4, BF16, F32) and ops.kd_head_native(_lib.KDHEAD_MAX_B, _lib.KDHEAD_MAX_K, BF16, BF16)
    assert not ops.kd_head_native(_lib.KDHEAD_MAX_B + 1, 4, BF16, F32) and not ops.kd_head_native(4, _lib.KDHEAD_MAX_K + 1, BF16, F32)
    assert not ops.kd_head_native(0, 4) and not ops.kd_head_native(4, 0)
    assert not ops.kd_head_native(64, 4, torch.float16, F32) and not ops.kd_head_native(64, 4, BF16, torch.float64)
    with pytest.raises(_lib.MomaHipError):
        ops.kd_head(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64), 4.0)      # no CPU path in the op


ARGV = ["--distill", "kd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4", "--batch_size", "8",
        "--steps_per_epoch", "1", "-c", "1", "-d", "1", "-b", "0", "--learning_rate", "0.01"]


def test_the_flag():
    from moma_amd.train_student_moma import parse_option
    assert parse_option(ARGV).student_head == "stock"
    assert parse_option(ARGV + ["--student_head", "fused"]).student_head == "fused"
    assert parse_option(ARGV + ["--student_head", "stock"]).student_head == "stock"
    with pytest.raises(SystemExit):
        parse_option(ARGV + ["--student_head", "both"])


def step_of(dev, head, extra=(), seed=5):
    """one MomaStep.run_eager step of --distill kd (resnet8x4 <- resnet32x4, B = 8, n_cls = 4) -> (loss, acc, {name: grad}, MomaStep)"""
    from moma_amd.dataset.synthetic import SyntheticLoader
    from moma_amd.helper.loops_moma import MomaStep
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(ARGV + ["--student_head", head, *extra])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, dev
    torch.manual_seed(0)
    model_s, model_t, module_list, criterion_list, _tr, contrast, optimizer = build_training(opt, dev)
    for m in module_list:
        m.train()
    module_list[-1].eval()
    st = MomaStep(module_list, criterion_list, None, contrast, optimizer, opt, dev)
    images, labels = next(iter(SyntheticLoader(1, 8, 32, 4, seed, dev)))
    loss, loss_kd, acc = st.run_eager(images, labels, model_t)
    assert loss_kd == 0 and len(criterion_list) == 3
    return float(loss), float(acc), {n: p.grad.detach().double().cpu().numpy() for n, p in model_s.named_parameters() if p.grad is not None}, st


def compare_steps(fused, stock, allow, extra_dz=0.0):
    """loss and every student gradient of the two heads.  The loss is cls loss_cls + div loss_div with both weights 1: each head's terms
    are within their allowance of float64 (the stock chain is the reference's arithmetic: half the allowance), both of order 1, so the
    sum's distance is bounded by 1.5 (allow_cls + allow_div) of the total plus the rounding of the sum.  The gradients are a linear map
    of dz: 1.5 allow_dz in rel()'s metric (+ extra_dz where dz is stored in bf16), plus one fp32 ulp for the map's own rounding"""
    ok = _report("loss of the step", _relerr(fused[0], stock[0]), 1.5 * (allow["cls"] + allow["div"]) + ULP32)
    assert fused[1] == stock[1] and set(fused[2]) == set(stock[2]) and len(fused[2]) > 10
    worst = max(rel(fused[2][n], stock[2][n]) for n in fused[2])
    ok &= _report("student gradients (worst tensor)", worst, 1.5 * allow["dz"] + extra_dz + ULP32)
    return ok


def test_one_cpu_step_per_head():
    _cases, allow = kdhead_fixture.load()
    torch.set_num_threads(1)
    fused = step_of(CPU, "fused")
    stock = step_of(CPU, "stock")
    assert isinstance(fused[3].student_head, StudentHead) and fused[3].student_head.T == 4.0 and stock[3].student_head is None
    assert np.isfinite(fused[0]) and fused[0] > 0
    assert compare_steps(fused, stock, allow)

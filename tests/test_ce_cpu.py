"""CPU tests of the teacher trainer: the classification head's composite (helper/ce_head.py) against the golden fixture and the
float64 restatement (tests/ce_ref.py), the label rules, the parser, one epoch of the trainer with its files, the hand-over of its
checkpoint to a student run, `--resume`, and the absence of host reads between the prints of train_vanilla.

Allowance for every floating-point result: TWICE the largest distance of that kind that the reference's own fp32 results keep from
float64 over the fixture's cases, never below one fp32 ulp; the composite's float32 result adds half an ulp of its own rounding.
Predictions, hits, counts and the confusion matrix are compared exactly."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from moma_amd.helper.ce_head import CrossEntropyHead
from moma_amd.helper import loops_vanilla
from moma_amd import train_teacher as TT
from tests import ce_fixture, ce_ref as V
from tests.crd_ref import rel

CPU = torch.device("cpu")
ULP32 = 2.0 ** -23
N_CASES = ce_fixture.N_CASES


def _report(name, got, allowed):
    print(f"  {name}: {got:.3e} (allowed {allowed:.3e}, ratio {got / allowed:.2f})")
    return got <= allowed


@pytest.mark.parametrize("ci", range(N_CASES))
def test_composite_against_the_fixture(ci):
    cases, allow = ce_fixture.load()
    c = cases[ci]
    want = V.ce(c["logits"], c["labels"])
    head = CrossEntropyHead(c["K"], meter=True)
    z = torch.from_numpy(c["logits"]).requires_grad_(True)
    y = torch.from_numpy(c["labels"])
    loss = head(z, y)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * 3.0).backward()
    ok = _report("loss vs float64", abs(float(loss) - want["loss"]) / max(abs(want["loss"]), 1e-300), allow["loss"] + ULP32 / 2)
    ok &= _report("loss vs reference", abs(float(loss) - c["loss"]) / max(abs(c["loss"]), 1e-300),
                  allow["loss"] + ULP32 / 2 + c["ref_vs_f64_loss"])
    ok &= _report("dz vs float64", rel(z.grad.numpy(), 3.0 * want["dz"]), allow["dz"] + ULP32 / 2)
    ok &= _report("dz vs reference", rel(z.grad.numpy(), 3.0 * c["dz"].astype(np.float64)), allow["dz"] + ULP32 / 2 + c["ref_vs_f64_dz"])
    assert ok
    acc, mean, conf = head.read()
    s = head.stats.tolist()
    assert s[1] == want["hits"] and s[2] == want["n_valid"] and s[3] == 0
    assert np.array_equal(conf, want["conf"]) and np.array_equal(conf, c["conf"])
    assert abs(100.0 * s[1] / c["B"] - c["acc"]) < 1e-4                     # the reference's accuracy counts every row
    assert abs(s[0] - want["sum"]) <= 1e-12 * max(1.0, abs(want["sum"]))
    assert abs(mean - want["sum"] / max(want["n_valid"], 1)) <= 1e-12 * max(1.0, abs(mean)) and acc == 100.0 * s[1] / max(s[2], 1)
    # drop-in for nn.CrossEntropyLoss without the meter
    plain = CrossEntropyHead()(torch.from_numpy(c["logits"]), y)
    assert torch.equal(plain, loss.detach()) and abs(float(plain) - float(nn.CrossEntropyLoss()(torch.from_numpy(c["logits"]), y))) \
        <= (allow["loss"] + ULP32) * max(abs(c["loss"]), 1e-30)


def test_meter_sums_over_two_batches():
    cases, _allow = ce_fixture.load()
    c = cases[3]                                                            # (65, 4), cut in two; two rows of the second part ignored
    za, ya, zb, yb = c["logits"][:40], c["labels"][:40], c["logits"][40:], c["labels"][40:].copy()
    yb[[3, 7]] = V.IGNORE
    head = CrossEntropyHead(4, meter=True)
    wa, wb = V.ce(za, ya), V.ce(zb, yb)
    head(torch.from_numpy(za), torch.from_numpy(ya))
    head(torch.from_numpy(zb), torch.from_numpy(yb))
    s = head.stats.numpy()
    assert s[1] == wa["hits"] + wb["hits"] and s[2] == wa["n_valid"] + wb["n_valid"] == 63 and s[3] == 0
    assert abs(s[0] - (wa["sum"] + wb["sum"])) <= 1e-12 * s[0]
    assert np.array_equal(head.conf.numpy(), wa["conf"] + wb["conf"])
    acc, mean, conf = head.read()
    assert acc == 100.0 * s[1] / s[2] and mean == s[0] / s[2] and conf.sum() == 63
    head.reset()
    assert not head.stats.any() and not head.conf.any()
    with pytest.raises(ValueError):
        head(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))          # another number of classes than the meter's
    with pytest.raises(RuntimeError):
        CrossEntropyHead().read()


def test_ignored_rows_an_all_ignored_batch_and_a_bad_label():
    cases, allow = ce_fixture.load()
    c = cases[11]
    z0, y0 = c["logits"], c["labels"]
    head = CrossEntropyHead(5, meter=True)
    z = torch.from_numpy(z0).requires_grad_(True)
    loss = head(z, torch.from_numpy(y0))
    loss.backward()
    ign = y0 == V.IGNORE
    assert ign.sum() == 2 and not z.grad[torch.from_numpy(ign)].any() and z.grad[torch.from_numpy(~ign)].abs().sum() > 0
    keep = V.ce(z0[~ign], y0[~ign])                                         # the same batch without the ignored rows
    assert abs(float(loss) - keep["loss"]) <= (allow["loss"] + ULP32 / 2) * keep["loss"]
    assert head.stats.tolist()[1:] == [keep["hits"], 4.0, 0.0] and np.array_equal(head.conf.numpy(), keep["conf"])
    # an all-ignored batch: NaN, as torch; nothing counted
    head.reset()
    z = torch.from_numpy(z0).requires_grad_(True)
    ya = torch.full((6,), V.IGNORE, dtype=torch.int64)
    loss = head(z, ya)
    loss.backward()
    assert torch.isnan(loss) and torch.isnan(nn.CrossEntropyLoss()(torch.from_numpy(z0), ya))
    assert not z.grad.any() and not head.stats.any() and not head.conf.any()
    # a bad label: NaN loss, a zero row, stats[3] = 1, no exception; the other rows keep their gradient
    for bad in (5, -1, 1 << 40):
        head.reset()
        yb = y0.copy()
        yb[0] = bad
        z = torch.from_numpy(z0).requires_grad_(True)
        loss = head(z, torch.from_numpy(yb))
        loss.backward()
        others = V.ce(z0[1:][~ign[1:]], y0[1:][~ign[1:]])
        assert torch.isnan(loss) and not z.grad[0].any() and not z.grad[torch.from_numpy(ign)].any()
        assert rel(z.grad.numpy()[1:][~ign[1:]], others["dz"]) <= allow["dz"] + ULP32 / 2
        assert head.stats.tolist()[1:] == [others["hits"], 3.0, 1.0] and np.array_equal(head.conf.numpy(), others["conf"])
        assert np.array_equal(V.ce(z0, yb)["conf"], others["conf"]) and np.isnan(V.ce(z0, yb)["loss"])
    # float16 / float64 logits and int32 labels take the composite too
    assert CrossEntropyHead()(torch.from_numpy(z0).double(), torch.from_numpy(y0)).dtype == torch.float32
    assert torch.isfinite(CrossEntropyHead()(torch.from_numpy(z0).half(), torch.from_numpy(y0).int()))


# the reference's parser (train_teacher.py:36-90) on the line of scripts/run_vanilla.sh, name by name
RUN_VANILLA = ["--dataset", "prostate_hv", "--cosine", "--aug_train", "RA", "--pretrain", "PANDA", "--batch_size", "64", "--epochs", "50",
               "--n_cls", "4", "--image_size", "512", "--model", "effiB0", "--num_workers", "8", "--gpu_id", "0,1", "--dist-url",
               "tcp://127.0.0.1:23345", "--multiprocessing-distributed", "--trial", "0"]
REFERENCE_VALUES = dict(
    print_freq=50, batch_size=64, num_workers=8, epochs=50, gpu_id="0,1", seed=12345, trial="0", learning_rate=0.05,
    lr_decay_epochs=[30, 40, 60], lr_decay_rate=0.1, weight_decay=1e-4, momentum=0.9, cosine=True, dataset="prostate_hv", model="effiB0",
    pretrain="PANDA", pre_strict=True, aug_train="RA", crop=0.2, image_size=512, image_resize=False, n_cls=4, skip_test=False, dali=None,
    multiprocessing_distributed=True, dist_url="tcp://127.0.0.1:23345", deterministic=True, skip_validation=True)


def test_parser_equals_the_reference_on_the_run_vanilla_line(monkeypatch):
    from moma_amd import devices
    monkeypatch.setattr(devices, "visible_gpu_count", lambda: 2)
    opt = TT.parse_option(RUN_VANILLA)
    for k, v in REFERENCE_VALUES.items():
        assert getattr(opt, k) == v, k
    assert opt.model_path == "./save/vanilla/Class_ce_prostate_hv_StdPre_PANDA_strict_True_CPU8_GPU2/"
    assert opt.model_name == "Class_ce_model_effiB0_prostate_hv_IS_512_BS64_StdPre_PANDA_CPU8_GPU2_seed12345_epoch50_trial_0"
    assert opt.save_folder == os.path.join(opt.model_path, opt.model_name)
    # bare defaults, and this implementation's additions
    d = TT.parse_option([])
    assert (d.epochs, d.n_cls, d.trial, d.cosine, d.gpu_id, d.dist_url) == (60, 8, "1", False, "0", "tcp://127.0.0.1:23451")
    assert (d.amp, d.channels_last, d.dp, d.steps_per_epoch, d.miopen_find, d.reproducible, d.save_root, d.resume, d.no_fused) == \
        (None, False, None, 100, "on", False, "./save", None, False)


ARGV = ["--model", "resnet8", "--dataset", "cifar100", "--n_cls", "4", "--batch_size", "8", "--steps_per_epoch", "2", "--print_freq", "1",
        "--learning_rate", "0.05", "--skip_test", "--num_workers", "0"]


def _run(tmp, epochs, extra=()):
    opt = TT.parse_option(ARGV + ["--epochs", str(epochs), "--save_root", str(tmp), *extra])
    opt.multiprocessing_distributed, opt.world_size, opt.trace = False, 1, []
    TT.main_worker(0, 0, opt)
    return opt, [float(t) for t in opt.trace]


def test_one_epoch_writes_the_files_hands_over_to_a_student_and_resumes(tmp_path, monkeypatch):
    monkeypatch.setattr(TT, "_REQUIRE_GPU", False)
    torch.set_num_threads(1)
    opt, first = _run(tmp_path / "a", 1)
    assert len(first) == 2 and np.isfinite(first).all()
    names = set(os.listdir(opt.save_folder))
    assert {"net_best_acc.pth", "ckpt_last.pth", "ckpt_last_rank0.pth", "stat.json", "parameters.json"} <= names
    best = torch.load(os.path.join(opt.save_folder, "net_best_acc.pth"), map_location="cpu")
    assert set(best) == {"epoch", "model", "best_acc", "optimizer"} and best["epoch"] == 1            # the reference's keys
    if "net_best_f1.pth" in names:
        assert set(torch.load(os.path.join(opt.save_folder, "net_best_f1.pth"), map_location="cpu")) == {"epoch", "model", "best_f1", "optimizer"}
    stat = json.load(open(os.path.join(opt.save_folder, "stat.json")))
    assert set(stat["1"]) == {"val_cf", "val_loss", "val_acc"} and np.asarray(stat["1"]["val_cf"]).shape == (4, 4)
    assert np.asarray(stat["1"]["val_cf"]).sum() == 8
    params = json.load(open(os.path.join(opt.save_folder, "parameters.json")))
    assert params["model"] == "resnet8" and "Total params" in params and "Total time" in params
    # the checkpoint as a student run's --path_t, through load_model unchanged: the teacher is bit-equal to what was saved
    from moma_amd.train_student_moma import build_training, parse_option
    so = parse_option(["--distill", "kd", "--path_t", os.path.join(opt.save_folder, "net_best_acc.pth"), "--model_s", "resnet8",
                       "--model_t", "resnet8", "--dataset", "cifar100", "--n_cls", "4", "--batch_size", "4", "--steps_per_epoch", "1",
                       "--save_root", str(tmp_path / "s")])
    so.gpu, so.multiprocessing_distributed, so.rank, so.world_size, so.device = 0, False, 0, 1, CPU
    model_t = build_training(so, CPU)[1]
    sd = model_t.state_dict()
    assert set(sd) == set(best["model"]) and all(torch.equal(sd[k], best["model"][k]) for k in sd)
    # --resume: the second epoch's losses, exactly, against an uninterrupted run
    _o2, straight = _run(tmp_path / "b", 2)
    _o3, resumed = _run(tmp_path / "c", 2, ["--resume", os.path.join(opt.save_folder, "ckpt_last.pth")])
    assert straight[:2] == first and len(straight) == 4 and len(resumed) == 2
    assert resumed == straight[2:], (resumed, straight)
    assert straight[2:] != straight[:2]
    # --no_fused: nn.CrossEntropyLoss + accuracy, the same first step within the allowance
    _o4, stock = _run(tmp_path / "d", 1, ["--no_fused"])
    _cases, allow = ce_fixture.load()
    assert abs(stock[0] - first[0]) <= (allow["loss"] + ULP32) * first[0]


def test_cli_refuses_to_run_without_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    opt = TT.parse_option(ARGV + ["--save_root", str(tmp_path)])
    opt.multiprocessing_distributed, opt.world_size = False, 1
    with pytest.raises(RuntimeError, match="no GPU"):
        TT.main_worker(0, 0, opt)


def test_train_vanilla_reads_the_host_only_where_it_prints(monkeypatch, capsys):
    """six steps at print_freq 3: the meter is read at steps 0 and 3 and once at the end, and NO tensor's .item() / .tolist() runs
    anywhere else -- counted by patching both on torch.Tensor and read() on the head"""
    from moma_amd.backbones import model_dict
    from moma_amd.dataset.synthetic import SyntheticLoader
    torch.manual_seed(0)
    model = model_dict["resnet8"](num_classes=4)
    head = CrossEntropyHead(4, meter=True)
    opt = TT.parse_option(ARGV + ["--print_freq", "3"])
    opt.gpu, opt.multiprocessing_distributed, opt.device = 0, False, CPU
    optimizer = TT.make_optimizer(model.parameters(), opt, CPU)
    log = []
    state = {"in_read": False}
    for name in ("item", "tolist"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            log.append((_name, state["in_read"]))
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    real_read = CrossEntropyHead.read

    def read(self):
        state["in_read"] = True
        try:
            log.append(("read", True))
            return real_read(self)
        finally:
            state["in_read"] = False
    monkeypatch.setattr(CrossEntropyHead, "read", read)
    acc, loss = loops_vanilla.train_vanilla(1, SyntheticLoader(6, 4, 32, 4, 5, CPU), model, head, optimizer, opt)
    monkeypatch.undo()
    assert [e for e in log if e[0] == "read"] == [("read", True)] * 3                       # steps 0 and 3, and the end
    assert all(inside for _n, inside in log), log                                          # no host read outside read()
    assert sum(1 for n, _i in log if n == "tolist") == 3
    s = head.stats.tolist()
    assert s[2] == 24 and acc == 100.0 * s[1] / 24 and abs(loss - s[0] / 24) < 1e-12 and np.isfinite(loss)
    out = capsys.readouterr().out
    assert out.count("Epoch: [1][") == 2 and "Epoch: [1][3/6]\tGPU 0\tTime: " in out and "\tLoss " in out and "\tAcc@1 " in out


def test_validate_vanilla_matches_numpy_on_both_routes():
    from moma_amd.backbones import model_dict
    from moma_amd.dataset.synthetic import SyntheticLoader
    torch.manual_seed(1)
    model = model_dict["resnet8"](num_classes=4)
    opt = TT.parse_option(ARGV)
    opt.gpu, opt.multiprocessing_distributed, opt.device = 0, False, CPU
    loader = SyntheticLoader(3, 4, 32, 4, 9, CPU, last_batch=3)
    model.eval()
    with torch.no_grad():
        zs = [(model(x).numpy(), y.numpy()) for x, y in loader]
    want = [V.ce(z, y) for z, y in zs]
    n = sum(w["n_valid"] for w in want)
    a1, l1, s1 = loops_vanilla.validate_vanilla(loader, model, CrossEntropyHead(4, meter=True), opt, prefix="Val")
    a2, l2, s2 = loops_vanilla.validate_vanilla(loader, model, nn.CrossEntropyLoss(), opt, prefix="Val")
    assert n == 11 and a1 == a2 == 100.0 * sum(w["hits"] for w in want) / n
    assert np.array_equal(s1["conf_mat"], sum(w["conf"] for w in want)) and np.array_equal(s1["conf_mat"], s2["conf_mat"])
    mean = sum(w["sum"] for w in want) / n
    assert abs(l1 - mean) < 1e-6 * mean and abs(l2 - mean) < 1e-6 * mean and s1["acc"] == a1


def test_simkd_still_raises_in_build_training():
    from moma_amd.train_student_moma import build_training, parse_option
    opt = parse_option(["--distill", "simkd", "--model_s", "resnet8x4", "--model_t", "resnet32x4", "--dataset", "cifar100", "--n_cls", "4",
                        "--batch_size", "8", "--steps_per_epoch", "1"])
    opt.gpu, opt.multiprocessing_distributed, opt.rank, opt.world_size, opt.device = 0, False, 0, 1, CPU
    with pytest.raises(NotImplementedError):
        build_training(opt, CPU)

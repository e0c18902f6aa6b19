"""`train_teacher.py` CLI: plain cross-entropy training of one backbone -- what produces the checkpoint every `--distill` run loads
through `--path_t` (reference: train_teacher.py, launched by scripts/run_vanilla.sh as
`--dataset prostate_hv --cosine --aug_train RA --pretrain PANDA --batch_size 64 --epochs 50 --n_cls 4 --image_size 512 --model effiB0
--num_workers 8 --gpu_id 0,1 --dist-url ... --multiprocessing-distributed --trial N`).

Keeps every flag and default of the reference's argument parser (train_teacher.py:36-90; `--skip_validation` is a store_false there,
so the DEFAULT skips the initial validation -- kept), its folder and run names (:97, :106), the order of its main_worker (seed -> model
-> SGD -> criterion -> wrap -> loaders -> optional validation -> epochs of adjust_learning_rate / train / validate / test / best-acc and
best-F1 checkpoints / stat.json -> parameters.json) and the keys of its checkpoints (`epoch`, `model`, `best_acc` | `best_f1`,
`optimizer`), so `net_best_acc.pth` loads as a student run's `--path_t` through model_def.load_model unchanged.  The reference's
file imports its loops from a module that does not exist (helper.loops_RFF, :29); the two functions it wants sit in its
helper/loops_moma.py and are served here by helper/loops_vanilla.py.  What differs:
  * the criterion is helper.ce_head.CrossEntropyHead: loss, top-1 and the confusion matrix on the kernels of csrc/ce.hip with a device
    meter instead of two `.item()` reads per step; `--no_fused` restores nn.CrossEntropyLoss + helper.util.accuracy;
  * the reference's dataset lists point at author-local folders: `--data_pack PATH` trains on a pack of uint8 images (dataset/pack.py:
    `--aug_train NULL` = flip, `RRC` = random-resized-crop + flip, both inside one launch of csrc/input.hip per batch; `RA` is not
    built); without it the synthetic loader feeds batches of the same shape (`--steps_per_epoch`);
  * one process per GPU through torchrun or, as in the reference, `--multiprocessing-distributed` + spawn of fresh processes; the
    parent of the ranks counts the GPUs from sysfs (devices.visible_gpu_count) and never opens the device; the model is wrapped by
    learning/ddp.py's wrap_student (`--dp`);
  * new optional flags: --amp, --channels_last, --dp, --steps_per_epoch, --miopen_find, --reproducible (the reference's default
    cudnn.deterministic mode is opt-in here, as in train_student_moma.py), --save_root, --resume (ckpt_last.pth plus the per-rank RNG
    state, written every epoch), --no_fused;
  * checkpoints are written through a temporary name and a rename."""
from __future__ import print_function

import argparse
import os
import random
import time

from .miopen_env import use_shipped_db

use_shipped_db(tag=os.environ.get("LOCAL_RANK", ""))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from .dataset import pack  # noqa: E402
from .dataset.synthetic import SyntheticLoader  # noqa: E402
from .helper.ce_head import CrossEntropyHead  # noqa: E402
from .helper.loops_moma import macro_f1  # noqa: E402
from .helper.loops_vanilla import train_vanilla as train, validate_vanilla  # noqa: E402
from .helper.util import adjust_learning_rate, reduce_tensor, save_dict_to_json, update_dict_to_json  # noqa: E402
from .learning.base_trainer import BaseTrainer  # noqa: E402
from .model_def import load_model  # noqa: E402
from .train_student_moma import (IMAGE_SIZE, _atomic_save, _get_rng_state, _load_rank_state, _rank_state_path, _set_rng_state,  # noqa: E402
                                 make_optimizer, parent_gpu_count)

# The kernels need a GPU; the trainer's host logic also runs on the CPU (the head's composite), which the CLI refuses unless a test
# sets this module attribute to False.
_REQUIRE_GPU = True


def build_parser():
    p = argparse.ArgumentParser("argument for training")
    # basic
    p.add_argument("--print_freq", type=int, default=50, help="print frequency")
    p.add_argument("--batch_size", type=int, default=64, help="batch_size")
    p.add_argument("--num_workers", type=int, default=8, help="num_workers")
    p.add_argument("--epochs", type=int, default=60, help="number of training epochs")
    p.add_argument("--gpu_id", type=str, default="0", help="id(s) for CUDA_VISIBLE_DEVICES")
    p.add_argument("--seed", default=12345, type=int, help="seed for initializing training")
    p.add_argument("--trial", type=str, default="1", help="trial id")
    # optimization
    p.add_argument("--learning_rate", type=float, default=0.05, help="learning rate")
    p.add_argument("--lr_decay_epochs", type=str, default="30,40,60", help="where to decay lr, can be a list")
    p.add_argument("--lr_decay_rate", type=float, default=0.1, help="decay rate for learning rate")
    p.add_argument("--weight_decay", type=float, default=1e-4, help="weight decay")
    p.add_argument("--momentum", type=float, default=0.9, help="momentum")
    p.add_argument("--cosine", action="store_true", help="using cosine annealing")
    # dataset and model
    p.add_argument("--dataset", type=str, default="prostate_hv", help="dataset")
    p.add_argument("--model", type=str, default="effiB0")
    p.add_argument("--pretrain", type=str, default="PANDA", help="a local checkpoint file, or a name (random init)")
    p.add_argument("--pre_strict", action="store_false", help="strict by default")
    # augment
    p.add_argument("--aug_train", type=str, default="RA", choices=["NULL", "RA", "RRC"], help="aug_train")
    p.add_argument("--crop", type=float, default=0.2, help="crop threshold for RandomResizedCrop")
    p.add_argument("--image_size", type=int, default=512, help="image_size")
    p.add_argument("--image_resize", action="store_true")
    p.add_argument("--n_cls", type=int, default=8, help="number of classes")
    p.add_argument("--skip_test", action="store_true")
    p.add_argument("--dali", type=str, choices=["cpu", "gpu"], default=None)
    # multiprocessing
    p.add_argument("--multiprocessing-distributed", action="store_true")
    p.add_argument("--dist-url", default="tcp://127.0.0.1:23451", type=str, help="url used to set up distributed training")
    p.add_argument("--deterministic", action="store_false", help="Make results reproducible, true by default")
    p.add_argument("--skip_validation", action="store_false", help="Skip validation of teacher")
    # ---- additions of this implementation ----
    p.add_argument("--amp", default=None, choices=["bf16", "fp16"], help="autocast dtype for the backbone")
    p.add_argument("--channels_last", action="store_true")
    p.add_argument("--dp", default=None, choices=["flat", "ddp", "auto"],
                   help="model wrap at world size > 1: one flat gradient all-reduce per step (default) or stock DDP")
    p.add_argument("--steps_per_epoch", type=int, default=100, help="synthetic loader length")
    p.add_argument("--miopen_find", default="on", choices=["on", "off"],
                   help="on = cudnn.benchmark as in the reference (MIOpen find mode); off = immediate mode with the shipped find-db")
    p.add_argument("--reproducible", action="store_true",
                   help="the reference's default semantics (cudnn.deterministic with the seed, no benchmark mode)")
    p.add_argument("--save_root", type=str, default="./save")
    p.add_argument("--resume", type=str, default=None, help="checkpoint written by this trainer (ckpt_last.pth)")
    p.add_argument("--no_fused", action="store_true",
                   help="nn.CrossEntropyLoss + helper.util.accuracy, the reference's sequence, instead of the fused head")
    pack.add_arguments(p)
    return p


def parse_option(argv=None):
    opt = build_parser().parse_args(argv)
    # (the reference names the run after torch.cuda.device_count(), :97 and :106.  Counted from sysfs here: this code also runs in the
    #  parent of the ranks, which must not open the device; the HIP runtime is asked only where there is no KFD sysfs to read)
    from .devices import visible_gpu_count
    ngpu = visible_gpu_count()
    if ngpu is None:
        ngpu = torch.cuda.device_count()
    opt.model_path = os.path.join(
        opt.save_root, "vanilla",
        f"Class_ce_{opt.dataset}_StdPre_{opt.pretrain}_strict_{opt.pre_strict}_CPU{opt.num_workers}_GPU{ngpu}/")
    opt.tb_path = os.path.join(opt.save_root, "students", "tensorboard")
    opt.lr_decay_epochs = [int(it) for it in opt.lr_decay_epochs.split(",")]
    opt.model_name = (f"Class_ce_model_{opt.model}_{opt.dataset}_IS_{opt.image_size}_BS{opt.batch_size}_StdPre_{opt.pretrain}"
                      f"_CPU{opt.num_workers}_GPU{ngpu}_seed{opt.seed}_epoch{opt.epochs}_trial_{opt.trial}")
    if opt.dali is not None:
        opt.model_name += "_dali:" + opt.dali
    opt.tb_folder = os.path.join(opt.tb_path, opt.model_name)
    opt.save_folder = os.path.join(opt.model_path, opt.model_name)
    return opt


def main_worker(gpu, ngpus_per_node, opt):
    opt.gpu = int(gpu)
    opt.gpu_id = int(gpu)
    opt.rank = int(os.environ.get("GROUP_RANK", os.environ.get("NODE_RANK", 0)))
    opt.dist_backend = os.environ.get("MOMA_DIST_BACKEND", "nccl")      # 'nccl' = RCCL on ROCm (reference :151)
    if not torch.cuda.is_available() and _REQUIRE_GPU:
        raise RuntimeError("train_teacher: no GPU visible. The classification head is a HIP library for gfx950.")
    trainer = BaseTrainer(opt)
    trainer.init_ddp_environment(gpu, ngpus_per_node)
    if opt.seed is not None:                                            # (:160-171)
        random.seed(opt.seed)
        torch.manual_seed(opt.seed)
        np.random.seed(opt.seed)
    if opt.reproducible:
        if opt.seed is None:
            opt.seed = 12345
            random.seed(opt.seed); torch.manual_seed(opt.seed); np.random.seed(opt.seed)
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False
    else:
        torch.backends.cudnn.benchmark = opt.miopen_find == "on"
    device = torch.device("cuda", opt.gpu) if torch.cuda.is_available() else torch.device("cpu")
    opt.device = device
    print("opt.n_cls:", opt.n_cls)
    if opt.data_pack:
        pack.prepare(opt, IMAGE_SIZE.get(opt.dataset, opt.image_size))

    model = load_model(opt.model, opt.pretrain, opt.n_cls, opt.pre_strict, opt.gpu, opt.multiprocessing_distributed)     # (:177)
    criterion = nn.CrossEntropyLoss() if opt.no_fused else CrossEntropyHead(opt.n_cls, meter=True)                         # (:184)
    model.to(device)
    criterion.to(device)
    if opt.channels_last:
        model.to(memory_format=torch.channels_last)
    optimizer = make_optimizer(model.parameters(), opt, device)         # (:180-183; after the moves: its state follows the parameters)
    bare = model
    if opt.multiprocessing_distributed:
        from .learning.ddp import wrap_student
        model = wrap_student(bare, device_ids=[opt.gpu] if device.type == "cuda" else None, mode=opt.dp)
    if opt.amp == "fp16":
        opt._grad_scaler = torch.amp.GradScaler("cuda")

    size = IMAGE_SIZE.get(opt.dataset, opt.image_size)
    seed = (opt.seed or 0) + opt.rank
    if opt.data_pack:
        train_loader, val_loader, test_loader = pack.build_loaders(opt, size, device)
    else:
        train_loader = SyntheticLoader(opt.steps_per_epoch, opt.batch_size, size, opt.n_cls, seed, device)
        val_loader = SyntheticLoader(max(1, opt.steps_per_epoch // 10), opt.batch_size, size, opt.n_cls, seed + 1, device)
        test_loader = val_loader                                        # (the synthetic set doubles as test)
    is_main = (not opt.multiprocessing_distributed) or opt.rank % ngpus_per_node == 0
    if is_main:
        os.makedirs(opt.save_folder, exist_ok=True)
    best_acc, best_f1, t_total = 0.0, 0.0, time.time()
    start_epoch = 1
    if opt.resume:
        ck = torch.load(opt.resume, map_location=device, weights_only=False)
        bare.load_state_dict(ck["model"])
        optimizer.load_state_dict(ck["optimizer"])
        if getattr(opt, "_grad_scaler", None) is not None and ck.get("grad_scaler"):
            opt._grad_scaler.load_state_dict(ck["grad_scaler"])
        rs = _load_rank_state(os.path.dirname(opt.resume), opt.rank, ck["epoch"], device)
        if rs is not None and rs.get("rng") is not None:
            _set_rng_state(rs["rng"], device)
        best_acc, best_f1, start_epoch = ck.get("best_acc", 0.0), ck.get("best_f1", 0.0), ck["epoch"] + 1
        print("==> resumed from {} (epoch {}, per-rank state {})".format(opt.resume, ck["epoch"], "found" if rs else "absent"))

    if not opt.skip_validation:                                         # (:230-241; a store_false: the default skips it)
        teacher_acc, _avg, output_stat = validate_vanilla(test_loader, model, criterion, opt)
        print(output_stat)
        if is_main:
            print("teacher accuracy: ", teacher_acc)
    else:
        print("Skipping teacher validation.")

    for epoch in range(start_epoch, opt.epochs + 1):
        adjust_learning_rate(epoch, opt, optimizer)
        print("==> training...")
        if opt.data_pack:
            train_loader.set_epoch(epoch)
        time1 = time.time()
        train_acc, train_loss = train(epoch, train_loader, model, criterion, optimizer, opt)
        if device.type == "cuda":
            torch.cuda.synchronize()
        time2 = time.time()
        if opt.multiprocessing_distributed:
            metrics = torch.tensor([train_acc, train_loss], device=device)
            train_acc, train_loss = reduce_tensor(metrics, opt.world_size).tolist()
        if is_main:
            ips = opt.steps_per_epoch * opt.batch_size * max(1, getattr(opt, "world_size", 1)) / (time2 - time1)
            print(" * Epoch {}, Acc@1 {:.3f}, Loss {:.4f}, Time {:.2f}, {:.1f} images/sec".format(
                epoch, train_acc, train_loss, time2 - time1, ips))
        print("GPU %d validating" % (opt.gpu))
        val_acc, val_loss, val_stat = validate_vanilla(val_loader, model, criterion, opt, prefix="Val")
        test_acc = test_loss = test_stat = None
        if not opt.skip_test:
            print("GPU %d testing" % (opt.gpu))
            test_acc, test_loss, test_stat = validate_vanilla(test_loader, model, criterion, opt, prefix="Test")
        if is_main:
            print(" ** Acc_val@1 {:.3f}".format(val_acc))
            val_f1 = macro_f1(val_stat["conf_mat"])
            if test_acc is not None:
                print(" ** Acc_test@1 {:.3f}".format(test_acc))
            if val_acc > best_acc:                                      # (:306-318)
                best_acc = val_acc
                print("saving the best acc model!")
                _atomic_save({"epoch": epoch, "model": model.state_dict(), "best_acc": best_acc, "optimizer": optimizer.state_dict()},
                             os.path.join(opt.save_folder, "net_best_acc.pth"))
            if val_f1 > best_f1:                                        # (:320-332)
                best_f1 = val_f1
                print("saving the best f1 model!")
                _atomic_save({"epoch": epoch, "model": model.state_dict(), "best_f1": best_f1, "optimizer": optimizer.state_dict()},
                             os.path.join(opt.save_folder, "net_best_f1.pth"))
            metrics = {"val_cf": val_stat["conf_mat"].tolist(), "val_loss": val_loss, "val_acc": val_acc}
            if test_stat is not None:
                metrics.update(test_cf=test_stat["conf_mat"].tolist(), test_loss=test_loss, test_acc=test_acc)
            update_dict_to_json(epoch, metrics, os.path.join(opt.save_folder, "stat.json"))
            _atomic_save({"epoch": epoch, "model": bare.state_dict(), "optimizer": optimizer.state_dict(), "best_acc": best_acc,
                          "best_f1": best_f1,
                          "grad_scaler": opt._grad_scaler.state_dict() if getattr(opt, "_grad_scaler", None) is not None else None},
                         os.path.join(opt.save_folder, "ckpt_last.pth"))
        os.makedirs(opt.save_folder, exist_ok=True)
        _atomic_save({"epoch": epoch, "rng": _get_rng_state(device)}, _rank_state_path(opt.save_folder, opt.rank))
        if opt.multiprocessing_distributed and torch.distributed.is_initialized():
            torch.distributed.barrier()                         # no rank starts the next epoch before every file of this one exists
    if is_main:
        print("best accuracy:", best_acc)
        state = {k: v for k, v in vars(opt).items() if not k.startswith("_") and k != "trace"}
        state["Total params"] = sum(p.numel() for p in model.parameters()) / 1000000.0
        state["Total time"] = float("%.2f" % ((time.time() - t_total) / 3600.0))
        save_dict_to_json(state, os.path.join(opt.save_folder, "parameters.json"))
    if opt.multiprocessing_distributed and torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def main(argv=None):
    opt = parse_option(argv)
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:         # launched by torchrun: 1 process / GPU
        opt.multiprocessing_distributed = True
        opt.world_size = int(os.environ["WORLD_SIZE"])
        n_local = int(os.environ.get("LOCAL_WORLD_SIZE", opt.world_size))
        main_worker(int(os.environ.get("LOCAL_RANK", 0)), n_local, opt)
        return
    os.environ["CUDA_VISIBLE_DEVICES"] = opt.gpu_id
    if opt.multiprocessing_distributed:
        # (the reference's launch mode, :134-141.  This process only starts the ranks: it counts the devices from sysfs and never asks
        #  the HIP runtime -- see train_student_moma.main)
        import torch.multiprocessing as mp
        ngpus_per_node = parent_gpu_count(opt.gpu_id)
        opt.ngpus_per_node = ngpus_per_node
        opt.world_size = ngpus_per_node
        mp.spawn(main_worker, nprocs=ngpus_per_node, args=(ngpus_per_node, opt))
    else:
        ngpus_per_node = torch.cuda.device_count()                 # (this process IS the worker)
        opt.ngpus_per_node = ngpus_per_node
        opt.world_size = 1
        main_worker(0, ngpus_per_node, opt)


if __name__ == "__main__":
    main()

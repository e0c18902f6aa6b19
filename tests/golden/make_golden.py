#!/usr/bin/env python3
"""Generate the golden vectors in tests/golden/ by RUNNING THE REFERENCE (trinhvg/MoMA) on CPU.

Run in the build container only (needs /root/reference; the GPU box has no reference and only ever
reads the committed .npz files):

    python tests/golden/make_golden.py

What is captured:
  G1 attention   MoMA/criterion_moco_att.py:141-167   y and, for the atts_q role, dx/dW*/db*
  G2 queue       MoMA/mem_moco.py:69-100              index/out_ids/memory/logits/labels traces
  G3 ema         learning/contrast_trainer.py:207-211 momentum_update on a ragged tensor list
  G4 infonce     MoCo.forward + nn.CrossEntropyLoss   loss, dq, top-1 accuracy
  G5 step trace  helper/loops_moma.py:221-373         10 steps of train_distill_moma (resnet8 pair)
  G6 dual queue  MoMA/mem_moco.py:165-253             MoCoST / MoCoSSTT logits, queues, pointer
  G7 MoCoAtt     MoMA/mem_moco.py:103-161             cross-attention variants: logits, dq, queue
  G5b step trace helper/loops_moma.py:221-373         the same loop at K = 65536, --head mlp, d in {128, 512}
  G8 shuffle-BN + attention  learning/contrast_trainer.py:135-187   _shuffle_bn_attn, attn in {self_mix, self_nomix}
  G9 world size 2 learning/contrast_trainer.py:90-187 + MoMA/mem_moco.py:77-100   the reference's Shuffle-BN collectives (image
                 all_gather, id broadcast, key all_gather) and the global enqueue on TWO gloo ranks: per-rank k / all_k / queue
  G5c step trace helper/loops_moma.py:221-373         the loop at the BENCHMARK's batch: B = 256, K = 65536, d = 512
  G10 step trace helper/loops_moma.py:221-373         G5's loop with the CMO heads 'linear' and 'mlp_byol' (MoMA/criterion_moco_att.py:269-297)

Only arrays (inputs / expected outputs) are written; no reference source text is stored.
Shims needed to import the reference on a CPU-only box: a stub
`tensorboard_logger` module, `.cuda()` patched to identity, gloo world_size=1 process group.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import golden_npz  # noqa: E402  (fixtures above 1 MiB are written in parts)


def _shims():
    sys.path.insert(0, REF)
    sys.modules.setdefault("tensorboard_logger", types.ModuleType("tensorboard_logger"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self


def g1_attention():
    from MoMA.criterion_moco_att import Attention
    out = {}
    cases = [(8, 64, 4), (16, 128, 4), (32, 96, 8), (5, 32, 4), (1, 32, 4)]
    for ci, (n, d, h) in enumerate(cases):
        torch.manual_seed(1000 + ci)
        att = Attention(d, num_heads=h, qkv_bias=True)
        x = torch.randn(n, d, requires_grad=True)
        dy = torch.randn(n, d)
        y = att(x)
        (y * dy).sum().backward()
        p = f"c{ci}_"
        out[p + "shape"] = np.array([n, d, h], dtype=np.int64)
        out[p + "x"] = x.detach().numpy()
        out[p + "dy"] = dy.numpy()
        out[p + "w_qkv"] = att.qkv.weight.detach().numpy()
        out[p + "b_qkv"] = att.qkv.bias.detach().numpy()
        out[p + "w_proj"] = att.proj.weight.detach().numpy()
        out[p + "b_proj"] = att.proj.bias.detach().numpy()
        out[p + "y"] = y.detach().numpy()
        out[p + "dx"] = x.grad.numpy()
        out[p + "d_wqkv"] = att.qkv.weight.grad.numpy()
        out[p + "d_bqkv"] = att.qkv.bias.grad.numpy()
        out[p + "d_wproj"] = att.proj.weight.grad.numpy()
        out[p + "d_bproj"] = att.proj.bias.grad.numpy()
    out["n_cases"] = np.array(len(cases))
    golden_npz.save(os.path.join(OUT, "g1_attention.npz"), out)


def g2_queue():
    from MoMA.mem_moco import MoCo
    out = {}
    # (K, d, B, n_all, steps): K not divisible by n, n == B, n == 2B (all_k larger than k), n > K wrap
    cases = [(40, 8, 16, 16, 7), (64, 16, 8, 8, 10), (50, 8, 6, 12, 9), (10, 4, 4, 12, 3), (33, 8, 5, 5, 15)]
    for ci, (K, d, B, n, steps) in enumerate(cases):
        torch.manual_seed(2000 + ci)
        mem = MoCo(d, K, 0.15)
        p = f"c{ci}_"
        out[p + "cfg"] = np.array([K, d, B, n, steps], dtype=np.int64)
        out[p + "memory0"] = mem.memory.numpy().copy()
        idx_trace, mem_trace, logit_trace, q_trace, k_trace, allk_trace, label_trace = [], [], [], [], [], [], []
        for s in range(steps):
            q = torch.randn(B, d)
            k = torch.randn(B, d)
            all_k = k if n == B else torch.randn(n, d)
            logits, labels = mem(q, k, all_k=None if n == B else all_k)
            idx_trace.append(mem.index)
            mem_trace.append(mem.memory.numpy().copy())
            logit_trace.append(logits.numpy().copy())
            label_trace.append(labels.numpy().copy())
            q_trace.append(q.numpy()); k_trace.append(k.numpy()); allk_trace.append(all_k.numpy())
        out[p + "index"] = np.array(idx_trace, dtype=np.int64)
        out[p + "memory"] = np.stack(mem_trace)
        out[p + "logits"] = np.stack(logit_trace)
        out[p + "labels"] = np.stack(label_trace)
        out[p + "q"] = np.stack(q_trace)
        out[p + "k"] = np.stack(k_trace)
        out[p + "all_k"] = np.stack(allk_trace)
    out["n_cases"] = np.array(len(cases))
    golden_npz.save(os.path.join(OUT, "g2_queue.npz"), out)


def g3_ema():
    from learning.contrast_trainer import ContrastTrainer

    class Rag(nn.Module):
        def __init__(self):
            super().__init__()
            shapes = [(1,), (3,), (7, 5), (64,), (33, 17), (4, 3, 3, 3), (1025,), (2, 2)]
            self.ps = nn.ParameterList([nn.Parameter(torch.randn(*s)) for s in shapes])

    out = {}
    for ci, m in enumerate([0.999, 0.0, 0.5, 0.9]):
        torch.manual_seed(3000 + ci)
        a, b = Rag(), Rag()
        p = f"c{ci}_"
        out[p + "m"] = np.array(m, dtype=np.float64)
        for i, (pa, pb) in enumerate(zip(a.parameters(), b.parameters())):
            out[p + f"p{i}"] = pa.detach().numpy().copy()
            out[p + f"e{i}"] = pb.detach().numpy().copy()
        for _ in range(3):   # three successive updates
            ContrastTrainer.momentum_update(a, b, m)
        for i, pb in enumerate(b.parameters()):
            out[p + f"r{i}"] = pb.detach().numpy().copy()
        out[p + "n"] = np.array(len(list(a.parameters())))
    out["n_cases"] = np.array(4)
    golden_npz.save(os.path.join(OUT, "g3_ema.npz"), out)


def g4_infonce():
    from MoMA.mem_moco import MoCo
    from learning.contrast_trainer import ContrastTrainer
    out = {}
    cases = [(8, 64, 40), (8, 256, 64), (3, 32, 17), (16, 128, 300)]
    for ci, (B, d, K) in enumerate(cases):
        torch.manual_seed(4000 + ci)
        mem = MoCo(d, K, 0.15)
        # structured, non-degenerate inputs: correlated q/k, a few rows aligned with queue entries
        base = torch.randn(B, d)
        q = torch.nn.functional.normalize(base + 0.3 * torch.randn(B, d), dim=1)
        k = torch.nn.functional.normalize(base + 0.3 * torch.randn(B, d), dim=1)
        q = q.clone()
        q[1] = torch.nn.functional.normalize(mem.memory[3] + 0.05 * torch.randn(d), dim=0)  # top-1 miss
        q.requires_grad_(True)
        mem0 = mem.memory.numpy().copy()
        logits, labels = mem(q, k)
        crit = nn.CrossEntropyLoss()
        losses, accs = ContrastTrainer._compute_loss_accuracy(logits=[logits], target=labels, criterion=crit)
        losses[0].backward()
        p = f"c{ci}_"
        out[p + "cfg"] = np.array([B, d, K], dtype=np.int64)
        out[p + "memory0"] = mem0
        out[p + "q"] = q.detach().numpy(); out[p + "k"] = k.numpy()
        out[p + "logits"] = logits.detach().numpy()
        out[p + "loss"] = np.array(losses[0].item(), dtype=np.float64)
        out[p + "acc"] = np.array(accs[0].item(), dtype=np.float64)
        out[p + "dq"] = q.grad.numpy()
        out[p + "memory1"] = mem.memory.numpy().copy()
        out[p + "index1"] = np.array(mem.index)
    out["n_cases"] = np.array(len(cases))
    golden_npz.save(os.path.join(OUT, "g4_infonce.npz"), out)


def g6_dual_queue():
    """MoCoST / MoCoSSTT (MoMA/mem_moco.py:165-253): logits, labels, both queues and the pointer over 3 steps."""
    from MoMA.mem_moco import MoCoST, MoCoSSTT
    out = {}
    K, d, B = 48, 16, 10
    for ci, cls in enumerate([MoCoST, MoCoSSTT]):
        torch.manual_seed(6000 + ci)
        mem = cls(d, K, 0.15)
        p = f"c{ci}_"
        out[p + "cfg"] = np.array([K, d, B], dtype=np.int64)
        out[p + "ms0"] = mem.memory_s.numpy().copy(); out[p + "mt0"] = mem.memory_t.numpy().copy()
        for s in range(3):
            q, k, kt, qt = [torch.randn(B, d) for _ in range(4)]
            if cls is MoCoST:
                res = mem(q, k, kt)
            else:
                res = mem(q, k, q_t=qt, k_t=kt)
            for j, t in enumerate(res[:-1]):
                out[p + f"s{s}_logits{j}"] = t.numpy().copy()
            out[p + f"s{s}_q"] = q.numpy(); out[p + f"s{s}_k"] = k.numpy(); out[p + f"s{s}_kt"] = kt.numpy(); out[p + f"s{s}_qt"] = qt.numpy()
            out[p + f"s{s}_ms"] = mem.memory_s.numpy().copy(); out[p + f"s{s}_mt"] = mem.memory_t.numpy().copy()
            out[p + f"s{s}_index"] = np.array(mem.index)
    golden_npz.save(os.path.join(OUT, "g6_dual_queue.npz"), out)


def g7_mocoatt():
    """MoCoAtt.forward cross-attention variants (MoMA/mem_moco.py:103-161) with the CMO attention modules."""
    import argparse
    from MoMA.mem_moco import MoCoAtt
    from MoMA.criterion_moco_att import CMO
    out = {}
    K, d, B = 24, 32, 6
    variants = [("qk", "qk"), ("dual2", "dual2"), ("self_qk", "self_qk"), ("all", "all"), ("dual", "dual"), ("self", "self")]
    for ci, (cmo_attn, fw_attn) in enumerate(variants):
        torch.manual_seed(7000 + ci)
        opt = argparse.Namespace(head="None", s_dim=d, t_dim=d, feat_dim=d, attn=cmo_attn)
        kd = CMO(opt)
        mem = MoCoAtt(d, K, 0.15)
        p = f"c{ci}_"
        out[p + "attn"] = np.array(fw_attn)
        out[p + "mem0"] = mem.memory.numpy().copy()
        for name, t in kd.state_dict().items():
            out[p + "kd." + name] = t.numpy().copy()
        q = torch.nn.functional.normalize(torch.randn(B, d)).requires_grad_(True)
        k = torch.nn.functional.normalize(torch.randn(B, d))
        logits, labels = mem(q, k, attn=fw_attn, criterion_kd=kd)
        w = torch.randn_like(logits)
        (logits * w).sum().backward()
        out[p + "q"] = q.detach().numpy(); out[p + "k"] = k.numpy(); out[p + "w"] = w.numpy()
        out[p + "logits"] = logits.detach().numpy(); out[p + "dq"] = q.grad.numpy()
        out[p + "mem1"] = mem.memory.numpy().copy(); out[p + "index"] = np.array(mem.index)
    out["n_cases"] = np.array(len(variants))
    golden_npz.save(os.path.join(OUT, "g7_mocoatt.npz"), out)


def g5_step_trace():
    """10 steps of the reference loop, resnet8 student/teacher (same arch so the zip-EMA is defined,
    SURVEY Q4), B=8, 32x32, n_cls=100, K=64, head in {None, mlp}, -c 1 -d 1 -b 1, attn=self."""
    _step_trace([("None", 64), ("mlp", 32)], "g5_step_trace.npz", 0)


def g10_step_trace_heads():
    """G5's loop with the remaining CMO heads (MoMA/criterion_moco_att.py:269-297): 'linear' (a CLI choice) and 'mlp_byol'
    (Linear - BatchNorm1d - ReLU - Linear).  As the reference's train_student_moma.py:339-343 only registers embed_s with the
    optimizer (and puts embed_t in eval mode) for head == 'mlp', these heads stay at their initial weights, both BatchNorm1d
    layers stay in training mode (batch statistics, running statistics updated on every forward), and the loop's EMA leaves
    embed_t alone (helper/loops_moma.py:310-312): the fixture also records the heads' final state."""
    _step_trace([("linear", 32), ("mlp_byol", 32)], "g10_step_trace_heads.npz", 100)


def _step_trace(cases, fname, seed_off):
    import argparse
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    import helper.loops_moma as L
    from models.resnet import resnet8
    from MoMA.mem_moco import build_mem
    from MoMA.criterion_moco_att import CMO
    from learning.contrast_trainer import ContrastTrainer
    from distiller_zoo import DistillKL

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29631")
        dist.init_process_group("gloo", rank=0, world_size=1)

    out = {}
    for ci0, (head, feat_dim) in enumerate(cases):
        ci = ci0 + seed_off                                 # (seeds; the keys are numbered from 0 in every file)
        opt = argparse.Namespace(
            distill="moma", head=head, feat_dim=feat_dim, attn="self", mem="MoCo", nce_k=64, nce_t=0.15,
            alpha=0.999, cls=1.0, div=1.0, beta=1.0, kd_T=4.0, gpu=None, multiprocessing_distributed=True,
            print_freq=1000, batch_size=8, local_rank=0, node_rank=0, ngpus_per_node=1, rank=0, world_size=1)
        torch.manual_seed(5000 + ci)
        model_s = resnet8(num_classes=100)
        model_t = resnet8(num_classes=100)
        opt.s_dim = opt.t_dim = 64
        if head == "None":
            opt.feat_dim = opt.s_dim
        contrast = build_mem(opt)
        criterion_kd = CMO(opt)
        trainer = ContrastTrainer(opt)
        trainer.local_group = dist.new_group([0])
        module_list = nn.ModuleList([model_s])
        trainable = nn.ModuleList([model_s])
        trainable.append(criterion_kd.atts_q)
        trainable.append(criterion_kd.atts_k)
        trainable.append(criterion_kd.atts_queue)
        if head == "mlp":
            trainable.append(criterion_kd.embed_s)
        optimizer = torch.optim.SGD(trainable.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        p = f"c{ci0}_"
        for name, t in model_s.state_dict().items():
            out[p + "s." + name] = t.numpy().copy()
        for name, t in model_t.state_dict().items():
            out[p + "t." + name] = t.numpy().copy()
        for name, t in criterion_kd.state_dict().items():
            out[p + "kd." + name] = t.numpy().copy()
        out[p + "memory0"] = contrast.memory.numpy().copy()
        ddp_s = DDP(model_s)
        mods = nn.ModuleList([ddp_s, model_t])
        crits = nn.ModuleList([nn.CrossEntropyLoss(), DistillKL(opt.kd_T), criterion_kd])

        steps_per_epoch, epochs = 5, 2
        g = torch.Generator().manual_seed(777 + ci)
        images = torch.randn(steps_per_epoch * epochs, 8, 3, 32, 32, generator=g)
        labels = torch.randint(0, 100, (steps_per_epoch * epochs, 8), generator=g)
        out[p + "data_seed"] = np.array(777 + ci)
        out[p + "images_sum"] = np.array(images.double().sum().item())
        out[p + "labels"] = labels.numpy()

        rec = {"loss": [], "acc": [], "index": [], "memsum": []}

        class RecMeter(L.AverageMeter):
            pass

        # record per-step loss / acc through the meters the loop updates (helper/loops_moma.py:351-356)
        orig_update = L.AverageMeter.update
        calls = {"n": 0}

        def upd(self, val, n=1):
            k = calls["n"] % 3
            if k == 0:
                rec["loss"].append(val)
            elif k == 1:
                rec["acc"].append(val)
            calls["n"] += 1
            return orig_update(self, val, n)

        L.AverageMeter.update = upd
        torch.manual_seed(9000 + ci)      # RNG stream for the per-step randperm of _shuffle_bn
        out[p + "loop_seed"] = np.array(9000 + ci)
        try:
            for ep in range(epochs):
                loader = [(images[ep * steps_per_epoch + i], labels[ep * steps_per_epoch + i])
                          for i in range(steps_per_epoch)]

                class Rec(list):
                    pass
                # run one batch at a time inside an epoch by wrapping the loader to record queue state
                def gen():
                    for it in loader:
                        yield it
                        rec["index"].append(contrast.index)
                        rec["memsum"].append(contrast.memory.double().sum().item())

                class LL:
                    def __len__(self): return steps_per_epoch
                    def __iter__(self): return gen()
                L.train_distill_moma(ep + 1, LL(), mods, crits, trainer, contrast, optimizer, opt)
        finally:
            L.AverageMeter.update = orig_update
        out[p + "loss"] = np.array(rec["loss"], dtype=np.float64)
        out[p + "acc"] = np.array(rec["acc"], dtype=np.float64)
        out[p + "index"] = np.array(rec["index"], dtype=np.int64)
        out[p + "memsum"] = np.array(rec["memsum"], dtype=np.float64)
        out[p + "memory_final"] = contrast.memory.numpy().copy()
        out[p + "atts_k_grad_none"] = np.array(all(q.grad is None for q in criterion_kd.atts_k.parameters()))
        out[p + "atts_queue_grad_none"] = np.array(all(q.grad is None for q in criterion_kd.atts_queue.parameters()))
        for name, t in model_s.state_dict().items():
            if name.endswith("fc.weight") or name.endswith("conv1.weight"):
                out[p + "s_final." + name] = t.numpy().copy()
        for name, t in model_t.state_dict().items():
            if name.endswith("fc.weight"):
                out[p + "t_final." + name] = t.numpy().copy()
        out[p + "kd_final.atts_q.proj.weight"] = criterion_kd.atts_q.proj.weight.detach().numpy().copy()
        out[p + "kd_final.atts_k.proj.weight"] = criterion_kd.atts_k.proj.weight.detach().numpy().copy()
        out[p + "head"] = np.array(head)
        if seed_off:                                        # G10: the heads' final state (weights untouched, BN statistics moved)
            for name, t in criterion_kd.state_dict().items():
                if name.startswith("embed_"):
                    out[p + "kd_final." + name] = t.numpy().copy()
    out["n_cases"] = np.array(len(cases))
    golden_npz.save(os.path.join(OUT, fname), out)


def g8_shuffle_bn_attn():
    """ContrastTrainer._shuffle_bn_attn (learning/contrast_trainer.py:135-187) at world size 1 for attn = 'self_mix' (one
    module over [q ; k]) and 'self_nomix' (atts_q / atts_k): outputs (q, k, all_k) and the gradients that flow back through
    the attention into q and into the module weights (the attention runs OUTSIDE no_grad here, on q and on k)."""
    import argparse
    import torch.distributed as dist
    from models.resnet import resnet8
    from MoMA.criterion_moco_att import CMO
    from learning.contrast_trainer import ContrastTrainer

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29631")
        dist.init_process_group("gloo", rank=0, world_size=1)
    out = {}
    B = 12
    for ci, (attn, head, d) in enumerate([("self_mix", "None", 64), ("self_nomix", "None", 64), ("self_mix", "mlp", 32)]):
        torch.manual_seed(8000 + ci)
        opt = argparse.Namespace(head=head, s_dim=64, t_dim=64, feat_dim=d, attn=attn, local_rank=0, node_rank=0,
                                 ngpus_per_node=1, rank=0, world_size=1)
        model_t = resnet8(num_classes=10)
        model_t.train()
        kd = CMO(opt)
        trainer = ContrastTrainer(opt)
        trainer.local_group = dist.new_group([0])
        x = torch.randn(B, 3, 32, 32)
        q = torch.nn.functional.normalize(torch.randn(B, d)).requires_grad_(True)
        w1, w2, w3 = torch.randn(B, d), torch.randn(B, d), torch.randn(B, d)
        p = f"c{ci}_"
        out[p + "attn"] = np.array(attn); out[p + "head"] = np.array(head); out[p + "d"] = np.array(d)
        for name, t in model_t.state_dict().items():
            out[p + "t." + name] = t.numpy().copy()
        for name, t in kd.state_dict().items():
            out[p + "kd." + name] = t.numpy().copy()
        torch.manual_seed(8100 + ci)                       # the randperm stream
        out[p + "perm_seed"] = np.array(8100 + ci)
        q2, k, all_k = trainer._shuffle_bn_attn(x, model_t, kd.embed_t, kd, q)
        ((q2 * w1).sum() + (k * w2).sum() + (all_k * w3).sum()).backward()
        out[p + "x"] = x.numpy(); out[p + "q"] = q.detach().numpy()
        out[p + "w1"] = w1.numpy(); out[p + "w2"] = w2.numpy(); out[p + "w3"] = w3.numpy()
        out[p + "q_out"] = q2.detach().numpy(); out[p + "k_out"] = k.detach().numpy(); out[p + "all_k"] = all_k.detach().numpy()
        out[p + "dq"] = q.grad.numpy().copy()
        for name, prm in kd.named_parameters():
            if prm.grad is not None:
                out[p + "grad." + name] = prm.grad.numpy().copy()
        for name, t in model_t.state_dict().items():       # BN running statistics moved by the train-mode forward
            if "running_mean" in name:
                out[p + "t_after." + name] = t.numpy().copy()
    out["n_cases"] = np.array(3)
    golden_npz.save(os.path.join(OUT, "g8_shuffle_bn_attn.npz"), out)


def seeded_uniform_(t, gen, bound):
    """t <- U(-bound, bound) from a dedicated generator (reproducible in the tests without shipping the tensor)."""
    with torch.no_grad():
        t.copy_((torch.rand(t.shape, generator=gen) * 2 - 1) * bound)


def g5b_step_trace_big():
    """The loop at the sizes the benchmark's kernels run at: K = 65536, --head mlp, feat_dim in {128, 512}, resnet8 pair,
    B = 8, 10 steps.  The big tensors (queue 65536 x d, attention weights) are NOT stored: they are drawn from dedicated
    seeded generators (same distribution as the reference's default init: normalised randn rows / U(-1/sqrt(fan_in), ..))
    that the tests re-run; stored are the small weights, per-step total loss AND per-step loss_kd, the pointer trace,
    the enqueued rows of the final queue and a few checksums."""
    import argparse
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    import helper.loops_moma as L
    from models.resnet import resnet8
    from MoMA.mem_moco import build_mem
    from MoMA.criterion_moco_att import CMO
    from learning.contrast_trainer import ContrastTrainer
    from distiller_zoo import DistillKL

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29631")
        dist.init_process_group("gloo", rank=0, world_size=1)
    torch.set_num_threads(8)
    out = {}
    K = 65536
    cases = [(128, 0.05), (512, 0.05), (512, 0.002)]          # (feat_dim, lr): at lr 0.05 loss_kd collapses to 0 within 4 steps
    for ci, (feat_dim, lr) in enumerate(cases):
        opt = argparse.Namespace(
            distill="moma", head="mlp", feat_dim=feat_dim, attn="self", mem="MoCo", nce_k=K, nce_t=0.15,
            alpha=0.999, cls=1.0, div=1.0, beta=1.0, kd_T=4.0, gpu=None, multiprocessing_distributed=True,
            print_freq=1000, batch_size=8, local_rank=0, node_rank=0, ngpus_per_node=1, rank=0, world_size=1)
        torch.manual_seed(5100 + ci)
        model_s = resnet8(num_classes=100)
        model_t = resnet8(num_classes=100)
        opt.s_dim = opt.t_dim = 64
        contrast = build_mem(opt)
        criterion_kd = CMO(opt)
        # big tensors from dedicated generators (re-drawn by the tests)
        gq = torch.Generator().manual_seed(5200 + ci)
        with torch.no_grad():
            contrast.memory.copy_(torch.nn.functional.normalize(torch.randn(K, feat_dim, generator=gq)))
        gw = torch.Generator().manual_seed(5300 + ci)
        for name in ("atts_q", "atts_k", "atts_queue"):
            att = getattr(criterion_kd, name)
            for lin in (att.qkv, att.proj):
                b = 1.0 / np.sqrt(lin.in_features)
                seeded_uniform_(lin.weight, gw, b)
                seeded_uniform_(lin.bias, gw, b)
        p = f"c{ci}_"
        out[p + "feat_dim"] = np.array(feat_dim)
        out[p + "seeds"] = np.array([5200 + ci, 5300 + ci])
        trainer = ContrastTrainer(opt)
        trainer.local_group = dist.new_group([0])
        trainable = nn.ModuleList([model_s, criterion_kd.atts_q, criterion_kd.atts_k, criterion_kd.atts_queue,
                                   criterion_kd.embed_s])
        optimizer = torch.optim.SGD(trainable.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
        out[p + "lr"] = np.array(lr)
        for name, t in model_s.state_dict().items():
            out[p + "s." + name] = t.numpy().copy()
        for name, t in model_t.state_dict().items():
            out[p + "t." + name] = t.numpy().copy()
        for name, t in criterion_kd.state_dict().items():
            if name.startswith("embed_"):
                out[p + "kd." + name] = t.numpy().copy()
        out[p + "memory0_sum"] = np.array(contrast.memory.double().sum().item())
        out[p + "memory0_row7"] = contrast.memory[7].numpy().copy()
        out[p + "attsq_qkv_w_sum"] = np.array(criterion_kd.atts_q.qkv.weight.double().sum().item())
        ddp_s = DDP(model_s)
        mods = nn.ModuleList([ddp_s, model_t])
        crits = nn.ModuleList([nn.CrossEntropyLoss(), DistillKL(opt.kd_T), criterion_kd])
        steps_per_epoch, epochs = 5, 2
        g = torch.Generator().manual_seed(787 + ci)
        images = torch.randn(steps_per_epoch * epochs, 8, 3, 32, 32, generator=g)
        labels = torch.randint(0, 100, (steps_per_epoch * epochs, 8), generator=g)
        out[p + "data_seed"] = np.array(787 + ci)
        rec = {"loss": [], "loss_kd": [], "index": []}
        orig_update = L.AverageMeter.update
        calls = {"n": 0}

        def upd(self, val, n=1):
            if calls["n"] % 3 == 0:
                rec["loss"].append(val)
            calls["n"] += 1
            return orig_update(self, val, n)

        orig_cla = ContrastTrainer._compute_loss_accuracy

        def cla(logits, target, criterion):          # helper/loops_moma.py:332-335 -> the step's loss_kd
            losses, accs = orig_cla(logits=logits, target=target, criterion=criterion)
            rec["loss_kd"].append(float(losses[0].item()))
            return losses, accs

        L.AverageMeter.update = upd
        trainer._compute_loss_accuracy = cla
        torch.manual_seed(9100 + ci)
        out[p + "loop_seed"] = np.array(9100 + ci)
        try:
            for ep in range(epochs):
                loader = [(images[ep * steps_per_epoch + i], labels[ep * steps_per_epoch + i])
                          for i in range(steps_per_epoch)]

                def gen():
                    for it in loader:
                        yield it
                        rec["index"].append(contrast.index)

                class LL:
                    def __len__(self): return steps_per_epoch
                    def __iter__(self): return gen()
                L.train_distill_moma(ep + 1, LL(), mods, crits, trainer, contrast, optimizer, opt)
        finally:
            L.AverageMeter.update = orig_update
        out[p + "loss"] = np.array(rec["loss"], dtype=np.float64)
        out[p + "loss_kd"] = np.array(rec["loss_kd"], dtype=np.float64)
        out[p + "index"] = np.array(rec["index"], dtype=np.int64)
        out[p + "memory_rows_final"] = contrast.memory[:80].numpy().copy()        # the 10 x 8 enqueued rows
        out[p + "memory_final_sum"] = np.array(contrast.memory.double().sum().item())
        out[p + "kd_final.atts_q.proj.weight_8x8"] = criterion_kd.atts_q.proj.weight.detach()[:8, :8].numpy().copy()
        out[p + "kd_final.atts_q.qkv.bias_16"] = criterion_kd.atts_q.qkv.bias.detach()[:16].numpy().copy()
        out[p + "t_final.fc.weight"] = model_t.state_dict()["fc.weight"].numpy().copy()
        out[p + "s_final.fc.weight"] = model_s.state_dict()["fc.weight"].numpy().copy()
    out["n_cases"] = np.array(len(cases))
    golden_npz.save(os.path.join(OUT, "g5b_step_trace_big.npz"), out)


def _g9_worker(rank, world, port, path):
    """One of the two gloo ranks of G9: the reference's _shuffle_bn / _shuffle_bn_attn + MoCo.forward, 3 steps each."""
    import argparse
    import torch.distributed as dist
    _shims()
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from models.resnet import resnet8
    from MoMA.mem_moco import MoCo
    from MoMA.criterion_moco_att import CMO
    from learning.contrast_trainer import ContrastTrainer
    B, K, d, steps = 6, 40, 32, 3
    out = {"B": np.array(B), "K": np.array(K), "d": np.array(d), "steps": np.array(steps), "world": np.array(world)}
    for ci, attn in enumerate(["self", "self_nomix", "self_mix"]):
        p = f"c{ci}_"
        opt = argparse.Namespace(head="mlp", s_dim=64, t_dim=64, feat_dim=d, attn=attn, mem="MoCo", nce_k=K, nce_t=0.15,
                                 local_rank=rank, node_rank=0, ngpus_per_node=world, rank=rank, world_size=world)
        torch.manual_seed(9900 + ci)                           # identical weights / queue on both ranks
        model_t = resnet8(num_classes=10)
        model_t.train()
        kd = CMO(opt)
        contrast = MoCo(d, K, 0.15)
        trainer = ContrastTrainer(opt)
        trainer.local_group = dist.new_group(list(range(world)))
        g = torch.Generator().manual_seed(9910 + 10 * ci + rank)   # this rank's images and queries
        xs = torch.randn(steps, B, 3, 32, 32, generator=g)
        qs = torch.nn.functional.normalize(torch.randn(steps, B, d, generator=g), dim=2)
        torch.manual_seed(9950 + 10 * ci + rank)               # host randperm stream (rank 0's permutation is broadcast)
        if rank == 0:
            out[p + "attn"] = np.array(attn)
            for name, t in model_t.state_dict().items():
                out[p + "t." + name] = t.numpy().copy()
            for name, t in kd.state_dict().items():
                out[p + "kd." + name] = t.numpy().copy()
            out[p + "memory0"] = contrast.memory.numpy().copy()
            out[p + "perm_seed_rank0"] = np.array(9950 + 10 * ci)
        r = f"{p}r{rank}_"
        out[r + "x"] = xs.numpy(); out[r + "q"] = qs.numpy()
        ks, aks, qouts, logits, idx, mems = [], [], [], [], [], []
        for t in range(steps):
            if attn == "self":
                k, all_k = trainer._shuffle_bn(xs[t], model_t, kd.embed_t)
                q = qs[t]
            else:
                with torch.no_grad():
                    q, k, all_k = trainer._shuffle_bn_attn(xs[t], model_t, kd.embed_t, kd, qs[t])
            lg, _lab = contrast(q=q, k=k, all_k=all_k)
            ks.append(k.detach().numpy().copy()); aks.append(all_k.detach().numpy().copy())
            qouts.append(q.detach().numpy().copy()); logits.append(lg.detach().numpy().copy())
            idx.append(contrast.index); mems.append(contrast.memory.numpy().copy())
        out[r + "k"] = np.stack(ks); out[r + "all_k"] = np.stack(aks); out[r + "q_out"] = np.stack(qouts)
        out[r + "logits"] = np.stack(logits); out[r + "index"] = np.array(idx, dtype=np.int64); out[r + "memory"] = np.stack(mems)
        out[r + "t_after.bn1.running_mean"] = model_t.state_dict()["bn1.running_mean"].numpy().copy()
    np.savez_compressed(f"{path}.rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def g9_gather_w2():
    """The reference's W > 1 behaviour that the per-rank build replaces and `--shuffle_bn gather` reproduces
    (learning/contrast_trainer.py:90-133 and :135-187, MoMA/mem_moco.py:77-100): two gloo ranks, 3 steps per case."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    path = os.path.join(OUT, "_g9_tmp")
    mp.spawn(_g9_worker, args=(2, port, path), nprocs=2, join=True)
    out = {}
    for r in range(2):
        f = f"{path}.rank{r}.npz"
        with np.load(f) as z:
            for k in z.files:
                out[k] = z[k]
        os.remove(f)
    out["n_cases"] = np.array(3)
    golden_npz.save(os.path.join(OUT, "g9_gather_w2.npz"), out)


def g5c_step_trace_b256():
    """The loop at the benchmark's per-rank batch (B = 256: two 128-row blocks in the one-pass K2, eight key tiles per K1
    workgroup), K = 65536, --head mlp, d = 512, lr = 0.002, 5 steps.  As in G5b the big tensors (queue, attention weights,
    images) are re-drawn from seeds by the tests; stored: small weights, per-step loss / loss_kd, pointer, a sample of the
    enqueued rows and checksums."""
    import argparse
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    import helper.loops_moma as L
    from models.resnet import resnet8
    from MoMA.mem_moco import build_mem
    from MoMA.criterion_moco_att import CMO
    from learning.contrast_trainer import ContrastTrainer
    from distiller_zoo import DistillKL

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29631")
        dist.init_process_group("gloo", rank=0, world_size=1)
    torch.set_num_threads(8)
    out = {}
    K, B, steps, feat_dim, lr = 65536, 256, 5, 512, 0.002
    opt = argparse.Namespace(
        distill="moma", head="mlp", feat_dim=feat_dim, attn="self", mem="MoCo", nce_k=K, nce_t=0.15,
        alpha=0.999, cls=1.0, div=1.0, beta=1.0, kd_T=4.0, gpu=None, multiprocessing_distributed=True,
        print_freq=1000, batch_size=B, local_rank=0, node_rank=0, ngpus_per_node=1, rank=0, world_size=1)
    torch.manual_seed(5400)
    model_s = resnet8(num_classes=100)
    model_t = resnet8(num_classes=100)
    opt.s_dim = opt.t_dim = 64
    contrast = build_mem(opt)
    criterion_kd = CMO(opt)
    gq = torch.Generator().manual_seed(5500)
    with torch.no_grad():
        contrast.memory.copy_(torch.nn.functional.normalize(torch.randn(K, feat_dim, generator=gq)))
    gw = torch.Generator().manual_seed(5600)
    for name in ("atts_q", "atts_k", "atts_queue"):
        att = getattr(criterion_kd, name)
        for lin in (att.qkv, att.proj):
            b = 1.0 / np.sqrt(lin.in_features)
            seeded_uniform_(lin.weight, gw, b)
            seeded_uniform_(lin.bias, gw, b)
    p = "c0_"
    out[p + "feat_dim"] = np.array(feat_dim); out[p + "B"] = np.array(B); out[p + "steps"] = np.array(steps)
    out[p + "seeds"] = np.array([5500, 5600]); out[p + "lr"] = np.array(lr)
    trainer = ContrastTrainer(opt)
    trainer.local_group = dist.new_group([0])
    trainable = nn.ModuleList([model_s, criterion_kd.atts_q, criterion_kd.atts_k, criterion_kd.atts_queue, criterion_kd.embed_s])
    optimizer = torch.optim.SGD(trainable.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    for name, t in model_s.state_dict().items():
        out[p + "s." + name] = t.numpy().copy()
    for name, t in model_t.state_dict().items():
        out[p + "t." + name] = t.numpy().copy()
    for name, t in criterion_kd.state_dict().items():
        if name.startswith("embed_"):
            out[p + "kd." + name] = t.numpy().copy()
    out[p + "memory0_sum"] = np.array(contrast.memory.double().sum().item())
    out[p + "memory0_row7"] = contrast.memory[7].numpy().copy()
    out[p + "attsq_qkv_w_sum"] = np.array(criterion_kd.atts_q.qkv.weight.double().sum().item())
    mods = nn.ModuleList([DDP(model_s), model_t])
    crits = nn.ModuleList([nn.CrossEntropyLoss(), DistillKL(opt.kd_T), criterion_kd])
    g = torch.Generator().manual_seed(797)
    images = torch.randn(steps, B, 3, 32, 32, generator=g)
    labels = torch.randint(0, 100, (steps, B), generator=g)
    out[p + "data_seed"] = np.array(797)
    out[p + "images_sum"] = np.array(images.double().sum().item())
    rec = {"loss": [], "loss_kd": [], "index": []}
    orig_update = L.AverageMeter.update
    calls = {"n": 0}

    def upd(self, val, n=1):
        if calls["n"] % 3 == 0:
            rec["loss"].append(val)
        calls["n"] += 1
        return orig_update(self, val, n)

    orig_cla = ContrastTrainer._compute_loss_accuracy

    def cla(logits, target, criterion):          # helper/loops_moma.py:332-335 -> the step's loss_kd
        losses, accs = orig_cla(logits=logits, target=target, criterion=criterion)
        rec["loss_kd"].append(float(losses[0].item()))
        return losses, accs

    L.AverageMeter.update = upd
    trainer._compute_loss_accuracy = cla
    torch.manual_seed(9200)
    out[p + "loop_seed"] = np.array(9200)
    try:
        loader = [(images[i], labels[i]) for i in range(steps)]

        def gen():
            for it in loader:
                yield it
                rec["index"].append(contrast.index)

        class LL:
            def __len__(self): return steps
            def __iter__(self): return gen()
        L.train_distill_moma(1, LL(), mods, crits, trainer, contrast, optimizer, opt)
    finally:
        L.AverageMeter.update = orig_update
    out[p + "loss"] = np.array(rec["loss"], dtype=np.float64)
    out[p + "loss_kd"] = np.array(rec["loss_kd"], dtype=np.float64)
    out[p + "index"] = np.array(rec["index"], dtype=np.int64)
    rows = np.concatenate([np.arange(0, 32), np.arange(B * steps - 32, B * steps)])      # first and last enqueued rows
    out[p + "memory_rows_ids"] = rows
    out[p + "memory_rows_final"] = contrast.memory[rows].numpy().copy()
    out[p + "memory_final_sum"] = np.array(contrast.memory.double().sum().item())
    out[p + "kd_final.atts_q.proj.weight_8x8"] = criterion_kd.atts_q.proj.weight.detach()[:8, :8].numpy().copy()
    out[p + "t_final.fc.weight"] = model_t.state_dict()["fc.weight"].numpy().copy()
    out[p + "s_final.fc.weight"] = model_s.state_dict()["fc.weight"].numpy().copy()
    out["n_cases"] = np.array(1)
    golden_npz.save(os.path.join(OUT, "g5c_step_trace_b256.npz"), out)


if __name__ == "__main__":
    _shims()
    torch.set_num_threads(1)          # deterministic reduction order for the captured vectors
    which = sys.argv[1:] or ["g1", "g2", "g3", "g4", "g5", "g6", "g7", "g5b", "g8", "g9", "g5c", "g10"]
    gens = {"g1": g1_attention, "g2": g2_queue, "g3": g3_ema, "g4": g4_infonce, "g5": g5_step_trace, "g6": g6_dual_queue,
            "g7": g7_mocoatt, "g5b": g5b_step_trace_big, "g8": g8_shuffle_bn_attn, "g9": g9_gather_w2, "g5c": g5c_step_trace_b256,
            "g10": g10_step_trace_heads}
    for name in ["g1", "g2", "g3", "g4", "g5", "g6", "g7", "g5b", "g8", "g9", "g5c", "g10"]:
        if name in which:
            # every generator starts from ONE thread: g5b / g5c raise the count for their big matrix products (their vectors
            # were captured that way) and must not leak it into the generators that run after them (round 3: the default
            # all-in-one run reproduced G10 only to 9e-5, alone bit for bit)
            torch.set_num_threads(1)
            gens[name]()
    for f in sorted(os.listdir(OUT)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(OUT, f)))

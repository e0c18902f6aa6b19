"""Pin the CPU step oracle (oracle/step_oracle.py) against the 10-step trace captured from the reference's
own train_distill_moma (tests/golden/g5_step_trace.npz): loss per step, queue pointer (bit exact), queue
contents, grad=None on atts_k / atts_queue, final weights.  This is BASELINE.json configs[0]-style plumbing
(CIFAR-shaped inputs, B=8, CPU), with a same-arch resnet8 pair so the reference's zip-EMA is defined."""
import os

import numpy as np
import pytest
import torch

from oracle.step_oracle import OracleCMO, OracleMoCo, StepOracle
from moma_amd.backbones.resnet_cifar import resnet8
from tests import golden_npz


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


@pytest.mark.parametrize("fixture,ci", [("g5_step_trace.npz", 0), ("g5_step_trace.npz", 1),
                                        # G10: the remaining CMO heads ('linear', 'mlp_byol'), which the reference leaves untrained
                                        ("g10_step_trace_heads.npz", 0), ("g10_step_trace_heads.npz", 1)])
def test_step_trace_matches_reference(golden_dir, fixture, ci):
    torch.set_num_threads(1)
    g = golden_npz.load(os.path.join(golden_dir, fixture))
    p = f"c{ci}_"
    head = str(g[p + "head"])
    feat_dim = 64 if head == "None" else 32
    ms, mt = resnet8(num_classes=100), resnet8(num_classes=100)
    ms.load_state_dict(_sd(g, p + "s."))
    mt.load_state_dict(_sd(g, p + "t."))
    cmo = OracleCMO(head, 64, 64, feat_dim)
    cmo.load_state_dict(_sd(g, p + "kd."))
    contrast = OracleMoCo(feat_dim, 64, 0.15)
    contrast.memory.copy_(torch.from_numpy(g[p + "memory0"]))
    run = StepOracle(ms, mt, cmo, contrast, head=head)

    gen = torch.Generator().manual_seed(int(g[p + "data_seed"]))
    images = torch.randn(10, 8, 3, 32, 32, generator=gen)
    labels = torch.randint(0, 100, (10, 8), generator=gen)
    assert abs(images.double().sum().item() - float(g[p + "images_sum"])) < 1e-6, "torch RNG stream changed"
    assert np.array_equal(labels.numpy(), g[p + "labels"])

    torch.manual_seed(int(g[p + "loop_seed"]))
    losses, accs, idxs, memsums = [], [], [], []
    for ep in range(2):
        run.start_epoch()
        for i in range(5):
            s = ep * 5 + i
            loss, acc, _ = run.step(images[s], labels[s])
            losses.append(loss); accs.append(acc)
            idxs.append(contrast.index); memsums.append(contrast.memory.double().sum().item())
    assert idxs == [int(v) for v in g[p + "index"]]                      # pointer: bit exact
    np.testing.assert_allclose(losses, g[p + "loss"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(accs, g[p + "acc"], atol=1e-4)
    np.testing.assert_allclose(memsums, g[p + "memsum"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(contrast.memory.numpy(), g[p + "memory_final"], rtol=1e-4, atol=1e-5)
    assert bool(g[p + "atts_k_grad_none"]) and all(q.grad is None for q in cmo.atts_k.parameters())
    assert bool(g[p + "atts_queue_grad_none"]) and all(q.grad is None for q in cmo.atts_queue.parameters())
    np.testing.assert_allclose(ms.fc.weight.detach().numpy(), g[p + "s_final.fc.weight"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(mt.fc.weight.detach().numpy(), g[p + "t_final.fc.weight"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(cmo.atts_q.proj.weight.detach().numpy(), g[p + "kd_final.atts_q.proj.weight"],
                               rtol=1e-4, atol=1e-5)
    # atts_k is in the optimizer but never gets a gradient -> not even weight decay touches it
    assert np.array_equal(cmo.atts_k.proj.weight.detach().numpy(), g[p + "kd_final.atts_k.proj.weight"])
    if fixture.startswith("g10"):
        # heads other than 'mlp' are not registered with the optimizer (reference train_student_moma.py:339-343): weights as
        # initialised; the BatchNorm1d layers of 'mlp_byol' stay in training mode and their running statistics move
        final = _sd(g, p + "kd_final.")
        for name, t in cmo.state_dict().items():
            if not name.startswith("embed_"):
                continue
            if "running" in name or "num_batches" in name:
                np.testing.assert_allclose(t.numpy(), final[name].numpy(), rtol=1e-4, atol=1e-6)
                assert not np.array_equal(final[name].numpy(), g[p + "kd." + name])
            else:
                assert np.array_equal(t.numpy(), final[name].numpy()) and np.array_equal(t.numpy(), g[p + "kd." + name])


def test_step_trace_big_queue_matches_reference(golden_dir):
    """The same loop at the benchmark's KD sizes (K = 65536, --head mlp, d = 512; G5b, lr 0.002 case): per-step total
    loss AND per-step loss_kd, pointer, the enqueued rows of the final queue."""
    from tests.g5b_util import K_BIG, batches, big_queue, fill_attention_, sd
    torch.set_num_threads(8)
    g = golden_npz.load(os.path.join(golden_dir, "g5b_step_trace_big.npz"))
    ci = 2
    p = f"c{ci}_"
    d = int(g[p + "feat_dim"])
    ms, mt = resnet8(num_classes=100), resnet8(num_classes=100)
    ms.load_state_dict(sd(g, p + "s.")); mt.load_state_dict(sd(g, p + "t."))
    cmo = OracleCMO("mlp", 64, 64, d)
    fill_attention_(cmo, g, p)
    contrast = OracleMoCo(d, K_BIG, 0.15)
    contrast.memory.copy_(big_queue(g, p, d))
    run = StepOracle(ms, mt, cmo, contrast, head="mlp", lr=float(g[p + "lr"]))
    images, labels = batches(g, p)
    torch.manual_seed(int(g[p + "loop_seed"]))
    losses, kds, idxs = [], [], []
    for ep in range(2):
        run.start_epoch()
        for i in range(5):
            loss, _, kd = run.step(images[ep * 5 + i], labels[ep * 5 + i])
            losses.append(loss); kds.append(kd); idxs.append(contrast.index)
    assert idxs == [int(v) for v in g[p + "index"]]
    np.testing.assert_allclose(losses, g[p + "loss"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(kds, g[p + "loss_kd"], rtol=2e-5, atol=1e-4)
    np.testing.assert_allclose(contrast.memory[:80].numpy(), g[p + "memory_rows_final"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(cmo.atts_q.proj.weight.detach()[:8, :8].numpy(), g[p + "kd_final.atts_q.proj.weight_8x8"],
                               rtol=1e-4, atol=1e-6)


def test_step_trace_bench_batch_matches_reference(golden_dir):
    """The loop at the benchmark's per-rank batch (G5c: B = 256, K = 65536, --head mlp, d = 512, lr 0.002, 5 steps): the oracle
    against the reference's own per-step total loss and loss_kd, the pointer and a sample of the enqueued rows."""
    from tests.g5b_util import K_BIG, batches, big_queue, fill_attention_, sd
    torch.set_num_threads(8)
    g = golden_npz.load(os.path.join(golden_dir, "g5c_step_trace_b256.npz"))
    p = "c0_"
    d, B, steps = int(g[p + "feat_dim"]), int(g[p + "B"]), int(g[p + "steps"])
    ms, mt = resnet8(num_classes=100), resnet8(num_classes=100)
    ms.load_state_dict(sd(g, p + "s.")); mt.load_state_dict(sd(g, p + "t."))
    cmo = OracleCMO("mlp", 64, 64, d)
    fill_attention_(cmo, g, p)
    contrast = OracleMoCo(d, K_BIG, 0.15)
    contrast.memory.copy_(big_queue(g, p, d))
    run = StepOracle(ms, mt, cmo, contrast, head="mlp", lr=float(g[p + "lr"]))
    images, labels = batches(g, p, steps, B)
    torch.manual_seed(int(g[p + "loop_seed"]))
    losses, kds, idxs = [], [], []
    run.start_epoch()
    for i in range(steps):
        loss, _, kd = run.step(images[i], labels[i])
        losses.append(loss); kds.append(kd); idxs.append(contrast.index)
    assert idxs == [int(v) for v in g[p + "index"]]
    np.testing.assert_allclose(losses, g[p + "loss"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(kds, g[p + "loss_kd"], rtol=2e-5, atol=1e-4)
    np.testing.assert_allclose(contrast.memory[torch.from_numpy(g[p + "memory_rows_ids"])].numpy(), g[p + "memory_rows_final"],
                               rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_shuffle_bn_attn_oracle_matches_reference(golden_dir, ci):
    """oracle/step_oracle.py:shuffle_bn_attn against the vectors captured from the reference's _shuffle_bn_attn (G8)."""
    import torch.nn as nn
    from oracle.step_oracle import OracleAttention, _head, shuffle_bn_attn
    torch.set_num_threads(1)
    g = golden_npz.load(os.path.join(golden_dir, "g8_shuffle_bn_attn.npz"))
    p = f"c{ci}_"
    attn, head, d = str(g[p + "attn"]), str(g[p + "head"]), int(g[p + "d"])
    mt = resnet8(num_classes=10)
    mt.load_state_dict(_sd(g, p + "t."))
    mt.train()

    class C(nn.Module):
        def __init__(self):
            super().__init__()
            self.embed_s, self.embed_t = _head(head, 64, d), _head(head, 64, d)
            if attn == "self_mix":
                self.atts = OracleAttention(d)
            else:
                self.atts_q, self.atts_k = OracleAttention(d), OracleAttention(d)
    cmo = C()
    cmo.load_state_dict(_sd(g, p + "kd."))
    q = torch.from_numpy(g[p + "q"]).requires_grad_(True)
    torch.manual_seed(int(g[p + "perm_seed"]))
    q2, k, all_k = shuffle_bn_attn(torch.from_numpy(g[p + "x"]), mt, cmo.embed_t, cmo, q, attn)
    ((q2 * torch.from_numpy(g[p + "w1"])).sum() + (k * torch.from_numpy(g[p + "w2"])).sum()
     + (all_k * torch.from_numpy(g[p + "w3"])).sum()).backward()
    np.testing.assert_allclose(q2.detach().numpy(), g[p + "q_out"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(k.detach().numpy(), g[p + "k_out"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(all_k.detach().numpy(), g[p + "all_k"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(q.grad.numpy(), g[p + "dq"], rtol=1e-4, atol=1e-6)
    for name, prm in cmo.named_parameters():
        if prm.grad is not None:
            np.testing.assert_allclose(prm.grad.numpy(), g[p + "grad." + name], rtol=1e-4, atol=1e-5)

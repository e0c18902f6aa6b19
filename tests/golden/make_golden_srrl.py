#!/usr/bin/env python3
"""Generate tests/golden/g20_srrl*.npz by RUNNING THE REFERENCE's SRRL (models/util.py) + nn.MSELoss + an nn.Linear classifier on the
CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_srrl.py

Cases (B, t_n, n_cls, s_n, note): the smallest legal shape, small ragged shapes, odd rows (no 16-byte access), a batch past one wave,
channels that divide nothing, classes across a tile edge, the widest classifier, a small case with inputs offset by +3, and the
benchmark's regime (1280 channels).  Where t_n <= 16 the whole chain runs: SRRL.forward on a student feature [B, s_n].  The wider cases
are tail-only: the reference's own BatchNorm2d -> ReLU of `transfer`, the classifier and both MSELoss run on a drawn [B, t_n] map
without the convolution (hundreds of outputs from a handful of inputs leave no student feature with every element clear of the kink:
tests/golden/make_golden_hint.py, its 1280-channel case).  SRRL and the classifier are built under torch.manual_seed(2000 + case): the
convolution's and the classifier's weights are what their initialisation draws; gamma and beta are the hint fixture's `affine` (every
third gamma negative).  The inputs (student feature, teacher feature, teacher logits) are standard normal draws (numpy, seed
2000 + case) rounded to multiples of 1/32 and clipped to |.| <= 4 (exact in bf16), then moved clear of the ReLU's kink
(tests/srrl_ref.clear; for the chain: the input a near element depends on most is moved by +1/8 until none is left).

Per case: the inputs, the convolution's weight, the classifier, gamma, beta, the convolution's output and its gradient, the loss, the
gradients of the student feature, the convolution's weight, gamma and beta, the running statistics after the step, and the distances
of those fp32 results from float64: `ref_vs_f64_loss / _dx / _dgamma / _dbeta / _rmean / _rvar` from the restatement of the tail
(tests/srrl_ref.py) on the reference's own convolution output -- what the kernels are handed; `_chain_loss / _dxs / _dw` from the same
modules run in float64.  The loss distances are relative to the loss, the others in crd_ref.rel's metric.  Only arrays are written;
no reference source text."""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import golden_npz, srrl_ref as V  # noqa: E402
from tests.crd_ref import rel  # noqa: E402
from tests.golden.make_golden_hint import affine, draw  # noqa: E402

CASES = [  # (B, t_n, n_cls, s_n (0: tail only), note)
    (2, 1, 1, 2, ""),
    (2, 3, 2, 4, ""),
    (3, 8, 5, 6, ""),
    (5, 5, 3, 7, ""),
    (65, 3, 4, 2, ""),
    (2, 130, 7, 0, ""),
    (7, 72, 33, 0, ""),
    (3, 24, 1000, 0, ""),
    (3, 8, 5, 6, "+3"),
    (4, 1280, 4, 0, ""),
]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clear_inputs(conv64, f, gamma, beta, eps):
    """move the student feature until no element of the convolution's float64 output is within TAU of the kink"""
    f = torch.from_numpy(f.astype(np.float64))
    for _ in range(1000):
        fg = f.clone().requires_grad_(True)
        z = conv64(fg[:, :, None, None])[:, :, 0, 0]
        near = np.abs(V.pre_activation(z.detach().numpy(), gamma, beta, eps)) < V.TAU
        if not near.any():
            return f.numpy().astype(np.float32)
        g = torch.autograd.grad((z * torch.from_numpy(near)).sum(), fg)[0].abs()      # (no gradient is left on the module)
        f = f + 0.125 * (g >= 0.5 * g.max())
    raise RuntimeError("no input clear of the kink found")


def main():
    SRRL = _load(os.path.join(REF, "models", "util.py"), "ref_models_util").SRRL
    crit = nn.MSELoss()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (Bn, t_n, n_cls, s_n, note) in enumerate(CASES):
        tail_only = s_n == 0
        torch.manual_seed(2000 + ci)
        mod = SRRL(s_n=s_n if s_n else 1, t_n=t_n)
        cls_t = nn.Linear(t_n, n_cls)
        conv, bn, relu = mod.transfer[0], mod.transfer[1], mod.transfer[2]
        w0 = conv.weight.detach().numpy().copy()
        Wc, bc = cls_t.weight.detach().numpy().copy(), cls_t.bias.detach().numpy().copy()
        gamma, beta = affine(t_n)
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(gamma))
            bn.bias.copy_(torch.from_numpy(beta))
        eps, mom = bn.eps, bn.momentum
        rng = np.random.default_rng(2000 + ci)
        off = 3.0 if note == "+3" else 0.0
        f_s = draw(rng, (Bn, max(s_n, 1)), off)
        t, l = draw(rng, (Bn, t_n), off), draw(rng, (Bn, n_cls))
        mod64, cls64 = copy.deepcopy(mod).double(), copy.deepcopy(cls_t).double()
        mod.train(); mod64.train()
        if tail_only:
            z_in = V.clear(draw(rng, (Bn, t_n)), gamma, beta, eps).astype(np.float32)
            tz = torch.from_numpy(z_in).requires_grad_(True)
            trans = relu(bn(tz[:, :, None, None])).view(Bn, -1)
            pred = cls_t(trans)
            loss = crit(trans, torch.from_numpy(t)) + crit(pred, torch.from_numpy(l))
            loss.backward()
            z, dz = z_in, tz.grad.numpy().copy()
        else:
            f_s = clear_inputs(mod64.transfer[0], f_s, gamma, beta, eps)
            kept = {}
            hook = conv.register_forward_hook(lambda _m, _i, o: (o.retain_grad(), kept.update(z=o))[0])
            tf = torch.from_numpy(f_s).requires_grad_(True)
            trans, pred = mod(tf, cls_t)
            loss = crit(trans, torch.from_numpy(t)) + crit(pred, torch.from_numpy(l))
            loss.backward()
            hook.remove()
            z, dz = kept["z"].detach().numpy().reshape(Bn, t_n).copy(), kept["z"].grad.numpy().reshape(Bn, t_n).copy()
        alone = V.tail(z, t, Wc, bc, l, gamma, beta, eps, 1.0, np.zeros(t_n), np.ones(t_n), mom)
        assert not (np.abs(V.pre_activation(z, gamma, beta, eps)) < V.TAU / 2).any()
        res = {"loss": np.array(loss.item(), np.float32), "d_conv_out": dz, "trans": trans.detach().numpy().copy(),
               "pred": pred.detach().numpy().copy(),
               "d_gamma": bn.weight.grad.numpy().copy(), "d_beta": bn.bias.grad.numpy().copy(),
               "running_mean": bn.running_mean.numpy().copy(), "running_var": bn.running_var.numpy().copy()}
        d = {"loss": abs(float(loss.item()) - alone["loss"]) / alone["loss"], "dx": rel(dz, alone["dx"]),
             "dgamma": rel(res["d_gamma"], alone["d_gamma"]), "dbeta": rel(res["d_beta"], alone["d_beta"]),
             "rmean": rel(res["running_mean"], alone["running_mean"]), "rvar": rel(res["running_var"], alone["running_var"])}
        if not tail_only:
            tf64 = torch.from_numpy(f_s.astype(np.float64)).requires_grad_(True)
            tr64, pr64 = mod64(tf64, cls64)
            loss64 = crit(tr64, torch.from_numpy(t.astype(np.float64))) + crit(pr64, torch.from_numpy(l.astype(np.float64)))
            loss64.backward()
            dw = conv.weight.grad.numpy().copy()
            res.update(dx_s=tf.grad.numpy().copy(), dw=dw)
            d.update(chain_loss=abs(float(loss.item()) - float(loss64.item())) / float(loss64.item()),
                     dxs=rel(res["dx_s"], tf64.grad.numpy()), dw=rel(dw, mod64.transfer[0].weight.grad.numpy()))
        p = f"c{ci}_"
        out[p + "shape"] = np.array((Bn, t_n, n_cls, s_n), np.int64)
        out[p + "tail_only"] = np.array(int(tail_only))
        if not tail_only:
            out[p + "f_s"], out[p + "w"] = f_s, w0
        out[p + "t"], out[p + "l"], out[p + "W"], out[p + "b"] = t, l, Wc, bc
        out[p + "gamma"], out[p + "beta"], out[p + "conv_out"] = gamma, beta, z
        out[p + "eps"], out[p + "momentum"] = np.array(eps, np.float64), np.array(mom, np.float64)
        out[p + "state_keys"] = np.array(list(mod.state_dict()))
        for k_, v_ in res.items():
            assert np.isfinite(v_).all(), k_
            out[p + k_] = v_
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} B {Bn} t_n {t_n} n_cls {n_cls} s_n {s_n} {note}: loss {loss.item():.6e}  "
              + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g20_srrl.npz"), out))


if __name__ == "__main__":
    main()

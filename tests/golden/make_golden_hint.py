#!/usr/bin/env python3
"""Generate tests/golden/g18_hint*.npz by RUNNING THE REFERENCE's ConvReg (models/util.py) + HintLoss (distiller_zoo/FitNet.py) on the
CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_hint.py

Cases (student shape, teacher shape, note): nine on a common grid (the 1 x 1 branch) -- M = 2, the smallest legal shape, small ragged
shapes, P = 49, inputs offset by +3, a plane that crosses one chunk boundary, a batch of 65, a channel count that divides nothing, the
head map's regime (1280 channels, teacher through max(., 0); there the reference's bn -> relu -> MSE run on a drawn map without the
convolution: 1280 outputs per pixel from 16 inputs leave no student map with every element clear of the kink) -- and one for each
other branch of ConvReg (s_H = 2 t_H, 2 s_H = t_H, s_H > t_H, s_H < t_H with the teacher pooled).  ConvReg is built under torch.manual_seed(1800 + case): the convolution's weight and
bias are what its initialisation draws; gamma and beta are set to non-trivial values (every third gamma negative).  The inputs are
standard normal draws (numpy, seed 1800 + case) rounded to multiples of 1/32 and clipped to |.| <= 4 (exact in bf16), then moved clear
of the ReLU's kink (tests/hint_ref.py: every element of the convolution's output whose float64 |pre-activation| is below 2^-10 has the
input it depends on most moved by +1/8, until none is left).

Per case: the inputs, the convolution's weight and bias, gamma, beta, the convolution's output and its gradient, the loss, the gradients
of the student map, the weight, the bias, gamma and beta, the running statistics after the step, and the distances of those fp32
results from float64: `ref_vs_f64_loss / _dx / _dgamma / _dbeta / _rmean / _rvar` from the restatement of the tail (tests/hint_ref.py)
on the reference's own convolution output -- what the kernels are handed; `_chain_loss / _dxs / _dw` from the same modules run in
float64 (which tests/test_hint_cpu.py ties to the restatement of the whole chain on the 1 x 1 cases).  The loss distances are relative
to the loss (a sum of squares: nothing cancels), the others in crd_ref.rel's metric.  `db_noise` is the reference's bias gradient
(analytically 0) in units of the largest weight-gradient entry.  Only arrays are written; no reference source text."""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import hint_ref as V, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (student [B, C, H, W], teacher [B, C, H, W], note)
    ((2, 1, 1, 1), (2, 1, 1, 1), ""),
    ((2, 4, 4, 4), (2, 3, 4, 4), ""),
    ((3, 6, 7, 7), (3, 8, 7, 7), ""),
    ((2, 3, 3, 5), (2, 5, 3, 5), ""),
    ((2, 8, 9, 9), (2, 16, 9, 9), "+3"),
    ((1, 5, 33, 33), (1, 4, 33, 33), ""),
    ((65, 2, 2, 2), (65, 3, 2, 2), ""),
    ((2, 7, 6, 6), (2, 130, 6, 6), ""),
    ((4, 16, 2, 2), (4, 1280, 2, 2), "relu"),
    ((2, 3, 8, 8), (2, 4, 4, 4), "down"),
    ((2, 3, 4, 4), (2, 4, 8, 8), "up"),
    ((2, 3, 7, 7), (2, 4, 5, 5), "valid"),
    ((2, 3, 5, 5), (2, 4, 8, 8), "pool_t"),
]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def affine(C):
    c = np.arange(C)
    gamma = 0.5 + ((c * 7) % 5) * 0.25
    gamma[c % 3 == 1] *= -1.0
    beta = ((c * 3) % 4 - 1.5) * 0.2
    return gamma.astype(np.float32), beta.astype(np.float32)


def draw(rng, shape, off=0.0):
    return (np.clip(np.round(rng.standard_normal(shape) * 32) / 32, -4, 4) + off).astype(np.float32)


def clear_inputs(reg64, x, gamma, beta, eps):
    """move the student map until no element of the convolution's float64 output is within TAU of the kink"""
    x = torch.from_numpy(x.astype(np.float64))
    for _ in range(1000):
        xg = x.clone().requires_grad_(True)
        z = reg64.conv(xg)
        near = np.abs(V.pre_activation(z.detach().numpy(), gamma, beta, eps)) < V.TAU
        if not near.any():
            return x.numpy().astype(np.float32)
        g = torch.autograd.grad((z * torch.from_numpy(near)).sum(), xg)[0].abs()      # (no gradient is left on the module)
        x = x + 0.125 * (g >= 0.5 * g.max())
    raise RuntimeError("no input clear of the kink found")


def main():
    ConvReg = _load(os.path.join(REF, "models", "util.py"), "ref_models_util").ConvReg
    HintLoss = _load(os.path.join(REF, "distiller_zoo", "FitNet.py"), "ref_fitnet").HintLoss
    out = {"n_cases": np.array(len(CASES))}
    for ci, (ss, ts, note) in enumerate(CASES):
        torch.manual_seed(1800 + ci)
        reg = ConvReg(ss, ts)
        crit = HintLoss()
        w0, b0 = reg.conv.weight.detach().numpy().copy(), reg.conv.bias.detach().numpy().copy()
        gamma, beta = affine(ts[1])
        with torch.no_grad():
            reg.bn.weight.copy_(torch.from_numpy(gamma))
            reg.bn.bias.copy_(torch.from_numpy(beta))
        eps, mom = reg.bn.eps, reg.bn.momentum
        rng = np.random.default_rng(1800 + ci)
        off = 3.0 if note == "+3" else 0.0
        x, t = draw(rng, ss, off), draw(rng, ts, off)
        if note == "relu":
            t = np.maximum(t, 0)
        reg64 = copy.deepcopy(reg).double()
        reg.train(); reg64.train()
        tail_only = note == "relu"
        if tail_only:
            # 1280 outputs per pixel from 16 inputs: no student map keeps all of them clear of the kink.  The case is about the
            # tail on the head map's shape: the reference's bn -> relu -> MSE on a drawn, cleared map; the convolution is not run
            z_in = V.clear_of_kink(draw(rng, ts), gamma, beta, eps).astype(np.float32)
            tz = torch.from_numpy(z_in).requires_grad_(True)
            f_s, f_t = reg.relu(reg.bn(tz)), torch.from_numpy(t)
            loss = crit(f_s, f_t)
            loss.backward()
            z, dz = z_in, tz.grad.numpy().copy()
        else:
            x = clear_inputs(reg64, x, gamma, beta, eps)
            kept = {}
            hook = reg.conv.register_forward_hook(lambda _m, _i, o: (o.retain_grad(), kept.update(z=o))[0])
            tx = torch.from_numpy(x).requires_grad_(True)
            f_s, f_t = reg(tx, torch.from_numpy(t))
            loss = crit(f_s, f_t)
            loss.backward()
            hook.remove()
            z, dz = kept["z"].detach().numpy().copy(), kept["z"].grad.numpy().copy()
        t_grid = f_t.detach().numpy().copy()                         # (pooled where the case pools)
        # the tail alone, from the reference's own convolution output: what the kernels are handed
        alone = V.tail(z, t_grid, gamma, beta, eps, 1.0, np.zeros(ts[1]), np.ones(ts[1]), mom)
        assert not (np.abs(V.pre_activation(z, gamma, beta, eps)) < V.TAU / 2).any()
        # the whole chain in float64, by the same modules
        res = {"loss": np.array(loss.item(), np.float32), "d_conv_out": dz,
               "d_gamma": reg.bn.weight.grad.numpy().copy(), "d_beta": reg.bn.bias.grad.numpy().copy(),
               "running_mean": reg.bn.running_mean.numpy().copy(), "running_var": reg.bn.running_var.numpy().copy()}
        # (the running mean carries the bias: the tail's own is taken on z, which includes it)
        d = {"loss": abs(float(loss.item()) - alone["loss"]) / alone["loss"], "dx": rel(dz, alone["dx"]),
             "dgamma": rel(res["d_gamma"], alone["d_gamma"]), "dbeta": rel(res["d_beta"], alone["d_beta"]),
             "rmean": rel(res["running_mean"], alone["running_mean"]), "rvar": rel(res["running_var"], alone["running_var"])}
        db_noise = 0.0
        if not tail_only:
            tx64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
            f64 = reg64(tx64, torch.from_numpy(t.astype(np.float64)))
            loss64 = crit(*f64)
            loss64.backward()
            dw, db = reg.conv.weight.grad.numpy().copy(), reg.conv.bias.grad.numpy().copy()
            res.update(dx_s=tx.grad.numpy().copy(), dw=dw, db=db)
            d.update(chain_loss=abs(float(loss.item()) - float(loss64.item())) / float(loss64.item()),
                     dxs=rel(res["dx_s"], tx64.grad.numpy()), dw=rel(dw, reg64.conv.weight.grad.numpy()))
            db_noise = np.abs(db).max() / max(np.abs(dw).max(), 1e-300)
        p = f"c{ci}_"
        out[p + "s_shape"], out[p + "t_shape"] = np.array(ss, np.int64), np.array(ts, np.int64)
        out[p + "tail_only"] = np.array(int(tail_only))
        if not tail_only:
            out[p + "x"] = x
        out[p + "t"], out[p + "t_grid"], out[p + "w"], out[p + "b"] = t, t_grid, w0, b0
        out[p + "gamma"], out[p + "beta"], out[p + "conv_out"] = gamma, beta, z
        out[p + "eps"], out[p + "momentum"] = np.array(eps, np.float64), np.array(mom, np.float64)
        out[p + "db_noise"] = np.array(db_noise, np.float64)
        out[p + "state_keys"] = np.array(list(reg.state_dict()))
        for k_, v_ in res.items():
            assert np.isfinite(v_).all(), k_
            out[p + k_] = v_
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {ss} -> {ts} {note}: loss {loss.item():.6e}  db_noise {float(out[p + 'db_noise']):.1e}  "
              + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g18_hint.npz"), out))


if __name__ == "__main__":
    main()

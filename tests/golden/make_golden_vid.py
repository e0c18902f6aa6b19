#!/usr/bin/env python3
"""Generate tests/golden/g17_vid*.npz by RUNNING THE REFERENCE's VIDLoss criterion (distiller_zoo/VID.py) on the CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_vid.py

Cases (B, Cs, Ct, H, W, note): the smallest shape, small ragged shapes, a rectangular grid, both sides offset by +3, a log_scale
spread over [-3, 8] (`ls`), a student map of twice the grid (`pool_s`: the input is pooled in front of the regressor), a teacher map
of twice the grid (`pool_t`), a batch of 65 with two channels, channel counts that are no multiple of anything, and the regime of the
head map (`relu`: both sides through max(., 0), 1280 target channels).  The criterion is VIDLoss(Cs, min(Ct, 48), Ct) built under
torch.manual_seed(1700 + case): the weights are what its initialisation draws (the middle width is capped so that the 1280-channel
case stays a fixture and not a model file).  The inputs are standard normal draws (numpy, seed 1700 + case) rounded to multiples of
1/32.  log_scale stays inside [-3, 8]: further down the reference's fp32 softplus alone is 1e-3 away from float64.

Per case: the input, the target, the three weights, log_scale, the regressor's output pred_mean and its gradient, the loss, the
gradients of the input, the weights and log_scale, and the distances of those fp32 results from the float64 restatement
(tests/vid_ref.py): `ref_vs_f64_loss` in units of abs_terms = 0.5 (mean d^2 / var + mean_c |log var_c|) (the loss is a cancelling
sum where var < 1), `ref_vs_f64_dmean / _dls / _dx / _dw` in crd_ref.rel's metric (_dw: the largest of the three).  Large tensors are
stored image by image (tests/vid_fixture.py puts them together).  Only arrays are written; no reference source text."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import vid_ref as V, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (B, Cs, Ct, H, W, note)
    (1, 1, 1, 1, 1, ""),
    (2, 3, 5, 4, 4, ""),
    (3, 8, 8, 7, 7, ""),
    (2, 5, 4, 3, 5, ""),
    (2, 16, 24, 9, 9, "+3"),
    (4, 24, 24, 16, 16, "ls"),
    (2, 40, 40, 8, 8, "pool_s"),
    (2, 12, 12, 4, 4, "pool_t"),
    (65, 3, 2, 2, 2, ""),
    (2, 130, 257, 6, 6, ""),
    (4, 64, 1280, 4, 4, "relu"),
]
MID_CAP = 48


def main():
    sys.path.insert(0, REF)
    from distiller_zoo.VID import VIDLoss
    out = {"n_cases": np.array(len(CASES))}
    for ci, (B, Cs, Ct, H, W, note) in enumerate(CASES):
        torch.manual_seed(1700 + ci)
        mid = min(Ct, MID_CAP)
        crit = VIDLoss(Cs, mid, Ct)
        rng = np.random.default_rng(1700 + ci)
        off = 3.0 if note == "+3" else 0.0
        ks, kt = (2 if note == "pool_s" else 1), (2 if note == "pool_t" else 1)
        x = (np.round(rng.standard_normal((B, Cs, H * ks, W * ks)) * 32) / 32 + off).astype(np.float32)
        t = (np.round(rng.standard_normal((B, Ct, H * kt, W * kt)) * 32) / 32 + off).astype(np.float32)
        if note == "relu":
            x, t = np.maximum(x, 0), np.maximum(t, 0)
        if note == "ls":
            with torch.no_grad():
                crit.log_scale.copy_(torch.linspace(-3, 8, Ct))
        tx, tt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(t)
        kept = {}
        hook = crit.regressor.register_forward_hook(lambda _m, _i, o: (o.retain_grad(), kept.update(pm=o))[0])
        loss = crit(tx, tt)
        loss.backward()
        hook.remove()
        ws = [crit.regressor[i].weight.detach().numpy().reshape(crit.regressor[i].weight.shape[:2]).copy() for i in (0, 2, 4)]
        dws = [crit.regressor[i].weight.grad.numpy().reshape(crit.regressor[i].weight.shape[:2]).copy() for i in (0, 2, 4)]
        ls, dls = crit.log_scale.detach().numpy().copy(), crit.log_scale.grad.numpy().copy()
        pm, dpm, dx = kept["pm"].detach().numpy().copy(), kept["pm"].grad.numpy().copy(), tx.grad.numpy().copy()
        want = V.criterion(x, t, ws, ls, crit.eps)
        # the likelihood alone, from the reference's own pred_mean: what the kernels are handed
        alone = V.nll(pm, want["target"], ls, crit.eps)
        d = {"loss": abs(float(loss.item()) - alone["loss"]) / alone["abs_terms"], "dmean": rel(dpm, alone["d_mean"]),
             "dls": rel(dls, alone["d_ls"]), "dx": rel(dx, want["dx"]), "dw": max(rel(a, b) for a, b in zip(dws, want["dw"])),
             "chain_loss": abs(float(loss.item()) - want["loss"]) / want["abs_terms"]}
        p = f"c{ci}_"
        out[p + "shape"] = np.array([B, Cs, Ct, H, W, mid, ks, kt], dtype=np.int64)
        for b in range(B):                           # one array per image: a part of the fixture stays below a committed file's limit
            out[f"{p}x_b{b}"], out[f"{p}target_b{b}"], out[f"{p}dx_b{b}"] = x[b], t[b], dx[b]
            out[f"{p}pred_mean_b{b}"], out[f"{p}d_pred_mean_b{b}"] = pm[b], dpm[b]
        for i in range(3):
            out[f"{p}w{i}"], out[f"{p}dw{i}"] = ws[i], dws[i]
        out[p + "log_scale"], out[p + "d_log_scale"] = ls, dls
        out[p + "loss"] = np.array(loss.item(), np.float32)
        out[p + "eps"] = np.array(crit.eps, np.float64)
        assert all(np.isfinite(v).all() for v in (pm, dpm, dx, dls, *dws)) and np.isfinite(loss.item())
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {CASES[ci]}: loss {loss.item():.6e}  " + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g17_vid.npz"), out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/g19_semckd*.npz by RUNNING THE REFERENCE's SelfA (models/util.py) + SemCKDLoss (distiller_zoo/SemCKD.py) on
the CPU in fp32, and again in float64.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_semckd.py

Cases (B; student (C, H)...; teacher (C, H)...), maps square: three general ones (grids that pool either side, a 130-channel teacher,
a 4 x 4 group), one 1 x 1 group (the softmax is identically 1: the head's gradient is 0) and one with B // 4 = 1 (the l2-normalised
embedding is +-1: the head's weight gradients are analytically 0 and the reference returns rounding noise there).  SelfA is built
under torch.manual_seed(seed), soft = 1; the inputs are standard normal draws (numpy, the same seed) rounded to multiples of 1/32 and
clipped to |.| <= 4 (exact in bf16).  SemCKDLoss calls .cuda(): torch.Tensor.cuda is patched to the identity for that call, and the
loss's formula applied to SelfA's outputs gives `ind` (the two losses are asserted to agree).

The ReLU's kink: the maker measures `kink_margin`, the smallest float64 |pre-activation| over every ReLU of the module (two per
projection, one per head), and takes the next seed until it is at least 2^-10 -- where that can happen.  The general cases have
about 1e5 pre-activations of unit scale each, so about 1e5 x 0.8 x 2^-10 = 80 of them lie that close to 0 under ANY seed; for a
case that no seed of the first 8 clears at 2^-10 the maker takes the first seed whose margin is at least 2^-18 (eight times the
rounding error of an fp32 pre-activation of unit scale: the fp32 and the float64 run still take the same branch everywhere) and
records the margin it got.

Per case: the inputs, the seed, the state dict before the step (tensors above 65536 elements as two checksums), s_value and target
of every pair with the gradient that reaches the s_value, weight, ind, loss, the gradients of the student maps, of weight, of regressor00's first weight and of query_0.linear1.weight, the
state-dict key list, and the distances of those fp32 results from float64: `ref_vs_f64_loss / _ind / _dsv / _dw` from the restatement
of the tail (tests/semckd_ref.py) on the reference's own s_value, target and weight -- what the kernels are handed; `_chain_loss /
_weight / _dxs / _dproj / _dhead` from the same modules run in float64.  The loss distances are relative to the loss, the others in
crd_ref.rel's metric.  `head_noise` is the head's weight gradient in units of the largest entry of the projection's.  Only arrays are
written; no reference source text."""
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
from tests import semckd_ref as V, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (B, student (C, H)..., teacher (C, H)...)
    (8, [(3, 8), (5, 4)], [(4, 8), (6, 4), (7, 2)]),
    (9, [(2, 6), (3, 3)], [(3, 5), (130, 3)]),
    (12, [(3, 9), (4, 5), (6, 3), (16, 2)], [(3, 9), (4, 5), (6, 3), (20, 2)]),
    (8, [(3, 4)], [(2, 7)]),
    (4, [(3, 8), (5, 4)], [(4, 8), (6, 4), (7, 2)]),
]
TAU, TAU_FLOOR, TRIES_AT_TAU, TRIES = 2.0 ** -10, 2.0 ** -18, 8, 64
STATE_FULL = 1 << 16


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw(rng, shape):
    return np.clip(np.round(rng.standard_normal(shape) * 32) / 32, -4, 4).astype(np.float32)


def run(mod, crit, fs, ft, dtype):
    """one forward + backward of the reference's modules -> dict of numpy arrays"""
    xs = [torch.from_numpy(f).to(dtype).requires_grad_(True) for f in fs]
    ts = [torch.from_numpy(f).to(dtype) for f in ft]
    margin = [np.inf]
    hooks = [m.register_forward_pre_hook(lambda _m, a: margin.__setitem__(0, min(margin[0], float(a[0].detach().abs().min()))))
             for m in mod.modules() if isinstance(m, nn.ReLU)]
    s_value, target, weight = mod(xs, ts)
    for h in hooks:
        h.remove()
    weight.retain_grad()
    for row in s_value:
        for y in row:
            y.retain_grad()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        loss_ref = crit(s_value, target, weight)
    finally:
        torch.Tensor.cuda = real_cuda
    B, S, T = weight.shape
    ind = torch.stack([torch.stack([((s_value[i][j] - target[i][j]) ** 2).reshape(B, -1).mean(-1) for j in range(T)], 1)
                       for i in range(S)], 1)
    loss = (weight * ind).sum() / (1.0 * B * S)
    assert abs(float(loss) - float(loss_ref)) <= 1e-6 * abs(float(loss)), (float(loss), float(loss_ref))
    loss_ref.backward()
    n = lambda t: t.detach().numpy().copy()  # noqa: E731
    return {"margin": margin[0], "loss": float(loss_ref), "weight": n(weight), "ind": n(ind), "dw": n(weight.grad),
            "s_value": [n(y) for row in s_value for y in row], "target": [n(t) for row in target for t in row],
            "dsv": [n(y.grad) for row in s_value for y in row], "dxs": [n(x.grad) for x in xs],
            "dproj": n(mod.regressor00.regressor[0].weight.grad), "dhead": n(mod.query_0.linear1.weight.grad)}


def main():
    util = _load(os.path.join(REF, "models", "util.py"), "ref_models_util")
    crit = _load(os.path.join(REF, "distiller_zoo", "SemCKD.py"), "ref_semckd").SemCKDLoss()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (B, stu, tea) in enumerate(CASES):
        for attempt in range(TRIES):
            seed = 1900 + 100 * ci + attempt
            torch.manual_seed(seed)
            mod = util.SelfA(B, [c for c, _ in stu], [c for c, _ in tea], 1.0)
            mod.train()
            state0 = {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()}
            rng = np.random.default_rng(seed)
            fs = [draw(rng, (B, c, h, h)) for c, h in stu]
            ft = [draw(rng, (B, c, h, h)) for c, h in tea]
            r64 = run(copy.deepcopy(mod).double(), crit, fs, ft, torch.float64)
            if r64["margin"] >= (TAU if attempt < TRIES_AT_TAU else TAU_FLOOR):
                break
        else:
            raise RuntimeError(f"case {ci}: no seed clear of the kink")
        r32 = run(mod, crit, fs, ft, torch.float32)
        S, T = len(stu), len(tea)
        alone = V.tail(r32["s_value"], r32["target"], r32["weight"])
        d = {"loss": abs(r32["loss"] - alone["loss"]) / alone["loss"], "ind": rel(r32["ind"], alone["ind"]),
             "dsv": max(rel(a, b) for a, b in zip(r32["dsv"], alone["dx"])), "dw": rel(r32["dw"], alone["dw"]),
             "chain_loss": abs(r32["loss"] - r64["loss"]) / r64["loss"], "weight": rel(r32["weight"], r64["weight"]),
             "dxs": max(rel(a, b) for a, b in zip(r32["dxs"], r64["dxs"])), "dproj": rel(r32["dproj"], r64["dproj"]),
             "dhead": rel(r32["dhead"], r64["dhead"])}
        head_noise = float(np.abs(r32["dhead"]).max() / np.abs(r32["dproj"]).max())
        assert r64["weight"].min() > 1e-6 or T == 1, "a softmax row degenerates"
        p = f"c{ci}_"
        out[p + "B"], out[p + "seed"] = np.array(B), np.array(seed)
        out[p + "stu"], out[p + "tea"] = np.array(stu, np.int64), np.array(tea, np.int64)
        out[p + "kink_margin"], out[p + "head_noise"] = np.array(r64["margin"]), np.array(head_noise)
        out[p + "state_keys"] = np.array(list(state0))
        for k, v in state0.items():
            # (a tensor above STATE_FULL elements -- the 260-channel 3 x 3 convolutions of case 1, 2.4 MB each -- is recorded as its
            #  float64 sum and sum of absolute values: the tests rebuild the module under `seed`, which the recorded tensors pin)
            if v.size <= STATE_FULL:
                out[p + "state_" + k] = v
            else:
                out[p + "statesum_" + k] = np.array([v.astype(np.float64).sum(), np.abs(v.astype(np.float64)).sum()])
        for i, f in enumerate(fs):
            out[p + f"fs{i}"], out[p + f"dxs{i}"] = f, r32["dxs"][i]
        for j, f in enumerate(ft):
            out[p + f"ft{j}"] = f
        for q in range(S * T):
            out[p + f"s_value{q}"], out[p + f"target{q}"], out[p + f"dsv{q}"] = r32["s_value"][q], r32["target"][q], r32["dsv"][q]
        for k in ("weight", "ind", "dw", "dproj", "dhead"):
            out[p + k] = r32[k]
        out[p + "loss"] = np.array(r32["loss"], np.float32)
        for k, v in d.items():
            out[p + "ref_vs_f64_" + k] = np.array(v, np.float64)
        print(f"case {ci} B {B} seed {seed} margin 2^{np.log2(r64['margin']):.1f} loss {r32['loss']:.6e} head_noise {head_noise:.1e}  "
              + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g19_semckd.npz"), out))


if __name__ == "__main__":
    main()

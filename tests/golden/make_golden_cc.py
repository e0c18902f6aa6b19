#!/usr/bin/env python3
"""Generate tests/golden/g21_cc*.npz by RUNNING THE REFERENCE's LinearEmbed (models/util.py) and Correlation (distiller_zoo/CC.py) on the
CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_cc.py

Cases (B, Cs, Ct, D): the smallest legal shape (both boundary rows are the only rows), small ragged shapes, segment tails (33, 65, 17), a
batch and an embedding width one past a 64-tile, and 1280-wide rows on both sides.  The heads are built under
torch.manual_seed(2100 + case), the student's first: their weights and biases are what nn.Linear's initialisation draws.  The inputs
are standard normal draws (numpy, seed 2100 + case) rounded to multiples of 1/32 and clipped to |.| <= 4 (exact in bf16); single
elements of x_s are then moved by 1/8 until every float64 |f_s - f_t| is at least 2^-10 (tests/cc_ref.clear).

Per case: the inputs, both heads, d = f_s - f_t, the loss, the gradients of x_s and of both heads' weights and biases, and the distances
of those fp32 results from the float64 restatement (tests/cc_ref.py): `ref_vs_f64_d / _loss / _dxs / _dws / _dbs / _dwt / _dbt`.  The
loss distance is relative to the loss, the others in crd_ref.rel's metric.  Only arrays are written; no reference source text."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import cc_ref as V, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402
from tests.golden.make_golden_hint import draw  # noqa: E402

CASES = [(2, 1, 1, 1), (2, 3, 5, 2), (3, 7, 4, 5), (5, 33, 65, 17), (65, 6, 9, 3), (66, 40, 24, 70), (7, 130, 72, 129), (4, 1280, 1280, 16)]
SEED0 = 2100


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    LinearEmbed = _load(os.path.join(REF, "models", "util.py"), "ref_models_util").LinearEmbed
    Correlation = _load(os.path.join(REF, "distiller_zoo", "CC.py"), "ref_cc").Correlation
    crit = Correlation()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (Bn, Cs, Ct, D) in enumerate(CASES):
        torch.manual_seed(SEED0 + ci)
        embed_s = LinearEmbed(Cs, D)
        embed_t = LinearEmbed(Ct, D)
        W_s, b_s = embed_s.linear.weight.detach().numpy().copy(), embed_s.linear.bias.detach().numpy().copy()
        W_t, b_t = embed_t.linear.weight.detach().numpy().copy(), embed_t.linear.bias.detach().numpy().copy()
        rng = np.random.default_rng(SEED0 + ci)
        x_s, x_t = draw(rng, (Bn, Cs)), draw(rng, (Bn, Ct))
        x64, nudges = V.clear(x_s, x_t, W_s, b_s, W_t, b_t)
        x_s = x64.astype(np.float32)
        assert np.array_equal(x_s.astype(np.float64), x64) and np.array_equal(x_s * 32, np.round(x_s * 32))
        ts = torch.from_numpy(x_s).requires_grad_(True)
        f_s, f_t = embed_s(ts), embed_t(torch.from_numpy(x_t))
        d = (f_s - f_t).detach().numpy().copy()
        loss = crit(f_s, f_t)
        loss.backward()
        w = V.cc(x_s, x_t, W_s, b_s, W_t, b_t)
        assert not (np.abs(w["d"]) < V.TAU).any()
        res = {"d": d, "loss": np.array(loss.item(), np.float32), "dx_s": ts.grad.numpy().copy(),
               "dW_s": embed_s.linear.weight.grad.numpy().copy(), "db_s": embed_s.linear.bias.grad.numpy().copy(),
               "dW_t": embed_t.linear.weight.grad.numpy().copy(), "db_t": embed_t.linear.bias.grad.numpy().copy()}
        dist = {"d": rel(d, w["d"]), "loss": abs(float(loss.item()) - w["loss"]) / w["loss"], "dxs": rel(res["dx_s"], w["dx_s"]),
                "dws": rel(res["dW_s"], w["dW_s"]), "dbs": rel(res["db_s"], w["db_s"]), "dwt": rel(res["dW_t"], w["dW_t"]),
                "dbt": rel(res["db_t"], w["db_t"])}
        assert np.array_equal(np.sign(d), np.sign(w["d"]))
        p = f"c{ci}_"
        out[p + "shape"] = np.array((Bn, Cs, Ct, D), np.int64)
        out[p + "x_s"], out[p + "x_t"] = x_s, x_t
        out[p + "W_s"], out[p + "b_s"], out[p + "W_t"], out[p + "b_t"] = W_s, b_s, W_t, b_t
        out[p + "state_keys"] = np.array(list(embed_s.state_dict()))
        for k_, v_ in res.items():
            assert np.isfinite(v_).all(), k_
            out[p + k_] = v_
        for k_, v_ in dist.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} B {Bn} Cs {Cs} Ct {Ct} D {D}: {nudges} nudges, loss {loss.item():.6e}  "
              + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in dist.items()) + f"  min |d| {np.abs(w['d']).min():.2e}")
    print(golden_npz.save(os.path.join(OUT, "g21_cc.npz"), out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/g22_ce.npz by RUNNING THE REFERENCE's classification head on the CPU in fp32: nn.CrossEntropyLoss() as
train_teacher.py:184 builds it, helper/util.accuracy (top-1, helper/loops_moma.py:44) and the confusion matrix of
helper/util.process_accumulated_output (helper/loops_moma.py:425).

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_ce.py

Cases (B, K): one row of two classes; one class (the loss is exactly 0); K = 5 (fp32 rows on 20-byte boundaries: element accesses);
65 rows of 4 classes (one lane per row, a second, ragged wave); 64 x 9; 100 and 1000 classes; K = 1024, the longest row the rows kernel
reads once, and 1025, the shortest it walks twice; 2500 (several trips of the two-walk loop); (3, 5) with the logits times 32, which
overflows exp without the maximum; (6, 5) with two rows labelled -100.
The logits are standard normal draws (numpy, seed 2200 + case) rounded to multiples of 1/32 and clipped to |z| <= 4 (exact in bf16);
the first occurrence of each row's maximum is then raised by 1/8, so every argmax is unique with a margin of 1/8 (asserted here and
again by the loader) -- on the 1/32 grid alone most of these shapes have exactly tied maxima.  Labels: the row's argmax on the even
rows (hits, and the rows whose loss is a small log1p), a uniform draw on the odd ones.

Per case: logits, labels, the reference's loss, dz (the gradient of the loss to the logits), accuracy and confusion matrix, and the
distances `ref_vs_f64_loss / _dz` of those fp32 results from the float64 restatement (tests/ce_ref.py): the loss relative to its own
value, dz in crd_ref.rel's metric.  Only arrays are written; no reference source text."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import ce_ref as V, golden_npz  # noqa: E402
from tests.ce_fixture import CASES, SEED0  # noqa: E402
from tests.crd_ref import rel  # noqa: E402
from tests.golden.make_golden_hint import draw  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    util = _load(os.path.join(REF, "helper", "util.py"), "ref_helper_util")
    crit = torch.nn.CrossEntropyLoss()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (Bn, K, scale, n_ignored) in enumerate(CASES):
        rng = np.random.default_rng(SEED0 + ci)
        z = draw(rng, (Bn, K))
        top = z.argmax(axis=1)
        z[np.arange(Bn), top] += np.float32(V.MARGIN)
        z *= np.float32(scale)
        assert V.margin(z) >= V.MARGIN * scale and np.array_equal(z * 32, np.round(z * 32))
        assert np.array_equal(torch.from_numpy(z).to(torch.bfloat16).float().numpy(), z)          # exact in bf16
        y = rng.integers(0, K, Bn).astype(np.int64)
        y[::2] = top[::2]
        if n_ignored:
            y[1:1 + 2 * n_ignored:2] = V.IGNORE
        tz = torch.from_numpy(z).requires_grad_(True)
        ty = torch.from_numpy(y)
        loss = crit(tz, ty)
        loss.backward()
        acc = util.accuracy(tz.detach(), ty, topk=(1,))[0]
        stat = util.process_accumulated_output({"logit": [z], "true": [y]}, Bn, K)
        w = V.ce(z, y)
        res = {"logits": z, "labels": y, "loss": np.array(loss.item(), np.float32), "dz": tz.grad.numpy().copy(),
               "acc": np.array(float(acc.item()), np.float64), "conf": np.asarray(stat["conf_mat"], np.int64)}
        assert np.array_equal(res["conf"], w["conf"]) and abs(float(res["acc"]) - w["acc"]) < 1e-4, ci
        dist = {"loss": abs(float(loss.item()) - w["loss"]) / max(abs(w["loss"]), 1e-300), "dz": rel(res["dz"], w["dz"])}
        p = f"c{ci}_"
        for k_, v_ in res.items():
            assert np.isfinite(v_).all(), k_
            out[p + k_] = v_
        for k_, v_ in dist.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} B {Bn} K {K} x{scale}: loss {loss.item():.6e}  acc {float(acc):.2f}  "
              + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in dist.items()) + f"  margin {V.margin(z):.3f}")
    print(golden_npz.save(os.path.join(OUT, "g22_ce.npz"), out))


if __name__ == "__main__":
    main()

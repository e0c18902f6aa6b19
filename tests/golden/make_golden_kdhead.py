#!/usr/bin/env python3
"""Generate tests/golden/g23_kdhead.npz by RUNNING THE REFERENCE's student head on the CPU in fp32: nn.CrossEntropyLoss(), the
reference's distiller_zoo/KD.py DistillKL(T) and helper/util.accuracy (top-1), as helper/loops_moma.py:278-279 and the accuracy call
behind them use them.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_kdhead.py

Cases (B, K, T), tests/kdhead_fixture.py: one row of two classes; one class (both losses exactly 0); K = 5 (fp32 rows on 20-byte
boundaries: element accesses); 65 rows of 4 classes (one lane per row, a second, ragged wave); 64 x 9 at T = 1; 7 x 100 at T = 2.5 (no
power of two); 1000 classes (a long row read once); K = 1024, the longest row the rows kernel reads once, and 1025, the shortest it
walks twice; 2500 (several trips of the two-walk loop); (3, 5) at T = 1 with both sides times 32, which overflows exp without the
maximum; (6, 5) with two rows labelled -100; (4, 9) with the teacher's logits equal to the student's (loss_div = 0).
Both sides' logits are standard normal draws (numpy, seed 2300 + case, the student's first) rounded to multiples of 1/32 and clipped
to |z| <= 4 (exact in bf16); the first occurrence of each STUDENT row's maximum is then raised by 1/8, so every argmax is unique with a
margin of 1/8 (asserted here and again by the loader).  The teacher's rows are drawn independently, so the divergence is not near 0.
Labels: the student row's argmax on the even rows, a uniform draw on the odd ones.

Per case: both logit matrices, the labels, the reference's loss_cls, loss_div and accuracy, dz_s = d (loss_cls + loss_div) / d logit_s
(both weights 1), and the distances `ref_vs_f64_cls / _div / _dz` of those fp32 results from the float64 restatement
(tests/kdhead_ref.py): each loss relative to its own value, dz in crd_ref.rel's metric.  For the identical-rows case, whose float64
divergence is 0, ref_vs_f64_div is the reference's |loss_div| itself.  Only arrays are written; no reference source text."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import golden_npz, kdhead_ref as V  # noqa: E402
from tests.crd_ref import rel  # noqa: E402
from tests.golden.make_golden_hint import draw  # noqa: E402
from tests.kdhead_fixture import CASES, SEED0  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    util = _load(os.path.join(REF, "helper", "util.py"), "ref_helper_util")
    kd = _load(os.path.join(REF, "distiller_zoo", "KD.py"), "ref_distiller_zoo_kd")
    crit = torch.nn.CrossEntropyLoss()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (Bn, K, T, scale, n_ignored, same) in enumerate(CASES):
        rng = np.random.default_rng(SEED0 + ci)
        zs = draw(rng, (Bn, K))
        zt = draw(rng, (Bn, K))
        top = zs.argmax(axis=1)
        zs[np.arange(Bn), top] += np.float32(V.MARGIN)
        zs *= np.float32(scale)
        zt *= np.float32(scale)
        if same:
            zt = zs.copy()
        assert V.margin(zs) >= V.MARGIN * scale
        for z in (zs, zt):
            assert np.array_equal(z * 32, np.round(z * 32))
            assert np.array_equal(torch.from_numpy(z).to(torch.bfloat16).float().numpy(), z)          # exact in bf16
        y = rng.integers(0, K, Bn).astype(np.int64)
        y[::2] = top[::2]
        if n_ignored:
            y[1:1 + 2 * n_ignored:2] = V.IGNORE
        ts = torch.from_numpy(zs).requires_grad_(True)
        tt, ty = torch.from_numpy(zt), torch.from_numpy(y)
        loss_cls = crit(ts, ty)
        loss_div = kd.DistillKL(T)(ts, tt)
        (loss_cls + loss_div).backward()
        acc = util.accuracy(ts.detach(), ty, topk=(1,))[0]
        w = V.head(zs, zt, y, T)
        res = {"logit_s": zs, "logit_t": zt, "labels": y, "loss_cls": np.array(loss_cls.item(), np.float32),
               "loss_div": np.array(loss_div.item(), np.float32), "dz": ts.grad.numpy().copy(), "acc": np.array(float(acc.item()), np.float64)}
        assert abs(float(res["acc"]) - w["acc"]) < 1e-4, ci
        dist = {"cls": abs(float(loss_cls.item()) - w["loss_cls"]) / max(abs(w["loss_cls"]), 1e-300),
                "div": abs(float(loss_div.item()) - w["loss_div"]) / max(abs(w["loss_div"]), 1e-300), "dz": rel(res["dz"], w["dz"])}
        if same:
            assert w["loss_div"] == 0.0
            dist["div"] = abs(float(loss_div.item()))
        p = f"c{ci}_"
        for k_, v_ in res.items():
            assert np.isfinite(v_).all(), k_
            out[p + k_] = v_
        for k_, v_ in dist.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} B {Bn} K {K} T {T} x{scale}: cls {loss_cls.item():.6e}  div {loss_div.item():.6e}  acc {float(acc):.2f}  "
              + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in dist.items()) + f"  margin {V.margin(zs):.3f}")
    print(golden_npz.save(os.path.join(OUT, "g23_kdhead.npz"), out))


if __name__ == "__main__":
    main()

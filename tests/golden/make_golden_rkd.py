#!/usr/bin/env python3
"""Generate tests/golden/g14_rkd.npz by RUNNING THE REFERENCE's RKDLoss criterion (distiller_zoo/RKD.py) on the CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_rkd.py

Cases (B, Ds, Dt, note): two points (both terms vanish identically: finiteness only), the smallest real batch, D = 1 on the teacher's
side, ragged widths, a student row multiplied by 8 (normalised distances more than 1 apart: the linear branch of the smooth L1),
one past a 32-tile, one past 64, inputs offset by +3, a student row and a teacher row duplicated exactly, the same rows differing by
1/32 in one coordinate on top of the offset, and the workload's width with a ragged tail.  The inputs are standard normal draws
rounded to multiples of 1/32 (exact in fp32 and in bf16), seed 1400 + case.  Per case: f_s, f_t, the reference's loss and
d loss / d f_s, and next to them their distance from the float64 evaluation of the formulas (tests/rkd_ref.py): `ref_vs_f64_loss`
relative to the loss (w_d l_d + w_a l_a, both terms >= 0), `ref_vs_f64_grad` (crd_ref.rel's metric) and `ref_vs_f64_S` for the
reference's fp32 squared pdist, off the diagonal.  In the duplicate-row case the reference's autograd divides by F.normalize's clamp
on the duplicated student rows (gradients of 1e10 there, the documented deviation): its `ref_vs_f64_grad` is taken over the other
rows, and the reference's largest |gradient| per row is recorded as `row_max`.  The tests allow the kernels twice the largest
distance of each kind.  Only arrays are written; no reference source text."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import rkd_ref as R, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (B, Ds, Dt, note)
    (2, 3, 5, ""),
    (3, 8, 8, ""),
    (5, 3, 1, ""),
    (5, 17, 33, ""),
    (8, 64, 40, "row0x8"),
    (33, 100, 60, ""),
    (65, 24, 24, ""),
    (16, 128, 256, "+3"),
    (12, 32, 32, "dup"),
    (12, 32, 32, "+3 near"),
    (16, 1283, 1280, ""),
]
DUP_S, DUP_T = (3, 7), (2, 5)


def inputs(ci):
    B, Ds, Dt, note = CASES[ci]
    rng = np.random.default_rng(1400 + ci)
    f_s = np.round(rng.standard_normal((B, Ds)) * 32) / 32
    f_t = np.round(rng.standard_normal((B, Dt)) * 32) / 32
    if note == "row0x8":
        f_s[0] *= 8
    if "+3" in note:
        f_s, f_t = f_s + 3, f_t + 3
    if note == "dup" or "near" in note:
        f_s[DUP_S[1]], f_t[DUP_T[1]] = f_s[DUP_S[0]], f_t[DUP_T[0]]
    if "near" in note:
        f_s[DUP_S[1], 5] += 1 / 32
        f_t[DUP_T[1], 5] += 1 / 32
    return f_s.astype(np.float32), f_t.astype(np.float32)


def main():
    sys.path.insert(0, REF)
    from distiller_zoo.RKD import RKDLoss
    crit = RKDLoss()
    out = {"n_cases": np.array(len(CASES))}
    branches = {"d<1": False, "d>=1": False, "a<1": False, "a>=1": False}
    for ci, (B, Ds, Dt, note) in enumerate(CASES):
        f_s, f_t = inputs(ci)
        ts, tt = torch.from_numpy(f_s).requires_grad_(True), torch.from_numpy(f_t)
        loss = crit(ts, tt)
        loss.backward()
        dF_s = ts.grad.numpy().copy()
        with torch.no_grad():
            S32 = RKDLoss.pdist(ts, squared=True).numpy()
        want = R.pair(f_s, f_t)
        assert np.isfinite(loss.item()) and np.isfinite(dF_s).all()
        off = ~np.eye(B, dtype=bool)
        d_s, d_t = np.sqrt(want["S_s"]) / want["mu_s"], np.sqrt(want["S_t"]) / want["mu_t"]
        zd, za = np.abs(d_s - d_t)[off], np.abs(R.angles(want["S_s"]) - R.angles(want["S_t"]))
        branches["d<1"] |= bool(((zd > 0) & (zd < 1)).any())
        branches["d>=1"] |= bool((zd >= 1).any())
        branches["a<1"] |= bool(((za > 0) & (za < 1)).any())
        branches["a>=1"] |= bool((za >= 1).any())
        p = f"c{ci}_"
        rows = np.ones(B, bool)
        if note == "dup":
            rows[list(DUP_S)] = False
            out[p + "row_max"] = np.abs(dF_s).max(1).astype(np.float64)
        out[p + "shape"] = np.array([B, Ds, Dt], dtype=np.int64)
        out[p + "f_s"], out[p + "f_t"], out[p + "dF_s"] = f_s, f_t, dF_s
        out[p + "loss"] = np.array(loss.item(), np.float32)
        d = {"loss": abs(float(loss.item()) - want["loss"]) / want["loss"] if B > 2 else abs(float(loss.item()) - want["loss"]) / (crit.w_d + crit.w_a),
             "grad": rel(dF_s[rows], want["dF_s"][rows]) if B > 2 else 0.0,
             "S": rel(S32[off], want["S_s"][off])}
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {CASES[ci]}: loss {loss.item():.6e}  " + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    assert all(branches.values()), branches
    print(golden_npz.save(os.path.join(OUT, "g14_rkd.npz"), out))


if __name__ == "__main__":
    main()

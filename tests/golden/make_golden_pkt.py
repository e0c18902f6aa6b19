#!/usr/bin/env python3
"""Generate tests/golden/g16_pkt.npz by RUNNING THE REFERENCE's PKT criterion (distiller_zoo/PKT.py) on the CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_pkt.py

Cases (B, Ds, Dt, note): a single row (P = T = 1: loss 0, gradient 0), the smallest real batch, the next, D = 1 on the teacher's side,
ragged widths, a student row multiplied by 8 (cosines do not change, the gradient of that row shrinks), one past a 32-tile, one past
64, inputs offset by +3 (all cosines near 1: the loss is a nearly cancelling sum), a student row and a teacher row duplicated exactly,
an all-zero student row and an all-zero teacher row (the documented deviation), the workload's width with a ragged tail, and the
workload's shape after max(., 0) -- the post-ReLU regime of feat[-1].  No exactly antiparallel rows: there K = 0 exactly and the
log's argument is eps against fp32 rounding of the same size, so the reference's own fp32 loss is 1e-3 away from float64 and
would hollow out the allowance of every other case (they have a GPU test of their own against float64).
The inputs are standard normal draws rounded to multiples of 1/32 (exact in fp32 and in bf16), seed 1600 + case.  Per case: f_s, f_t,
the reference's loss and d loss / d f_s, and next to them their distance from the float64 evaluation of the formulas
(tests/pkt_ref.py): `ref_vs_f64_loss` in units of abs_terms = mean_ij |T_ij log((T_ij + eps) / (P_ij + eps))| (the loss itself is a
nearly cancelling sum of these), `ref_vs_f64_grad` (crd_ref.rel's metric) and `ref_vs_f64_G` for an fp32 torch.mm Gram of the
student.  In the zero-row case the reference's gradient row is NaN: its `ref_vs_f64_grad` is taken over the other rows and the NaN
rows are recorded as `nan_rows`.  The tests allow the kernels twice the largest distance of each kind.  Only arrays are written; no
reference source text."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import pkt_ref as R, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (B, Ds, Dt, note)
    (1, 4, 4, ""),
    (2, 3, 5, ""),
    (3, 8, 8, ""),
    (5, 3, 1, ""),
    (5, 17, 33, ""),
    (8, 64, 40, "row0x8"),
    (33, 100, 60, ""),
    (65, 24, 24, ""),
    (16, 128, 256, "+3"),
    (12, 32, 32, "dup"),
    (12, 32, 32, "zero"),
    (16, 1283, 1280, ""),
    (64, 1280, 1280, "relu"),
]
DUP_S, DUP_T = (3, 7), (2, 5)
ZERO_S, ZERO_T = 4, 9


def inputs(ci):
    B, Ds, Dt, note = CASES[ci]
    rng = np.random.default_rng(1600 + ci)
    f_s = np.round(rng.standard_normal((B, Ds)) * 32) / 32
    f_t = np.round(rng.standard_normal((B, Dt)) * 32) / 32
    if note == "row0x8":
        f_s[0] *= 8
    if note == "+3":
        f_s, f_t = f_s + 3, f_t + 3
    if note == "dup":
        f_s[DUP_S[1]], f_t[DUP_T[1]] = f_s[DUP_S[0]], f_t[DUP_T[0]]
    if note == "zero":
        f_s[ZERO_S], f_t[ZERO_T] = 0, 0
    if note == "relu":
        f_s, f_t = np.maximum(f_s, 0), np.maximum(f_t, 0)
    return f_s.astype(np.float32), f_t.astype(np.float32)


def main():
    sys.path.insert(0, REF)
    from distiller_zoo.PKT import PKT
    crit = PKT()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (B, Ds, Dt, note) in enumerate(CASES):
        f_s, f_t = inputs(ci)
        ts, tt = torch.from_numpy(f_s).requires_grad_(True), torch.from_numpy(f_t)
        loss = crit(ts, tt)
        loss.backward()
        dF_s = ts.grad.numpy().copy()
        with torch.no_grad():
            G32 = torch.mm(ts, ts.t()).numpy()
        want = R.pair(f_s, f_t)
        nan_rows = np.isnan(dF_s).any(1)
        assert np.isfinite(loss.item()) and np.isfinite(want["dF_s"]).all()
        assert nan_rows.any() == (note == "zero") and (note != "zero" or list(np.flatnonzero(nan_rows)) == [ZERO_S])
        rows = ~nan_rows
        p = f"c{ci}_"
        out[p + "shape"] = np.array([B, Ds, Dt], dtype=np.int64)
        out[p + "f_s"], out[p + "f_t"], out[p + "dF_s"] = f_s, f_t, dF_s
        out[p + "loss"] = np.array(loss.item(), np.float32)
        if note == "zero":
            out[p + "nan_rows"] = nan_rows
        d = {"loss": abs(float(loss.item()) - want["loss"]) / want["abs_terms"] if B > 1 else abs(float(loss.item())),
             "grad": rel(dF_s[rows], want["dF_s"][rows]) if B > 1 else float(np.abs(dF_s).max()),
             "G": rel(G32, want["G_s"])}
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {CASES[ci]}: loss {loss.item():.6e} (f64 {want['loss']:.6e}, abs_terms {want['abs_terms']:.3e})  "
              + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g16_pkt.npz"), out))


if __name__ == "__main__":
    main()

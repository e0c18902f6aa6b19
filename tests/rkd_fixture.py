"""Reading tests/golden/g14_rkd.npz (written by tests/golden/make_golden_rkd.py): the Relational Knowledge Distillation cases and the
allowance the tests share."""
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("loss", "grad", "S")
DUP_CASE, NEAR_CASE, DUP_S, DUP_T = 8, 9, (3, 7), (2, 5)
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(shape=(B, Ds, Dt), f_s, f_t, dF_s, loss, ref_vs_f64_{loss,grad,S}[, row_max]);
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distances
    are relative to the loss (a weighted sum of two non-negative terms), the two-point case's to w_d + w_a"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g14_rkd.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            c = {"shape": tuple(int(v) for v in g[p + "shape"]), "loss": float(g[p + "loss"])}
            for k in ("f_s", "f_t", "dF_s"):
                c[k] = np.asarray(g[p + k])
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            if p + "row_max" in g.files:
                c["row_max"] = np.asarray(g[p + "row_max"])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

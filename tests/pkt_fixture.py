"""Reading tests/golden/g16_pkt.npz (written by tests/golden/make_golden_pkt.py): the Probabilistic Knowledge Transfer cases and the
allowance the tests share."""
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("loss", "grad", "G")
DUP_CASE, ZERO_CASE, DUP_S, DUP_T, ZERO_S, ZERO_T = 9, 10, (3, 7), (2, 5), 4, 9
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(shape=(B, Ds, Dt), f_s, f_t, dF_s, loss, ref_vs_f64_{loss,grad,G}[, nan_rows]);
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distances
    are in units of abs_terms = mean_ij |T_ij log((T_ij + eps) / (P_ij + eps))| (tests/pkt_ref.py), the single-row case's absolute"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g16_pkt.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            c = {"shape": tuple(int(v) for v in g[p + "shape"]), "loss": float(g[p + "loss"])}
            for k in ("f_s", "f_t", "dF_s"):
                c[k] = np.asarray(g[p + k])
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            if p + "nan_rows" in g.files:
                c["nan_rows"] = np.asarray(g[p + "nan_rows"])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

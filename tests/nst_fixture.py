"""Reading tests/golden/g13_nst.npz (written by tests/golden/make_golden_nst.py): the Neuron Selectivity Transfer cases, with the
per-image pieces of f_s, f_t and dF_s put together again, and the allowance the tests share."""
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("loss", "grad", "gram")
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(shape=(B, Cs, Ct, Hs, Ws, Ht, Wt), f_s, f_t, dF_s, loss, ref_vs_f64_{loss,grad,gram});
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distances
    are relative to t1 + 2 t2 (the loss is their difference and crosses zero)"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g13_nst.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            shape = tuple(int(v) for v in g[p + "shape"])
            c = {"shape": shape, "loss": float(g[p + "loss"])}
            for k in ("f_s", "f_t", "dF_s"):
                c[k] = np.stack([g[f"{p}{k}_b{b}"] for b in range(shape[0])])
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

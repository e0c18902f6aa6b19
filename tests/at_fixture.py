"""Reading tests/golden/g12_at.npz (written by tests/golden/make_golden_at.py): the Attention Transfer cases, with the per-image
pieces of f_s, f_t and dF_s put together again, and the allowance the tests share."""
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(shape=(B, Cs, Ct, Hs, Ht), f_s, f_t, dF_s, loss, ref_vs_f64_{loss,grad,map});
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative)"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g12_at.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            shape = tuple(int(v) for v in g[p + "shape"])
            c = {"shape": shape, "loss": float(g[p + "loss"])}
            for k in ("f_s", "f_t", "dF_s"):
                c[k] = np.stack([g[f"{p}{k}_b{b}"] for b in range(shape[0])])
            for k in ("loss", "grad", "map"):
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in ("loss", "grad", "map")}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

"""Reading tests/golden/g17_vid*.npz (written by tests/golden/make_golden_vid.py): the Variational Information Distillation cases,
with the per-image pieces of the maps put together again, and the allowances the tests share."""
import glob
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("loss", "dmean", "dls", "dx", "dw", "chain_loss")
_CACHE = {}


def files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g17_vid*.npz")))


def load():
    """-> (cases, allowance): cases[i] = dict(shape=(B, Cs, Ct, H, W) of the common grid, mid, x, target (as handed to the
    criterion: a pooled side is larger), w [3], log_scale, eps, pred_mean, d_pred_mean, loss, dx, dw [3], d_log_scale,
    ref_vs_f64_<kind>); allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).
    The loss distances are in units of abs_terms (tests/vid_ref.py), the others in crd_ref.rel's metric"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g17_vid.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            sh = [int(v) for v in g[p + "shape"]]
            c = {"shape": tuple(sh[:5]), "mid": sh[5], "loss": float(g[p + "loss"]), "eps": float(g[p + "eps"])}
            for k in ("x", "target", "dx", "pred_mean", "d_pred_mean"):
                c[k] = np.stack([g[f"{p}{k}_b{b}"] for b in range(sh[0])])
            c["w"] = [g[f"{p}w{i}"] for i in range(3)]
            c["dw"] = [g[f"{p}dw{i}"] for i in range(3)]
            c["log_scale"], c["d_log_scale"] = g[p + "log_scale"], g[p + "d_log_scale"]
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

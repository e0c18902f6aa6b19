"""Reading tests/golden/g18_hint*.npz (written by tests/golden/make_golden_hint.py): the FitNets hint cases recorded from the
reference's ConvReg + HintLoss, and the allowances the tests share."""
import glob
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
TAIL_KINDS = ("loss", "dx", "dgamma", "dbeta", "rmean", "rvar")          # from the restatement of the tail on the reference's conv output
CHAIN_KINDS = ("chain_loss", "dxs", "dw")                                # from the reference's modules run in float64
N_CASES = 13
_CACHE = {}


def files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g18_hint*.npz")))


def load():
    """-> (cases, allowance): cases[i] = dict(s_shape, t_shape, tail_only, x (the student's map; absent when tail_only), t, t_grid (the
    teacher's map on the regressor's grid), w, b, gamma, beta, eps, momentum, conv_out, d_conv_out, loss, dx_s, dw, db, d_gamma, d_beta,
    running_mean, running_var (after one step from 0 / 1), state_keys, db_noise, ref_vs_f64_<kind>); allowance[kind] = twice the largest
    ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distances are relative to the loss, the others in
    crd_ref.rel's metric"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g18_hint.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            c = {"s_shape": tuple(int(v) for v in g[p + "s_shape"]), "t_shape": tuple(int(v) for v in g[p + "t_shape"]),
                 "tail_only": bool(int(g[p + "tail_only"])), "loss": float(g[p + "loss"]), "eps": float(g[p + "eps"]),
                 "momentum": float(g[p + "momentum"]), "db_noise": float(g[p + "db_noise"]),
                 "state_keys": [str(k) for k in g[p + "state_keys"]]}
            for k in ("t", "t_grid", "w", "b", "gamma", "beta", "conv_out", "d_conv_out", "d_gamma", "d_beta", "running_mean", "running_var"):
                c[k] = g[p + k]
            kinds = TAIL_KINDS
            if not c["tail_only"]:
                for k in ("x", "dx_s", "dw", "db"):
                    c[k] = g[p + k]
                kinds = TAIL_KINDS + CHAIN_KINDS
            for k in kinds:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c.get("ref_vs_f64_" + k, 0.0) for c in cases), ULP32) for k in TAIL_KINDS + CHAIN_KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

"""Reading tests/golden/g20_srrl*.npz (written by tests/golden/make_golden_srrl.py): the SRRL cases recorded from the reference's
SRRL + nn.MSELoss + a Linear classifier, and the allowances the tests share."""
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
TAIL_KINDS = ("loss", "dx", "dgamma", "dbeta", "rmean", "rvar")          # from the restatement of the tail on the reference's conv output
CHAIN_KINDS = ("chain_loss", "dxs", "dw")                                # from the reference's modules run in float64
N_CASES = 10
SEED0 = 2000                                                             # case i was built under torch.manual_seed(SEED0 + i)
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(B, t_n, n_cls, s_n, tail_only, f_s and w (the student's feature and the convolution's
    weight; absent when tail_only), t, l, W, b, gamma, beta, eps, momentum, conv_out, d_conv_out, trans, pred, loss, dx_s, dw, d_gamma,
    d_beta, running_mean, running_var (after one step from 0 / 1), state_keys, ref_vs_f64_<kind>); allowance[kind] = twice the largest
    ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distances are relative to the loss, the others in
    crd_ref.rel's metric.  (The cases with B = 2 set the gradient allowance of x: there xh = +-1 whatever x is, dx is 0 but for eps,
    and the reference's fp32 result is 8e-3 of that remainder away from float64.)"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g20_srrl.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            Bn, t_n, n_cls, s_n = (int(v) for v in g[p + "shape"])
            c = {"B": Bn, "t_n": t_n, "n_cls": n_cls, "s_n": s_n, "tail_only": bool(int(g[p + "tail_only"])),
                 "loss": float(g[p + "loss"]), "eps": float(g[p + "eps"]), "momentum": float(g[p + "momentum"]),
                 "state_keys": [str(k) for k in g[p + "state_keys"]]}
            for k in ("t", "l", "W", "b", "gamma", "beta", "conv_out", "d_conv_out", "trans", "pred", "d_gamma", "d_beta",
                      "running_mean", "running_var"):
                c[k] = g[p + k]
            kinds = TAIL_KINDS
            if not c["tail_only"]:
                for k in ("f_s", "w", "dx_s", "dw"):
                    c[k] = g[p + k]
                kinds = TAIL_KINDS + CHAIN_KINDS
            for k in kinds:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c.get("ref_vs_f64_" + k, 0.0) for c in cases), ULP32) for k in TAIL_KINDS + CHAIN_KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

"""Reading tests/golden/g19_semckd*.npz (written by tests/golden/make_golden_semckd.py): the SemCKD cases recorded from the reference's
SelfA + SemCKDLoss, the allowances the tests share, and the recorded module rebuilt."""
import glob
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
TAIL_KINDS = ("loss", "ind", "dsv", "dw")                        # from the restatement of the tail on the reference's s_value, target, weight
CHAIN_KINDS = ("chain_loss", "weight", "dxs", "dproj", "dhead")  # from the reference's modules run in float64
N_CASES = 5
_CACHE = {}


def files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g19_semckd*.npz")))


def head_is_zero(c):
    """cases whose head gradient is analytically 0 (one pair: the softmax is 1; B // 4 = 1: the normalised embedding is +-1): its
    relative distance from float64 is meaningless there, the tests compare it in absolute terms against the projection's gradient"""
    return c["B"] // 4 == 1 or len(c["stu"]) * len(c["tea"]) == 1


def load():
    """-> (cases, allowance): cases[i] = dict(B, seed, stu, tea ((C, H) per map), fs, ft (lists of maps), state (name -> array, the
    tensors recorded in full), state_sums (name -> (sum, sum of |.|) of the others), state_keys, s_value, target, dsv (lists over the
    pairs p = i T + j), weight, ind, loss, dw, dxs (list), dproj, dhead, kink_margin, head_noise, ref_vs_f64_<kind>);
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases (dhead: over those whose head gradient is not analytically
    0), never below one fp32 ulp (relative).  The loss distances are relative to the loss, the others in crd_ref.rel's metric"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g19_semckd.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            c = {"B": int(g[p + "B"]), "seed": int(g[p + "seed"]), "stu": [tuple(int(v) for v in r) for r in g[p + "stu"]],
                 "tea": [tuple(int(v) for v in r) for r in g[p + "tea"]], "loss": float(g[p + "loss"]),
                 "kink_margin": float(g[p + "kink_margin"]), "head_noise": float(g[p + "head_noise"]),
                 "state_keys": [str(k) for k in g[p + "state_keys"]]}
            S, T = len(c["stu"]), len(c["tea"])
            c["fs"], c["dxs"] = [g[p + f"fs{i}"] for i in range(S)], [g[p + f"dxs{i}"] for i in range(S)]
            c["ft"] = [g[p + f"ft{j}"] for j in range(T)]
            for k in ("s_value", "target", "dsv"):
                c[k] = [g[p + f"{k}{q}"] for q in range(S * T)]
            for k in ("weight", "ind", "dw", "dproj", "dhead"):
                c[k] = g[p + k]
            c["state"] = {k: g[p + "state_" + k] for k in c["state_keys"] if p + "state_" + k in g.files}
            c["state_sums"] = {k: g[p + "statesum_" + k] for k in c["state_keys"] if p + "statesum_" + k in g.files}
            for k in TAIL_KINDS + CHAIN_KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {}
        for k in TAIL_KINDS + CHAIN_KINDS:
            over = [c for c in cases if not (k == "dhead" and head_is_zero(c))]
            allow[k] = max(2 * max(c["ref_vs_f64_" + k] for c in over), ULP32)
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]


def module_of(c, dtype=None):
    """the recorded module: moma_amd.distiller_zoo.SelfA built under the case's seed (its construction order is the reference's, so
    it draws the reference's weights), every tensor recorded in full compared bit for bit and the others by their checksums"""
    import torch
    from moma_amd.distiller_zoo import SelfA
    torch.manual_seed(c["seed"])
    mod = SelfA(c["B"], [ch for ch, _ in c["stu"]], [ch for ch, _ in c["tea"]], 1.0)
    sd = mod.state_dict()
    assert list(sd) == c["state_keys"]
    for k, v in c["state"].items():
        assert np.array_equal(sd[k].numpy(), v), k
    for k, (s, a) in c["state_sums"].items():
        v = sd[k].numpy().astype(np.float64)
        assert v.sum() == s and np.abs(v).sum() == a, k
    mod.train()
    return mod if dtype is None else mod.to(dtype)

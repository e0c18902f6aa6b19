"""Reading tests/golden/g22_ce.npz (written by tests/golden/make_golden_ce.py): the classification-head cases recorded from the
reference's nn.CrossEntropyLoss, helper/util.accuracy and process_accumulated_output, and the allowances the tests share."""
import os

import numpy as np

from tests import ce_ref, golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("loss", "dz")
ONE_WALK_K = 1024                                                        # MOMA_CE_ONE_WALK_K: the longest row the rows kernel reads once
# (B, K, scale of the logits, rows labelled -100)
CASES = [(1, 2, 1, 0), (2, 1, 1, 0), (3, 5, 1, 0), (65, 4, 1, 0), (64, 9, 1, 0), (7, 100, 1, 0), (5, 1000, 1, 0), (4, ONE_WALK_K, 1, 0),
         (3, ONE_WALK_K + 1, 1, 0), (3, 2500, 1, 0), (3, 5, 32, 0), (6, 5, 1, 2)]
N_CASES = len(CASES)
SEED0 = 2200                                                             # case i was drawn from numpy's default_rng(SEED0 + i)
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(B, K, logits, labels, loss, dz, acc, conf, ref_vs_f64_<kind>); allowance[kind] = twice the
    largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distance is relative to the loss, dz's in
    crd_ref.rel's metric.  Every row's maximum is unique by at least ce_ref.MARGIN times the case's scale (asserted)."""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g22_ce.npz"))
        assert int(g["n_cases"]) == N_CASES
        cases = []
        for ci, (Bn, K, scale, n_ignored) in enumerate(CASES):
            p = f"c{ci}_"
            c = {"B": Bn, "K": K, "loss": float(g[p + "loss"]), "acc": float(g[p + "acc"])}
            for k in ("logits", "labels", "dz", "conf"):
                c[k] = g[p + k]
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            assert c["logits"].shape == (Bn, K) and c["labels"].shape == (Bn,) and c["labels"].dtype == np.int64
            assert ce_ref.margin(c["logits"]) >= ce_ref.MARGIN * scale, ci
            assert int((c["labels"] == ce_ref.IGNORE).sum()) == n_ignored
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

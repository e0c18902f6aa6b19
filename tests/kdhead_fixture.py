"""Reading tests/golden/g23_kdhead.npz (written by tests/golden/make_golden_kdhead.py): the student-head cases recorded from the
reference's nn.CrossEntropyLoss, distiller_zoo/KD.py DistillKL(T) and helper/util.accuracy, and the allowances the tests share."""
import os

import numpy as np

from tests import golden_npz, kdhead_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("cls", "div", "dz")
ONE_WALK_K = 1024                                                        # MOMA_KDHEAD_ONE_WALK_K: the longest row the rows kernel reads once
# (B, K, T, scale of both sides' logits, rows labelled -100, the teacher's logits ARE the student's)
CASES = [(1, 2, 4.0, 1, 0, False), (2, 1, 4.0, 1, 0, False), (3, 5, 4.0, 1, 0, False), (65, 4, 4.0, 1, 0, False), (64, 9, 1.0, 1, 0, False),
         (7, 100, 2.5, 1, 0, False), (5, 1000, 4.0, 1, 0, False), (4, ONE_WALK_K, 4.0, 1, 0, False), (3, ONE_WALK_K + 1, 4.0, 1, 0, False),
         (3, 2500, 4.0, 1, 0, False), (3, 5, 1.0, 32, 0, False), (6, 5, 4.0, 1, 2, False), (4, 9, 4.0, 1, 0, True)]
N_CASES = len(CASES)
SAME = 12                                                                # the case whose teacher rows are the student's
SEED0 = 2300                                                             # case i was drawn from numpy's default_rng(SEED0 + i)
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(B, K, T, same, logit_s, logit_t, labels, loss_cls, loss_div, acc, dz, ref_vs_f64_<kind>);
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The losses' distances
    are relative to the loss, dz's in crd_ref.rel's metric.  The identical-rows case has loss_div = 0 in float64: its
    ref_vs_f64_div is |the reference's loss_div|, an absolute figure that stays out of the allowance (the tests check that case in
    absolute terms).  Every student row's maximum is unique by at least kdhead_ref.MARGIN times the case's scale (asserted)."""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g23_kdhead.npz"))
        assert int(g["n_cases"]) == N_CASES
        cases = []
        for ci, (Bn, K, T, scale, n_ignored, same) in enumerate(CASES):
            p = f"c{ci}_"
            c = {"B": Bn, "K": K, "T": T, "same": same}
            for k in ("loss_cls", "loss_div", "acc"):
                c[k] = float(g[p + k])
            for k in ("logit_s", "logit_t", "labels", "dz"):
                c[k] = g[p + k]
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            assert c["logit_s"].shape == c["logit_t"].shape == c["dz"].shape == (Bn, K)
            assert c["labels"].shape == (Bn,) and c["labels"].dtype == np.int64
            assert kdhead_ref.margin(c["logit_s"]) >= kdhead_ref.MARGIN * scale, ci
            assert int((c["labels"] == kdhead_ref.IGNORE).sum()) == n_ignored
            assert np.array_equal(c["logit_s"], c["logit_t"]) == same or K == 1, ci      # (the teacher's rows are draws of their own)
            cases.append(c)
        assert cases[SAME]["same"] and sum(c["same"] for c in cases) == 1
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases if not (k == "div" and c["same"])), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

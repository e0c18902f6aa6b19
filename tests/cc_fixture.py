"""Reading tests/golden/g21_cc*.npz (written by tests/golden/make_golden_cc.py): the Correlation Congruence cases recorded from the
reference's LinearEmbed heads and Correlation, and the allowances the tests share."""
import os

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("d", "loss", "dxs", "dws", "dbs", "dwt", "dbt")
SHAPES = [(2, 1, 1, 1), (2, 3, 5, 2), (3, 7, 4, 5), (5, 33, 65, 17), (65, 6, 9, 3), (66, 40, 24, 70), (7, 130, 72, 129), (4, 1280, 1280, 16)]
N_CASES = len(SHAPES)
SEED0 = 2100                                                             # case i was built under torch.manual_seed(SEED0 + i)
_CACHE = {}


def load():
    """-> (cases, allowance): cases[i] = dict(B, Cs, Ct, D, x_s, x_t, W_s, b_s, W_t, b_t, d, loss, dx_s, dW_s, db_s, dW_t, db_t,
    state_keys, ref_vs_f64_<kind>); allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp
    (relative).  The loss distance is relative to the loss, the others in crd_ref.rel's metric."""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g21_cc.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            Bn, Cs, Ct, D = (int(v) for v in g[p + "shape"])
            c = {"B": Bn, "Cs": Cs, "Ct": Ct, "D": D, "loss": float(g[p + "loss"]), "state_keys": [str(k) for k in g[p + "state_keys"]]}
            for k in ("x_s", "x_t", "W_s", "b_s", "W_t", "b_t", "d", "dx_s", "dW_s", "db_s", "dW_t", "db_t"):
                c[k] = g[p + k]
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]


def args(c):
    return c["x_s"], c["x_t"], c["W_s"], c["b_s"], c["W_t"], c["b_t"]

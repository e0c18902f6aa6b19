"""Reading tests/golden/g15_sp*.npz (written by tests/golden/make_golden_sp.py): the Similarity-Preserving distillation cases and the
allowance the tests share."""
import os

import numpy as np

from tests import golden_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
KINDS = ("loss", "grad", "G", "H")
# (B, shape of one student sample, shape of one teacher sample, note) -- the generator's table, repeated here for the tests' ids
CASES = [
    (1, (5,), (3,), ""),
    (2, (7,), (4,), ""),
    (3, (2,), (3,), ""),
    (5, (6,), (1,), ""),
    (8, (131,), (67,), ""),
    (17, (24,), (40,), ""),
    (33, (100,), (60,), ""),
    (65, (24,), (24,), ""),
    (129, (20,), (12,), ""),
    (16, (128,), (256,), "+3"),
    (16, (32, 7, 7), (48, 7, 7), "silu"),
    (12, (32,), (32,), "dup"),
    (6, (10,), (9,), "zero"),
    (4, (1280, 7, 7), (640, 7, 7), "long"),
]
DUP, ZERO_S, ZERO_T = (3, 7), 2, 4
LONG_STRIDE = 4            # the long case keeps every 4th column of the reference's gradient (`dF_s_cols`)
_CACHE = {}


def bf16_bits(a):
    """float32 values that are exact in bfloat16 -> their 16 bits"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (u & 0xffff).any()
    return (u >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def load():
    """-> (cases, allowance): cases[i] = dict(shape=(B, sample shape s, sample shape t), note, f_s, f_t (float32, exact in bfloat16),
    loss, dF_s (the long case: dF_s_cols, every LONG_STRIDE-th column of the flattened gradient), ref_vs_f64_{loss,grad,G,H});
    allowance[kind] = twice the largest ref_vs_f64_<kind> over the cases, never below one fp32 ulp (relative).  The loss distances
    are relative to the loss, the one-sample case's (loss 0) absolute"""
    if not _CACHE:
        g = golden_npz.load(os.path.join(ROOT, "tests", "golden", "g15_sp.npz"))
        cases = []
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            B, ss, st, note = CASES[ci]
            c = {"shape": (B, ss, st), "note": note, "loss": float(g[p + "loss"])}
            c["f_s"] = from_bf16_bits(np.asarray(g[p + "f_s_bf16"])).reshape((B,) + ss)
            c["f_t"] = from_bf16_bits(np.asarray(g[p + "f_t_bf16"])).reshape((B,) + st)
            for k in ("dF_s", "dF_s_cols"):
                if p + k in g.files:
                    c[k] = np.asarray(g[p + k])
            for k in KINDS:
                c["ref_vs_f64_" + k] = float(g[p + "ref_vs_f64_" + k])
            cases.append(c)
        allow = {k: max(2 * max(c["ref_vs_f64_" + k] for c in cases), ULP32) for k in KINDS}
        _CACHE["v"] = (cases, allow)
    return _CACHE["v"]

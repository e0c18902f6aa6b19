#!/usr/bin/env python3
"""Generate tests/golden/g13_nst.npz by RUNNING THE REFERENCE's NSTLoss criterion (distiller_zoo/NST.py) on the CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_nst.py

Cases (B, Cs, Ct, Hs, Ws, Ht, Wt, offset): the smallest shape, an odd pixel count, ragged channel counts on a 5 x 3 map, the 14 x 14,
28 x 28 and 56 x 56 stages of EfficientNet-B0, one case with the inputs offset by +3 (maps far from zero mean), more student rows than
one row block on a 4 x 4 map, and two cases whose student map is pooled to the teacher's grid (integer and non-integer ratio).  In
every case row 1 of the student's image 0 is all zeros (norm 0: the clamp of F.normalize; the reference's gradient there is finite
and exactly 0).  The inputs are standard normal draws rounded to multiples of 1/32 (exact in fp32 and in bf16; the fixture
compresses).  Per case: f_s, f_t, the reference's loss and d loss / d f_s (the three tensors image by image, `_b<i>`;
tests/nst_fixture.py puts them together), and next to them their distance from the float64 evaluation of the formulas
(tests/nst_ref.py): `ref_vs_f64_loss` relative to t1 + 2 t2 (the loss is a difference and crosses zero), `ref_vs_f64_grad`
(crd_ref.rel's metric) and `ref_vs_f64_gram` for the normalised Gram [Gss | Gst] evaluated with F.normalize + bmm in fp32.  The tests
allow the kernels twice the largest of each kind.  Only arrays are written; no reference source text."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import nst_ref as N, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (B, Cs, Ct, Hs, Ws, Ht, Wt, offset)
    (2, 3, 5, 4, 4, 4, 4, 0.0),
    (3, 24, 40, 7, 7, 7, 7, 0.0),
    (2, 33, 65, 5, 3, 5, 3, 0.0),
    (2, 112, 112, 14, 14, 14, 14, 0.0),
    (2, 24, 24, 56, 56, 56, 56, 0.0),
    (2, 64, 128, 8, 8, 8, 8, 3.0),
    (2, 40, 40, 28, 28, 28, 28, 0.0),
    (2, 200, 136, 4, 4, 4, 4, 0.0),
    (2, 8, 12, 8, 8, 4, 4, 0.0),
    (2, 8, 12, 7, 7, 4, 4, 0.0),
]


def main():
    sys.path.insert(0, REF)
    from distiller_zoo.NST import NSTLoss
    crit = NSTLoss()
    out = {"n_cases": np.array(len(CASES))}
    for ci, (B, Cs, Ct, Hs, Ws, Ht, Wt, off) in enumerate(CASES):
        rng = np.random.default_rng(1300 + ci)
        f_s = (np.round(rng.standard_normal((B, Cs, Hs, Ws)) * 32) / 32 + off).astype(np.float32)
        f_t = (np.round(rng.standard_normal((B, Ct, Ht, Wt)) * 32) / 32 + off).astype(np.float32)
        f_s[0, 1] = 0
        ts, tt = torch.from_numpy(f_s).requires_grad_(True), torch.from_numpy(f_t)
        loss = crit([ts], [tt])[0]
        loss.backward()
        with torch.no_grad():                        # the normalised Gram, with the reference's own normalisation, as a bmm
            ps = F.adaptive_avg_pool2d(ts, (Ht, Ht)) if Hs > Ht else ts
            xs, xt = F.normalize(ps.reshape(B, Cs, -1), dim=2), F.normalize(tt.reshape(B, Ct, -1), dim=2)
            gram = torch.bmm(xs, torch.cat([xs, xt], 1).transpose(1, 2)).numpy()
        want = N.pair(f_s, f_t)
        p = f"c{ci}_"
        out[p + "shape"] = np.array([B, Cs, Ct, Hs, Ws, Ht, Wt], dtype=np.int64)
        dF_s = ts.grad.numpy().copy()
        for b in range(B):                           # one array per image: a part of the fixture stays below a committed file's limit
            out[f"{p}f_s_b{b}"], out[f"{p}f_t_b{b}"], out[f"{p}dF_s_b{b}"] = f_s[b], f_t[b], dF_s[b]
        out[p + "loss"] = np.array(loss.item(), np.float32)
        d = {"loss": abs(float(loss.item()) - want["loss"]) / (want["t1"] + 2 * want["t2"]), "grad": rel(dF_s, want["dF_s"]),
             "gram": rel(gram, want["G"])}
        assert np.isfinite(dF_s).all() and not dF_s[0, 1].any() and np.isfinite(loss.item())
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {CASES[ci]}: loss {loss.item():.6e}  " + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g13_nst.npz"), out))


if __name__ == "__main__":
    main()

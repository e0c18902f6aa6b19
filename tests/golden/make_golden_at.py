#!/usr/bin/env python3
"""Generate tests/golden/g12_at.npz by RUNNING THE REFERENCE's Attention criterion (distiller_zoo/AT.py, p = 2) on the CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_at.py

Cases (B, Cs, Ct, Hs, Ht), square maps: equal sizes, integer pool ratios on either side, a non-integer ratio, the 4 x 4 and 7 x 7
maps with many channels, one case with the inputs offset by +3 (maps far from zero mean), the 56 x 56 stage of EfficientNet-B0.  In
every case with B > 1 the student's image 0 is all zeros (norm 0: the clamp of F.normalize).  The inputs are standard normal draws
rounded to multiples of 1/32 (exact in fp32 and in bf16; the fixture compresses).  Per case: f_s, f_t, the reference's loss and
d loss / d f_s (the three tensors image by image, `_b<i>`; tests/at_fixture.py puts them together), and next to them their distance from the float64 evaluation of the formulas (tests/at_ref.py; crd_ref.rel's metric,
relative for the scalar): `ref_vs_f64_loss`, `ref_vs_f64_grad`, and `ref_vs_f64_map` for the normalised maps the reference's own
`at()` returns.  The tests allow the kernels twice the largest of each kind.  Only arrays are written; no reference source text."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import at_ref as A, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402

CASES = [  # (B, Cs, Ct, Hs, Ht, offset)
    (2, 3, 5, 7, 7, 0.0),
    (3, 16, 64, 8, 4, 0.0),
    (2, 8, 8, 16, 4, 0.0),
    (2, 3, 5, 7, 4, 0.0),
    (4, 64, 256, 4, 4, 0.0),
    (4, 64, 256, 32, 32, 3.0),
    (2, 24, 40, 56, 56, 0.0),
    (2, 1280, 1280, 7, 7, 0.0),
]


def main():
    sys.path.insert(0, REF)
    from distiller_zoo.AT import Attention
    crit = Attention(p=2)
    out = {"n_cases": np.array(len(CASES))}
    for ci, (B, Cs, Ct, Hs, Ht, off) in enumerate(CASES):
        rng = np.random.default_rng(1200 + ci)
        f_s = (np.round(rng.standard_normal((B, Cs, Hs, Hs)) * 32) / 32 + off).astype(np.float32)
        f_t = (np.round(rng.standard_normal((B, Ct, Ht, Ht)) * 32) / 32 + off).astype(np.float32)
        if B > 1:
            f_s[0] = 0
        ts, tt = torch.from_numpy(f_s).requires_grad_(True), torch.from_numpy(f_t)
        loss = crit([ts], [tt])[0]
        loss.backward()
        with torch.no_grad():                        # the normalised maps the loss compares, by the reference's own at()
            h = min(Hs, Ht)
            ah_s = crit.at(F.adaptive_avg_pool2d(ts, (h, h)) if Hs > h else ts).numpy()
            ah_t = crit.at(F.adaptive_avg_pool2d(tt, (h, h)) if Ht > h else tt).numpy()
        want = A.pair(f_s, f_t)
        p = f"c{ci}_"
        out[p + "shape"] = np.array([B, Cs, Ct, Hs, Ht], dtype=np.int64)
        dF_s = ts.grad.numpy().copy()
        for b in range(B):                           # one array per image: the largest case alone would exceed a committed file
            out[f"{p}f_s_b{b}"], out[f"{p}f_t_b{b}"], out[f"{p}dF_s_b{b}"] = f_s[b], f_t[b], dF_s[b]
        out[p + "loss"] = np.array(loss.item(), np.float32)
        d = {"loss": abs(float(loss.item()) - want["loss"]) / abs(want["loss"]), "grad": rel(dF_s, want["dF_s"]),
             "map": max(rel(ah_s, want["ah_s"]), rel(ah_t, want["ah_t"]))}
        assert np.isfinite(dF_s).all() and (B == 1 or not dF_s[0].any())
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {CASES[ci]}: loss {loss.item():.6e}  " + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    print(golden_npz.save(os.path.join(OUT, "g12_at.npz"), out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/g15_sp*.npz by RUNNING THE REFERENCE's Similarity criterion (distiller_zoo/SP.py) on the CPU in fp32.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_sp.py

Cases (tests/sp_fixture.py CASES): one sample, two, three with a tiny K, K = 1 on the teacher's side, ragged K on both sides with
Ks != Kt, B one past each tile size of the kernels (16, 32, 64, 128), inputs offset by +3, SiLU applied to the draws (every Gram
entry positive, the loss far below the entries of H), an exactly duplicated row, an all-zero student row and an all-zero teacher row
(the clamp of F.normalize: Q_i = E_i / 1e-12), and one long-K case at B = 4 (student 1280 x 7 x 7, teacher 640 x 7 x 7) so that the
allowance is not taken from short sums only.  The inputs are standard normal draws ROUNDED TO BFLOAT16, seed 1500 + case, so that
fp32 and bf16 storage hold the same values; they are stored as their 16 bits.  (Not a 1/32 grid: on it the fp32 Gram is exact and
the G allowance would collapse to its floor.)  Per case: f_s, f_t, the reference's loss and d loss / d f_s (the long case: every 4th
column of it, to stay far below the size limit of a committed file), and their distance from the float64 evaluation of the formulas
(tests/sp_ref.py): `ref_vs_f64_loss` relative to the loss (B = 1: absolute), `ref_vs_f64_grad` over the whole gradient,
`ref_vs_f64_G` and `ref_vs_f64_H` for the reference's fp32 mm and F.normalize of both sides (crd_ref.rel's metric).  The tests
allow the kernels twice the largest distance of each kind.  Only arrays are written; no reference source text."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import sp_ref as R, sp_fixture as FX, golden_npz  # noqa: E402
from tests.crd_ref import rel  # noqa: E402


def inputs(ci):
    B, ss, st, note = FX.CASES[ci]
    rng = np.random.default_rng(1500 + ci)
    f_s, f_t = rng.standard_normal((B,) + ss), rng.standard_normal((B,) + st)
    if note == "+3":
        f_s, f_t = f_s + 3, f_t + 3
    if note == "silu":
        f_s, f_t = f_s / (1 + np.exp(-f_s)), f_t / (1 + np.exp(-f_t))
    if note == "dup":
        f_s[FX.DUP[1]], f_t[FX.DUP[1]] = f_s[FX.DUP[0]], f_t[FX.DUP[0]]
    if note == "zero":
        f_s[FX.ZERO_S], f_t[FX.ZERO_T] = 0, 0
    to = lambda a: torch.from_numpy(a).float().bfloat16().float().numpy()          # noqa: E731  (round to nearest even)
    return to(f_s), to(f_t)


def main():
    sys.path.insert(0, REF)
    from distiller_zoo.SP import Similarity
    crit = Similarity()
    out = {"n_cases": np.array(len(FX.CASES))}
    any_G = False
    for ci, (B, ss, st, note) in enumerate(FX.CASES):
        f_s, f_t = inputs(ci)
        ts, tt = torch.from_numpy(f_s).requires_grad_(True), torch.from_numpy(f_t)
        loss, = crit([ts], [tt])
        assert tuple(loss.shape) == (1,)
        loss.sum().backward()
        dF_s = ts.grad.numpy().copy()
        want = R.pair(f_s, f_t)
        assert np.isfinite(loss.item()) and np.isfinite(dF_s).all()
        dG = dH = 0.0
        with torch.no_grad():
            for f, side in ((ts, "s"), (tt, "t")):
                x = f.detach().reshape(B, -1)
                G32 = torch.mm(x, x.t())
                H32 = torch.nn.functional.normalize(G32, dim=1)
                dG = max(dG, rel(G32.numpy(), want["G_" + side]))
                dH = max(dH, rel(H32.numpy(), want["H_" + side]))
        any_G |= dG > 0
        p = f"c{ci}_"
        out[p + "f_s_bf16"], out[p + "f_t_bf16"] = FX.bf16_bits(f_s), FX.bf16_bits(f_t)
        if note == "long":
            out[p + "dF_s_cols"] = np.ascontiguousarray(dF_s.reshape(B, -1)[:, ::FX.LONG_STRIDE])
        else:
            out[p + "dF_s"] = dF_s
        out[p + "loss"] = np.array(loss.item(), np.float32)
        d = {"loss": abs(float(loss.item()) - want["loss"]) / want["loss"] if B > 1 else abs(float(loss.item()) - want["loss"]),
             "grad": rel(dF_s, want["dF_s"]) if np.abs(want["dF_s"]).max() > 0 else float(np.abs(dF_s).max()), "G": dG, "H": dH}
        for k_, v_ in d.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
        print(f"case {ci} {FX.CASES[ci]}: loss {loss.item():.6e} (f64 {want['loss']:.6e})  " + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in d.items()))
    assert any_G, "the fp32 Gram is exact in every case: the G allowance would be its floor"
    for k_, v_ in out.items():
        assert v_.nbytes < (600 << 10), (k_, v_.nbytes)
    print(golden_npz.save(os.path.join(OUT, "g15_sp.npz"), out))


if __name__ == "__main__":
    main()

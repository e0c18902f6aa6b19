#!/usr/bin/env python3
"""Generate tests/golden/g11_crd.npz by RUNNING THE REFERENCE's CRD criterion (crd/criterion.py, crd/memory.py) on the CPU.

Run where the reference checkout is available (MOMA_REFERENCE, default /root/reference); the tests only read the committed .npz:

    python tests/golden/make_golden_crd.py

Cases (B, d, nce_k, n_data): (8, 64, 256, 600) and (6, 128, 1000, 900) with distinct y, three consecutive steps each (step 1 sets
Z, steps 2 - 3 reuse it and see the updated banks), and (8, 64, 256, 600) with a repeated y, one step.  Per step: f_s, f_t, idx
(int32), out_v1, out_v2, the two loss terms, dL/dv1, dL/dv2, the gradients of the embed weights, params, the bank rows at y after the
update; per case the embed weights and the initial banks.  Next to every floating-point result: its distance (tests/crd_ref.rel,
or relative for scalars) from the float64 evaluation of the formulas (tests/crd_ref.py) with Z taken as the reference's stored fp32
value -- `ref_vs_f64_*`: the tests allow the kernels twice that.  Only arrays are written; no reference source text is stored.
Shims: `.cuda()` patched to identity (tensors, modules, AliasMethod)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("MOMA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import crd_ref as R, golden_npz  # noqa: E402

CASES = [  # (B, d, nce_k, n_data, s_dim, t_dim, steps, repeated y)
    (8, 64, 256, 600, 24, 40, 3, False),
    (6, 128, 1000, 900, 32, 48, 3, False),
    (8, 64, 256, 600, 24, 40, 1, True),
]


def _shims():
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    from crd import memory
    memory.AliasMethod.cuda = lambda self: None


def main():
    _shims()
    from crd.criterion import CRDLoss
    out = {"n_cases": np.array(len(CASES))}
    for ci, (B, d, K, n_data, s_dim, t_dim, steps, rep) in enumerate(CASES):
        torch.manual_seed(1100 + ci)
        rng = np.random.default_rng(1100 + ci)
        opt = types.SimpleNamespace(s_dim=s_dim, t_dim=t_dim, feat_dim=d, nce_k=K, nce_t=0.07, nce_m=0.5, n_data=n_data)
        crit = CRDLoss(opt)
        p = f"c{ci}_"
        out[p + "shape"] = np.array([B, d, K, n_data, s_dim, t_dim, steps, int(rep)], dtype=np.int64)
        for n_, t_ in (("ws", crit.embed_s.linear.weight), ("bs", crit.embed_s.linear.bias), ("wt", crit.embed_t.linear.weight),
                       ("bt", crit.embed_t.linear.bias), ("memory_v1", crit.contrast.memory_v1),
                       ("memory_v2", crit.contrast.memory_v2), ("params0", crit.contrast.params)):
            out[p + n_] = t_.detach().numpy().copy()
        worst = {}
        for st in range(steps):
            q = f"{p}s{st}_"
            y = rng.permutation(n_data)[:B].astype(np.int64)
            if rep:
                y[5] = y[2]
                y[7] = y[2]
            idx = rng.integers(0, n_data, size=(B, K + 1)).astype(np.int64)
            idx[:, 0] = y
            f_s = torch.randn(B, s_dim, requires_grad=True)
            f_t = torch.randn(B, t_dim, requires_grad=True)
            m1 = crit.contrast.memory_v1.numpy().copy()
            m2 = crit.contrast.memory_v2.numpy().copy()
            # the reference's forward, step by step as CRDLoss.forward runs it, keeping the intermediate tensors
            crit.zero_grad()
            v1 = crit.embed_s(f_s); v1.retain_grad()
            v2 = crit.embed_t(f_t); v2.retain_grad()
            o1, o2 = crit.contrast(v1, v2, torch.from_numpy(y), torch.from_numpy(idx))
            l1, l2 = crit.criterion_s(o1), crit.criterion_t(o2)
            (l1 + l2).sum().backward()
            params = crit.contrast.params.detach().numpy().copy()
            got = {"out_v1": o1.detach().numpy()[:, :, 0], "out_v2": o2.detach().numpy()[:, :, 0],
                   "loss": np.array([l1.item(), l2.item()], np.float32), "dv1": v1.grad.numpy(), "dv2": v2.grad.numpy(),
                   "dws": crit.embed_s.linear.weight.grad.numpy(), "dbs": crit.embed_s.linear.bias.grad.numpy(),
                   "dwt": crit.embed_t.linear.weight.grad.numpy(), "dbt": crit.embed_t.linear.bias.grad.numpy(),
                   "rows_v1": crit.contrast.memory_v1.numpy()[y], "rows_v2": crit.contrast.memory_v2.numpy()[y]}
            out[q + "f_s"], out[q + "f_t"] = f_s.detach().numpy(), f_t.detach().numpy()
            out[q + "idx"] = idx.astype(np.int32)
            out[q + "params"] = params
            for k_, a_ in got.items():
                out[q + k_] = np.ascontiguousarray(a_).copy()
            # float64 evaluation with the reference's stored fp32 Z
            T, mom = float(params[1]), float(params[4])
            e1, c1 = R.embed(out[q + "f_s"], out[p + "ws"], out[p + "bs"])
            e2, c2 = R.embed(out[q + "f_t"], out[p + "wt"], out[p + "bt"])
            s1 = R.side(e1, m2, idx, T, float(params[2]))
            s2 = R.side(e2, m1, idx, T, float(params[3]))
            dws, dbs = R.embed_bwd(s1["dv"], c1)
            dwt, dbt = R.embed_bwd(s2["dv"], c2)
            want = {"out_v1": s1["x"], "out_v2": s2["x"], "dv1": s1["dv"], "dv2": s2["dv"], "dws": dws, "dbs": dbs, "dwt": dwt,
                    "dbt": dbt, "rows_v1": R.update(m1, e1, y, mom)[y], "rows_v2": R.update(m2, e2, y, mom)[y]}
            dist = {k_: R.rel(got[k_], w_) for k_, w_ in want.items()}
            dist["loss"] = max(abs(float(got["loss"][0]) - s1["loss"]) / abs(s1["loss"]), abs(float(got["loss"][1]) - s2["loss"]) / abs(s2["loss"]))
            dist["dv"] = max(dist.pop("dv1"), dist.pop("dv2"))
            dist["out"] = max(dist.pop("out_v1"), dist.pop("out_v2"))
            dist["rows"] = max(dist.pop("rows_v1"), dist.pop("rows_v2"))
            dist["dw"] = max(dist.pop("dws"), dist.pop("dwt"))
            dist["db"] = max(dist.pop("dbs"), dist.pop("dbt"))
            if st == 0:
                z1, z2 = R.z_of(s1["e"], n_data), R.z_of(s2["e"], n_data)
                dist["z"] = max(abs(float(params[2]) - z1) / z1, abs(float(params[3]) - z2) / z2)
            for k_, v_ in dist.items():
                worst[k_] = max(worst.get(k_, 0.0), v_)
            print(f"case {ci} step {st}: loss {got['loss']}  Z {params[2:4]}  " + "  ".join(f"{k_} {v_:.2e}" for k_, v_ in dist.items()))
        for k_, v_ in worst.items():
            out[p + "ref_vs_f64_" + k_] = np.array(v_, np.float64)
    print(golden_npz.save(os.path.join(OUT, "g11_crd.npz"), out))


if __name__ == "__main__":
    main()

"""numpy restatement of the Neuron Selectivity Transfer formulas (include/moma_hip.h, NST section; reference distiller_zoo/NST.py,
its `full_loss = False` branch), evaluated in float64 unless told otherwise.  The yardstick of the NST tests: the golden fixture
records how far the reference's own fp32 results are from this evaluation, and the kernels are allowed twice that."""
import numpy as np

from tests.at_ref import pool, pool_bwd

EPS = 1e-12


def common_grid(f_s, f_t):
    """the reference's pooling: equal heights pass as they are, otherwise the larger map goes to (h, h), h the smaller height
    -> (f_s, f_t, which side was pooled: 's', 't' or None)"""
    hs, ht = f_s.shape[2], f_t.shape[2]
    if hs > ht:
        return pool(f_s, ht, ht), f_t, "s"
    if hs < ht:
        return f_s, pool(f_t, hs, hs), "t"
    return f_s, f_t, None


def pair(f_s, f_t, g_loss=1.0, dtype=np.float64):
    """-> dict(G [B,Cs,Cs+Ct], norms [B,Cs+Ct] (clamped), rows [B,Cs,2], t1, t2, loss, dF_s) for one feature pair"""
    f_s0, f_t = np.asarray(f_s, dtype), np.asarray(f_t, dtype)
    f_s, f_t, pooled = common_grid(f_s0, f_t)
    B, Cs = f_s.shape[:2]
    Ct = f_t.shape[1]
    X, Y = f_s.reshape(B, Cs, -1), f_t.reshape(B, Ct, -1)
    n = np.maximum(np.sqrt((X * X).sum(-1)), EPS)                  # [B, Cs]
    m = np.maximum(np.sqrt((Y * Y).sum(-1)), EPS)                  # [B, Ct]
    Gss = np.einsum("bip,bjp->bij", X, X) / (n[:, :, None] * n[:, None, :])
    Gst = np.einsum("bip,bjp->bij", X, Y) / (n[:, :, None] * m[:, None, :])
    t1, t2 = (Gss * Gss).mean(), (Gst * Gst).mean()
    alpha, beta = 4.0 / (B * Cs * Cs), 4.0 / (B * Cs * Ct)
    rows = np.stack([(Gss * Gss).sum(-1), (Gst * Gst).sum(-1)], -1)
    r = alpha * rows[..., 0] - beta * rows[..., 1]
    dX = (np.einsum("bij,bjp->bip", alpha * Gss / n[:, None, :], X) - np.einsum("bij,bjp->bip", beta * Gst / m[:, None, :], Y)
          - (r / n)[:, :, None] * X) / n[:, :, None]
    dF = g_loss * dX.reshape(f_s.shape)
    if pooled == "s":
        dF = pool_bwd(dF, f_s0.shape[2], f_s0.shape[3])
    return {"G": np.concatenate([Gss, Gst], -1), "norms": np.concatenate([n, m], -1), "rows": rows, "t1": t1, "t2": t2,
            "loss": t1 - 2.0 * t2, "dF_s": dF}


def loss_of(feats_s, feats_t):
    """the loop's KD term: sum of the pair losses over zip(feats_s, feats_t)"""
    return sum(pair(a, b)["loss"] for a, b in zip(feats_s, feats_t))

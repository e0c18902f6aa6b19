"""numpy restatement of the Probabilistic Knowledge Transfer formulas (include/moma_hip.h, PKT section; reference
distiller_zoo/PKT.py), evaluated in float64.  The yardstick of the PKT tests: the golden fixture records how far the reference's own
fp32 results are from this evaluation, and the kernels are allowed twice that.

Everything is a function of the two raw B x B Gram matrices G = F F^T; the norms are the square roots of their diagonals.  An
all-zero student row gets the finite gradient sum_j M'_ij x_j -- the derivative of x / (|x| + eps) at 0, no diagonal term -- where the
reference's autograd returns NaN (sqrt's backward at 0); the documented deviation."""
import numpy as np

EPS = 1e-7


def side(f):
    """[B, ...] -> G [B, B], n [B], C [B, B], K [B, B], r [B], P [B, B] in float64"""
    X = np.asarray(f, np.float64).reshape(len(f), -1)
    G = X @ X.T
    G = np.triu(G) + np.triu(G, 1).T                                      # (BLAS need not be symmetric to the bit)
    n = np.sqrt(np.diag(G))
    C = G / ((n[:, None] + EPS) * (n[None, :] + EPS))
    K = (C + 1.0) / 2.0
    r = K.sum(1)
    return G, n, C, K, r, K / r[:, None]


def pair(f_s, f_t, g_loss=1.0):
    """-> dict(G_s, G_t, C_s, C_t, P, T, W, M (the M' of the header: dF_s = g M X), loss, abs_terms, dF_s (shape of f_s))"""
    X = np.asarray(f_s, np.float64).reshape(len(f_s), -1)
    B = len(X)
    G_s, n, C_s, _K, r, P = side(f_s)
    G_t, _n, C_t, _Kt, _rt, T = side(f_t)
    terms = T * np.log((T + EPS) / (P + EPS))
    U = -T / (P + EPS) / B ** 2
    s = (U * P).sum(1)
    W = (U - s[:, None]) / (2.0 * r[:, None])
    M = W + W.T
    c = (M * C_s).sum(1)
    Mp = M / ((n[:, None] + EPS) * (n[None, :] + EPS))
    with np.errstate(divide="ignore", invalid="ignore"):
        Mp[np.arange(B), np.arange(B)] -= np.where(n > 0, c / (n * (n + EPS)), 0.0)
    dF = g_loss * (Mp @ X)
    return {"G_s": G_s, "G_t": G_t, "C_s": C_s, "C_t": C_t, "P": P, "T": T, "W": W, "M": Mp, "loss": terms.sum() / B ** 2,
            "abs_terms": np.abs(terms).sum() / B ** 2, "dF_s": dF.reshape(np.shape(f_s))}

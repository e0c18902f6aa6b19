"""numpy restatement of the Similarity-Preserving distillation formulas (include/moma_hip.h, SP section; reference
distiller_zoo/SP.py), evaluated in float64.  The yardstick of the SP tests: the golden fixture records how far the reference's own
fp32 results are from this evaluation, and the kernels are allowed twice that.

X = f_s as [B, Ks], Y = f_t as [B, Kt]; G = X X^T, n_i = |G_i|_2, H = G / max(n, 1e-12) row-wise (per side);
loss = (1/B^2) sum_ij (H^t_ij - H^s_ij)^2; E = -(2/B^2) (H^t - H^s); Q_i = (E_i - (E_i . H^s_i) H^s_i) / n^s_i where n^s_i >= 1e-12 and
E_i / 1e-12 where the clamp holds (F.normalize's backward); dX = g (Q + Q^T) X.  G does not depend on the order of the K columns, so
`pair` may be fed a map in any memory order as long as dF_s is read back in the same one."""
import numpy as np

EPS = 1e-12


def gram(f):
    """[B, ...] -> G [B, B] float64"""
    X = np.asarray(f, np.float64).reshape(len(f), -1)
    return X @ X.T


def normalised(G):
    """-> (H, n): every row of G divided by max(its L2 norm, 1e-12); n is the norm itself, not clamped"""
    n = np.sqrt((G * G).sum(1))
    return G / np.maximum(n, EPS)[:, None], n


def pair(f_s, f_t, g_loss=1.0):
    """-> dict(G_s, G_t, H_s, H_t, n_s, n_t, loss, Q, M, dF_s (shape of f_s))"""
    X = np.asarray(f_s, np.float64).reshape(len(f_s), -1)
    B = len(X)
    G_s, G_t = gram(f_s), gram(f_t)
    (H_s, n_s), (H_t, n_t) = normalised(G_s), normalised(G_t)
    D = H_t - H_s
    E = -(2.0 / B ** 2) * D
    r = (E * H_s).sum(1)
    Q = np.where((n_s >= EPS)[:, None], (E - r[:, None] * H_s) / np.maximum(n_s, EPS)[:, None], E / EPS)
    M = Q + Q.T
    return {"G_s": G_s, "G_t": G_t, "H_s": H_s, "H_t": H_t, "n_s": n_s, "n_t": n_t, "loss": float((D * D).sum() / B ** 2), "Q": Q,
            "M": M, "dF_s": (g_loss * (M @ X)).reshape(np.shape(f_s))}

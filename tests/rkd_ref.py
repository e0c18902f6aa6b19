"""numpy restatement of the Relational Knowledge Distillation formulas (include/moma_hip.h, RKD section; reference
distiller_zoo/RKD.py), evaluated in float64.  The yardstick of the RKD tests: the golden fixture records how far the reference's own
fp32 results are from this evaluation, and the kernels are allowed twice that.

Everything is a function of the B x B matrices of pairwise SQUARED distances S (summed from the differences: exactly 0 on the
diagonal and for equal rows); the angle term follows from the law of cosines, (x_b - x_a).(x_c - x_a) = (S_ab + S_ac - S_bc) / 2.
A pair of exactly equal student rows contributes value 0 and gradient 0 to the angle term (the documented deviation from the
reference's autograd, which divides by F.normalize's clamp 1e-12 there)."""
import numpy as np

EPS = 1e-12


def sqdist(f):
    """[B, ...] -> S [B, B] float64, S_ij = sum_k (x_ik - x_jk)^2 from the differences"""
    X = np.asarray(f, np.float64).reshape(len(f), -1)
    S = np.empty((len(X), len(X)))
    for i in range(len(X)):
        d = X - X[i]
        S[i] = (d * d).sum(-1)
    return S


def sl1(z):
    a = np.abs(z)
    return np.where(a < 1, 0.5 * z * z, a - 0.5)


def _dist(S):
    B = len(S)
    d = np.sqrt(np.maximum(S, EPS))
    d[np.arange(B), np.arange(B)] = 0
    return d, d.sum() / (B * (B - 1))


def _recip(S):
    """1 / n with n = max(sqrt(S), 1e-12), and 0 where S = 0 (that entry's angles are 0 and carry no gradient)"""
    return np.where(S > 0, 1.0 / np.maximum(np.sqrt(S), EPS), 0.0)


def angles(S):
    """A[a, b, c] = (S_ab + S_ac - S_bc) / (2 n_ab n_ac), 0 wherever S_ab = 0 or S_ac = 0"""
    R = _recip(S)
    return (S[:, :, None] + S[:, None, :] - S[None, :, :]) * 0.5 * R[:, :, None] * R[:, None, :]


def pair(f_s, f_t, w_d=25.0, w_a=50.0, g_loss=1.0):
    """-> dict(S_s, S_t, mu_s, mu_t, l_d, l_a, loss, Q [B,B] = d loss / d S_s (entries independent), dF_s (shape of f_s))"""
    X = np.asarray(f_s, np.float64).reshape(len(f_s), -1)
    B = len(X)
    S_s, S_t = sqdist(f_s), sqdist(f_t)
    d_s, mu_s = _dist(S_s)
    d_t, mu_t = _dist(S_t)
    z = d_s / mu_s - d_t / mu_t
    l_d = sl1(z).sum() / B ** 2
    e = np.clip(z, -1, 1) / B ** 2
    E = (e * d_s / mu_s).sum()
    off = ~np.eye(B, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        Q = np.where(off & (S_s >= EPS), w_d * (e - E / (B * (B - 1))) / mu_s / (2 * d_s), 0.0)
    A_s, A_t = angles(S_s), angles(S_t)
    zA = A_s - A_t
    l_a = sl1(zA).sum() / B ** 3
    h = w_a * np.clip(zA, -1, 1) / B ** 3
    R = _recip(S_s)
    RR = R[:, :, None] * R[:, None, :]                                    # 1 / (n_ab n_ac)
    Q = Q + (h * (-0.5) * RR).sum(0)                                      # S_bc, the side opposite the anchor
    own = np.where(np.sqrt(S_s) >= EPS, R * R, 0.0)                       # 1 / n_ab^2 where n_ab follows S_ab (not clamped)
    Q = Q + 2 * (h * (0.5 * RR - A_s * 0.5 * own[:, :, None])).sum(2)     # S_ab and, by the b <-> c symmetry, S_ac
    M = -2.0 * (Q + Q.T)
    M[~off] = 0
    M[~off] = -M.sum(1)
    dF = g_loss * (M @ (X - X.mean(0)))
    return {"S_s": S_s, "S_t": S_t, "mu_s": mu_s, "mu_t": mu_t, "l_d": l_d, "l_a": l_a, "loss": w_d * l_d + w_a * l_a, "Q": Q,
            "dF_s": dF.reshape(np.shape(f_s))}

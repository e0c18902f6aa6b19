"""numpy float64 restatement of Variational Information Distillation (include/moma_hip.h, section VID; reference
distiller_zoo/VID.py): the Gaussian negative log-likelihood with its gradients, and the whole criterion -- pooling to the common
grid, the bias-free regressor conv1x1 -> ReLU -> conv1x1 -> ReLU -> conv1x1, the likelihood -- with the gradients of the input and of
every parameter.  The yardstick of tests/test_vid_cpu.py and tests/test_gpu_vid.py."""
import numpy as np


def softplus(x):
    """log(1 + exp(x)) without overflow"""
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def nll(mean, target, log_scale, eps=1e-5, g_loss=1.0):
    """mean, target [B,C,H,W], log_scale [C] -> dict(loss, d_mean, d_ls (both times g_loss), S [C], var [C], abs_terms: the sum of
    the loss's terms taken by magnitude, 0.5 (mean d^2 / var + mean_c |log var_c|))"""
    m, t, ls = np.asarray(mean, np.float64), np.asarray(target, np.float64), np.asarray(log_scale, np.float64)
    B, C, H, W = m.shape
    n = B * H * W
    var = softplus(ls) + np.float64(eps)
    d = m - t
    S = (d * d).sum(axis=(0, 2, 3))
    loss = 0.5 / C * (S / (n * var) + np.log(var)).sum()
    d_var = 0.5 / C * (1 / var - S / (n * var * var))
    return {"loss": float(loss), "d_mean": g_loss * d / (var.reshape(1, C, 1, 1) * n * C), "d_ls": g_loss * d_var * sigmoid(ls),
            "S": S, "var": var, "abs_terms": float(0.5 / C * (S / (n * var) + np.abs(np.log(var))).sum())}


def pool_matrix(n_in, n_out):
    """[n_out, n_in]: adaptive_avg_pool's windows [floor(i n_in / n_out), ceil((i + 1) n_in / n_out)) along one axis"""
    A = np.zeros((n_out, n_in))
    for i in range(n_out):
        lo, hi = (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)
        A[i, lo:hi] = 1.0 / (hi - lo)
    return A


def pool(x, h):
    """adaptive_avg_pool2d(x, (h, h)) -> (pooled, backward: gradient of the pooled map -> gradient of x)"""
    x = np.asarray(x, np.float64)
    Ah, Aw = pool_matrix(x.shape[2], h), pool_matrix(x.shape[3], h)
    return np.einsum("yh,bchw,xw->bcyx", Ah, x, Aw), lambda g: np.einsum("yh,bcyx,xw->bchw", Ah, g, Aw)


def conv1x1(x, w):
    return np.einsum("oi,bihw->bohw", np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1]), x)


def criterion(x, target, weights, log_scale, eps=1e-5, g_loss=1.0):
    """VIDLoss.forward and its backward: x [B,Cs,Hs,Ws], target [B,Ct,Ht,Wt], weights (w0, w1, w2) of the regressor ([out, in] or
    [out, in, 1, 1]) -> dict(pred_mean, target (on the common grid), loss, d_mean, d_ls, dx, dw (list of three, [out, in]), S, var,
    abs_terms).  No gradient goes to the target."""
    x, target = np.asarray(x, np.float64), np.asarray(target, np.float64)
    back = None
    if x.shape[2] > target.shape[2]:
        x_in, back = pool(x, target.shape[2])
    else:
        x_in = x
        if x.shape[2] < target.shape[2]:
            target, _ = pool(target, x.shape[2])
    w = [np.asarray(v, np.float64).reshape(v.shape[0], v.shape[1]) for v in weights]
    z0 = conv1x1(x_in, w[0])
    a0 = np.maximum(z0, 0)
    z1 = conv1x1(a0, w[1])
    a1 = np.maximum(z1, 0)
    pm = conv1x1(a1, w[2])
    out = nll(pm, target, log_scale, eps, g_loss)
    g2 = out["d_mean"]
    dw2 = np.einsum("bohw,bihw->oi", g2, a1)
    g1 = np.einsum("oi,bohw->bihw", w[2], g2) * (z1 > 0)
    dw1 = np.einsum("bohw,bihw->oi", g1, a0)
    g0 = np.einsum("oi,bohw->bihw", w[1], g1) * (z0 > 0)
    dw0 = np.einsum("bohw,bihw->oi", g0, x_in)
    dx = np.einsum("oi,bohw->bihw", w[0], g0)
    out.update(pred_mean=pm, target=target, dx=back(dx) if back is not None else dx, dw=[dw0, dw1, dw2])
    return out

"""Float64 numpy restatement of what csrc/semckd.hip and moma_sp_gram_sum compute (`--distill semckd`): the attention-weighted
per-sample mean squared error of a group of (student, teacher) pairs with its gradients, and the batch Gram matrix with its backward.
Written from the formulas of include/moma_hip.h, not from any implementation."""
import numpy as np


def tail(xs, ts, w, g=1.0):
    """xs[p], ts[p]: [B, ...] arrays of pair p = i T + j; w [B, S, T]; g the upstream gradient of the loss ->
    dict(ind [B, S, T], loss, dx (list, each in xs[p]'s shape), dw [B, S, T]), all float64"""
    w = np.asarray(w, np.float64)
    B, S, T = w.shape
    assert len(xs) == len(ts) == S * T
    ind = np.empty((B, S * T))
    dx = []
    for p, (x, t) in enumerate(zip(xs, ts)):
        d = np.asarray(x, np.float64) - np.asarray(t, np.float64)
        n = d[0].size
        ind[:, p] = (d.reshape(B, -1) ** 2).sum(1) / n
        wp = w.reshape(B, S * T)[:, p].reshape((B,) + (1,) * (d.ndim - 1))
        dx.append(g * 2.0 * wp / (n * B * S) * d)
    ind = ind.reshape(B, S, T)
    return {"ind": ind, "loss": float((w * ind).sum() / (B * S)), "dx": dx, "dw": g * ind / (B * S)}


def gram(x):
    """G = X X^T of x [B, ...] read as [B, K], float64"""
    X = np.asarray(x, np.float64).reshape(len(x), -1)
    return X @ X.T


def gram_abs(x):
    """|X| |X|^T: what the rounding bound of moma_sp_gram_sum is stated in"""
    X = np.abs(np.asarray(x, np.float64).reshape(len(x), -1))
    return X @ X.T


def gram_bwd(x, dG):
    """dX = (dG + dG^T) X in x's shape, float64"""
    X = np.asarray(x, np.float64).reshape(len(x), -1)
    dG = np.asarray(dG, np.float64)
    return ((dG + dG.T) @ X).reshape(np.shape(x))

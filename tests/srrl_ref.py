"""numpy float64 restatement of SRRL (include/moma_hip.h, section SRRL; reference models/util.py SRRL with nn.MSELoss twice):
training-mode BatchNorm -> ReLU -> mean squared error against the teacher's feature, plus the teacher's classifier -> mean squared
error against the teacher's logits, with every gradient and the running statistics, and the chain with the bias-free 1 x 1
convolution in front.  The yardstick of tests/test_srrl_cpu.py and tests/test_gpu_srrl.py.

The ReLU has the kink of the FitNets hint: every test input goes through tests/hint_ref.clear_of_kink (`clear`, tau = 2^-10), a
condition on the inputs: no element is left out of a comparison."""
import numpy as np

from tests import hint_ref

TAU = hint_ref.TAU


def clear(x, gamma, beta, eps):
    """x [B, C] -> x with no float64 |pre-activation| below TAU"""
    x = np.asarray(x, np.float64)
    return hint_ref.clear_of_kink(x[:, :, None, None], gamma, beta, eps, TAU)[:, :, 0, 0]


def pre_activation(x, gamma, beta, eps):
    return hint_ref.pre_activation(np.asarray(x, np.float64)[:, :, None, None], gamma, beta, eps)[:, :, 0, 0]


def tail(x, t, W, b, l, gamma, beta, eps=1e-5, g_loss=1.0, running_mean=None, running_var=None, momentum=0.1):
    """x (the convolution's output), t [B, C], W [K, C], b [K] or None, l [B, K], gamma, beta [C] -> dict(loss, loss_feat, loss_pred, dx,
    d_gamma, d_beta (the three gradients times g_loss), mean, var, invstd, A, B, y, p, running_mean, running_var (after the step))"""
    x, t, W, l = (np.asarray(v, np.float64) for v in (x, t, W, l))
    ga, be = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    Bn, C = x.shape
    K = W.shape[0]
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    invstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * invstd
    y = np.maximum(ga * xh + be, 0)
    p = y @ W.T + (0.0 if b is None else np.asarray(b, np.float64))
    d, e = y - t, p - l
    dY = 2.0 / (Bn * C) * d + 2.0 / (Bn * K) * (e @ W)
    g = dY * (y > 0)
    A, Bs = g.sum(axis=0), (g * xh).sum(axis=0)
    dx = g_loss * ga * invstd * (g - A / Bn - xh * Bs / Bn)
    lf, lp = float((d * d).sum() / (Bn * C)), float((e * e).sum() / (Bn * K))
    out = {"loss": lf + lp, "loss_feat": lf, "loss_pred": lp, "dx": dx, "d_gamma": g_loss * Bs, "d_beta": g_loss * A, "mean": mean,
           "var": var, "invstd": invstd, "A": A, "B": Bs, "y": y, "p": p}
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
        out["running_var"] = (1 - momentum) * np.asarray(running_var, np.float64) + momentum * var * Bn / (Bn - 1)
    return out


def chain(f_s, t, w, W, b, l, gamma, beta, eps=1e-5, g_loss=1.0, running_mean=None, running_var=None, momentum=0.1):
    """the connector's bias-free 1 x 1 convolution in front: f_s [B, s_n], w [t_n, s_n(, 1, 1)] -> tail's dict for the convolution's
    output plus conv_out, dx_s, dw"""
    w2 = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1])
    f = np.asarray(f_s, np.float64)
    z = f @ w2.T
    out = tail(z, t, W, b, l, gamma, beta, eps, g_loss, running_mean, running_var, momentum)
    out["conv_out"] = z
    out["dx_s"] = out["dx"] @ w2
    out["dw"] = out["dx"].T @ f
    return out

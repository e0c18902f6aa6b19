"""numpy float64 restatement of the FitNets hint (include/moma_hip.h, section HINT; reference models/util.py ConvReg and
distiller_zoo/FitNet.py HintLoss): training-mode BatchNorm -> ReLU -> mean squared error with every gradient and the running
statistics, and the whole ConvReg chain for the 1 x 1 branch (convolution with bias in front).  The yardstick of
tests/test_hint_cpu.py and tests/test_gpu_hint.py.

The loss has a kink where the pre-activation gamma xh + beta crosses 0: there the gradient jumps by (y - t), so a comparison of
gradients means something only away from it.  `clear_of_kink` moves every input element whose float64 |pre-activation| is below tau by
+1/8 until none is left; every test input goes through it.  It is a condition on the inputs: no element is left out of a comparison."""
import numpy as np

TAU = 2.0 ** -10            # far above fp32's error in the pre-activation for inputs of magnitude below 8


def bn_stats(x, eps):
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=(0, 2, 3))
    var = ((x - mean.reshape(1, -1, 1, 1)) ** 2).mean(axis=(0, 2, 3))          # (sum x^2 / M - mean^2 without the cancellation)
    return mean, var, 1.0 / np.sqrt(var + eps)


def pre_activation(x, gamma, beta, eps):
    x = np.asarray(x, np.float64)
    mean, _var, invstd = bn_stats(x, eps)
    sh = (1, -1, 1, 1)
    xh = (x - mean.reshape(sh)) * invstd.reshape(sh)
    return np.asarray(gamma, np.float64).reshape(sh) * xh + np.asarray(beta, np.float64).reshape(sh)


def clear_of_kink(x, gamma, beta, eps, tau=TAU):
    """-> x with every element whose float64 |pre-activation| is below tau moved by +1/8, repeated until none is left (moving an element
    moves the statistics, so the others are looked at again).  A channel whose pre-activation does not depend on x (gamma = 0, or a
    constant channel) is left alone."""
    x = np.array(x, dtype=np.float64)
    g = np.asarray(gamma, np.float64).reshape(1, -1, 1, 1)
    for _ in range(1000):
        _m, var, _i = bn_stats(x, eps)
        live = (g != 0) & (var.reshape(1, -1, 1, 1) > 0)
        near = (np.abs(pre_activation(x, gamma, beta, eps)) < tau) & live
        if not near.any():
            return x
        x[near] += 0.125
    raise RuntimeError("clear_of_kink: no input clear of the kink found")


def tail(x, t, gamma, beta, eps=1e-5, g_loss=1.0, running_mean=None, running_var=None, momentum=0.1, conv_bias=None):
    """x (the convolution's output), t [B,C,H,W], gamma, beta [C] -> dict(loss, dx, d_gamma, d_beta (all three times g_loss), mean, var,
    invstd, A, B, y, running_mean, running_var (after the step; conv_bias, when given, is added to the mean for running_mean))"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    ga, be = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    Bn, C, H, W = x.shape
    M, N = Bn * H * W, x.size
    sh = (1, C, 1, 1)
    mean, var, invstd = bn_stats(x, eps)
    xh = (x - mean.reshape(sh)) * invstd.reshape(sh)
    y = np.maximum(ga.reshape(sh) * xh + be.reshape(sh), 0)
    d = y - t
    g = d * (y > 0)
    A, Bs = g.sum(axis=(0, 2, 3)), (g * xh).sum(axis=(0, 2, 3))
    k = 2.0 * g_loss / N
    dx = k * (ga * invstd).reshape(sh) * (g - A.reshape(sh) / M - xh * Bs.reshape(sh) / M)
    out = {"loss": float((d * d).sum() / N), "dx": dx, "d_gamma": k * Bs, "d_beta": k * A, "mean": mean, "var": var, "invstd": invstd,
           "A": A, "B": Bs, "y": y}
    if running_mean is not None:
        cb = 0.0 if conv_bias is None else np.asarray(conv_bias, np.float64)
        out["running_mean"] = (1 - momentum) * np.asarray(running_mean, np.float64) + momentum * (mean + cb)
        out["running_var"] = (1 - momentum) * np.asarray(running_var, np.float64) + momentum * var * M / (M - 1)
    return out


def conv1x1(x, w):
    return np.einsum("oi,bihw->bohw", np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1]), np.asarray(x, np.float64))


def chain(x_s, t, w, b, gamma, beta, eps=1e-5, g_loss=1.0, running_mean=None, running_var=None, momentum=0.1):
    """ConvReg (1 x 1 branch) + HintLoss and their backward: x_s [B,Cs,H,W], w [Ct,Cs(,1,1)], b [Ct] -> tail's dict for the
    convolution's output (bias included) plus conv_out, dx_s, dw, db (the analytic 0: sum xh = 0 per channel)"""
    w2 = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1])
    z = conv1x1(x_s, w2) + np.asarray(b, np.float64).reshape(1, -1, 1, 1)
    out = tail(z, t, gamma, beta, eps, g_loss, running_mean, running_var, momentum)
    out["conv_out"] = z
    out["dx_s"] = np.einsum("oi,bohw->bihw", w2, out["dx"])
    out["dw"] = np.einsum("bohw,bihw->oi", out["dx"], np.asarray(x_s, np.float64))
    out["db"] = out["dx"].sum(axis=(0, 2, 3))
    return out

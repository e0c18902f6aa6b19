"""numpy restatement of the Attention Transfer formulas (include/moma_hip.h, AT section; reference distiller_zoo/AT.py for p = 2),
evaluated in float64 unless told otherwise.  The yardstick of the attention tests: the golden fixture records how far the reference's
own fp32 results are from this evaluation, and the kernels are allowed twice that."""
import numpy as np

EPS = 1e-12


def _edges(n_in, n_out):
    """windows of adaptive average pooling: output i covers [floor(i n_in / n_out), ceil((i + 1) n_in / n_out))"""
    i = np.arange(n_out)
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


def pool(f, oh, ow):
    """adaptive_avg_pool2d(f, (oh, ow)); for H % oh == 0 and W % ow == 0 the windows are the H/oh x W/ow tiles"""
    B, C, H, W = f.shape
    if (oh, ow) == (H, W):
        return f
    y0, y1 = _edges(H, oh)
    x0, x1 = _edges(W, ow)
    out = np.empty((B, C, oh, ow), f.dtype)
    for i in range(oh):
        for j in range(ow):
            out[:, :, i, j] = f[:, :, y0[i]:y1[i], x0[j]:x1[j]].mean(axis=(2, 3))
    return out


def pool_bwd(dp, H, W):
    """gradient of `pool` w.r.t. its input: every window spreads its gradient evenly over its elements"""
    B, C, oh, ow = dp.shape
    if (oh, ow) == (H, W):
        return dp
    y0, y1 = _edges(H, oh)
    x0, x1 = _edges(W, ow)
    out = np.zeros((B, C, H, W), dp.dtype)
    for i in range(oh):
        for j in range(ow):
            out[:, :, y0[i]:y1[i], x0[j]:x1[j]] += dp[:, :, i:i + 1, j:j + 1] / ((y1[i] - y0[i]) * (x1[j] - x0[j]))
    return out


def grid(shape_s, shape_t):
    """the common output grid of a pair: the maps as they are for equal heights, (h, h) with h the smaller height otherwise"""
    hs, ht = shape_s[2], shape_t[2]
    if hs == ht:
        return hs, shape_s[3]
    h = min(hs, ht)
    return h, h


def amap(f, oh, ow):
    """a[b, y ow + x] = mean_c pool(f)[b,c,y,x]^2 -> (a [B, oh ow], pooled f)"""
    p = pool(f, oh, ow)
    return (p * p).mean(axis=1).reshape(f.shape[0], -1), p


def normalise(a):
    """-> (ah, norm [B,1], denominator [B,1])"""
    n = np.sqrt((a * a).sum(axis=1, keepdims=True))
    d = np.maximum(n, EPS)
    return a / d, n, d


def pair(f_s, f_t, g_loss=1.0, dtype=np.float64):
    """-> dict(a_s, a_t, ah_s, ah_t, norms [B,2], loss, g_s, g_t, dF_s, dF_t) for one feature pair"""
    f_s, f_t = np.asarray(f_s, dtype), np.asarray(f_t, dtype)
    oh, ow = grid(f_s.shape, f_t.shape)
    out = {}
    a_s, p_s = amap(f_s, oh, ow)
    a_t, p_t = amap(f_t, oh, ow)
    ah_s, n_s, d_s = normalise(a_s)
    ah_t, n_t, d_t = normalise(a_t)
    B, n = a_s.shape
    diff = ah_s - ah_t
    out.update(a_s=a_s, a_t=a_t, ah_s=ah_s, ah_t=ah_t, norms=np.concatenate([n_s, n_t], 1), loss=(diff * diff).sum() / (B * n))
    for side, sign, ah, nrm, d, p, f in (("s", 1.0, ah_s, n_s, d_s, p_s, f_s), ("t", -1.0, ah_t, n_t, d_t, p_t, f_t)):
        g_ah = sign * 2.0 * diff / (B * n)
        proj = np.where(nrm >= EPS, (ah * g_ah).sum(axis=1, keepdims=True), 0.0)      # under the clamp the denominator is constant
        g_a = (g_ah - ah * proj) / d
        C = f.shape[1]
        dp = g_loss * g_a.reshape(B, 1, oh, ow) * (2.0 / C) * p
        out["g_" + side] = g_a
        out["dF_" + side] = pool_bwd(dp, f.shape[2], f.shape[3])
    return out


def loss_of(feats_s, feats_t):
    """the loop's KD term: sum of the pair losses over zip(feats_s, feats_t)"""
    return sum(pair(a, b)["loss"] for a, b in zip(feats_s, feats_t))

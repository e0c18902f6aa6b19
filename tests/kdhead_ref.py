"""numpy restatement of the student head's formulas (include/moma_hip.h, section KDHEAD; reference: nn.CrossEntropyLoss,
distiller_zoo/KD.py DistillKL(T) and helper/util.accuracy as helper/loops_moma.py:278-279 calls them), evaluated in float64.  The
yardstick of the KD-head tests: the golden fixture records how far the reference's own fp32 results are from this evaluation, and the
kernels are allowed twice that.

    a = z / T                 p = softmax(a) per row
    lse_b = logsumexp z_s[b,:]       lseS_b = logsumexp a_s[b,:]       lseT_b = logsumexp a_t[b,:]
    ce_b  = lse_b - z_s[b, y_b]                              (a valid row: 0 <= y_b < K)
    kl_b  = sum_k p_t[b,k] (log p_t[b,k] - log p_s[b,k])     (a term with p_t = 0 counts 0)
    loss_cls = sum_valid ce_b / n_valid                      (n_valid = 0 -> NaN; a label outside [0, K) other than -100 -> NaN)
    loss_div = T^2 sum_b kl_b / B
    pred_b = the LOWEST index k with z_s[b,k] = max;  acc = 100 #{pred_b == y_b} / B
    dz_s[b,k] = g_cls (softmax(z_s)[b,k] - [k == y_b]) / n_valid    (zero for a row that is not valid)
              + g_div T (p_s[b,k] - p_t[b,k]) / B
"""
import numpy as np

from tests.ce_ref import IGNORE, MARGIN, margin  # noqa: F401  (one label rule and one margin for both heads)


def _lse(x):
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def head(z_s, z_t, y, T, g_cls=1.0, g_div=1.0):
    """-> dict(loss_cls, loss_div, acc, hits, n_valid, n_bad, lse, lseS, lseT [B], pred [B], kl [B], dz_cls, dz_div, dz [B, K]);
    dz = g_cls dz_cls + g_div dz_div, the two parts at weight 1"""
    zs, zt = np.asarray(z_s, np.float64), np.asarray(z_t, np.float64)
    y = np.asarray(y, np.int64)
    T = float(T)
    B, K = zs.shape
    lse, lseS, lseT = _lse(zs), _lse(zs / T), _lse(zt / T)
    pred = zs.argmax(axis=1)                                      # (numpy: the first occurrence)
    valid = (y >= 0) & (y < K)
    bad = ~valid & (y != IGNORE)
    ys = np.where(valid, y, 0)
    rows = np.where(valid, lse - zs[np.arange(B), ys], 0.0)
    n = int(valid.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss_cls = float("nan") if bad.any() else float(np.float64(rows.sum()) / np.float64(n))
    log_ps, log_pt = zs / T - lseS[:, None], zt / T - lseT[:, None]
    pt = np.exp(log_pt)
    with np.errstate(invalid="ignore"):
        kl = np.where(pt > 0, pt * (log_pt - log_ps), 0.0).sum(axis=1)
    loss_div = float(T * T * kl.sum() / B)
    onehot = np.zeros((B, K))
    onehot[np.arange(B), ys] = 1.0
    dz_cls = np.zeros((B, K))
    if n:
        dz_cls = np.where(valid[:, None], (np.exp(zs - lse[:, None]) - onehot) / n, 0.0)
    dz_div = T * (np.exp(log_ps) - pt) / B
    hit = valid & (pred == y)
    return {"loss_cls": loss_cls, "loss_div": loss_div, "acc": 100.0 * float(hit.sum()) / B, "hits": int(hit.sum()), "n_valid": n,
            "n_bad": int(bad.sum()), "lse": lse, "lseS": lseS, "lseT": lseT, "pred": pred.astype(np.int64), "kl": kl,
            "dz_cls": dz_cls, "dz_div": dz_div, "dz": g_cls * dz_cls + g_div * dz_div}

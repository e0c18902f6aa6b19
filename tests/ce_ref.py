"""numpy restatement of the classification head's formulas (include/moma_hip.h, section CE; reference: nn.CrossEntropyLoss as
train_teacher.py:184 builds it, helper/util.accuracy, helper/util.process_accumulated_output), evaluated in float64.  The yardstick of the
CE tests: the golden fixture records how far the reference's own fp32 results are from this evaluation, and the kernels are allowed
twice that.

    m_b = max_k z[b,k]      S_b = sum_k exp(z[b,k] - m_b)      lse_b = m_b + log S_b
    row_b  = lse_b - z[b, y_b]                    (a valid row: 0 <= y_b < K)
    loss   = sum_valid row_b / n_valid            (n_valid = 0 -> NaN; a label outside [0, K) other than -100 -> NaN)
    pred_b = the LOWEST index k with z[b,k] = m_b
    hit_b  = [pred_b == y_b]
    dz[b,k] = g_loss (exp(z[b,k] - lse_b) - [k == y_b]) / n_valid    (a row that is not valid: exact zeros)
"""
import numpy as np

IGNORE = -100
MARGIN = 1.0 / 8            # the fixture's logits: every row's maximum is unique and at least this far above the rest


def ce(z, y, g_loss=1.0):
    """-> dict(loss, lse [B], rows [B] (0 where not valid), pred [B], hits, n_valid, n_bad, sum (of the valid rows' losses),
    acc (percent of ALL rows, as helper/util.accuracy), conf [K, K] int64 (row = label, column = prediction), dz [B, K])"""
    z = np.asarray(z, np.float64)
    y = np.asarray(y, np.int64)
    B, K = z.shape
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    pred = z.argmax(axis=1)                                       # (numpy: the first occurrence)
    valid = (y >= 0) & (y < K)
    bad = ~valid & (y != IGNORE)
    ys = np.where(valid, y, 0)
    rows = np.where(valid, lse - z[np.arange(B), ys], 0.0)
    n = int(valid.sum())
    total = float(rows.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = float("nan") if bad.any() else float(np.float64(total) / np.float64(n))
    onehot = np.zeros((B, K))
    onehot[np.arange(B), ys] = 1.0
    dz = np.zeros((B, K))
    if n:
        dz = np.where(valid[:, None], g_loss * (np.exp(z - lse[:, None]) - onehot) / n, 0.0)
    hit = valid & (pred == y)
    conf = np.zeros((K, K), np.int64)
    np.add.at(conf, (ys[valid], pred[valid]), 1)
    return {"loss": loss, "lse": lse, "rows": rows, "pred": pred.astype(np.int64), "hits": int(hit.sum()), "n_valid": n,
            "n_bad": int(bad.sum()), "sum": total, "acc": 100.0 * float(hit.sum()) / B, "conf": conf, "dz": dz}


def margin(z):
    """the smallest distance of a row's maximum from the rest of its row (inf for K = 1); 0 where a maximum is tied"""
    z = np.asarray(z, np.float64)
    if z.shape[1] < 2:
        return float("inf")
    s = np.sort(z, axis=1)
    return float((s[:, -1] - s[:, -2]).min())

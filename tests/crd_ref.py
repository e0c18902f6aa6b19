"""numpy restatement of the CRD formulas (include/moma_hip.h, CRD section; reference crd/memory.py:39-77, crd/criterion.py:57-74),
evaluated in float64 unless told otherwise.  The yardstick of the CRD tests: the golden fixture records how far the reference's own
fp32 results are from this evaluation, and the kernels are allowed twice that."""
import numpy as np

EPS = 1e-7


def scores(v, M, idx, T, dtype=np.float64):
    """e[b,j] = exp(<M[idx[b,j]], v[b]> / T); entries of idx outside [0, n_data) give 0 (they contribute nothing)"""
    v, M = np.asarray(v, dtype), np.asarray(M, dtype)
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < M.shape[0])
    rows = M[np.where(ok, idx, 0)]                               # [B, K1, d]
    s = np.einsum("bkd,bd->bk", rows, v)
    return np.where(ok, np.exp(s / dtype(T)), 0).astype(dtype), ok, rows


def z_of(e, n_data):
    """Z = mean(e) * n_data over all B * K1 entries (crd/memory.py:50-57)"""
    return e.mean() * n_data


def side(v, M, idx, T, Z, dtype=np.float64):
    """one side: -> dict(x [B,K1], loss, dv [B,d]) with c = nce_k / n_data"""
    e, ok, rows = scores(v, M, idx, T, dtype)
    B, K1 = e.shape
    n_data = M.shape[0]
    c = dtype(K1 - 1) / dtype(n_data)
    x = e / dtype(Z)
    with np.errstate(divide="ignore", invalid="ignore"):
        lpos = np.where(ok[:, 0], np.log(x[:, 0] / (x[:, 0] + c + EPS)), 0)
        lneg = np.where(ok[:, 1:], np.log(c / (x[:, 1:] + c + EPS)), 0)
        g = np.empty_like(x)
        g[:, 0] = -(1 / x[:, 0] - 1 / (x[:, 0] + c + EPS)) / B
        g[:, 1:] = 1 / (x[:, 1:] + c + EPS) / B
    loss = -(lpos.sum() + lneg.sum()) / B
    coef = np.where(ok, g * x / dtype(T), 0)
    dv = np.einsum("bk,bkd->bd", coef, rows)
    return {"x": x, "loss": loss, "dv": dv, "e": e}


def scores_bwd(dout, x, M, idx, T, dtype=np.float64):
    """dv[b,:] = sum_j dout[b,j] x[b,j] / T * M[idx[b,j]]"""
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < M.shape[0])
    rows = np.asarray(M, dtype)[np.where(ok, idx, 0)]
    return np.einsum("bk,bkd->bd", np.where(ok, np.asarray(dout, dtype) * np.asarray(x, dtype) / dtype(T), 0), rows)


def update(M, v, y, momentum, dtype=np.float64):
    """M[y[i]] = normalise(M[y[i]] * m + v[i] * (1 - m)) from the PRE-update rows; repeated y: the last in batch order wins;
    y outside [0, n_data) is skipped.  Returns the new bank."""
    M0 = np.asarray(M, dtype)
    out = M0.copy()
    for i, yi in enumerate(np.asarray(y, np.int64)):
        if 0 <= yi < M0.shape[0]:
            r = M0[yi] * dtype(momentum) + np.asarray(v[i], dtype) * (1 - dtype(momentum))
            out[yi] = r / np.sqrt((r * r).sum())
    return out


def embed(f, W, b, dtype=np.float64):
    """Embed: Linear + L2 normalise (crd/criterion.py:77-100) -> (v, cache)"""
    f, W, b = np.asarray(f, dtype), np.asarray(W, dtype), np.asarray(b, dtype)
    z = f.reshape(f.shape[0], -1) @ W.T + b
    n = np.sqrt((z * z).sum(1, keepdims=True))
    return z / n, (f.reshape(f.shape[0], -1), z / n, n)


def embed_bwd(dv, cache):
    """-> (dW, db) of Embed for the gradient dv of its output"""
    f, v, n = cache
    dz = (dv - v * (v * dv).sum(1, keepdims=True)) / n
    return dz.T @ f, dz.sum(0)


def rel(a, b):
    """distance of a from b in units of b's largest element"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def side_dense(v, M, idx, T, Z, dtype=np.float64):
    """`side` for a bank small enough to score every row: the same sums, organised as v M^T and a scatter of the coefficients, so that
    no [B, K1, d] array is formed (the sweeps run nce_k = 16384 over n_data = 2048)"""
    v, M = np.asarray(v, dtype), np.asarray(M, dtype)
    idx = np.asarray(idx, np.int64)
    B, K1 = idx.shape
    n_data = M.shape[0]
    ok = (idx >= 0) & (idx < n_data)
    safe = np.where(ok, idx, 0)
    s = np.take_along_axis(v @ M.T, safe, 1)
    e = np.where(ok, np.exp(s / dtype(T)), 0)
    c = dtype(K1 - 1) / dtype(n_data)
    x = e / dtype(Z)
    with np.errstate(divide="ignore", invalid="ignore"):
        lpos = np.where(ok[:, 0], np.log(x[:, 0] / (x[:, 0] + c + EPS)), 0)
        lneg = np.where(ok[:, 1:], np.log(c / (x[:, 1:] + c + EPS)), 0)
        g = np.empty_like(x)
        g[:, 0] = -(1 / x[:, 0] - 1 / (x[:, 0] + c + EPS)) / B
        g[:, 1:] = 1 / (x[:, 1:] + c + EPS) / B
    coef = np.where(ok, g * x / dtype(T), 0)
    w = np.zeros((B, n_data), dtype)
    for b in range(B):
        np.add.at(w[b], safe[b], coef[b])
    return {"x": x, "loss": -(lpos.sum() + lneg.sum()) / B, "dv": w @ M, "e": e}

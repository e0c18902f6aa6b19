"""numpy float64 restatement of Correlation Congruence behind its two LinearEmbed heads (include/moma_hip.h, section CC; reference
distiller_zoo/CC.py Correlation, models/util.py LinearEmbed): the difference of both embeddings, the product of neighbouring rows of
its absolute value, and every gradient in closed form.  The yardstick of tests/test_cc_cpu.py and tests/test_gpu_cc.py.

|d| has a kink at d = 0, where a result rounded to fp32 may take the other sign.  Every test input goes through `clear` (TAU = 2^-10):
single elements of x_s are nudged by 1/8 until no float64 |d| is below TAU -- a condition on the inputs, so no element is left out of a
comparison."""
import numpy as np

TAU = 2.0 ** -10
STEP = 0.125


def diff(x_s, x_t, W_s, b_s, W_t, b_t):
    """-> d [B, D] in float64"""
    x_s, x_t, W_s, b_s, W_t, b_t = (np.asarray(v, np.float64) for v in (x_s, x_t, W_s, b_s, W_t, b_t))
    return (x_s @ W_s.T + b_s) - (x_t @ W_t.T + b_t)


def cc(x_s, x_t, W_s, b_s, W_t, b_t, g_loss=1.0):
    """x_s [B, Cs], x_t [B, Ct], W_s [D, Cs], b_s [D], W_t [D, Ct], b_t [D] -> dict(d, loss, G (for g_loss = 1), dx_s, dW_s, db_s, dW_t,
    db_t (the five gradients times g_loss))"""
    x_s, x_t, W_s, W_t = (np.asarray(v, np.float64) for v in (x_s, x_t, W_s, W_t))
    d = diff(x_s, x_t, W_s, b_s, W_t, b_t)
    Bn = d.shape[0]
    delta = np.abs(d)
    if Bn < 2:
        return {"d": d, "loss": float("nan")}
    loss = float((delta[:-1] * delta[1:]).sum() / (Bn - 1))
    nb = np.zeros_like(delta)
    nb[1:] += delta[:-1]
    nb[:-1] += delta[1:]
    G = np.sign(d) * nb / (Bn - 1)
    return {"d": d, "loss": loss, "G": G, "dx_s": g_loss * (G @ W_s), "dW_s": g_loss * (G.T @ x_s), "db_s": g_loss * G.sum(axis=0),
            "dW_t": -g_loss * (G.T @ x_t), "db_t": -g_loss * G.sum(axis=0)}


def clear(x_s, x_t, W_s, b_s, W_t, b_t, tau=TAU, limit=100000):
    """x_s with single elements moved by +1/8 until every float64 |d| is at least tau: the element of d nearest to 0 picks its row, the
    largest |W_s| of its column picks the input.  -> (x_s as float64, number of nudges)"""
    x = np.array(x_s, np.float64)
    W = np.asarray(W_s, np.float64)
    nudges = 0
    while True:
        d = diff(x, x_t, W_s, b_s, W_t, b_t)
        while True:
            i, k = np.unravel_index(np.argmin(np.abs(d)), d.shape)
            if abs(d[i, k]) >= tau:
                break
            c = int(np.argmax(np.abs(W[k])))
            x[i, c] += STEP
            d[i] += STEP * W[:, c]
            nudges += 1
            if nudges > limit:
                raise RuntimeError("no input clear of the kink found")
        if not (np.abs(diff(x, x_t, W_s, b_s, W_t, b_t)) < tau).any():          # (the rows were updated in place: checked from scratch)
            return x, nudges

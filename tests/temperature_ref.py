"""Reference of the temperature record (include/dsrl_hip.h, "temperature"): a numpy float64 restatement of the definitions and a plain float32
restatement (float32 per-pixel terms with numpy's float32 exp and log, c ascending, sums over the pixels in float64).

beta = 1 / T.  A live pixel is one whose label t is neither ignore_index nor >= C.  For its logits v_0..v_{C-1}: m = max_c v_c, d_c = v_c - m, and
    e_c = exp(beta d_c), s = sum e_c, a = sum e_c d_c, q = sum (e_c d_c) d_c
    L = log(s) - beta d_t,  mu = a / s,  G = mu - d_t = dL/dbeta,  H = q / s - mu^2 = d2L/dbeta2
The record is [live pixels, then (sum L, sum G, sum H) for each beta]."""
import numpy as np


def live_rows(logits, target, ignore_index=255):
    """logits (P, C) or (N, C, H, W), target (P,) or (N, H, W) -> (rows (n, C) of the live pixels, their labels (n,))"""
    logits, target = np.asarray(logits), np.asarray(target)
    if logits.ndim == 4:
        logits = np.moveaxis(logits, 1, -1).reshape(-1, logits.shape[1])
    target = target.reshape(-1).astype(np.int64)
    C = logits.shape[1]
    live = (target != ignore_index) & (target < C)
    return logits[live], target[live]


def terms(rows, labels, beta, dtype=np.float64):
    """per live pixel L, G, H at one beta, every operation in `dtype`, c ascending"""
    v = rows.astype(dtype)
    beta = dtype(beta)
    m = v[:, 0].copy()
    for c in range(1, v.shape[1]):
        m = np.fmax(m, v[:, c])
    d = v - m[:, None]
    dt = d[np.arange(d.shape[0]), labels]
    s, a, q = (np.zeros(d.shape[0], dtype) for _ in range(3))
    with np.errstate(under='ignore', invalid='ignore', over='ignore'):
        for c in range(d.shape[1]):
            e = np.exp(beta * d[:, c])
            ed = e * d[:, c]
            s = s + e
            a = a + ed
            q = q + ed * d[:, c]
        mu = a / s
        return np.log(s) - beta * dt, mu - dt, q / s - mu * mu


def record(logits, target, betas, ignore_index=255, dtype=np.float64):
    """-> (record float64 [1 + 3 K], magnitude float64 [1 + 3 K]): the sums over the live pixels of the per-pixel terms computed in `dtype`
    (added in float64), and the sums of their absolute values - what an error of an entry is measured against"""
    rows, labels = live_rows(logits, target, ignore_index)
    betas = np.asarray(betas, np.float64).reshape(-1)
    rec, mag = np.zeros(1 + 3 * betas.size), np.zeros(1 + 3 * betas.size)
    rec[0] = mag[0] = rows.shape[0]
    for k, b in enumerate(betas):
        for j, x in enumerate(terms(rows, labels, b, dtype)):
            rec[1 + 3 * k + j] = x.astype(np.float64).sum()
            mag[1 + 3 * k + j] = np.abs(x.astype(np.float64)).sum()
    return rec, mag


def newton_beta(logits, target, ignore_index=255, beta=1.0, iters=100):
    """the minimiser of the float64 NLL in beta by Newton's method on G (monotone: the NLL is convex), every step kept inside (beta / 4, 4 beta)"""
    rows, labels = live_rows(logits, target, ignore_index)
    for _ in range(iters):
        _, G, H = terms(rows, labels, beta)
        step = G.sum() / H.sum()
        new = min(max(beta - step, 0.25 * beta), 4.0 * beta)
        if abs(new - beta) <= 1e-15 * beta:
            return new
        beta = new
    return beta

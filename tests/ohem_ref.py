"""The OHEM rule restated for the tests (mmseg's OHEMPixelSampler, HRNet's OhemCrossEntropy), on the host.

    candidate   label != ignore and label < C
    p           softmax probability of the label (a NaN counts as 0)
    n           candidates; n == 0: nothing changes
    k           min(min_kept, n - 1);  v = the k-th smallest p (from 0);  thr = max(v, thresh)
    kept        p < thr, strictly; every other candidate gets the label `ignore`

select() is exact on float32 values.  rewrite() takes the probabilities in float64 and is only as good as the distance of every p from thr:
make_case() retries seeds until that distance is beyond what fp32 arithmetic can move a p (the guard), so that the kernels' fp32 p and the
float64 p select the same pixels and the rewritten target is a byte-exact expectation.

The guard's 1e-5 is derived, not measured: an fp32 p = e_t / s carries at most about (C + 3) ulp - exp_nonpos within 2 ulp, a C-term sum, one
division - which is 22 * 2^-23 * p <= 2.7e-6 at C = 19 for p <= 1; v - m itself rounds by at most 2^-20 relative at the logits of these cases
(|v - m| < 32), 1e-6 more.  1e-5 leaves a factor of two."""
import numpy as np

SENTINEL = np.float32(2.0)              # p of a pixel that is not a candidate
GUARD = 1e-5


def keys(p32):
    """the unsigned key the select orders by: the bit pattern of p; a NaN and anything <= 0 is 0"""
    p32 = np.asarray(p32, np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(p32 > 0, p32.view(np.uint32), np.uint32(0)).astype(np.uint32)


def select(p32, thresh, min_kept):
    """-> (bits of thr, n, number kept, number with p < thresh, keep mask over all of p32).  Exact: float32 values, np.sort.  An entry >= 2 is no
    candidate (its mask entry is True: it keeps its label)."""
    p32 = np.asarray(p32, np.float32).reshape(-1)
    with np.errstate(invalid='ignore'):
        cand = ~(p32 >= SENTINEL)
        val = np.where(p32 > 0, p32, np.float32(0)).astype(np.float32)      # NaN, -0 and negatives: 0
    th = np.float32(thresh) if np.float32(thresh) > 0 else np.float32(0)
    c = np.sort(val[cand])
    n = int(c.size)
    v = c[min(int(min_kept), n - 1)] if n else np.float32(0)
    thr = np.float32(max(v, th))
    keep = ~cand | (val < thr)
    return int(thr.view(np.uint32)), n, int((val[cand] < thr).sum()), int((val[cand] < th).sum()), keep


def target_probability64(logits, target, ignore):
    """-> (p of every pixel in float64 from the fp32 logits (NaN -> 0; 2.0 where the pixel is no candidate), candidate mask)"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    P, C = x.shape
    t = np.asarray(target).astype(np.int64).reshape(-1)
    cand = (t != ignore) & (t < C)
    with np.errstate(invalid='ignore', over='ignore'):
        m = x.max(axis=1, keepdims=True)
        e = np.exp(x - m)
        p = e[np.arange(P), np.where(cand, t, 0)] / e.sum(axis=1)
    p = np.where(np.isnan(p), 0.0, p)
    return np.where(cand, p, 2.0), cand


def rewrite(logits, target, ignore, thresh, min_kept):
    """-> (rewritten target (uint8), thr, n, number kept) from float64 probabilities"""
    p, cand = target_probability64(logits, target, ignore)
    t = np.asarray(target, np.uint8).reshape(-1).copy()
    n = int(cand.sum())
    if n == 0:
        return t.reshape(np.shape(target)), float(thresh), 0, 0
    c = np.sort(p[cand])
    thr = max(float(c[min(int(min_kept), n - 1)]), float(thresh))
    keep = ~cand | (p < thr)
    t[~keep] = ignore
    return t.reshape(np.shape(target)), thr, n, int((cand & keep).sum())


def guard_holds(logits, target, ignore, thresh, min_kept):
    """no candidate's p within GUARD of thr except the k-th itself, and the k-th's neighbours in sorted order more than GUARD away"""
    p, cand = target_probability64(logits, target, ignore)
    c = np.sort(p[cand])
    n = c.size
    if n == 0:
        return True
    k = min(int(min_kept), n - 1)
    thr = max(float(c[k]), float(thresh))
    near = np.abs(c - thr) <= GUARD
    near[k] = False
    if near.any():
        return False
    return (k == 0 or c[k] - c[k - 1] > GUARD) and (k == n - 1 or c[k + 1] - c[k] > GUARD)


def ce64(logits, target, ignore, weights=None):
    """mean (weighted) cross entropy of the live pixels in float64; NaN when there is none"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    t = np.asarray(target).astype(np.int64).reshape(-1)
    live = t != ignore
    w = np.ones(x.shape[1]) if weights is None else np.asarray(weights, np.float64)
    m = x.max(axis=1)
    nll = m + np.log(np.exp(x - m[:, None]).sum(axis=1)) - x[np.arange(x.shape[0]), np.where(live, t, 0)]
    d = w[t[live]].sum()
    return float((w[t[live]] * nll[live]).sum() / d) if d > 0 else float('nan')


def make_case(P, C, seed, ignore=255, thresh=0.7, min_kept=None, scale=3.0):
    """-> (logits (P, C) float32, target (P,) uint8, thresh, min_kept, seed used).  Logits of a few units whose labels follow the logits' own ranking
    in part and a third of them has its label's logit lifted by 6, so that p runs from about 0 to about 1 with a confident share; 10 % of the labels
    are `ignore`.  Seeds are retried until the guard holds.  Asserted on the reference alone: the guard; at least 25 % of the candidates are
    dropped; the OHEM loss differs from the plain CE by more than 5 % - a path that ignores `ohem` then fails."""
    if min_kept is None:
        min_kept = P // 4
    for s in range(seed, seed + 200):
        rs = np.random.RandomState(s)
        lg = (rs.standard_normal((P, C)) * scale).astype(np.float32)
        tg = rs.randint(0, C, P).astype(np.int64)
        order = np.argsort(-lg, axis=1)
        pick = rs.randint(0, 3, P)
        tg = np.where(pick == 0, order[:, 0], np.where(pick == 1, order[:, min(1, C - 1)], tg))
        lg[np.arange(P), tg] += np.where(pick == 0, np.float32(6), np.float32(0))          # a third of the pixels is easy: p near 1
        tg[rs.uniform(size=P) < 0.1] = ignore
        if guard_holds(lg, tg, ignore, thresh, min_kept):
            break
    else:
        raise AssertionError('no seed satisfied the guard')
    assert guard_holds(lg, tg, ignore, thresh, min_kept)
    out, thr, n, kept = rewrite(lg, tg, ignore, thresh, min_kept)
    assert n > 0 and (n - kept) >= 0.25 * n, f'only {n - kept} of {n} candidates dropped'
    plain, mined = ce64(lg, tg, ignore), ce64(lg, out, ignore)
    assert abs(mined - plain) > 0.05 * abs(plain), f'OHEM loss {mined} within 5 % of the plain CE {plain}'
    return lg, tg.astype(np.uint8), float(thresh), int(min_kept), s

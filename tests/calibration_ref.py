"""numpy reference of the calibration record and the confidence map (include/dsrl_hip.h, "calibration"):
  * the confidence in fp64 (maximum softmax probability; of the flip and the multi-scale ensemble the winning averaged probability),
  * its fp32 restatement in the kernels' operation order (fmaxf chain, ascending sum of exp_nonpos, one division),
  * the bin rule and the record [n_b | hit_b | q_b] from a confidence map, a class map and a target,
  * the figures from a record, and ECE a second way (the per-pixel sum grouped by bin) to check the first,
  * the SSSR tail (ConvTranspose k2 s2 -> BatchNorm eval -> ReLU -> ConvTranspose k2 s2 + bias) in any dtype, for logits to take them of."""
import numpy as np

Q_SCALE = 16777216.0            # 2^24
DEFAULT_BINS = 15
F32 = np.float32


# ---------------------------------------------------------------------------------------------- the tail, in the dtype of its input
def convt_k2s2(x, w, bias=None):
    """x (N,Ci,H,W), w (Ci,Co,2,2) -> (N,Co,2H,2W): out[n,co,2h+i,2w+j] = sum_ci x[n,ci,h,w] w[ci,co,i,j] (+ bias[co]), in x's dtype"""
    N, Ci, H, W = x.shape
    y = np.einsum('nchw,cdij->ndhiwj', x, w.astype(x.dtype)).reshape(N, w.shape[1], 2 * H, 2 * W)
    return y if bias is None else y + bias.astype(x.dtype)[None, :, None, None]


def tail_logits(x, p, eps=1e-5, dtype=np.float64):
    """the logits (N,C,4H,4W) of tail parameters p = {w1, gamma, beta, mean, var, w2, b2} in `dtype`, BatchNorm as the kernel evaluates it:
    z = v * sc + sh with sc = gamma / sqrt(var + eps), sh = beta - mean * sc"""
    q = {k: None if v is None else np.asarray(v, dtype) for k, v in p.items()}
    y = convt_k2s2(np.asarray(x, dtype), q['w1'])
    sc = (q['gamma'] / np.sqrt(q['var'] + dtype(eps))).astype(dtype)
    sh = (q['beta'] - q['mean'] * sc).astype(dtype)
    y = np.maximum(y * sc[None, :, None, None] + sh[None, :, None, None], dtype(0))
    return convt_k2s2(y, q['w2'], q['b2'])


# ---------------------------------------------------------------------------------------------- confidence
def softmax64(L):
    L = np.asarray(L, np.float64)
    e = np.exp(L - L.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def confidence64(L):
    """logits (N,C,H,W) -> (confidence (N,H,W) fp64, class map: the first maximum)"""
    P = softmax64(L)
    return P.max(axis=1), np.argmax(np.asarray(L, np.float64), axis=1)


def confidence64_of_probabilities(P):
    """averaged class probabilities (N,C,H,W) of an ensemble -> (min(1, winning probability), first maximum)"""
    return np.minimum(P.max(axis=1), 1.0), np.argmax(P, axis=1)


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def exp_nonpos32(x):
    """csrc/common.h exp_nonpos in numpy fp32 (v_exp_f32 taken as the correctly rounded 2^t)"""
    x = np.asarray(x, F32)
    hi, lo, ln2 = F32(1.44269502162933349609375), F32(1.925963033500011e-08), F32(0.693147182464599609375)
    t = (x * hi).astype(F32)
    with np.errstate(invalid='ignore'):
        r = np.where(t > -np.inf, _fma32(x, np.full_like(x, lo), _fma32(x, np.full_like(x, hi), -t)), F32(0)).astype(F32)
    e0 = np.exp2(t.astype(np.float64)).astype(F32)
    return _fma32(e0, (r * ln2).astype(F32), e0)


def confidence32(L):
    """The kernels' fp32 arithmetic on fp32 logits (N,C,H,W): m = fmaxf chain, s = sum over ascending c of exp_nonpos(v_c - m), 1 / s -> (N,H,W) fp32"""
    L = np.asarray(L, F32)
    m = L[:, 0].copy()
    for c in range(1, L.shape[1]):
        m = np.maximum(m, L[:, c])
    s = np.zeros_like(m)
    for c in range(L.shape[1]):
        s = (s + exp_nonpos32((L[:, c] - m).astype(F32))).astype(F32)
    return (F32(1) / s).astype(F32)


# ---------------------------------------------------------------------------------------------- bins, record, figures
def bin_of(conf, bins=DEFAULT_BINS):
    """b = min(B - 1, (int)(conf * (float)B)) with ONE fp32 multiply; conf fp32 (an fp64 input is binned by its own exact product)"""
    conf = np.asarray(conf)
    prod = (conf.astype(F32) * F32(bins)).astype(F32) if conf.dtype == F32 else conf.astype(np.float64) * float(bins)
    return np.minimum(bins - 1, prod.astype(np.int64))


def record_of(conf, pred, target, bins=DEFAULT_BINS, num_classes=19, ignore_index=255):
    """[n_b | hit_b | q_b] int64 of a confidence map, a class map and a target of one shape; a NaN confidence is counted nowhere"""
    conf, pred, target = np.asarray(conf).reshape(-1), np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(target).reshape(-1).astype(np.int64)
    counted = (target != ignore_index) & (target < num_classes) & ~np.isnan(conf)
    c, b = conf[counted], None
    b = bin_of(c, bins)
    q = np.rint((c.astype(F32) * F32(Q_SCALE)).astype(F32) if c.dtype == F32 else c.astype(np.float64) * Q_SCALE).astype(np.int64)
    hit = (pred[counted] == target[counted]).astype(np.int64)
    return np.concatenate([np.bincount(b, minlength=bins), np.bincount(b, weights=hit, minlength=bins).astype(np.int64),
                           np.array([q[b == k].sum() for k in range(bins)], np.int64)]).astype(np.int64)


def figures(record):
    """ECE, MCE, mean_confidence, accuracy and the per-bin acc / conf from a record, fp64; an empty record gives NaN"""
    rec = np.asarray(record, np.int64).reshape(3, -1)
    n, hit, q = (rec[i].astype(np.float64) for i in range(3))
    N = n.sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        acc, conf = hit / n, q / (Q_SCALE * n)
    if N == 0:
        return {'ECE': np.nan, 'MCE': np.nan, 'mean_confidence': np.nan, 'accuracy': np.nan, 'acc': acc, 'conf': conf}
    live = n > 0
    gap = np.abs(acc[live] - conf[live])
    return {'ECE': float((n[live] / N * gap).sum()), 'MCE': float(gap.max()), 'mean_confidence': float(q.sum() / (Q_SCALE * N)),
            'accuracy': float(hit.sum() / N), 'acc': acc, 'conf': conf}


def ece_direct(conf, pred, target, bins=DEFAULT_BINS, num_classes=19, ignore_index=255):
    """ECE the second way: (1 / N) sum over the bins of |sum over the bin's pixels of ([pred == target] - conf_q)|, conf_q the pixel's fixed-point
    confidence rint(conf 2^24) / 2^24 - per-pixel terms grouped by bin, no record in between"""
    conf, pred, target = np.asarray(conf).reshape(-1), np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(target).reshape(-1).astype(np.int64)
    counted = (target != ignore_index) & (target < num_classes) & ~np.isnan(conf)
    c = conf[counted]
    b = bin_of(c, bins)
    cq = np.rint((c.astype(F32) * F32(Q_SCALE)).astype(F32) if c.dtype == F32 else c.astype(np.float64) * Q_SCALE) / Q_SCALE
    term = (pred[counted] == target[counted]).astype(np.float64) - cq.astype(np.float64)
    if c.size == 0:
        return float('nan')
    return float(sum(abs(term[b == k].sum()) for k in range(bins)) / c.size)

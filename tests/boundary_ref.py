"""numpy reference of the Boundary IoU counters (include/dsrl_hip.h: dsrl_boundary_counts), shared by test_boundary_host.py and
test_boundary_gpu.py.  Two formulations of the band, so that the reference has a check of its own:
  band_window   the rule of the header: a pixel is in the band iff its (2d+1) x (2d+1) window leaves the image or holds another byte - separable
                shifted minima and maxima over a padded copy
  band_erosion  the paper's: per label, mask - erode(mask, 3x3, d iterations) on the mask padded by a ring of zeros (Cheng et al., CVPR 2021)
Everything is integers: the tests compare with ==."""
import numpy as np

VOID, BAD = 255, 254

# (N, H, W, d) of the structured cases; the host test asserts the generator's conditions on every one of them
STRUCTURED = [(2, 13, 29, 1), (2, 37, 131, 2), (1, 50, 77, 3), (1, 70, 131, 5), (1, 200, 333, 16), (1, 400, 800, 64)]


def distance(H, W, ratio=0.02):
    return max(1, int(round(ratio * np.hypot(H, W))))


def normalise(pred, target, C, ignore_index=255):
    """step 1: -> (g', p') uint8: void 255 where the target is not counted (in both), bad 254 where a counted pixel's prediction is >= C"""
    pred, target = np.asarray(pred, np.uint8), np.asarray(target, np.uint8)
    live = (target < C) & (target != ignore_index)
    g = np.where(live, target, VOID).astype(np.uint8)
    p = np.where(live, np.where(pred < C, pred, BAD), VOID).astype(np.uint8)
    return g, p


def band_window(m, d):
    """(N, H, W) uint8 -> bool: the window rule.  The copy is padded with -1, which is no byte: a window that leaves the image has minimum -1."""
    m = np.asarray(m)
    N, H, W = m.shape
    a = np.full((N, H + 2 * d, W + 2 * d), -1, np.int16)
    a[:, d:d + H, d:d + W] = m
    lo = a[:, :, 0:W].copy()
    hi = lo.copy()
    for k in range(1, 2 * d + 1):                       # along the rows
        np.minimum(lo, a[:, :, k:k + W], out=lo)
        np.maximum(hi, a[:, :, k:k + W], out=hi)
    lo2, hi2 = lo[:, 0:H].copy(), hi[:, 0:H].copy()
    for k in range(1, 2 * d + 1):                       # along the columns
        np.minimum(lo2, lo[:, k:k + H], out=lo2)
        np.maximum(hi2, hi[:, k:k + H], out=hi2)
    own = m.astype(np.int16)
    return (lo2 != own) | (hi2 != own)


def erode3x3(mask):
    """one 3x3 erosion of (N, H, W) bool with zeros outside the image"""
    N, H, W = mask.shape
    p = np.zeros((N, H + 2, W + 2), bool)
    p[:, 1:-1, 1:-1] = mask
    out = np.ones((N, H, W), bool)
    for dy in range(3):
        for dx in range(3):
            out &= p[:, dy:dy + H, dx:dx + W]
    return out


def band_erosion(m, d):
    """(N, H, W) uint8 -> bool: per label present, the pixels of its mask that d erosions remove"""
    m = np.asarray(m)
    band = np.zeros(m.shape, bool)
    for v in np.unique(m):
        mask = m == v
        inner = mask
        for _ in range(d):
            inner = erode3x3(inner)
            if not inner.any():
                break
        band |= mask & ~inner
    return band


def counts(pred, target, C, d, ignore_index=255, band_of=band_window):
    """-> {'I', 'G', 'P'} int64 arrays of C, 'counts' their concatenation in the ABI's order, 'band' the uint8 map (bit 0 target band, bit 1
    prediction band, 0 on void pixels), 'bad' whether a counted pixel's prediction is >= C"""
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 2:
        pred, target = pred[None], target[None]
    g, p = normalise(pred, target, C, ignore_index)
    gb, pb = band_of(g, d), band_of(p, d)
    live = g != VOID
    G = np.bincount(g[live & gb].astype(np.int64), minlength=C)[:C]
    P = np.bincount(p[live & pb & (p < C)].astype(np.int64), minlength=C)[:C]
    I = np.bincount(g[live & gb & pb & (g == p)].astype(np.int64), minlength=C)[:C]
    band = np.where(live, gb.astype(np.uint8) | (pb.astype(np.uint8) << 1), 0).astype(np.uint8)
    I, G, P = I.astype(np.int64), G.astype(np.int64), P.astype(np.int64)
    return {'I': I, 'G': G, 'P': P, 'counts': np.concatenate([I, G, P]), 'band': band, 'bad': bool((p == BAD).any()), 'valid': int(live.sum())}


def figures(I, G, P):
    """-> (BIoU per class in percent, NaN at 0/0; their nan-mean)"""
    I, U = np.asarray(I, np.float64), np.asarray(G, np.float64) + np.asarray(P, np.float64) - np.asarray(I, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        b = np.where(U > 0, 100. * I / U, np.nan)
    ok = ~np.isnan(b)
    return b, (float(b[ok].mean()) if ok.any() else float('nan'))


def structured(N, H, W, d, C=19, seed=0):
    """-> (pred, target) uint8 (N, H, W): the target a grid of square cells of side 6d with random classes, the prediction the same grid rolled by
    (d // 2 + 1, d), one void rectangle of (2d+1) x 3d in the target.  Band and interior, hit and miss all occur (asserted by the host test)."""
    rs = np.random.RandomState(1000 * d + H + seed)
    side = 6 * d
    cells = rs.randint(0, C, (N, -(-H // side), -(-W // side))).astype(np.uint8)
    gt = np.repeat(np.repeat(cells, side, axis=1), side, axis=2)[:, :H, :W]
    pred = np.roll(gt, (d // 2 + 1, d), axis=(1, 2)).copy()
    target = gt.copy()
    y0, x0 = H // 3, W // 4
    target[:, y0:y0 + 2 * d + 1, x0:x0 + 3 * d] = VOID
    return np.ascontiguousarray(pred), np.ascontiguousarray(target)

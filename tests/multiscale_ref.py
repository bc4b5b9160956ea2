"""fp64 restatement of the multi-scale ensemble (include/dsrl_hip.h: dsrl_prob_merge / dsrl_prob_merge_finish) and the fixtures
test_multiscale_host.py and test_multiscale_gpu.py share.

  A view is the logits (N,C,h,w) of one scale, in the plain or the horizontally mirrored frame.  Every view is resampled onto the output grid
  (Ho,Wo) by align-corners bilinear interpolation of the logits (a mirrored view mirrored back along W first) with the exact-rational source
  coordinate n = o (S - 1), i0 = n div (O - 1), frac = (n mod (O - 1)) / (O - 1), i1 = min(i0 + 1, S - 1) (O = 1: i0 = 0, frac = 0);
  P = mean over the views of softmax over the classes, pred = first arg-max of P, ce = mean of -log P[target] over target != ignore_index."""
import functools

import numpy as np

import gen
import predict_fixtures as PF

NC = gen.NUM_CLASSES
# (seed, N, Ho, Wo, [(h, w) ...], flip): rs = RandomState(seed); for each size in order and v in range(2 if flip else 1) one draw of
# standard_normal((N,19,h,w)).astype(float32); the v = 1 draws are views in the mirrored frame
FIXTURES = [(81, 2, 12, 20, ((6, 10), (12, 20), (18, 28)), False),
            (82, 1, 8, 8, ((4, 4), (8, 8), (13, 11)), True),
            (83, 1, 1, 1, ((1, 1), (3, 2)), False),                                         # O - 1 = 0
            (84, 2, 5, 7, ((2, 3), (5, 7), (9, 16)), True),                                 # odd sizes, byte-aligned pred rows
            (85, 1, 64, 128, ((32, 64), (48, 96), (64, 128), (80, 160), (112, 224)), True),  # 10 views, 0.5 ... 1.75
            (86, 3, 16, 33, ((1, 5), (16, 33)), False)]                                     # a one-row source, an identity view, odd Wo
# Absolute band on the top-two margin of P.  Derived, not measured: weights are correct to 2^-23; a 4-term fp32 blend gives
# dL <~ 6 * 2^-24 * max |L| ~ 1.8e-6 at max |L| ~ 5; dp <= 2 p dL with p <= 0.4 on these fixtures; the exponential adds ~6e-7 relative; so
# dP <~ 2e-6 and the margin error <~ 4e-6.  The band is five times that.
BAND = 2e-5
# |ce - ref| <= CE_TOL * max(1, |ref|): each view's p[t] is relatively correct to <~ 4e-6, so -log P[t] to <~ 4e-6 absolute; five times that
CE_TOL = 2e-5


def fixture_id(f):
    return 's{}_n{}_{}x{}_{}views{}'.format(f[0], f[1], f[2], f[3], len(f[4]) * (2 if f[5] else 1), '_flip' if f[5] else '')


# ---------------------------------------------------------------------------------------------- the definition
def coords(S, O):
    """-> (i0, i1, frac) of the O output samples of an axis with S source samples; frac is the fp64 value of an exact rational"""
    o = np.arange(O, dtype=np.int64)
    if O > 1:
        n = o * (S - 1)
        i0 = n // (O - 1)
        frac = (n - i0 * (O - 1)).astype(np.float64) / float(O - 1)
    else:
        i0, frac = np.zeros(1, np.int64), np.zeros(1, np.float64)
    return i0, np.minimum(i0 + 1, S - 1), frac


def resize_ac(L, size):
    """L (N,C,h,w) -> (N,C,Ho,Wo) fp64: align-corners bilinear interpolation, rows of the source first"""
    L = np.asarray(L, np.float64)
    y0, y1, fy = coords(L.shape[2], size[0])
    x0, x1, fx = coords(L.shape[3], size[1])
    fy, fx = fy[None, None, :, None], fx[None, None, None, :]
    top = (1.0 - fx) * L[:, :, y0][:, :, :, x0] + fx * L[:, :, y0][:, :, :, x1]
    bot = (1.0 - fx) * L[:, :, y1][:, :, :, x0] + fx * L[:, :, y1][:, :, :, x1]
    return (1.0 - fy) * top + fy * bot


def softmax(L):
    e = np.exp(L - L.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def merge(views, out_size):
    """views: [(L (N,C,h,w), mirrored)] -> P (N,C,Ho,Wo) fp64"""
    P = 0.0
    for L, mirrored in views:
        L = np.asarray(L, np.float64)
        P = P + softmax(resize_ac(L[:, :, :, ::-1] if mirrored else L, out_size))
    return P / len(views)


def ce(P, target, ignore_index=gen.IGNORE, num_classes=NC):
    """mean of -log P[target] over target != ignore_index; NaN when every pixel is ignored or a label >= num_classes is not the ignore label"""
    target = target.astype(np.int64)
    counted = target != ignore_index
    if not counted.any() or (target[counted] >= num_classes).any():
        return float('nan')
    picked = np.take_along_axis(P, np.where(counted, target, 0)[:, None], axis=1)[:, 0]
    with np.errstate(divide='ignore'):
        return float(-np.log(picked[counted]).mean())


def band_of(P):
    """-> (best, second, in_band): the two best classes per pixel (lowest index first among equals) and the pixels whose top-two margin of P is
    below BAND"""
    order = np.argsort(-P, axis=1, kind='stable')
    top = np.take_along_axis(P, order[:, :2], axis=1)
    return order[:, 0], order[:, 1], (top[:, 0] - top[:, 1]) < BAND


def check_class_map(pred, P, what):
    """pred equals the fp64 arg-max outside the band; inside it either of the two best classes; at most PF.MAX_BAND_SHARE of the pixels are inside.
    Returns the band's share."""
    best, second, band = band_of(P)
    share = band.mean()
    assert share <= PF.MAX_BAND_SHARE, f'{what}: {100 * share:.3f} % of the pixels are inside the band'
    pred = pred.astype(np.int64)
    wrong = (pred != best) & ~band
    assert not wrong.any(), f'{what}: {int(wrong.sum())} pixels outside the band differ from the fp64 ensemble, first at {np.argwhere(wrong)[0]}'
    stray = band & (pred != best) & (pred != second)
    assert not stray.any(), f'{what}: {int(stray.sum())} band pixels took a class that is neither of the two best'
    return share


# ---------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def fixture(f):
    """-> (views [(L float32 (N,19,h,w), mirrored)], P (N,19,Ho,Wo) fp64); computed once and shared: treat as read-only"""
    seed, n, ho, wo, sizes, flip = f
    rs = np.random.RandomState(seed)
    views = []
    for h, w in sizes:
        for v in range(2 if flip else 1):
            L = rs.standard_normal((n, NC, h, w)).astype(np.float32)
            L.setflags(write=False)
            views.append((L, v == 1))
    P = merge(views, (ho, wo))
    P.setflags(write=False)
    return views, P

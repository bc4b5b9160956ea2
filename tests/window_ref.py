"""fp64 restatement of the sliding-window ensemble (include/dsrl_hip.h: dsrl_window_merge / dsrl_window_merge_finish) and the fixtures
test_window_host.py and test_window_gpu.py share.

  Plan: along an axis of S pixels with window side w and stride s there are n = max(S - w + s - 1, 0) // s + 1 positions a_i = max(min(i s + w, S) - w, 0).
  Ensemble: a view is the logits (N,C,wh,ww) of one window position, in the plain or the horizontally mirrored frame; tot = sum over the views
  covering a pixel of softmax over the classes (a mirrored view mirrored back first), cnt = covering y-positions x covering x-positions x views per
  position, P = tot / cnt, pred = first arg-max of tot, ce = mean of -log P[target] over target != ignore_index.

The tolerances are multiscale_ref's: its derivation holds every error term present here (the softmax, the accumulation) plus an interpolation term
that is absent; the one extra operation is the division by cnt, one rounding (6e-8 relative)."""
import functools

import numpy as np

import gen
import multiscale_ref as MR

NC = gen.NUM_CLASSES
BAND, CE_TOL = MR.BAND, MR.CE_TOL
# (seed, N, Ho, Wo, (wh, ww), ys, xs, flip): rs = RandomState(seed); for each position in row-major order and each view one draw of
# standard_normal((N,19,wh,ww)).astype(float32); the second draw of a position is the view in the mirrored frame
FIXTURES = [(181, 2, 12, 20, (8, 12), (0, 4), (0, 8), False),                         # cover counts 1, 2, 4: overlap on both axes
            (182, 1, 10, 70, (10, 33), (0,), (0, 12, 24, 36, 37), True),              # one row position, a one-pixel pull-back, two spans per row, 4 x 2
            (183, 3, 9, 7, (5, 4), (0, 2, 4), (0, 3), False),                         # odd offsets and sizes, byte-aligned pred rows
            (184, 1, 6, 6, (6, 6), (0,), (0,), True),                                 # one whole-image window, flip
            (185, 1, 64, 160, (32, 96), (0, 16, 32), (0, 32, 64), True)]              # 18 views, windows 1.5 spans wide, counts 2 to 12
COVER_COUNTS = {181: {1, 2, 4}, 182: {2, 4, 6, 8}, 183: {1, 2, 3, 4, 6}, 184: {2}, 185: {2, 4, 6, 8, 12}}


def fixture_id(f):
    return 's{}_n{}_{}x{}_{}x{}pos{}'.format(f[0], f[1], f[2], f[3], len(f[5]), len(f[6]), '_flip' if f[7] else '')


# ---------------------------------------------------------------------------------------------- the definition
def positions(S, w, s):
    n = max(S - w + s - 1, 0) // s + 1
    return tuple(max(min(i * s + w, S) - w, 0) for i in range(n))


def cover(ys, xs, win, out_size, views_per_position=1):
    """-> cnt (Ho,Wo) int64, by brute force over the positions"""
    cnt = np.zeros(out_size, np.int64)
    for y in ys:
        for x in xs:
            cnt[y:y + win[0], x:x + win[1]] += views_per_position
    return cnt


def merge(views, ys, xs, out_size, flip=False):
    """views: the windows' logits (N,C,wh,ww) in plan order (with flip two per position, the second in the mirrored frame)
    -> (P (N,C,Ho,Wo) fp64, cnt (Ho,Wo))"""
    vpp = 2 if flip else 1
    assert len(views) == len(ys) * len(xs) * vpp
    n, c, wh, ww = views[0].shape
    tot = np.zeros((n, c) + tuple(out_size), np.float64)
    for k, L in enumerate(views):
        pos, v = divmod(k, vpp)
        i, j = divmod(pos, len(xs))
        L = np.asarray(L, np.float64)
        tot[:, :, ys[i]:ys[i] + wh, xs[j]:xs[j] + ww] += MR.softmax(L[:, :, :, ::-1] if v == 1 else L)
    cnt = cover(ys, xs, (wh, ww), out_size, vpp)
    assert cnt.min() >= 1
    return tot / cnt, cnt


ce = MR.ce
check_class_map = MR.check_class_map


# ---------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def fixture(f):
    """-> (views [L float32 (N,19,wh,ww)], P (N,19,Ho,Wo) fp64, cnt (Ho,Wo)); computed once and shared: treat as read-only"""
    seed, n, ho, wo, win, ys, xs, flip = f
    rs = np.random.RandomState(seed)
    views = []
    for _ in range(len(ys) * len(xs) * (2 if flip else 1)):
        L = rs.standard_normal((n, NC) + tuple(win)).astype(np.float32)
        L.setflags(write=False)
        views.append(L)
    P, cnt = merge(views, ys, xs, (ho, wo), flip)
    P.setflags(write=False)
    return views, P, cnt

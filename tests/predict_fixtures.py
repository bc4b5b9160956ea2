"""Fixtures shared by test_predict_host.py and test_predict_gpu.py: the reduced-width head of gen.SMALL in eval mode, its fp64 oracle logits and the
band of pixels whose two best classes are too close for an fp32 evaluation to be held to the oracle's choice."""
import numpy as np

import gen
import oracle as O

# (parameter seed, input seed, batch, backbone rows, backbone columns): SSSR output is 32x the backbone size; the ragged one has N = 3 on 3x5
HEAD_FIXTURES = [(101, 202, 2, 4, 8), (7, 8, 2, 4, 8), (31, 32, 2, 4, 8), (101, 202, 3, 3, 5), (31, 32, 3, 3, 5), (7, 8, 1, 4, 8)]
BAND = 1e-4                 # of max |L|: ~20x the rounding of two chained 76-term fp32 dot products and of the f16x3 convs in front of them
MAX_BAND_SHARE = 0.005


def fixture_id(f):
    return 'p{}_i{}_n{}_{}x{}'.format(*f)


def head_fixture(f):
    pseed, iseed, batch, h16, w16 = f
    P = gen.make_head_params(pseed, gen.SMALL, 3)
    x16, x4, target, _ = gen.make_head_inputs(iseed, batch, h16, w16, gen.SMALL)
    return P, x16, x4, target


def oracle_logits(P, x16, x4):
    out = O.head_forward({k: v.astype(np.float64) for k, v in P.items()}, x16.astype(np.float64), x4.astype(np.float64), stage=1, bn_training=False)
    return out.SSSR.v


def band_of(L):
    """L (N,C,H,W) fp64 -> (best, second, in_band): the two best classes per pixel (lowest index first among equals) and the pixels whose
    top-two margin is below BAND * max |L|."""
    order = np.argsort(-L, axis=1, kind='stable')
    best, second = order[:, 0], order[:, 1]
    top = np.take_along_axis(L, order[:, :2], axis=1)
    return best, second, (top[:, 0] - top[:, 1]) < BAND * np.abs(L).max()


def check_class_map(pred, L, what):
    """pred equals the oracle's arg-max outside the band; inside it either of the oracle's two best classes.  Returns the band's share."""
    best, second, band = band_of(L)
    share = band.mean()
    assert share <= MAX_BAND_SHARE, f'{what}: {100 * share:.3f} % of the pixels are inside the band'
    pred = pred.astype(np.int64)
    wrong = (pred != best) & ~band
    assert not wrong.any(), f'{what}: {int(wrong.sum())} pixels outside the band differ from the oracle, first at {np.argwhere(wrong)[0]}'
    stray = band & (pred != best) & (pred != second)
    assert not stray.any(), f'{what}: {int(stray.sum())} band pixels took a class that is neither of the two best'
    return share


def counts_table(pred, target, num_classes=19, ignore_index=255):
    """[area_pred | area_inter | area_target | correct, valid] as dsrl_seg_metrics lays them out, from class maps"""
    valid = (target != ignore_index) & (target < num_classes)
    p, t = pred[valid].astype(np.int64), target[valid].astype(np.int64)
    out = np.zeros(3 * num_classes + 2, np.int64)
    out[:num_classes] = np.bincount(p, minlength=num_classes)
    out[num_classes:2 * num_classes] = np.bincount(p[p == t], minlength=num_classes)
    out[2 * num_classes:3 * num_classes] = np.bincount(t, minlength=num_classes)
    out[3 * num_classes], out[3 * num_classes + 1] = (p == t).sum(), valid.sum()
    return out

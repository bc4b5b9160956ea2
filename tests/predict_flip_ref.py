"""fp64 restatement of the horizontal-flip ensemble (include/dsrl_hip.h: dsrl_sssr_tail_predict_flip) and the fixtures test_predict_flip_host.py and
test_predict_flip_gpu.py share.

  La = logits of the images, Lb = logits of the mirrored images mirrored back along W,
  E  = logaddexp(log_softmax(La), log_softmax(Lb)) - ln 2 over the classes (the log of the averaged class probabilities),
  pred = first arg-max of E, ce = mean over the pixels with target != ignore_index of -E[target]."""
import functools

import numpy as np

import gen
import oracle as O
import predict_fixtures as PF

NC = gen.NUM_CLASSES
# (parameter seed, tail-input seed, class maps N, tail-input rows H, columns W); the tail input is (2N,19,H,W), two independent views
TAIL_FIXTURES = [(61, 62, 3, 9, 13), (63, 64, 2, 5, 7), (65, 66, 1, 1, 1), (67, 68, 2, 3, 1), (69, 70, 1, 4, 16), (71, 72, 4, 32, 64)]


def tail_fixture_id(f):
    return 'p{}_x{}_n{}_{}x{}'.format(*f)


# ---------------------------------------------------------------------------------------------- the definition
def log_softmax(L):
    z = L - L.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def ensemble(La, Lb_mirrored):
    """La (N,C,H,W), Lb_mirrored (N,C,H,W) still in the mirrored frame -> E (N,C,H,W), fp64"""
    la = log_softmax(np.asarray(La, np.float64))
    lb = log_softmax(np.asarray(Lb_mirrored, np.float64))[:, :, :, ::-1]
    return np.logaddexp(la, lb) - np.log(2.0)


def ensemble_of_views(L):
    """L (2N,C,H,W): the second half from the mirrored images"""
    n = L.shape[0] // 2
    return ensemble(L[:n], L[n:])


def ce(E, target, ignore_index=gen.IGNORE, num_classes=NC):
    """mean of -E[target] over target != ignore_index; NaN when every pixel is ignored or a label >= num_classes is not the ignore label"""
    target = target.astype(np.int64)
    counted = target != ignore_index
    if not counted.any() or (target[counted] >= num_classes).any():
        return float('nan')
    picked = np.take_along_axis(E, np.where(counted, target, 0)[:, None], axis=1)[:, 0]
    return float(-picked[counted].mean())


def band_of(E, L):
    """-> (best, second, in_band): PF.band_of's rule with E in place of L; the band is the pixels whose top-two margin of E is below
    PF.BAND * max |L| over both views' logits"""
    order = np.argsort(-E, axis=1, kind='stable')
    top = np.take_along_axis(E, order[:, :2], axis=1)
    return order[:, 0], order[:, 1], (top[:, 0] - top[:, 1]) < PF.BAND * np.abs(L).max()


def check_class_map(pred, E, L, what):
    """PF.check_class_map on the ensemble.  Returns the band's share."""
    best, second, band = band_of(E, L)
    share = band.mean()
    assert share <= PF.MAX_BAND_SHARE, f'{what}: {100 * share:.3f} % of the pixels are inside the band'
    pred = pred.astype(np.int64)
    wrong = (pred != best) & ~band
    assert not wrong.any(), f'{what}: {int(wrong.sum())} pixels outside the band differ from the fp64 ensemble, first at {np.argwhere(wrong)[0]}'
    stray = band & (pred != best) & (pred != second)
    assert not stray.any(), f'{what}: {int(stray.sum())} band pixels took a class that is neither of the two best'
    return share


# ---------------------------------------------------------------------------------------------- tail fixtures
def tail_params(seed, w2_scale=1.0, bias2=True, nc=NC):
    """the parameters of upsample16_pred[2], [3], [6] as test_predict_gpu._tail_modules draws them (float32), w2 scaled afterwards"""
    rs = np.random.RandomState(seed)
    p = {'w1': rs.standard_normal((nc, nc, 2, 2)) * np.sqrt(2.0 / (nc * 4)), 'w2': rs.standard_normal((nc, nc, 2, 2)) * np.sqrt(2.0 / (nc * 4)),
         'gamma': rs.uniform(0.5, 1.5, nc), 'beta': rs.standard_normal(nc) * 0.1, 'mean': rs.standard_normal(nc) * 0.1, 'var': rs.uniform(0.5, 1.5, nc),
         'b2': rs.standard_normal(nc) * 0.05}
    p['w2'] = p['w2'] * w2_scale
    if not bias2:
        p['b2'] = None
    return {k: None if v is None else np.asarray(v, np.float32) for k, v in p.items()}


def tail_input(seed, shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def tail_logits(x, p):
    p = {k: None if v is None else v.astype(np.float64) for k, v in p.items()}
    y = O.conv_transpose2d_k2s2(x.astype(np.float64), p['w1'])
    y = O.relu(O.batchnorm_eval(y, p['gamma'], p['beta'], p['mean'], p['var'])[0])
    return O.conv_transpose2d_k2s2(y, p['w2'], p['b2'])


def make_target(seed, shape, ignore=gen.IGNORE, share=0.1, nc=NC):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, nc, shape).astype(np.uint8)
    t[rs.uniform(size=shape) < share] = ignore
    return t


@functools.lru_cache(maxsize=None)
def tail_fixture(f, w2_scale=1.0):
    """-> (p, x (2N,19,H,W), L (2N,19,4H,4W) fp64, E (N,19,4H,4W) fp64); computed once and shared: treat as read-only"""
    pseed, xseed, n, h, w = f
    p = tail_params(pseed, w2_scale)
    x = tail_input(xseed, (2 * n, NC, h, w))
    L = tail_logits(x, p)
    return p, x, L, ensemble_of_views(L)


# ---------------------------------------------------------------------------------------------- head fixtures
@functools.lru_cache(maxsize=None)
def head_fixture(f):
    """PF.HEAD_FIXTURES entry -> (P, x16 (2N,..), x4 (2N,..), target (N,..), L (2N,..) fp64, E fp64): the second view's features are those of
    gen.make_head_inputs(input seed + 1000, ...), standing for the features of the mirrored images; computed once, read-only"""
    pseed, iseed, batch, h16, w16 = f
    P, x16, x4, target = PF.head_fixture(f)
    x16b, x4b, _, _ = gen.make_head_inputs(iseed + 1000, batch, h16, w16, gen.SMALL)
    x16, x4 = np.concatenate([x16, x16b]), np.concatenate([x4, x4b])
    L = PF.oracle_logits(P, x16, x4)
    return P, x16, x4, target, L, ensemble_of_views(L)

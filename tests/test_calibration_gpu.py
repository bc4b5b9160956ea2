"""GPU checks of the calibration record and the confidence map: every producer (the fused tails dsrl_sssr_tail_predict_ex / _flip_ex, the multi-scale
finish dsrl_prob_merge_finish_ex, dsrl_calibration_from_logits) and everything that hands them on (functional.sssr_tail_predict, multiscale_merge,
DSRL.predict, the benchmark command, validation inside training).  Counts are exact integers compared with ==: the reference bins the confidence map
the kernel itself returned (tests/calibration_ref.py); the map is compared with the fp64 reference under a bound taken from the fp32 restatement."""
import functools
import os

import numpy as np
import pytest
import torch

import calibration_ref as R
import gen
import multiscale_ref as MR

pytestmark = pytest.mark.gpu

NC = gen.NUM_CLASSES
IGNORE = gen.IGNORE
B = R.DEFAULT_BINS
SMALL, BIG = (2, NC, 5, 7), (1, NC, 96, 352)           # P = 70: a partial last tile, waves without a tile; 33792 px: 2112 tiles > 4 * 512, a second round
SHAPES = pytest.mark.parametrize('shape', [SMALL, BIG], ids=['70px_partial_tile', '33792px_second_round'])
# The map against fp64 (test_confidence_map_against_fp64): bound = MARGIN x the maximum absolute error of the fp32 restatement
# (calibration_ref.tail_logits in fp32 numpy -> confidence32) against fp64 on the same weights and inputs.  The margin is there because the MFMA
# accumulates its 20-term dot products in another order than numpy; it is the smallest power of two the kernel stayed within when measured on
# the MI355X (profiles/calibration.txt), not a figure taken from the kernel alone: the bound moves with the restatement's own error.
MARGIN = 2.0


def _helpers():
    import hip_helpers as H
    return H


def _tail_modules(seed, w2=None, bias2='random', NC=NC):
    """the recipe of test_confusion_gpu._tail_modules: upsample16_pred[2], [3], [6] with random parameters on the device, in eval mode; and the
    parameters as fp32 numpy arrays"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.nn_modules import HipBatchNorm2d, HipConvTranspose2d
    rs = np.random.RandomState(seed)
    p = {'w1': rs.standard_normal((NC, NC, 2, 2)) * np.sqrt(2.0 / (NC * 4)),
         'w2': rs.standard_normal((NC, NC, 2, 2)) * np.sqrt(2.0 / (NC * 4)) if w2 is None else w2,
         'gamma': rs.uniform(0.5, 1.5, NC), 'beta': rs.standard_normal(NC) * 0.1, 'mean': rs.standard_normal(NC) * 0.1, 'var': rs.uniform(0.5, 1.5, NC),
         'b2': rs.standard_normal(NC) * 0.05 if isinstance(bias2, str) else bias2}
    p = {k: None if v is None else np.asarray(v, np.float32) for k, v in p.items()}
    c1 = HipConvTranspose2d(NC, NC, kernel_size=2, stride=2, padding=0, bias=False)
    bn = HipBatchNorm2d(NC)
    c2 = HipConvTranspose2d(NC, NC, kernel_size=2, stride=2, padding=0, bias=p['b2'] is not None)
    with torch.no_grad():
        c1.weight.copy_(torch.from_numpy(p['w1'])); c2.weight.copy_(torch.from_numpy(p['w2']))
        bn.weight.copy_(torch.from_numpy(p['gamma'])); bn.bias.copy_(torch.from_numpy(p['beta']))
        bn.running_mean.copy_(torch.from_numpy(p['mean'])); bn.running_var.copy_(torch.from_numpy(p['var']))
        if p['b2'] is not None:
            c2.bias.copy_(torch.from_numpy(p['b2']))
    return [m.to(H.DEV).eval() for m in (c1, bn, c2)], p, bn.eps


def _tail_input(seed, shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _target(seed, shape, share=0.1, nc=NC):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, nc, shape).astype(np.uint8)
    t[rs.uniform(size=shape) < share] = IGNORE
    return t


def _zeros(n, dtype=torch.int64):
    return torch.zeros(n, dtype=dtype, device=_helpers().DEV)


def _flag():
    return torch.zeros((), dtype=torch.int32, device=_helpers().DEV)


def _np(t):
    return t.cpu().numpy()


def _own(rec, conf, pred, target, bins=B, nc=NC):
    """the record equals the reference binning of the kernel's own confidence map, class map and the target: integers, =="""
    want = R.record_of(_np(conf), _np(pred), target, bins, nc, IGNORE)
    assert np.array_equal(_np(rec), want), (_np(rec).reshape(3, -1), want.reshape(3, -1))
    return want


@functools.lru_cache(maxsize=None)
def _tail_case(shape, flip=False):
    """modules, input, target and the fp64 logits of a tail fixture (the reference is computed once and shared)"""
    H = _helpers()
    mods, p, eps = _tail_modules(101 + shape[2])
    n = shape[0]
    x = _tail_input(102 + shape[2], ((2 * n,) if flip else (n,)) + shape[1:])
    target = _target(103 + shape[2], (n, 4 * shape[2], 4 * shape[3]))
    L64 = R.tail_logits(x, p, eps, np.float64)
    return mods, p, eps, x, H.dev(x), target, H.dev(target), L64


def _flip_probabilities(L64, n):
    return 0.5 * (R.softmax64(L64[:n]) + R.softmax64(L64[n:])[:, :, :, ::-1])


# ---------------------------------------------------------------------------------------------- 1. the record against the kernel's own map
@SHAPES
@pytest.mark.parametrize('flip', [False, True], ids=['tail', 'flip_tail'])
def test_tail_record_equals_the_binning_of_its_own_map(shape, flip):
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods, _, _, _, xd, target, td, _ = _tail_case(shape, flip)
    rec, flag = _zeros(3 * B), _flag()
    pred, ce, conf = HF.sssr_tail_predict(xd, *mods, target=td, nan_flag=flag, flip=flip, calibration=rec, confidence=True)
    assert conf.dtype == torch.float32 and tuple(conf.shape) == tuple(target.shape) == tuple(pred.shape) and conf.is_contiguous()
    c = _np(conf)
    assert np.isfinite(c).all() and c.min() >= np.float32(1.0) / np.float32(NC) * 0.999 and c.max() <= 1.0 and int(flag.item()) == 0
    want = _own(rec, conf, pred, target)
    assert want[:B].sum() == (target != IGNORE).sum() and np.isfinite(float(ce))
    # the record alone and the map alone: other instantiations, the same bits
    rec2 = _zeros(3 * B)
    pred2, ce2 = HF.sssr_tail_predict(xd, *mods, target=td, flip=flip, calibration=rec2)
    pred3, ce3, conf3 = HF.sssr_tail_predict(xd, *mods, flip=flip, confidence=True)
    assert torch.equal(rec2, rec) and torch.equal(pred2, pred) and torch.equal(pred3, pred) and ce3 is None
    assert _np(conf3).tobytes() == c.tobytes() and _np(ce2).tobytes() == _np(ce).tobytes()


def _merge_views(seed=91, N=2, sizes=((13, 17), (20, 28), (27, 41))):
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal((N, NC, h, w)).astype(np.float32) * 2.0, k == 1) for k, (h, w) in enumerate(sizes)]


def test_merge_finish_record_equals_the_binning_of_its_own_map():
    """three views of unequal size (one of them mirrored) onto (20, 28)"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    views = _merge_views()
    target = _target(92, (2, 20, 28))
    dv = [(H.dev(L), m) for L, m in views]
    rec, flag = _zeros(3 * B), _flag()
    pred, ce, conf = HF.multiscale_merge(dv, (20, 28), target=H.dev(target), nan_flag=flag, calibration=rec, confidence=True)
    assert int(flag.item()) == 0 and conf.dtype == torch.float32 and tuple(conf.shape) == (2, 20, 28)
    _own(rec, conf, pred, target)
    # against fp64: the probabilities of this path are right to multiscale_ref.BAND (derived there), and so is their maximum
    P = MR.merge(views, (20, 28))
    c64, p64 = R.confidence64_of_probabilities(P)
    err = np.abs(_np(conf).astype(np.float64) - c64).max()
    print(f'merge finish: max |conf - fp64| = {err:.3e} (bound {MR.BAND:.1e})')
    assert err <= MR.BAND
    # a single view that is the output grid: the confidence of one softmax, min(1, .) never bites
    one = [(dv[1][0], False)]
    rec1 = _zeros(3 * B)
    pred1, _, conf1 = HF.multiscale_merge(one, (20, 28), target=H.dev(target), calibration=rec1, confidence=True)
    _own(rec1, conf1, pred1, target)
    assert np.abs(_np(conf1).astype(np.float64) - R.confidence64(views[1][0])[0]).max() <= MR.BAND


@pytest.mark.parametrize('C,ld', [(19, 19), (19, 24), (3, 3), (60, 60), (60, 64)])
def test_from_logits_record_map_stride_and_foreign_labels(C, ld):
    """P no multiple of 256 and above one sweep of the grid for the small class counts; pad channels holding 1e30 behind ld > C; labels 255 and 200;
    added to a record that already holds counts; the fp32 restatement is bit-exact where exp2 is (it is compared to 2 ulp of the sum)."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    rs = np.random.RandomState(C * 100 + ld)
    for P in ((1, 257, 1024 * 256 + 300) if C < 60 else (1, 70, 3000)):
        buf = np.full((P, ld), 1e30, np.float32)
        buf[:, :C] = (3.0 * rs.standard_normal((P, C))).astype(np.float32)
        buf[::7, :C] = 0.25                         # all-equal rows: the first maximum, confidence 1 / C
        tg = rs.randint(0, C, P)
        u = rs.uniform(size=P)
        tg[u < 0.1] = 255
        tg[u > 0.95] = 200
        tg = tg.astype(np.uint8)
        logits, target = torch.from_numpy(buf).to(H.DEV), torch.from_numpy(tg).to(H.DEV)
        pre = np.arange(3 * B, dtype=np.int64) * 1000 + 7
        rec, conf, flag = torch.from_numpy(pre.copy()).to(H.DEV), torch.full((P,), -1.0, device=H.DEV), _flag()
        HF.call('dsrl_calibration_from_logits', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, B, rec.data_ptr(), conf.data_ptr(), flag.data_ptr(),
                HF._stream())
        pred = np.argmax(buf[:, :C], axis=1)
        want = R.record_of(_np(conf), pred, tg, B, C, 255)
        assert np.array_equal(_np(rec), pre + want), f'C={C} ld={ld} P={P}'
        assert int(flag.item()) == (2 if (tg == 200).any() and C <= 200 else 0)
        c = _np(conf)
        L4 = buf[:, :C].T.reshape(1, C, 1, P)
        assert np.array_equal(c[::7], np.full(c[::7].shape, np.float32(1.0) / np.float32(C), np.float32))
        assert np.abs(c.astype(np.float64) - R.confidence64(L4)[0].reshape(-1)).max() <= 4 * (C + 1) * 2.0 ** -24
        assert np.abs(c - R.confidence32(L4).reshape(-1)).max() <= 4 * 2.0 ** -24
        # the map alone (no record, no target), and the record alone
        only = torch.empty(P, device=H.DEV)
        HF.call('dsrl_calibration_from_logits', logits.data_ptr(), ld, None, P, C, 255, 0, None, only.data_ptr(), None, HF._stream())
        alone = _zeros(3 * B)
        HF.call('dsrl_calibration_from_logits', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, B, alone.data_ptr(), None, None, HF._stream())
        assert _np(only).tobytes() == c.tobytes() and np.array_equal(_np(alone), want)


def test_from_logits_wrapper_and_the_metric_class():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.metrices import Calibration
    rs = np.random.RandomState(71)
    L = (3.0 * rs.standard_normal((2, NC, 12, 21))).astype(np.float32)
    tg = _target(72, (2, 12, 21))
    rec, conf = _zeros(3 * 10), torch.empty((2, 12, 21), device=H.DEV)
    out = HF.calibration_counts_(rec, H.dev(L), H.dev(tg), IGNORE, 10, conf)
    assert out is rec
    want = R.record_of(_np(conf), L.argmax(1), tg, 10)
    assert np.array_equal(_np(rec), want)
    a, b = Calibration(bins=10), Calibration(bins=10)
    a.update_from_logits(H.dev(L), H.dev(tg))
    assert a.record.is_cuda and np.array_equal(_np(a.record), want)
    b.merge(a); b.merge(a.record.cpu().to(H.DEV))
    fa, fb, fr = a.result(), b.result(), R.figures(want)
    assert fa['ECE'] == fb['ECE'] and abs(fa['ECE'] - fr['ECE']) <= 1e-15 and abs(fa['MCE'] - fr['MCE']) <= 1e-15 and fb['pixels'] == 2 * fa['pixels']
    assert 0.0 <= fa['ECE'] <= fa['MCE'] <= 1.0
    a.reset()
    assert a.result()['pixels'] == 0 and np.isnan(a.result()['ECE'])
    with pytest.raises(ValueError, match='lives on'):
        a.merge(torch.zeros(30, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- 2. the map against fp64
@SHAPES
def test_confidence_map_against_fp64(shape):
    """Bound: MARGIN x the error of the fp32 restatement (numpy fp32 tail -> confidence32) against the fp64 reference on the same weights and inputs.
    Measured on the MI355X when this test first passed (profiles/calibration.txt): 70 px - kernel 1.115e-7, restatement 8.58e-8 (ratio 1.30);
    33792 px - kernel 1.544e-7, restatement 1.722e-7 (ratio 0.90): the smallest power-of-two margin the kernel stays within is 2.  The flip tail
    averages two such probabilities and is held to the same bound against the larger of its two views' restatement errors (measured: kernel
    5.4e-8 / 8.4e-8 against 1.06e-7 / 1.76e-7)."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods, p, eps, x, xd, _, _, L64 = _tail_case(shape)
    c64, p64 = R.confidence64(L64)
    restated = R.confidence32(R.tail_logits(x, p, eps, np.float32))
    err32 = np.abs(restated.astype(np.float64) - c64).max()
    pred, _, conf = HF.sssr_tail_predict(xd, *mods, confidence=True)
    err = np.abs(_np(conf).astype(np.float64) - c64).max()
    print(f'tail {shape}: max |conf - fp64| kernel {err:.3e}, fp32 restatement {err32:.3e}, margin {MARGIN:g}')
    assert 0 < err32 < 1e-6
    assert err <= MARGIN * err32
    mods, p, eps, x, xd, _, _, L64f = _tail_case(shape, True)
    n = shape[0]
    c64f, _ = R.confidence64_of_probabilities(_flip_probabilities(L64f, n))
    L32 = R.tail_logits(x, p, eps, np.float32)
    err32f = max(np.abs(R.confidence32(L32[:n]).astype(np.float64) - R.confidence64(L64f[:n])[0]).max(),
                 np.abs(R.confidence32(L32[n:]).astype(np.float64) - R.confidence64(L64f[n:])[0]).max())
    _, _, conff = HF.sssr_tail_predict(xd, *mods, flip=True, confidence=True)
    errf = np.abs(_np(conff).astype(np.float64) - c64f).max()
    print(f'flip tail {shape}: max |conf - fp64| kernel {errf:.3e}, fp32 restatement of a view {err32f:.3e}, margin {MARGIN:g}')
    assert errf <= MARGIN * err32f


# ---------------------------------------------------------------------------------------------- 3. the record against fp64, end to end
def test_record_against_fp64_end_to_end():
    """Pixels whose fp64 confidence lies within 1e-5 of a bin edge, or whose top two fp64 logits differ by less than 1e-5, leave through the target;
    at most 2 % may (the reference alone decides).  After that n_b and hit_b are exact and q_b / 2^24 is within n_b x the bound of the map."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    H = _helpers()
    mods, p, eps, x, xd, target, _, L64 = _tail_case(SMALL)
    c64, p64 = R.confidence64(L64)
    top2 = np.sort(L64, axis=1)[:, -2:]
    frac = c64 * B - np.floor(c64 * B)
    near = (np.minimum(frac, 1.0 - frac) / B < 1e-5) | (top2[:, 1] - top2[:, 0] < 1e-5)
    assert near.mean() <= 0.02, near.mean()
    tg = np.where(near, IGNORE, target).astype(np.uint8)
    rec = _zeros(3 * B)
    HF.sssr_tail_predict(xd, *mods, target=H.dev(tg), calibration=rec)
    got, want = _np(rec), R.record_of(c64, p64, tg, B)
    assert np.array_equal(got[:2 * B], want[:2 * B])
    bound = MARGIN * np.abs(R.confidence32(R.tail_logits(x, p, eps, np.float32)).astype(np.float64) - c64).max() + 2.0 ** -25      # + the fixed-point step
    n = got[:B].astype(np.float64)
    assert (np.abs(got[2 * B:] - want[2 * B:]) / R.Q_SCALE <= n * bound).all()
    f, g = R.figures(got), R.figures(want)
    assert abs(f['ECE'] - g['ECE']) <= bound and 0 < f['ECE'] < 1


# ---------------------------------------------------------------------------------------------- 4. exclusions
@pytest.mark.parametrize('flip', [False, True], ids=['tail', 'flip_tail'])
def test_exclusions_ignored_foreign_and_nan(flip):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods, _, _, x, xd, target, td, _ = _tail_case(SMALL, flip)
    n, h, w = SMALL[0], SMALL[2], SMALL[3]
    rec, flag = _zeros(3 * B), _flag()
    HF.sssr_tail_predict(xd, *mods, target=H.dev(np.full_like(target, IGNORE)), nan_flag=flag, flip=flip, calibration=rec)
    assert not _np(rec).any() and int(flag.item()) == 0                 # every pixel ignored: a zero record
    foreign = target.copy()
    foreign[0, 3:9, 5:17] = 200
    foreign[n - 1, 4 * h - 1, 4 * w - 3:] = 77
    rec, flag = _zeros(3 * B), _flag()
    pred, _, conf = HF.sssr_tail_predict(xd, *mods, target=H.dev(foreign), nan_flag=flag, flip=flip, calibration=rec, confidence=True)
    assert int(flag.item()) == 2
    want = _own(rec, conf, pred, foreign)
    assert want[:B].sum() == (foreign < NC).sum()
    # one NaN input pixel: bit 0, its 4x4 patch in no bin (the ReLU hides the NaN from the logits), every other pixel as without it
    clean_rec = _zeros(3 * B)
    cpred, _, cconf = HF.sssr_tail_predict(xd, *mods, target=td, flip=flip, calibration=clean_rec, confidence=True)
    bad = x.copy()
    bad[1, 4, 2, 3] = np.nan
    rec, flag = _zeros(3 * B), _flag()
    npred, _, nconf = HF.sssr_tail_predict(H.dev(bad), *mods, target=td, nan_flag=flag, flip=flip, calibration=rec, confidence=True)
    assert int(flag.item()) & 1
    patch = np.zeros(target.shape, bool)
    patch[1, 8:12, 12:16] = True
    nc_, cc_ = _np(nconf), _np(cconf)
    assert np.isnan(nc_[patch]).all() and nc_[~patch].tobytes() == cc_[~patch].tobytes()
    without = np.where(patch, IGNORE, target).astype(np.uint8)
    assert np.array_equal(_np(rec), R.record_of(cc_, _np(cpred), without, B))
    assert _np(rec)[:B].sum() == _np(clean_rec)[:B].sum() - ((target != IGNORE) & patch).sum()


def test_exclusions_from_logits_and_merge():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    rs = np.random.RandomState(5)
    L = (2.0 * rs.standard_normal((1, NC, 9, 31))).astype(np.float32)
    tg = _target(6, (1, 9, 31))
    clean, cconf = _zeros(3 * B), torch.empty((1, 9, 31), device=H.DEV)
    HF.calibration_counts_(clean, H.dev(L), H.dev(tg), IGNORE, B, cconf)
    bad = L.copy()
    bad[0, 7, 4, 11] = np.nan
    rec, conf, flag = _zeros(3 * B), torch.empty((1, 9, 31), device=H.DEV), _flag()
    HF.calibration_counts_(rec, H.dev(bad), H.dev(tg), IGNORE, B, conf, flag)
    c = _np(conf)
    assert int(flag.item()) == 1 and np.isnan(c[0, 4, 11]) and np.isnan(c).sum() == 1
    without = tg.copy()
    without[0, 4, 11] = IGNORE
    assert np.array_equal(_np(rec), R.record_of(_np(cconf), L.argmax(1), without, B))
    zero = _zeros(3 * B)
    HF.calibration_counts_(zero, H.dev(L), H.dev(np.full_like(tg, IGNORE)))
    assert not _np(zero).any()
    # the merge finish: a NaN in one view reaches the last launch through the accumulator
    views = _merge_views()
    target = _target(92, (2, 20, 28))
    views[0][0][1, 3, 5, 6] = np.nan
    rec, flag = _zeros(3 * B), _flag()
    pred, _, conf = HF.multiscale_merge([(H.dev(v), m) for v, m in views], (20, 28), target=H.dev(target), nan_flag=flag, calibration=rec, confidence=True)
    assert int(flag.item()) & 1 and np.isnan(_np(conf)).any() and not np.isnan(_np(conf)[0]).any()
    _own(rec, conf, pred, target)
    assert _np(rec)[:B].sum() == ((target != IGNORE) & ~np.isnan(_np(conf))).sum()


# ---------------------------------------------------------------------------------------------- 5. extremes
def test_extremes_flat_logits_a_certain_class_and_the_bin_limits():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    maxb = _lib.load().dsrl_calibration_max_bins()
    assert maxb == 64 == HF.calibration_max_bins()
    x = H.dev(_tail_input(7, SMALL))
    target = _target(8, (2, 20, 28))
    td = H.dev(target)
    counted = int((target != IGNORE).sum())
    # w2 = 0, zero bias: all logits equal -> class 0, confidence 1.0f / 19 as the shared function forms it, every counted pixel in its bin
    mods, _, _ = _tail_modules(3, w2=np.zeros((NC, NC, 2, 2)), bias2=np.zeros(NC))
    one19 = np.float32(1.0) / np.float32(19.0)
    for bins in (1, B, maxb):
        rec = _zeros(3 * bins)
        pred, _, conf = HF.sssr_tail_predict(x, *mods, target=td, calibration=rec, confidence=True)
        assert not _np(pred).any() and np.array_equal(_np(conf), np.full(target.shape, one19, np.float32))
        b = int(R.bin_of(one19, bins))
        r = _np(rec).reshape(3, bins)
        assert r[0, b] == counted and r[0].sum() == counted and r[1, b] == (target == 0).sum()
        assert r[2, b] == counted * int(np.rint(np.float32(one19 * np.float32(R.Q_SCALE))))
    # one class's bias at +1e4: confidence exactly 1.0, the last bin, q = n 2^24
    bias = np.zeros(NC, np.float32)
    bias[7] = 1e4
    mods, _, _ = _tail_modules(4, bias2=bias)
    for bins in (1, B, maxb):
        for flip in (False, True):
            xx = torch.cat([x, x.flip(3)]) if flip else x
            rec = _zeros(3 * bins)
            pred, _, conf = HF.sssr_tail_predict(xx, *mods, target=td, flip=flip, calibration=rec, confidence=True)
            assert (_np(pred) == 7).all() and np.array_equal(_np(conf), np.ones(target.shape, np.float32))
            r = _np(rec).reshape(3, bins)
            assert r[0, bins - 1] == counted == r[0].sum() and r[2, bins - 1] == counted * 2 ** 24 and r[1, bins - 1] == (target == 7).sum()
    # beyond the limit, and malformed records: refused before any launch
    for bad in (_zeros(3 * (maxb + 1)), _zeros(3 * B, torch.int32), _zeros(3 * B + 1), _zeros((3 * B, 2))[:, 0], torch.zeros(3 * B, dtype=torch.int64)):
        with pytest.raises((ValueError, HF.DsrlHipError, RuntimeError)):
            HF.sssr_tail_predict(x, *mods, target=td, calibration=bad)
    with pytest.raises(HF.DsrlHipError, match='needs a target'):
        HF.sssr_tail_predict(x, *mods, calibration=_zeros(3 * B))
    lib = _lib.load()
    torch.cuda.synchronize()
    logits, rec = torch.zeros((64, NC), device=H.DEV), _zeros(3 * (maxb + 1))
    code = lib.dsrl_calibration_from_logits(logits.data_ptr(), NC, td.data_ptr(), 64, NC, 255, maxb + 1, rec.data_ptr(), None, None, HF._stream())
    assert code == -1 and b'bins' in lib.dsrl_last_error()
    code = lib.dsrl_calibration_from_logits(torch.zeros((64, 61), device=H.DEV).data_ptr(), 61, td.data_ptr(), 64, 61, 255, B, rec.data_ptr(), None, None,
                                            HF._stream())
    assert code == -2 and b'classes' in lib.dsrl_last_error()
    torch.cuda.synchronize()
    assert not _np(rec).any()


# ---------------------------------------------------------------------------------------------- 6. accumulation and determinism
@pytest.mark.parametrize('producer', ['tail', 'flip_tail', 'merge'])
def test_accumulation_determinism_and_an_image_alone_or_in_a_batch(producer):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    if producer == 'merge':
        views = _merge_views()
        target = _target(92, (2, 20, 28))

        def run(rec, sel=slice(None)):
            dv = [(H.dev(np.ascontiguousarray(L[sel])), m) for L, m in views]
            return HF.multiscale_merge(dv, (20, 28), target=H.dev(np.ascontiguousarray(target[sel])), calibration=rec, confidence=True)
    else:
        flip = producer == 'flip_tail'
        mods, _, _, x, _, target, _, _ = _tail_case(SMALL, flip)
        n = SMALL[0]

        def run(rec, sel=slice(None)):
            xs = np.concatenate([x[:n][sel], x[n:][sel]]) if flip else x[sel]
            return HF.sssr_tail_predict(H.dev(np.ascontiguousarray(xs)), *mods, target=H.dev(np.ascontiguousarray(target[sel])), flip=flip,
                                        calibration=rec, confidence=True)
    a, b, twice = _zeros(3 * B), _zeros(3 * B), _zeros(3 * B)
    pa, ca, fa = run(a)
    pb, cb, fb = run(b)
    assert _np(a).tobytes() == _np(b).tobytes() and _np(fa).tobytes() == _np(fb).tobytes() and torch.equal(pa, pb)      # two runs, equal bytes
    run(twice); run(twice)
    assert np.array_equal(_np(twice), 2 * _np(a))                                                                       # two calls into one record
    parts = _zeros(3 * B)
    for i in range(2):                                                                                                  # an image alone
        pi, _, fi = run(parts, slice(i, i + 1))
        assert _np(fi)[0].tobytes() == _np(fa)[i].tobytes() and torch.equal(pi[0], pa[i])
    assert np.array_equal(_np(parts), _np(a))


# ---------------------------------------------------------------------------------------------- 7. off means off
def test_off_means_off():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    for flip in (False, True):
        mods, _, _, _, xd, target, td, _ = _tail_case(SMALL, flip)
        base = dict(target=td, flip=flip)
        c0, m0, f0 = _zeros(3 * NC + 2), _zeros(NC * NC), _flag()
        p0, ce0 = HF.sssr_tail_predict(xd, *mods, counts=c0, confusion=m0, nan_flag=f0, **base)
        for kw in ({'calibration': True}, {'confidence': True}, {'calibration': True, 'confidence': True}):
            kw = dict(kw)
            if 'calibration' in kw:
                kw['calibration'] = _zeros(3 * B)
            c1, m1, f1 = _zeros(3 * NC + 2), _zeros(NC * NC), _flag()
            out = HF.sssr_tail_predict(xd, *mods, counts=c1, confusion=m1, nan_flag=f1, **base, **kw)
            assert len(out) == (3 if kw.get('confidence') else 2)
            assert torch.equal(out[0], p0) and torch.equal(c1, c0) and torch.equal(m1, m0) and int(f1.item()) == int(f0.item())
            assert _np(out[1]).tobytes() == _np(ce0).tobytes()
        assert len(HF.sssr_tail_predict(xd, *mods, flip=flip)) == 2
    views = [(H.dev(L), m) for L, m in _merge_views()]
    td = H.dev(_target(92, (2, 20, 28)))
    c0, m0 = _zeros(3 * NC + 2), _zeros(NC * NC)
    p0, ce0 = HF.multiscale_merge(views, (20, 28), target=td, counts=c0, confusion=m0)
    c1, m1 = _zeros(3 * NC + 2), _zeros(NC * NC)
    p1, ce1, _ = HF.multiscale_merge(views, (20, 28), target=td, counts=c1, confusion=m1, calibration=_zeros(3 * B), confidence=True)
    assert torch.equal(p1, p0) and torch.equal(c1, c0) and torch.equal(m1, m0) and _np(ce1).tobytes() == _np(ce0).tobytes()


def test_fallback_head_goes_through_the_logits_kernel():
    """a head the tail kernel does not implement (8 classes): modules -> logits -> dsrl_calibration_from_logits"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    assert _lib.query('dsrl_sssr_tail_predict_supported', 2, 6, 8, 8, 8, 8) == 0
    for flip in (False, True):
        mods, _, _ = _tail_modules(61, NC=8)
        x = H.dev(_tail_input(62, (4 if flip else 2, 8, 6, 8)))
        target = _target(63, (2, 24, 32), nc=8)
        rec = _zeros(3 * B)
        pred, _, conf = HF.sssr_tail_predict(x, *mods, target=H.dev(target), flip=flip, calibration=rec, confidence=True)
        _own(rec, conf, pred, target, nc=8)
        assert _np(conf).min() >= 0.125 * 0.999 and _np(conf).max() <= 1.0


def test_merge_of_a_class_count_the_kernel_refuses():
    """40 classes: dsrl_prob_merge_supported says no, the ensemble is composed from torch ops and the record binned by the same definition"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    assert _lib.query('dsrl_prob_merge_supported', 1, 1, 1, 1, 1, 40) == 0
    rs = np.random.RandomState(17)
    views = [(H.dev((2.0 * rs.standard_normal((1, 40, h, w))).astype(np.float32)), k == 1) for k, (h, w) in enumerate(((5, 9), (8, 12)))]
    target = _target(18, (1, 8, 12), nc=40)
    target[0, 2, 3] = 77
    rec = _zeros(3 * B)
    pred, _, conf = HF.multiscale_merge(views, (8, 12), target=H.dev(target), calibration=rec, confidence=True)
    _own(rec, conf, pred, target, nc=40)
    assert _np(rec)[:B].sum() == (target < 40).sum() and _np(conf).max() <= 1.0 and _np(conf).min() >= 1.0 / 40 * 0.999
    only = HF.multiscale_merge(views, (8, 12), confidence=True)
    assert len(only) == 3 and only[1] is None and _np(only[2]).tobytes() == _np(conf).tobytes()


# ---------------------------------------------------------------------------------------------- the model: predict, compiled predictor, commands
@pytest.fixture(scope='module')
def model():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    torch.manual_seed(1234)
    return DSRL(3, CS).to(H.DEV).to(memory_format=torch.channels_last).eval()


def _image(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(_helpers().DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize('kw', [{}, {'flip': True}, {'scales': (0.75, 1.0)}], ids=['plain', 'flip', 'scales'])
def test_predict_record_equals_the_binning_of_its_own_map(model, kw):
    H = _helpers()
    x, target = _image(200, (2, 3, 64, 128)), _target(210, (2, 128, 256))
    td = H.dev(target)
    rec = _zeros(3 * B)
    pred, counts, ce, conf = model.predict(x, td, calibration=rec, confidence=True, **kw)
    assert tuple(conf.shape) == (2, 128, 256) and conf.dtype == torch.float32
    _own(rec, conf, pred, target)
    pred0, counts0, ce0 = model.predict(x, td, **kw)
    assert torch.equal(pred0, pred) and torch.equal(counts0, counts) and _np(ce0).tobytes() == _np(ce).tobytes()
    out = model.predict(x, confidence=True, **kw)
    assert len(out) == 4 and out[1] is None and out[2] is None and _np(out[3]).tobytes() == _np(conf).tobytes()


def test_compiled_predictor_refuses_both_arguments(model):
    from dualsuperreslearningforsemseg_amd import functional as HF
    H = _helpers()
    x, td = _image(200, (2, 3, 64, 128)), H.dev(_target(210, (2, 128, 256)))
    with pytest.raises(HF.DsrlHipError, match='needs a target'):
        model.predict(x, calibration=_zeros(3 * B))
    cp = model.compile_predict()
    try:
        with pytest.raises(ValueError, match='calibration'):
            cp(x, td, calibration=_zeros(3 * B))
        with pytest.raises(ValueError, match='confidence'):
            cp(x, td, confidence=True)
        assert cp.replays == 0 and cp.num_graphs == 0
        pred, _, _ = cp(x, td)
        assert torch.equal(pred, model.predict(x, td)[0])
    finally:
        cp.release()


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_benchmark_reports_ece_and_writes_the_table(model, tmp_path, flip):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.metrices import Calibration
    weights = str(tmp_path / 'final.weights')
    torch.save({'model_state_dict': model.state_dict()}, weights)
    batches = [((_image(10 + i, (n, 3, 64, 128)), None), (H.dev(_target(20 + i, (n, 128, 256))), None)) for i, n in enumerate((2, 2, 1))]
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda split, batch_size, device, rank, world: batches}
    plain = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=str(tmp_path / 'plain'), flip=flip)
    text0 = open(os.path.join(str(tmp_path / 'plain'), 'benchmark.txt')).read()
    assert set(plain) == {'CE', 'mIoU', 'accuracy', 'mIoU_dataset', 'IoU_per_class', 'pixel_accuracy', 'mean_class_accuracy', 'fwIoU', 'confusion_matrix'}
    assert 'alibration' not in text0 and 'eliability' not in text0
    for arg, bins in ((True, 15), (7, 7)):
        out_dir = str(tmp_path / f'out{bins}')
        result = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=out_dir, flip=flip, calibration=arg)
        by_hand = Calibration(bins=bins, ignore_index=CS.IGNORE_CLASS_LABEL)
        for (img, _), (target, _) in batches:
            model.predict(img, target, flip=flip, calibration=by_hand.on(H.DEV))
        want = by_hand.result()
        assert result['ECE'] == want['ECE'] and result['MCE'] == want['MCE'] and result['mean_confidence'] == want['mean_confidence']
        assert 0 <= result['ECE'] <= result['MCE'] <= 1 and result['reliability']['n'] == [int(v) for v in want['bins']['n']]
        assert len(result['reliability']['acc']) == bins == len(result['reliability']['conf'])
        assert {k: v for k, v in result.items() if k in plain} == plain
        assert set(result) - set(plain) == {'ECE', 'MCE', 'mean_confidence', 'reliability'}
        text = open(os.path.join(out_dir, 'benchmark.txt')).read()
        assert 'Expected calibration error: {:.4f}, maximum: {:.4f}'.format(result['ECE'], result['MCE']) in text
        rows = [ln for ln in text.splitlines() if ln.startswith('[')]
        assert len(rows) == bins and sum(int(r.split()[2]) for r in rows) == want['pixels']
        strip = lambda s: '\n'.join(ln for ln in s.splitlines() if not ln.startswith('On: '))
        assert strip(text).startswith(strip(text0).replace(str(tmp_path / 'plain'), out_dir).rstrip('\n'))


def test_validation_reports_finite_ece(tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs

    def factory(split, batch_size, device, rank, world):
        return TR.SyntheticCityscapes(batch_size, (32, 64), device, rank=rank, length=2)

    hist = TR.train_or_resume(is_resuming_training=False, device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                              dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': factory}, val_interval=1, checkpoint_interval=1,
                              checkpoint_history=0, init_weights=None, batch_size=2, epochs=2, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9,
                              weights_decay=5e-4, poly_power=0.9, w1=0.1, w2=1.0, freeze_batch_norm=False, description='test', early_stopping=False,
                              pretrained_backbone=False, model_input_size=(32, 64), stage=1, experiment_id=str(tmp_path / 'exp'))
    recs = [r for r in hist if 'val' in r]
    assert len(recs) == 2
    for r in recs:
        assert len(r['val']) == 7 and np.isfinite(r['val_ECE']) and 0.0 <= r['val_ECE'] <= r['val_MCE'] <= 1.0

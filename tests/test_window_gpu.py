"""GPU checks of sliding-window inference: the merge kernels (dsrl_window_merge, dsrl_window_merge_finish(_ex)) behind functional.window_merge,
DSRL.predict(window=...), the refusal of CompiledPredictor and the benchmark / test commands with a window.  The reference is the fp64 restatement
in window_ref; bands and tolerances are multiscale_ref's (see window_ref for why they bound this path)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import calibration_ref as R
import gen
import multiscale_ref as MR
import predict_fixtures as PF
import predict_flip_ref as PFR
import window_ref as WR

pytestmark = pytest.mark.gpu

NC = gen.NUM_CLASSES
B = R.DEFAULT_BINS


def _helpers():
    import hip_helpers as H
    return H


def _counts(fill=0, nc=NC):
    return torch.full((3 * nc + 2,), fill, dtype=torch.int64, device=_helpers().DEV)


def _cm(fill=0, nc=NC):
    return torch.full((nc * nc,), fill, dtype=torch.int64, device=_helpers().DEV)


def _flag():
    return torch.zeros((), dtype=torch.int32, device=_helpers().DEV)


def _np(t):
    return t.cpu().numpy()


def _dev_views(views, ld=None):
    """[L numpy] -> [pixel-major device tensor]; `ld`: the logits sit in the first 19 channels of an ld-channel tensor"""
    H = _helpers()
    out = []
    for L in views:
        t = H.dev(np.asarray(L, np.float32))
        if ld is not None:
            wide = torch.full((t.shape[0], ld) + tuple(t.shape[2:]), 7.0, device=H.DEV).contiguous(memory_format=torch.channels_last)
            wide[:, :t.shape[1]] = t
            t = wide[:, :t.shape[1]]
            assert t.stride(1) == 1 and t.stride(3) == ld
        out.append(t)
    return out


def _numpy_cm(pred, target, nc=NC, ignore=gen.IGNORE):
    valid = (target != ignore) & (target < nc)
    return np.bincount(target[valid].astype(np.int64) * nc + pred[valid].astype(np.int64), minlength=nc * nc)


def _merge(fixture, dv, **kw):
    from dualsuperreslearningforsemseg_amd import functional as HF
    return HF.window_merge(dv, fixture[5], fixture[6], (fixture[2], fixture[3]), flip=fixture[7], **kw)


def _abi_launches(fixture, dv, acc, target=None, out=None, pred=None):
    """the launches of the plan through the C ABI itself, into the accumulator the caller prepared"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    seed, n, ho, wo, (wh, ww), ys, xs, flip = fixture
    vpp, st = (2 if flip else 1), HF._stream()
    k = 0
    for i in range(len(ys)):
        for j in range(len(xs)):
            for v in range(vpp):
                t = dv[k]
                k += 1
                assert HF._ld_of(t) == NC
                fy, fx = (wh, 0) if v else (HF.window_fresh(ys, wh, i), HF.window_fresh(xs, ww, j))
                _lib.call('dsrl_window_merge', t.data_ptr(), NC, n, wh, ww, NC, v, acc.data_ptr(), ho, wo, ys[i], xs[j], fy, fx, st)
    pred = torch.empty((n, ho, wo), device=H.DEV, dtype=torch.uint8) if pred is None else pred
    ws = torch.empty(max(_lib.query('dsrl_window_merge_workspace_bytes', n, ho, wo), 256), device=H.DEV, dtype=torch.uint8)
    cy, cx = (ctypes.c_int * len(ys))(*ys), (ctypes.c_int * len(xs))(*xs)
    _lib.call('dsrl_window_merge_finish', acc.data_ptr(), n, NC, ho, wo, cy, len(ys), cx, len(xs), wh, ww, vpp, pred.data_ptr(),
              None if target is None else target.data_ptr(), gen.IGNORE, None, None if out is None else out.data_ptr(), None, ws.data_ptr(), ws.numel(), None,
              st)
    return pred


def _acc(fixture, fill=None):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib
    n, ho, wo = fixture[1:4]
    nfl = _lib.query('dsrl_prob_merge_acc_bytes', n, ho, wo, NC) // 4
    assert nfl == n * NC * ho * wo
    return torch.empty(nfl, device=H.DEV, dtype=torch.float32) if fill is None else torch.full((nfl,), fill, device=H.DEV, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- class maps and the loss
@pytest.mark.parametrize('fixture', WR.FIXTURES, ids=WR.fixture_id)
def test_class_maps_and_loss_against_the_fp64_ensemble(fixture):
    """Every fixture: the class map against the fp64 arg-max under the band rule, and ce = [mean, counted pixels] through the C ABI directly."""
    H = _helpers()
    views, P, _ = WR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    dv = _dev_views(views)
    pred, ce = _merge(fixture, dv)
    assert ce is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (n, ho, wo)
    share = WR.check_class_map(_np(pred), P, 'window kernels vs fp64 ensemble')
    target = PFR.make_target(191 + fixture[0], (n, ho, wo))
    ref = WR.ce(P, target)
    td = H.dev(target)
    out = torch.zeros(2, device=H.DEV, dtype=torch.float32)
    pred_abi = _abi_launches(fixture, dv, _acc(fixture), td, out)
    got, cnt = (float(v) for v in out.cpu())
    print(f'{WR.fixture_id(fixture)}: band {100 * share:.3f} %, ce ref {ref:.9f}, kernel {got:.9f}, error {abs(got - ref):.3e}, '
          f'tolerance {WR.CE_TOL * max(1.0, abs(ref)):.3e}')
    assert torch.equal(pred_abi, pred)
    assert cnt == float((target != gen.IGNORE).sum())
    assert abs(got - ref) <= WR.CE_TOL * max(1.0, abs(ref))
    # functional.window_merge is these launches
    pred2, ce2 = _merge(fixture, dv, target=td)
    assert torch.equal(pred2, pred) and _np(ce2).tobytes() == _np(out[:1]).tobytes()
    # every pixel ignored: NaN, as torch
    _, cen = _merge(fixture, dv, target=H.dev(np.full((n, ho, wo), gen.IGNORE, np.uint8)))
    assert np.isnan(float(cen))


@pytest.mark.parametrize('poison', [1e30, float('nan')], ids=['1e30', 'nan'])
@pytest.mark.parametrize('fixture', WR.FIXTURES, ids=WR.fixture_id)
def test_a_poisoned_accumulator_gives_the_same_bytes(fixture, poison):
    """The same launches with acc pre-filled: nothing stale is read, and the fresh rule stores wherever it should."""
    H = _helpers()
    views, _, _ = WR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    dv = _dev_views(views)
    td = H.dev(PFR.make_target(7, (n, ho, wo)))
    pred, ce = _merge(fixture, dv, target=td)
    out = torch.zeros(2, device=H.DEV, dtype=torch.float32)
    got = _abi_launches(fixture, dv, _acc(fixture, poison), td, out)
    assert torch.equal(got, pred) and _np(out[:1]).tobytes() == _np(ce).tobytes() and np.isfinite(float(ce))


# ---------------------------------------------------------------------------------------------- counters, confusion, calibration
@pytest.mark.parametrize('fixture', [WR.FIXTURES[0], WR.FIXTURES[1], WR.FIXTURES[2], WR.FIXTURES[4]], ids=WR.fixture_id)
def test_counts_and_confusion_of_the_kernels_own_class_map(fixture):
    H = _helpers()
    views, _, _ = WR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    dv = _dev_views(views)
    target = PFR.make_target(13, (n, ho, wo))
    td = H.dev(target)
    counts, cm, flag = _counts(5), _cm(3), _flag()                     # both are ADDED into what the buffers hold
    pred, ce = _merge(fixture, dv, target=td, counts=counts, confusion=cm, nan_flag=flag)
    pred_h = _np(pred)
    assert np.array_equal(_np(counts), 5 + PF.counts_table(pred_h, target))
    assert np.array_equal(_np(cm), 3 + _numpy_cm(pred_h, target))
    assert int(flag.item()) == 0 and np.isfinite(float(ce))
    # counts without the matrix: the same bits; the class map is the same with and without a target
    only = _counts(5)
    pred2, ce2 = _merge(fixture, dv, target=td, counts=only)
    assert torch.equal(only, counts) and torch.equal(pred2, pred) and _np(ce2).tobytes() == _np(ce).tobytes()
    assert torch.equal(_merge(fixture, dv)[0], pred)
    # ignore_index = 0
    c0, m0 = _counts(), _cm()
    p0, _ = _merge(fixture, dv, target=td, ignore_index=0, counts=c0, confusion=m0)
    assert np.array_equal(_np(c0), PF.counts_table(_np(p0), target, NC, 0))
    assert np.array_equal(_np(m0), _numpy_cm(_np(p0), target, NC, 0))


@pytest.mark.parametrize('fixture', [WR.FIXTURES[1], WR.FIXTURES[2], WR.FIXTURES[4]], ids=WR.fixture_id)
def test_calibration_record_and_confidence_map(fixture):
    """The record is the reference binning of the kernel's own confidence map (integers, ==); the map against min(1, max P) of the fp64 ensemble
    under multiscale_ref.BAND, which bounds the error of P (tot / cnt adds one rounding)."""
    H = _helpers()
    views, P, _ = WR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    dv = _dev_views(views)
    target = PFR.make_target(17, (n, ho, wo))
    td = H.dev(target)
    pre = np.arange(3 * B, dtype=np.int64) * 10 + 1
    rec, flag = torch.from_numpy(pre.copy()).to(H.DEV), _flag()
    pred, ce, conf = _merge(fixture, dv, target=td, nan_flag=flag, calibration=rec, confidence=True)
    assert int(flag.item()) == 0 and conf.dtype == torch.float32 and tuple(conf.shape) == (n, ho, wo)
    assert np.array_equal(_np(rec) - pre, R.record_of(_np(conf), _np(pred), target, B, NC, gen.IGNORE))
    c64, _ = R.confidence64_of_probabilities(P)
    err = np.abs(_np(conf).astype(np.float64) - c64).max()
    print(f'{WR.fixture_id(fixture)}: max |conf - fp64| = {err:.3e} (bound {MR.BAND:.1e})')
    assert err <= MR.BAND
    # the record alone and the map alone: other instantiations, the same bits; and both leave pred and ce as they are
    rec2 = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
    pred2, ce2 = _merge(fixture, dv, target=td, calibration=rec2)
    pred3, ce3, conf3 = _merge(fixture, dv, confidence=True)
    pred0, ce0 = _merge(fixture, dv, target=td)
    assert np.array_equal(_np(rec2), _np(rec) - pre) and torch.equal(pred2, pred) and torch.equal(pred3, pred) and torch.equal(pred0, pred) and ce3 is None
    assert _np(conf3).tobytes() == _np(conf).tobytes() and _np(ce2).tobytes() == _np(ce).tobytes() == _np(ce0).tobytes()


# ---------------------------------------------------------------------------------------------- addressing, determinism, single window
def test_a_wider_pixel_stride_gives_the_same_bits():
    H = _helpers()
    for f in (WR.FIXTURES[1], WR.FIXTURES[2]):
        views, P, _ = WR.fixture(f)
        td = H.dev(PFR.make_target(90, (f[1], f[2], f[3])))
        pred, ce = _merge(f, _dev_views(views, ld=24), target=td)
        WR.check_class_map(_np(pred), P, 'ld = 24')
        pred19, ce19 = _merge(f, _dev_views(views), target=td)
        assert torch.equal(pred, pred19) and _np(ce).tobytes() == _np(ce19).tobytes()           # the stride is addressing only


def test_a_pixel_stride_too_wide_to_stage():
    """ld = 40: 64 pixels of 40 floats do not fit a wave's stage and every lane reads its pixel from memory; the 32-pixel span at the end of the 96-pixel
    window rows is staged.  Both paths in one launch, plain and mirrored."""
    H = _helpers()
    f = WR.FIXTURES[4]
    views, _, _ = WR.fixture(f)
    td = H.dev(PFR.make_target(90, (f[1], f[2], f[3])))
    pred, ce = _merge(f, _dev_views(views, ld=40), target=td)
    pred19, ce19 = _merge(f, _dev_views(views), target=td)
    assert torch.equal(pred, pred19) and _np(ce).tobytes() == _np(ce19).tobytes()


def test_run_to_run_bit_identical():
    H = _helpers()
    f = WR.FIXTURES[4]
    views, _, _ = WR.fixture(f)
    dv = _dev_views(views)
    td = H.dev(PFR.make_target(43, (f[1], f[2], f[3])))
    runs = []
    for _ in range(2):
        counts, cm, rec = _counts(), _cm(), torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
        pred, ce, conf = _merge(f, dv, target=td, counts=counts, confusion=cm, calibration=rec, confidence=True)
        runs.append((_np(pred), _np(counts), _np(ce).tobytes(), _np(cm), _np(rec), _np(conf).tobytes()))
    for a, b in zip(*runs):
        assert a == b if isinstance(a, bytes) else np.array_equal(a, b)


def test_a_single_whole_image_window_is_one_identity_view_of_the_multiscale_merge():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    L = np.random.RandomState(95).standard_normal((3, NC, 16, 70)).astype(np.float32)
    target = PFR.make_target(96, (3, 16, 70))
    td, t = H.dev(target), H.dev(L)
    for kw in ({}, {'target': td}):
        c1, c2 = (_counts(), _counts()) if kw else (None, None)
        rec1, rec2 = (torch.zeros(3 * B, dtype=torch.int64, device=H.DEV) for _ in range(2))
        more1 = dict(kw, counts=c1, calibration=rec1) if kw else {}
        more2 = dict(kw, counts=c2, calibration=rec2) if kw else {}
        a = HF.window_merge([t], (0,), (0,), (16, 70), confidence=True, **more1)
        b = HF.multiscale_merge([(t, False)], (16, 70), confidence=True, **more2)
        assert torch.equal(a[0], b[0]) and _np(a[2]).tobytes() == _np(b[2]).tobytes()
        if kw:
            assert _np(a[1]).tobytes() == _np(b[1]).tobytes() and torch.equal(c1, c2) and torch.equal(rec1, rec2)
    assert np.array_equal(_np(a[0]), L.argmax(1))


# ---------------------------------------------------------------------------------------------- NaN, bad labels, extreme logits
def test_nan_in_any_view_and_labels_outside_the_classes():
    H = _helpers()
    f = WR.FIXTURES[0]
    views, _, _ = WR.fixture(f)
    n, ho, wo = f[1:4]
    target = PFR.make_target(97, (n, ho, wo))
    td = H.dev(target)
    flag = _flag()
    _merge(f, _dev_views(views), target=td, nan_flag=flag)
    assert int(flag.item()) == 0
    for which in (0, 1, len(views) - 1):                    # the first, a middle and the last view
        bad = [L.copy() for L in views]
        bad[which][1, 4, 3, 5] = np.nan
        for kw in ({}, {'target': td}):
            flag.zero_()
            _merge(f, _dev_views(bad), nan_flag=flag, **kw)
            assert int(flag.item()) == 1, (which, bool(kw))
    # a label 19 that is not the ignore label: bit 1, out of the counters, and the loss is NaN
    tb = target.copy()
    tb[1, 7, 9] = NC
    counts, cm = _counts(), _cm()
    flag.zero_()
    pb, ceb = _merge(f, _dev_views(views), target=H.dev(tb), counts=counts, confusion=cm, nan_flag=flag)
    assert int(flag.item()) == 2 and np.isnan(float(ceb))
    assert np.array_equal(_np(counts), PF.counts_table(_np(pb), tb))
    assert np.array_equal(_np(cm), _numpy_cm(_np(pb), tb))


def test_loss_at_a_logit_gap_of_60_in_every_covering_view():
    """Grid pixel (5, 9) of fixture 181 lies in all four windows.  In each the target class's logit is put 60 below the maximum: P[t] ~ e^-60 = 9e-27,
    far inside fp32's range.  One-pixel target, everything else ignored; the tolerance is the loss tolerance on that pixel's term."""
    H = _helpers()
    f = WR.FIXTURES[0]
    views, _, cnt = WR.fixture(f)
    ys, xs = f[5], f[6]
    gy, gx, t_class = 5, 9, 7
    assert cnt[gy, gx] == 4
    edge = []
    for k, L in enumerate(views):
        i, j = divmod(k, len(xs))
        L = L.copy()
        wy, wx = gy - ys[i], gx - xs[j]
        L[0, t_class, wy, wx] = np.delete(L[0, :, wy, wx], t_class).max() - 60.0
        edge.append(L)
    P, _ = WR.merge(edge, ys, xs, (f[2], f[3]))
    target = np.full((f[1], f[2], f[3]), gen.IGNORE, np.uint8)
    target[0, gy, gx] = t_class
    ref = WR.ce(P, target)
    assert 58.0 < ref < 64.0
    flag = _flag()
    _, ce = _merge(f, _dev_views(edge), target=H.dev(target), nan_flag=flag)
    print(f'gap 60: ref {ref:.9f}, kernel {float(ce):.9f}, error {abs(float(ce) - ref):.3e}, tolerance {WR.CE_TOL * abs(ref):.3e}')
    assert int(flag.item()) == 0 and np.isfinite(float(ce))
    assert abs(float(ce) - ref) <= WR.CE_TOL * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------------- other class counts, memory, argument checks
def test_class_counts_the_kernel_refuses_are_composed_from_torch_ops():
    """40 classes: dsrl_window_merge_supported says 0 and the same definition is evaluated by torch ops"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    nc = 40
    assert _lib.query('dsrl_window_merge_supported', 2, 5, 4, 9, 7, nc) == 0
    rs = np.random.RandomState(98)
    ys, xs = (0, 2, 4), (0, 3)
    views = [rs.standard_normal((2, nc, 5, 4)).astype(np.float32) for _ in range(12)]
    P, _ = WR.merge(views, ys, xs, (9, 7), flip=True)
    target = PFR.make_target(99, (2, 9, 7), nc=nc)
    counts, cm, flag = _counts(nc=nc), _cm(nc=nc), _flag()
    rec = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
    pred, ce, conf = HF.window_merge(_dev_views(views), ys, xs, (9, 7), target=H.dev(target), counts=counts, confusion=cm, nan_flag=flag, calibration=rec,
                                     confidence=True, flip=True)
    pred_h = _np(pred)
    WR.check_class_map(pred_h, P, '40-class composition')
    assert int(flag.item()) == 0
    assert np.array_equal(_np(counts), PF.counts_table(pred_h, target, nc))
    assert np.array_equal(_np(cm), _numpy_cm(pred_h, target, nc))
    assert np.array_equal(_np(rec), R.record_of(_np(conf), pred_h, target, B, nc, gen.IGNORE))
    ref = WR.ce(P, target, num_classes=nc)
    assert abs(float(ce) - ref) <= WR.CE_TOL * max(1.0, abs(ref))


def test_allocates_the_accumulator_the_class_map_and_the_workspace():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib
    f = WR.FIXTURES[4]
    views, _, _ = WR.fixture(f)
    n, ho, wo = f[1:4]
    dv = _dev_views(views)
    td = H.dev(PFR.make_target(33, (n, ho, wo)))
    counts = _counts()
    _merge(f, dv, target=td, counts=counts)                                     # library load, allocator warm-up
    torch.cuda.synchronize()
    up = lambda b: (b + 511) // 512 * 512                                       # noqa: E731  (the caching allocator's granule)
    acc, pred = _lib.query('dsrl_prob_merge_acc_bytes', n, ho, wo, NC), n * ho * wo
    ws, ce = max(_lib.query('dsrl_window_merge_workspace_bytes', n, ho, wo), 256), 8
    for kw, bound in (({}, up(acc) + up(pred)), ({'target': td, 'counts': counts}, up(acc) + up(pred) + up(ws) + up(ce))):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = _merge(f, dv, **kw)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        assert rise <= bound + 512, (rise, bound)               # a canvas of counts or a second accumulator would be another `acc` bytes
        del out


def test_argument_checks():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    a = H.dev(np.zeros((2, NC, 8, 8), np.float32))
    target = H.dev(np.zeros((2, 12, 12), np.uint8))
    with pytest.raises(HF.DsrlHipError, match='target'):
        HF.window_merge([a] * 4, (0, 4), (0, 4), (12, 12), target=target[:, :4])
    with pytest.raises(HF.DsrlHipError, match='need a target'):
        HF.window_merge([a] * 4, (0, 4), (0, 4), (12, 12), counts=_counts())
    with pytest.raises(HF.DsrlHipError, match='counts'):
        HF.window_merge([a] * 4, (0, 4), (0, 4), (12, 12), target=target, counts=_counts()[:-1])
    with pytest.raises(HF.DsrlHipError, match='views'):
        HF.window_merge([a] * 3, (0, 4), (0, 4), (12, 12))
    with pytest.raises(HF.DsrlHipError, match='view 1'):
        HF.window_merge([a, a[:1], a, a], (0, 4), (0, 4), (12, 12))
    with pytest.raises(ValueError, match='ys'):
        HF.window_merge([a] * 4, (0, 3), (0, 4), (12, 12))
    pred, _ = HF.window_merge([a] * 8, (0, 4), (0, 4), (12, 12), flip=True)          # and nothing is left half done
    assert tuple(pred.shape) == (2, 12, 12) and int(pred.max()) == 0                  # all-equal probabilities: the lowest index


# ---------------------------------------------------------------------------------------------- the model, the compiled path and the commands
WINDOW, STRIDE = (32, 48), (21, 32)


def _make_model(stage):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    torch.manual_seed(1234)
    return DSRL(stage, CS).to(H.DEV).to(memory_format=torch.channels_last).eval()


@pytest.fixture(scope='module')
def model():
    return _make_model(1)


def _image_batch(seed, n, hw=(64, 96)):
    H = _helpers()
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, 3) + tuple(hw), generator=g).to(H.DEV).contiguous(memory_format=torch.channels_last)


def _host(out, cm=None):
    pred, counts, ce = out[:3]
    return (_np(pred).copy(), None if counts is None else _np(counts).copy(), None if ce is None else _np(ce).tobytes(),
            None if cm is None else _np(cm).copy()) + tuple(_np(v).tobytes() for v in out[3:])


def _same(a, b):
    return len(a) == len(b) and all((x is None) == (y is None) and (x is None or (x == y if isinstance(x, bytes) else np.array_equal(x, y)))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_predict_is_the_merge_of_the_forward_paths_logits(model, flip):
    """predict(window=...) against functional.window_merge on logits the test takes from model(crop)[0] itself: the same deterministic launches on both
    sides, so the plumbing (plan, crops, batch of the two views, view order, offsets on the output grid, release of the logits) is compared byte
    for byte."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    x = _image_batch(1, 2)
    target = torch.from_numpy(PFR.make_target(2, (2, 128, 192))).to(x.device)
    ys, xs = HF.window_plan(64, 96, WINDOW, STRIDE)
    assert (ys, xs) == ((0, 21, 32), (0, 32, 48))
    cm, rec = _cm(), torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
    got = _host(model.predict(x, target, window=WINDOW, stride=STRIDE, flip=flip, confusion=cm, calibration=rec, confidence=True), cm)
    views = []
    with torch.no_grad():
        for y0 in ys:
            for x0 in xs:
                crop = x[:, :, y0:y0 + 32, x0:x0 + 48].contiguous(memory_format=torch.channels_last)
                if flip:
                    L = model(torch.cat([crop, crop.flip(3)]).contiguous(memory_format=torch.channels_last))[0]
                    views += [L[:2], L[2:]]
                else:
                    views.append(model(crop)[0])
    counts, cm2, rec2 = _counts(), _cm(), torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
    pred, ce, conf = HF.window_merge(views, tuple(2 * y for y in ys), tuple(2 * v for v in xs), (128, 192), target=target, counts=counts, confusion=cm2,
                                     calibration=rec2, confidence=True, flip=flip)
    assert _same(got, _host((pred, counts, ce, conf), cm2)) and torch.equal(rec, rec2)
    assert got[0].shape == (2, 128, 192) and np.array_equal(got[1], PF.counts_table(got[0], _np(target)))
    # without a target: the same class map, nothing else
    pred3, counts3, ce3 = model.predict(x, window=WINDOW, stride=STRIDE, flip=flip)
    assert counts3 is None and ce3 is None and np.array_equal(_np(pred3), got[0])
    # the ensemble of windows is not the whole-image view
    assert not np.array_equal(_np(model.predict(x, flip=flip)[0]), got[0])


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_window_off_is_todays_predict(model, flip):
    x = _image_batch(3, 2)
    target = torch.from_numpy(PFR.make_target(4, (2, 128, 192))).to(x.device)
    want = _host(model.predict(x, target, flip=flip))
    for off in ({'window': None}, {'window': (64, 96)}, {'window': (64, 96), 'stride': (16, 16)}, {'window': None, 'stride': None}):
        assert _same(_host(model.predict(x, target, flip=flip, **off)), want), off


def test_predict_refuses_what_it_cannot_run(model):
    from dualsuperreslearningforsemseg_amd import functional as HF
    x = _image_batch(5, 1)
    with pytest.raises(ValueError, match='scales'):
        model.predict(x, window=WINDOW, scales=(0.5, 1.0))
    with pytest.raises(ValueError, match='temperature'):
        model.predict(x, window=WINDOW, temperature=1.5)
    with pytest.raises(ValueError, match='larger than the image'):
        model.predict(x, window=(80, 96))
    with pytest.raises(ValueError, match='uncovered'):
        model.predict(x, window=WINDOW, stride=(33, 48))
    with pytest.raises(ValueError, match='multiple of 16'):
        model.predict(x, window=(24, 48))
    xn = x.clone()
    xn[0, 2, 10, 20] = float('nan')
    with pytest.raises(HF.DsrlHipError, match='NaN'):
        model.predict(xn, window=WINDOW)
    flag = _flag()
    model.predict(xn, window=WINDOW, nan_flag=flag)             # a caller's flag is not read back here
    assert int(flag.item()) & 1


def test_compiled_predictor_refuses_a_window_and_stays_usable(model):
    x = _image_batch(8, 2)
    want = _host(model.predict(x))
    cp = model.compile_predict()
    try:
        with pytest.raises(ValueError, match='window'):
            cp(x, window=WINDOW)
        assert _same(_host(cp(x)), want) and _same(_host(cp(x, window=None, stride=None)), want)
    finally:
        cp.release()


def test_benchmark_and_test_commands_with_a_window(model, tmp_path):
    H = _helpers()
    from PIL import Image
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix
    weights = str(tmp_path / 'final.weights')
    torch.save({'model_state_dict': model.state_dict()}, weights)
    batches = [((_image_batch(10 + i, n), None), (torch.from_numpy(PFR.make_target(20 + i, (n, 128, 192))).to(H.DEV), None)) for i, n in enumerate((2, 1))]
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda *a: batches}
    out_dir = str(tmp_path / 'out')
    result = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 96), output_dir=out_dir, window=WINDOW, stride=STRIDE, flip=True)
    cm = _cm()
    ces = []
    for (img, _), (target, _) in batches:
        ces.append(float(model.predict(img, target, ignore_index=CS.IGNORE_CLASS_LABEL, window=WINDOW, stride=STRIDE, flip=True, confusion=cm)[2]))
    whole = ConfusionMatrix(NC, CS.IGNORE_CLASS_LABEL)
    whole.merge(cm.cpu())
    assert result['mIoU_dataset'] == whole.result()['mIoU']
    assert np.array_equal(np.array(result['confusion_matrix']), _np(cm).reshape(NC, NC))
    assert abs(result['CE'] - float(np.mean(ces))) < 1e-6           # both batches weigh the nominal batch size
    text = open(os.path.join(out_dir, 'benchmark.txt')).read()
    assert ('Sliding-window ensemble: windows of 32 x 48 at stride 21 x 32 over the 64 x 96 input -> 3 x 3 positions, class probabilities averaged where '
            'they overlap\n') in text and 'Horizontal-flip' in text
    plain = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 96), output_dir=out_dir)
    assert 'Sliding-window' not in open(os.path.join(out_dir, 'benchmark.txt')).read() and plain['confusion_matrix'] != result['confusion_matrix']
    # the test command writes its PNG
    img_dir = tmp_path / 'images'
    img_dir.mkdir()
    Image.fromarray(np.random.RandomState(5).randint(0, 256, (90, 160, 3)).astype(np.uint8), mode='RGB').save(str(img_dir / 'a.png'))
    vis_dir = str(tmp_path / 'vis')
    files = test_command(None, str(img_dir), None, vis_dir, weights, 'gpu', False, model_input_size=(64, 96), window=WINDOW, stride=STRIDE)
    assert files == [os.path.join(vis_dir, 'a.png')]
    palette = {tuple(v) for v in CS.CLASS_RGB_COLOR.values()}
    with Image.open(files[0]) as im:
        assert im.size == (3 * 192, 128) and im.mode == 'RGB'
        middle = np.array(im)[:, 192:384].reshape(-1, 3)
    assert {tuple(c) for c in np.unique(middle, axis=0).tolist()} <= palette

"""GPU checks of multi-scale inference: the resample-and-merge kernels (dsrl_prob_merge, dsrl_prob_merge_finish) behind functional.multiscale_merge,
DSRL.predict(scales=...), the refusal of CompiledPredictor and the benchmark / test commands with scales.  The reference is the fp64 restatement in
multiscale_ref; bands and tolerances are derived there."""
import os

import numpy as np
import pytest
import torch

import gen
import multiscale_ref as MR
import predict_fixtures as PF
import predict_flip_ref as PFR

pytestmark = pytest.mark.gpu

NC = gen.NUM_CLASSES


def _helpers():
    import hip_helpers as H
    return H


def _counts(fill=0):
    return torch.full((3 * NC + 2,), fill, dtype=torch.int64, device=_helpers().DEV)


def _cm(fill=0):
    return torch.full((NC * NC,), fill, dtype=torch.int64, device=_helpers().DEV)


def _flag():
    return torch.zeros((), dtype=torch.int32, device=_helpers().DEV)


def _dev_views(views, ld=None):
    """[(L numpy, mirrored)] -> [(pixel-major device tensor, mirrored)]; `ld`: the logits sit in the first 19 channels of an ld-channel tensor"""
    H = _helpers()
    out = []
    for L, m in views:
        t = H.dev(np.asarray(L, np.float32))
        if ld is not None:
            wide = torch.full((t.shape[0], ld) + tuple(t.shape[2:]), 7.0, device=H.DEV).contiguous(memory_format=torch.channels_last)
            wide[:, :t.shape[1]] = t
            t = wide[:, :t.shape[1]]
            assert t.stride(1) == 1 and t.stride(3) == ld
        out.append((t, m))
    return out


def _numpy_cm(pred, target, nc=NC, ignore=gen.IGNORE):
    valid = (target != ignore) & (target < nc)
    return np.bincount(target[valid].astype(np.int64) * nc + pred[valid].astype(np.int64), minlength=nc * nc)


# ---------------------------------------------------------------------------------------------- class maps
@pytest.mark.parametrize('order', ['given', 'reversed'])
@pytest.mark.parametrize('fixture', MR.FIXTURES, ids=MR.fixture_id)
def test_class_maps_against_the_fp64_ensemble(fixture, order):
    """Every fixture with its views in the given order and reversed: another view is the `finish` view and another one the `first`; outside the band the
    class map is the fp64 arg-max either way."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    views, P = MR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    dv = _dev_views(views)
    pred, ce = HF.multiscale_merge(dv if order == 'given' else dv[::-1], (ho, wo))
    assert ce is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (n, ho, wo)
    share = MR.check_class_map(pred.cpu().numpy(), P, f'merge kernels ({order} order) vs fp64 ensemble')
    print(f'{MR.fixture_id(fixture)} {order}: band {100 * share:.3f} %')


def test_class_map_from_views_too_wide_to_stage():
    """Views 200 and 150 columns wide on a 70-column grid: the 64-pixel span of a row reads 183 / 138 source columns, more than a wave stages in LDS
    (121 of 19 floats), and takes its four pixels from memory; the 6-pixel span at the row's end and the identity view are staged.  Both paths in one
    launch, plain and mirrored; the loss against the same reference."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = (87, 1, 4, 70, ((3, 200), (4, 70), (6, 150)), True)
    views, P = MR.fixture(f)
    target = PFR.make_target(88, (1, 4, 70))
    for order in (1, -1):
        pred, ce = HF.multiscale_merge(_dev_views(views)[::order], (4, 70), target=_helpers().dev(target))
        MR.check_class_map(pred.cpu().numpy(), P, 'wide views')
        ref = MR.ce(P, target)
        assert abs(float(ce) - ref) <= MR.CE_TOL * max(1.0, abs(ref)), (float(ce), ref)


def test_class_map_from_logits_with_a_wider_pixel_stride():
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = MR.FIXTURES[3]
    views, P = MR.fixture(f)
    target = PFR.make_target(90, (f[1], f[2], f[3]))
    td = _helpers().dev(target)
    pred, ce = HF.multiscale_merge(_dev_views(views, ld=24), (f[2], f[3]), target=td)
    MR.check_class_map(pred.cpu().numpy(), P, 'ld = 24')
    pred19, ce19 = HF.multiscale_merge(_dev_views(views), (f[2], f[3]), target=td)
    assert torch.equal(pred, pred19) and ce.cpu().numpy().tobytes() == ce19.cpu().numpy().tobytes()      # the stride is addressing only


# ---------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize('fixture', MR.FIXTURES, ids=MR.fixture_id)
def test_loss_and_its_pixel_count(fixture):
    """The C ABI itself: dsrl_prob_merge for all but the last view, dsrl_prob_merge_finish for the last; ce_out = [mean, counted pixels]."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    views, P = MR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    target = PFR.make_target(91 + fixture[0], (n, ho, wo))
    ref = MR.ce(P, target)
    dv, td = _dev_views(views), H.dev(target)
    acc = torch.empty(_lib.query('dsrl_prob_merge_acc_bytes', n, ho, wo, NC) // 4, device=H.DEV, dtype=torch.float32)
    ws = torch.empty(_lib.query('dsrl_prob_merge_workspace_bytes', n, ho, wo), device=H.DEV, dtype=torch.uint8)
    pred = torch.empty((n, ho, wo), device=H.DEV, dtype=torch.uint8)
    out = torch.zeros(2, device=H.DEV, dtype=torch.float32)
    st = HF._stream()
    for i, (t, m) in enumerate(dv[:-1]):
        assert HF._ld_of(t) == NC
        _lib.call('dsrl_prob_merge', t.data_ptr(), NC, n, t.shape[2], t.shape[3], NC, int(m), acc.data_ptr(), ho, wo, int(i == 0), st)
    t, m = dv[-1]
    _lib.call('dsrl_prob_merge_finish', t.data_ptr(), NC, n, t.shape[2], t.shape[3], NC, int(m), acc.data_ptr(), ho, wo, len(dv), pred.data_ptr(), td.data_ptr(),
              gen.IGNORE, None, out.data_ptr(), None, ws.data_ptr(), ws.numel(), None, st)
    ce, cnt = (float(v) for v in out.cpu())
    print(f'{MR.fixture_id(fixture)}: ref {ref:.9f}, kernel {ce:.9f}, error {abs(ce - ref):.3e}, tolerance {MR.CE_TOL * max(1.0, abs(ref)):.3e}')
    assert cnt == float((target != gen.IGNORE).sum())
    assert abs(ce - ref) <= MR.CE_TOL * max(1.0, abs(ref))
    # functional.multiscale_merge is these launches
    pred2, ce2 = HF.multiscale_merge(dv, (ho, wo), target=td)
    assert torch.equal(pred, pred2) and ce2.cpu().numpy().tobytes() == out[:1].cpu().numpy().tobytes()
    # every pixel ignored: NaN, as torch
    _, cen = HF.multiscale_merge(dv, (ho, wo), target=H.dev(np.full((n, ho, wo), gen.IGNORE, np.uint8)))
    assert np.isnan(float(cen))


def test_loss_at_a_logit_gap_of_60():
    """Output pixel (0, 0) reads exactly source pixel (0, 0) of every plain view and (0, w - 1) of every mirrored one (frac = 0).  There the target
    class's logit is put 60 below the maximum in every view: P[t] ~ e^-60 = 9e-27, far inside fp32's range.  One-pixel target, everything else ignored;
    the tolerance is the loss tolerance on that pixel's term."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = MR.FIXTURES[1]
    views, _ = MR.fixture(f)
    t_class = 7
    edge = []
    for L, m in views:
        L = L.copy()
        col = L.shape[3] - 1 if m else 0
        others = np.delete(L[0, :, 0, col], t_class)
        L[0, t_class, 0, col] = others.max() - 60.0
        edge.append((L, m))
    P = MR.merge(edge, (f[2], f[3]))
    target = np.full((f[1], f[2], f[3]), gen.IGNORE, np.uint8)
    target[0, 0, 0] = t_class
    ref = MR.ce(P, target)
    assert 58.0 < ref < 64.0
    flag = _flag()
    _, ce = HF.multiscale_merge(_dev_views(edge), (f[2], f[3]), target=H.dev(target), nan_flag=flag)
    print(f'gap 60: ref {ref:.9f}, kernel {float(ce):.9f}, error {abs(float(ce) - ref):.3e}, tolerance {MR.CE_TOL * abs(ref):.3e}')
    assert int(flag.item()) == 0 and np.isfinite(float(ce))
    assert abs(float(ce) - ref) <= MR.CE_TOL * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------------- counters and confusion matrix
@pytest.mark.parametrize('fixture', [MR.FIXTURES[0], MR.FIXTURES[3], MR.FIXTURES[4]], ids=MR.fixture_id)
def test_counts_and_confusion_of_the_kernels_own_class_map(fixture):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    views, _ = MR.fixture(fixture)
    n, ho, wo = fixture[1:4]
    dv = _dev_views(views)
    target = PFR.make_target(13, (n, ho, wo))
    td = H.dev(target)
    counts, cm, flag = _counts(5), _cm(3), _flag()                     # both are ADDED into what the buffers hold
    pred, ce = HF.multiscale_merge(dv, (ho, wo), target=td, counts=counts, confusion=cm, nan_flag=flag)
    pred_h = pred.cpu().numpy()
    assert np.array_equal(counts.cpu().numpy(), 5 + PF.counts_table(pred_h, target))
    assert np.array_equal(cm.cpu().numpy(), 3 + _numpy_cm(pred_h, target))
    assert int(flag.item()) == 0 and np.isfinite(float(ce))
    # counts without the matrix: the same bits; the class map is the same with and without a target
    only = _counts(5)
    pred2, ce2 = HF.multiscale_merge(dv, (ho, wo), target=td, counts=only)
    assert torch.equal(only, counts) and torch.equal(pred2, pred) and ce2.cpu().numpy().tobytes() == ce.cpu().numpy().tobytes()
    assert torch.equal(HF.multiscale_merge(dv, (ho, wo))[0], pred)
    # ignore_index = 0
    c0, m0 = _counts(), _cm()
    p0, _ = HF.multiscale_merge(dv, (ho, wo), target=td, ignore_index=0, counts=c0, confusion=m0)
    assert np.array_equal(c0.cpu().numpy(), PF.counts_table(p0.cpu().numpy(), target, NC, 0))
    assert np.array_equal(m0.cpu().numpy(), _numpy_cm(p0.cpu().numpy(), target, NC, 0))


# ---------------------------------------------------------------------------------------------- a single view
def test_a_single_identity_view_is_the_argmax_and_the_cross_entropy_of_its_logits():
    """first and last are the same launch and there is no accumulator: frac = 0 everywhere, so the kernel sees the logits themselves"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    L = np.random.RandomState(95).standard_normal((3, NC, 16, 33)).astype(np.float32)
    top = np.sort(L, axis=1)[:, -2:]
    assert (top[:, 1] > top[:, 0]).all()                                # no ties among the random normals
    target = PFR.make_target(96, (3, 16, 33))
    for mirrored in (False, True):
        view = L[:, :, :, ::-1] if mirrored else L
        pred, ce = HF.multiscale_merge(_dev_views([(view, mirrored)]), (16, 33), target=H.dev(target))
        assert np.array_equal(pred.cpu().numpy(), L.argmax(1))
        ref = MR.ce(MR.softmax(L.astype(np.float64)), target)
        assert abs(float(ce) - ref) <= MR.CE_TOL * max(1.0, abs(ref)), (float(ce), ref)


# ---------------------------------------------------------------------------------------------- NaN and bad labels
def test_nan_in_any_view_and_labels_outside_the_classes():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = MR.FIXTURES[0]
    views, _ = MR.fixture(f)
    n, ho, wo = f[1:4]
    target = PFR.make_target(97, (n, ho, wo))
    td = H.dev(target)
    flag = _flag()
    HF.multiscale_merge(_dev_views(views), (ho, wo), target=td, nan_flag=flag)
    assert int(flag.item()) == 0
    for which in range(len(views)):                     # the first, a middle and the last view
        bad = [(L.copy(), m) for L, m in views]
        bad[which][0][1, 4, 3, 5] = np.nan
        for kw in ({}, {'target': td}):
            flag.zero_()
            HF.multiscale_merge(_dev_views(bad), (ho, wo), nan_flag=flag, **kw)
            assert int(flag.item()) == 1, (which, bool(kw))
    # a label 19 that is not the ignore label: bit 1, out of the counters, and the loss is NaN
    tb = target.copy()
    tb[1, 7, 9] = NC
    counts, cm = _counts(), _cm()
    flag.zero_()
    pb, ceb = HF.multiscale_merge(_dev_views(views), (ho, wo), target=H.dev(tb), counts=counts, confusion=cm, nan_flag=flag)
    assert int(flag.item()) == 2 and np.isnan(float(ceb))
    assert np.array_equal(counts.cpu().numpy(), PF.counts_table(pb.cpu().numpy(), tb))
    assert np.array_equal(cm.cpu().numpy(), _numpy_cm(pb.cpu().numpy(), tb))


# ---------------------------------------------------------------------------------------------- determinism, memory, validation, other class counts
def test_run_to_run_bit_identical():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = MR.FIXTURES[4]
    views, _ = MR.fixture(f)
    dv = _dev_views(views)
    td = H.dev(PFR.make_target(43, (f[1], f[2], f[3])))
    runs = []
    for _ in range(2):
        counts, cm = _counts(), _cm()
        pred, ce = HF.multiscale_merge(dv, (f[2], f[3]), target=td, counts=counts, confusion=cm)
        runs.append((pred.cpu().numpy(), counts.cpu().numpy(), ce.cpu().numpy().tobytes(), cm.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert np.array_equal(runs[0][3], runs[1][3])


def test_allocates_the_accumulator_the_class_map_and_the_workspace():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    f = MR.FIXTURES[4]
    views, _ = MR.fixture(f)
    n, ho, wo = f[1:4]
    dv = _dev_views(views)
    td = H.dev(PFR.make_target(33, (n, ho, wo)))
    counts = _counts()
    HF.multiscale_merge(dv, (ho, wo), target=td, counts=counts)                 # library load, allocator warm-up
    torch.cuda.synchronize()
    up = lambda b: (b + 511) // 512 * 512                                       # noqa: E731  (the caching allocator's granule)
    acc, pred = _lib.query('dsrl_prob_merge_acc_bytes', n, ho, wo, NC), n * ho * wo
    ws, ce = max(_lib.query('dsrl_prob_merge_workspace_bytes', n, ho, wo), 256), 8
    assert acc == n * NC * ho * wo * 4
    for kw, bound in (({}, up(acc) + up(pred)), ({'target': td, 'counts': counts}, up(acc) + up(pred) + up(ws) + up(ce))):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = HF.multiscale_merge(dv, (ho, wo), **kw)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        assert rise <= bound + 512, (rise, bound)               # one more view's probabilities would be another `acc` bytes
        del out


def test_argument_checks():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    a, b = H.dev(np.zeros((2, NC, 4, 4), np.float32)), H.dev(np.zeros((2, NC, 6, 6), np.float32))
    target = H.dev(np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(HF.DsrlHipError, match='target'):
        HF.multiscale_merge([(a, False), (b, False)], (8, 8), target=target[:, :4])
    with pytest.raises(HF.DsrlHipError, match='need a target'):
        HF.multiscale_merge([(a, False)], (8, 8), counts=_counts())
    with pytest.raises(HF.DsrlHipError, match='counts'):
        HF.multiscale_merge([(a, False)], (8, 8), target=target, counts=_counts()[:-1])
    with pytest.raises(HF.DsrlHipError, match='confusion'):
        HF.multiscale_merge([(a, False)], (8, 8), target=target, confusion=_cm()[:-1])
    with pytest.raises(HF.DsrlHipError, match='view 1'):
        HF.multiscale_merge([(a, False), (b[:1], False)], (8, 8))
    pred, _ = HF.multiscale_merge([(a, False), (b, True)], (8, 8))          # and nothing is left half done
    assert tuple(pred.shape) == (2, 8, 8) and int(pred.max()) == 0           # all-equal probabilities: the lowest index


def test_class_counts_the_kernel_refuses_are_composed_from_torch_ops():
    """40 classes: dsrl_prob_merge_supported says 0 and the same definition is evaluated by torch ops"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    nc = 40
    assert _lib.query('dsrl_prob_merge_supported', 2, 5, 7, 10, 12, nc) == 0
    rs = np.random.RandomState(98)
    views = [(rs.standard_normal((2, nc, 5, 7)).astype(np.float32), False), (rs.standard_normal((2, nc, 10, 12)).astype(np.float32), True),
             (rs.standard_normal((2, nc, 13, 9)).astype(np.float32), False)]
    P = MR.merge(views, (10, 12))
    target = PFR.make_target(99, (2, 10, 12), nc=nc)
    counts, cm, flag = torch.zeros(3 * nc + 2, dtype=torch.int64, device=H.DEV), torch.zeros(nc * nc, dtype=torch.int64, device=H.DEV), _flag()
    pred, ce = HF.multiscale_merge(_dev_views(views), (10, 12), target=H.dev(target), counts=counts, confusion=cm, nan_flag=flag)
    pred_h = pred.cpu().numpy()
    MR.check_class_map(pred_h, P, '40-class composition')
    assert int(flag.item()) == 0
    assert np.array_equal(counts.cpu().numpy(), PF.counts_table(pred_h, target, nc))
    assert np.array_equal(cm.cpu().numpy(), _numpy_cm(pred_h, target, nc))
    ref = MR.ce(P, target, num_classes=nc)
    assert abs(float(ce) - ref) <= MR.CE_TOL * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------------- the model, the compiled path and the commands
SCALES = (0.5, 1.0, 1.5)


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
    pred, counts, ce = out
    return (pred.cpu().numpy().copy(), None if counts is None else counts.cpu().numpy().copy(), None if ce is None else ce.cpu().numpy().tobytes(),
            None if cm is None else cm.cpu().numpy().copy())


def _same(a, b):
    return all((x is None) == (y is None) and (x is None or (x == y if isinstance(x, bytes) else np.array_equal(x, y))) for x, y in zip(a, b))


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_predict_is_the_merge_of_the_forward_paths_logits(model, flip):
    """predict(scales=...) against functional.multiscale_merge on logits the test takes from model.forward itself: the same deterministic launches on
    both sides, so the plumbing (sizes, resize, batch of the two views, view order, release of the logits) is compared byte for byte."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    x = _image_batch(1, 2)
    target = torch.from_numpy(PFR.make_target(2, (2, 128, 192))).to(x.device)
    sizes = HF.multiscale_sizes(64, 96, SCALES)
    assert sizes == [(32, 48), (64, 96), (96, 144)]
    cm = _cm()
    got = _host(model.predict(x, target, scales=SCALES, flip=flip, confusion=cm), cm)
    views = []
    with torch.no_grad():
        for size in sizes:
            xk = HF.resize_image_ac(x, size)
            assert tuple(xk.shape) == (2, 3) + size and (size != (64, 96) or xk is x)
            if flip:
                L = model(torch.cat([xk, xk.flip(3)]).contiguous(memory_format=torch.channels_last))[0]
                views += [(L[:2], False), (L[2:], True)]
            else:
                views.append((model(xk)[0], False))
    counts, cm2 = _counts(), _cm()
    pred, ce = HF.multiscale_merge(views, (128, 192), target=target, counts=counts, confusion=cm2)
    assert _same(got, _host((pred, counts, ce), cm2))
    assert got[0].shape == (2, 128, 192) and np.array_equal(got[1], PF.counts_table(got[0], target.cpu().numpy()))
    # without a target: the same class map, nothing else
    pred3, counts3, ce3 = model.predict(x, scales=SCALES, flip=flip)
    assert counts3 is None and ce3 is None and np.array_equal(pred3.cpu().numpy(), got[0])
    # the ensemble is not the single view
    assert not np.array_equal(model.predict(x, flip=flip)[0].cpu().numpy(), got[0])


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_scales_off_is_todays_predict(model, flip):
    x = _image_batch(3, 2)
    target = torch.from_numpy(PFR.make_target(4, (2, 128, 192))).to(x.device)
    want = _host(model.predict(x, target, flip=flip))
    for off in (None, (), (1.0,)):
        assert _same(_host(model.predict(x, target, flip=flip, scales=off)), want), off


def test_predict_refuses_what_it_cannot_run(model):
    from dualsuperreslearningforsemseg_amd import functional as HF
    x = _image_batch(5, 1)
    with pytest.raises(ValueError, match='same'):
        model.predict(x, scales=(0.5, 0.55))
    with pytest.raises(ValueError, match='scales'):
        model.predict(x, scales=(0.5, float('nan')))
    xn = x.clone()
    xn[0, 2, 10, 20] = float('nan')
    with pytest.raises(HF.DsrlHipError, match='NaN'):
        model.predict(xn, scales=SCALES)
    flag = _flag()
    model.predict(xn, scales=SCALES, nan_flag=flag)             # a caller's flag is not read back here
    assert int(flag.item()) & 1


def test_a_stage_3_model_runs_without_its_sisr_branch(model):
    stage3 = _make_model(3)
    stage1 = _make_model(1)
    missing, unexpected = stage1.load_state_dict(stage3.state_dict(), strict=False)
    assert not missing and unexpected
    x = _image_batch(6, 1)
    target = torch.from_numpy(PFR.make_target(7, (1, 128, 192))).to(x.device)
    assert _same(_host(stage3.predict(x, target, scales=SCALES, flip=True)), _host(stage1.predict(x, target, scales=SCALES, flip=True)))


def test_compiled_predictor_refuses_scales_and_stays_usable(model):
    from dualsuperreslearningforsemseg_amd import functional as HF
    x = _image_batch(8, 2)
    want = _host(model.predict(x))
    cp = model.compile_predict()
    try:
        with pytest.raises(HF.DsrlHipError, match='eager'):
            cp(x, scales=SCALES)
        assert _same(_host(cp(x)), want) and _same(_host(cp(x, scales=(1.0,))), want)
    finally:
        cp.release()


def test_benchmark_and_test_commands_with_scales(model, tmp_path):
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
    result = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 96), output_dir=out_dir, scales=SCALES, flip=True)
    cm = _cm()
    ces = []
    for (img, _), (target, _) in batches:
        ces.append(float(model.predict(img, target, ignore_index=CS.IGNORE_CLASS_LABEL, scales=SCALES, flip=True, confusion=cm)[2]))
    whole = ConfusionMatrix(NC, CS.IGNORE_CLASS_LABEL)
    whole.merge(cm.cpu())
    assert result['mIoU_dataset'] == whole.result()['mIoU']
    assert np.array_equal(np.array(result['confusion_matrix']), cm.cpu().numpy().reshape(NC, NC))
    assert abs(result['CE'] - float(np.mean(ces))) < 1e-6           # both batches weigh the nominal batch size
    text = open(os.path.join(out_dir, 'benchmark.txt')).read()
    assert 'Multi-scale ensemble: scales 0.5, 1, 1.5 of the 64 x 96 input -> views of 32 x 48, 64 x 96, 96 x 144\n' in text and 'flip' in text
    plain = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 96), output_dir=out_dir)
    assert 'Multi-scale' not in open(os.path.join(out_dir, 'benchmark.txt')).read() and plain['confusion_matrix'] != result['confusion_matrix']
    # the test command writes its PNGs
    img_dir = tmp_path / 'images'
    img_dir.mkdir()
    Image.fromarray(np.random.RandomState(5).randint(0, 256, (90, 160, 3)).astype(np.uint8), mode='RGB').save(str(img_dir / 'a.png'))
    vis_dir = str(tmp_path / 'vis')
    files = test_command(None, str(img_dir), None, vis_dir, weights, 'gpu', False, model_input_size=(64, 96), scales=SCALES)
    assert files == [os.path.join(vis_dir, 'a.png')]
    palette = {tuple(v) for v in CS.CLASS_RGB_COLOR.values()}
    with Image.open(files[0]) as im:
        assert im.size == (3 * 192, 128) and im.mode == 'RGB'
        middle = np.array(im)[:, 192:384].reshape(-1, 3)
    assert {tuple(c) for c in np.unique(middle, axis=0).tolist()} <= palette

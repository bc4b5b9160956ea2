"""GPU checks of the device confusion matrix: the three producers (the fused tails dsrl_sssr_tail_predict_cm / _flip_cm, dsrl_seg_metrics_cm from
logits, dsrl_confusion_matrix from class maps) and everything that hands their matrix on: functional.sssr_tail_predict(confusion=), DSRL.predict,
CompiledPredictor, the benchmark command and validation inside training.  Every count is an exact integer compared with ==: the reference is
numpy's bincount of t * C + p over the class map the kernel itself returned."""
import os

import numpy as np
import pytest
import torch

import gen
import predict_fixtures as PF

pytestmark = pytest.mark.gpu

NC = gen.NUM_CLASSES
IGNORE = gen.IGNORE


def _helpers():
    import hip_helpers as H
    return H


def _tail_modules(seed, w2=None, bias2='random', NC=NC):
    """the recipe of test_predict_gpu._tail_modules: upsample16_pred[2], [3], [6] with random parameters on the device, in eval mode"""
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
    return [m.to(H.DEV).eval() for m in (c1, bn, c2)]


def _tail_input(seed, shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _target(seed, shape, share=0.1, nc=NC):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, nc, shape).astype(np.uint8)
    t[rs.uniform(size=shape) < share] = IGNORE
    return t


def _bincount_matrix(pred, target, C=NC, ignore=IGNORE):
    pred, target = np.asarray(pred), np.asarray(target)
    valid = (target != ignore) & (target < C) & (pred < C)
    t, p = target[valid].astype(np.int64), pred[valid].astype(np.int64)
    return np.bincount(t * C + p, minlength=C * C).reshape(C, C)


def _zeros(n, dtype=torch.int64):
    return torch.zeros(n, dtype=dtype, device=_helpers().DEV)


def _flag():
    return torch.zeros((), dtype=torch.int32, device=_helpers().DEV)


def _invariants(cm, counts, C=NC):
    """rows = area_target, columns = area_pred, diagonal = area_inter, total = valid, trace = correct"""
    cm, counts = np.asarray(cm).reshape(C, C), np.asarray(counts)
    assert np.array_equal(cm.sum(axis=1), counts[2 * C:3 * C]), 'row sums != area_target'
    assert np.array_equal(cm.sum(axis=0), counts[:C]), 'column sums != area_pred'
    assert np.array_equal(np.diag(cm), counts[C:2 * C]), 'diagonal != area_inter'
    assert cm.sum() == counts[3 * C + 1] and np.trace(cm) == counts[3 * C], 'total / trace != valid / correct'


def _figures(m):
    """numpy restatement of the dataset-level figures"""
    m = m.astype(np.float64)
    inter, tgt, prd = np.diag(m), m.sum(axis=1), m.sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = 100. * inter / (tgt + prd - inter)
    return iou, float(np.nanmean(iou))


# ---------------------------------------------------------------------------------------------- 1. the tail, single view
@pytest.mark.parametrize('shape', [(3, NC, 110, 100), (2, NC, 5, 7)], ids=['33000px_blocks_loop_partial_tile', '70px_one_partial_sweep'])
def test_tail_matrix_equals_bincount_of_its_own_class_map(shape):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods = _tail_modules(11)
    x = H.dev(_tail_input(12, shape))
    n, _, h, w = shape
    target = _target(13, (n, 4 * h, 4 * w))
    target[0, 3:9, 5:17] = 200                    # foreign labels: >= 19 and not the ignore label
    target[n - 1, 4 * h - 1, 4 * w - 3:] = 77
    td = H.dev(target)
    counts, cm, flag = _zeros(3 * NC + 2), _zeros(NC * NC), _flag()
    pred, ce = HF.sssr_tail_predict(x, *mods, target=td, counts=counts, nan_flag=flag, confusion=cm)
    pred_h = pred.cpu().numpy()
    assert np.array_equal(cm.cpu().numpy().reshape(NC, NC), _bincount_matrix(pred_h, target))
    assert np.array_equal(counts.cpu().numpy(), PF.counts_table(pred_h, target))
    _invariants(cm.cpu().numpy(), counts.cpu().numpy())
    assert int(flag.item()) == 2                  # the foreign labels, as without `confusion`
    # the same call without `confusion`: everything it returns is bit-identical
    counts0, flag0 = _zeros(3 * NC + 2), _flag()
    pred0, ce0 = HF.sssr_tail_predict(x, *mods, target=td, counts=counts0, nan_flag=flag0)
    assert torch.equal(pred, pred0) and torch.equal(counts, counts0) and int(flag0.item()) == 2
    assert ce.cpu().numpy().tobytes() == ce0.cpu().numpy().tobytes()
    # a finite loss too (no foreign labels)
    clean = np.where(target >= NC, IGNORE, target).astype(np.uint8)
    cm2, c2 = _zeros(NC * NC), _zeros(3 * NC + 2)
    pred2, ce2 = HF.sssr_tail_predict(x, *mods, target=H.dev(clean), counts=c2, confusion=cm2)
    _, ce3 = HF.sssr_tail_predict(x, *mods, target=H.dev(clean))
    assert np.isfinite(float(ce2)) and ce2.cpu().numpy().tobytes() == ce3.cpu().numpy().tobytes() and torch.equal(pred2, pred)
    assert np.array_equal(cm2.cpu().numpy().reshape(NC, NC), _bincount_matrix(pred_h, clean))
    _invariants(cm2.cpu().numpy(), c2.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 2. all mass in one bin
def test_skewed_labels_and_a_constant_prediction():
    """90 % of the targets are class 0 and every prediction is class 0 (w2 = 0 and a constant bias: all logits tie, the first maximum wins): every
    counted pixel of a block lands in column 0, most of them in bin (0, 0) - the worst case for same-address LDS atomics."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    shape = (3, NC, 110, 100)
    mods = _tail_modules(3, w2=np.zeros((NC, NC, 2, 2)), bias2=np.full(NC, 0.25))
    rs = np.random.RandomState(21)
    target = _target(22, (3, 440, 400))
    target[rs.uniform(size=target.shape) < 0.9] = 0
    cm, counts = _zeros(NC * NC), _zeros(3 * NC + 2)
    pred, _ = HF.sssr_tail_predict(H.dev(_tail_input(23, shape)), *mods, target=H.dev(target), counts=counts, confusion=cm)
    assert not pred.cpu().numpy().any()
    got = cm.cpu().numpy().reshape(NC, NC)
    class_count = np.bincount(target[target < NC].astype(np.int64), minlength=NC)
    assert got[0, 0] == class_count[0] and class_count[0] > 0.85 * target.size
    assert np.array_equal(got[:, 0], class_count) and not got[:, 1:].any()
    _invariants(got, counts.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 3. accumulation, optional outputs, arguments
def test_accumulation_and_optional_outputs():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods = _tail_modules(31)
    batches = [(H.dev(_tail_input(32 + i, (2, NC, 9, 13))), _target(40 + i, (2, 36, 52))) for i in range(2)]
    one = []
    for x, tg in batches:
        cm = _zeros(NC * NC)
        pred, _ = HF.sssr_tail_predict(x, *mods, target=H.dev(tg), counts=_zeros(3 * NC + 2), confusion=cm)
        one.append(cm.cpu().numpy())
        assert np.array_equal(one[-1].reshape(NC, NC), _bincount_matrix(pred.cpu().numpy(), tg))
    assert not np.array_equal(one[0], one[1])
    both = _zeros(NC * NC)
    for x, tg in batches:
        HF.sssr_tail_predict(x, *mods, target=H.dev(tg), confusion=both)           # counts=None
    assert np.array_equal(both.cpu().numpy(), one[0] + one[1])
    # straight at the entry point: cm without counts and without ce_out (the Python wrapper always asks for the loss)
    from dualsuperreslearningforsemseg_amd._lib import call
    x, tg = batches[0]
    td = H.dev(tg)
    xp, ldx = HF.pm(x)
    invstd = torch.rsqrt(mods[1].running_var + mods[1].eps)
    for flip_name, n in (('dsrl_sssr_tail_predict_cm', 2), ('dsrl_sssr_tail_predict_flip_cm', 1)):
        cm, pred = _zeros(NC * NC), torch.empty((n, 36, 52), dtype=torch.uint8, device=H.DEV)
        call(flip_name, xp.data_ptr(), ldx, n, 9, 13, NC, NC, NC, mods[0].weight.data_ptr(), mods[1].running_mean.data_ptr(), invstd.data_ptr(),
             mods[1].weight.data_ptr(), mods[1].bias.data_ptr(), mods[2].weight.data_ptr(), mods[2].bias.data_ptr(), pred.data_ptr(), td[:n].data_ptr(), IGNORE,
             None, None, None, None, 0, cm.data_ptr(), HF._stream())
        assert np.array_equal(cm.cpu().numpy().reshape(NC, NC), _bincount_matrix(pred.cpu().numpy(), tg[:n])), flip_name
    # argument errors, as for `counts`
    for bad in (_zeros(NC * NC, torch.int32), _zeros(NC * NC + 1), _zeros((NC * NC, 2))[:, 0], torch.zeros(NC * NC, dtype=torch.int64)):
        with pytest.raises(HF.DsrlHipError):
            HF.sssr_tail_predict(x, *mods, target=td, confusion=bad)
    with pytest.raises(HF.DsrlHipError, match='needs a target'):
        HF.sssr_tail_predict(x, *mods, confusion=_zeros(NC * NC))


# ---------------------------------------------------------------------------------------------- 4. the flip ensemble
def test_flip_matrix_is_the_ensembles():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods = _tail_modules(51)
    x = H.dev(_tail_input(52, (2 * 2, NC, 24, 40)))
    target = _target(53, (2, 96, 160))
    td = H.dev(target)
    counts, cm, flag = _zeros(3 * NC + 2), _zeros(NC * NC), _flag()
    pred, ce = HF.sssr_tail_predict(x, *mods, target=td, counts=counts, nan_flag=flag, flip=True, confusion=cm)
    counts0, flag0 = _zeros(3 * NC + 2), _flag()
    pred0, ce0 = HF.sssr_tail_predict(x, *mods, target=td, counts=counts0, nan_flag=flag0, flip=True)
    assert torch.equal(pred, pred0) and torch.equal(counts, counts0) and ce.cpu().numpy().tobytes() == ce0.cpu().numpy().tobytes()
    assert int(flag.item()) == 0 == int(flag0.item()) and tuple(pred.shape) == (2, 96, 160)
    assert np.array_equal(cm.cpu().numpy().reshape(NC, NC), _bincount_matrix(pred.cpu().numpy(), target))
    _invariants(cm.cpu().numpy(), counts.cpu().numpy())
    # and it is not the single view's matrix
    plain = _zeros(NC * NC)
    HF.sssr_tail_predict(x[:2], *mods, target=td, confusion=plain)
    assert not torch.equal(plain, cm)


# ---------------------------------------------------------------------------------------------- 5. a head the tail kernel does not implement
@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_fallback_head_counts_from_the_class_map(flip):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    assert _lib.query('dsrl_sssr_tail_predict_supported', 2, 6, 8, 8, 8, 8) == 0
    mods = _tail_modules(61, NC=8)
    x = H.dev(_tail_input(62, (4 if flip else 2, 8, 6, 8)))
    target = _target(63, (2, 24, 32), nc=8)
    target[1, 5, 5] = 100
    counts, cm, flag = _zeros(3 * 8 + 2), _zeros(64), _flag()
    pred, _ = HF.sssr_tail_predict(x, *mods, target=H.dev(target), counts=counts, nan_flag=flag, flip=flip, confusion=cm)
    assert int(flag.item()) == 2
    assert np.array_equal(cm.cpu().numpy().reshape(8, 8), _bincount_matrix(pred.cpu().numpy(), target, 8))
    _invariants(cm.cpu().numpy(), counts.cpu().numpy(), 8)


# ---------------------------------------------------------------------------------------------- 6. from logits
@pytest.mark.parametrize('C,ld', [(19, 19), (19, 24), (8, 8), (8, 24)])
def test_seg_metrics_cm_ties_stride_block_loop_and_foreign_labels(C, ld):
    """The construction of test_seg_metrics_ties_stride_block_loop_and_foreign_labels: tied and all-equal rows (the first maximum counts), pad channels
    holding 1e30 behind ld > C, P no multiple of the block and above one sweep of the grid, labels 255 and 200, added to buffers that already hold counts."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    rs = np.random.RandomState(C * 100 + ld)
    for P in (1, 257, 1024 * 256 + 300):
        buf = np.full((P, ld), 1e30, np.float32)
        buf[:, :C] = np.round(2.0 * rs.standard_normal((P, C))).clip(-2, 2) / 2.0
        buf[::7, :C] = 0.25
        tg = rs.randint(0, C, P)
        u = rs.uniform(size=P)
        tg[u < 0.1] = 255
        tg[u > 0.95] = 200
        if P == 1:
            tg[:] = C - 1
        tg = tg.astype(np.uint8)
        first_max = np.argmax(buf[:, :C], axis=1)                 # numpy's argmax is the first maximum
        want = _bincount_matrix(first_max, tg, C)
        logits, target = torch.from_numpy(buf).to(H.DEV), torch.from_numpy(tg).to(H.DEV)
        ref = _zeros(3 * C + 2)
        HF.call('dsrl_seg_metrics', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, ref.data_ptr(), HF._stream())
        pre = np.arange(C * C, dtype=np.int64) * 1000 + 7
        counts, cm = _zeros(3 * C + 2), torch.from_numpy(pre.copy()).to(H.DEV)
        HF.call('dsrl_seg_metrics_cm', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, counts.data_ptr(), cm.data_ptr(), HF._stream())
        assert np.array_equal(cm.cpu().numpy(), pre + want.reshape(-1)), f'C={C} ld={ld} P={P}'
        assert torch.equal(counts, ref)
        _invariants(cm.cpu().numpy() - pre, counts.cpu().numpy(), C)
        alone = _zeros(C * C)
        HF.call('dsrl_seg_metrics_cm', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, None, alone.data_ptr(), HF._stream())       # counts = NULL
        assert np.array_equal(alone.cpu().numpy(), want.reshape(-1))


def test_seg_metrics_cm_limit_and_the_metric_class():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix
    lib = _lib.load()
    limit = lib.dsrl_seg_metrics_cm_max_classes()
    assert 19 <= limit == ConfusionMatrix.max_classes_from_logits()
    C = limit + 1
    logits, target, cm = torch.zeros((64, C), device=H.DEV), torch.zeros(64, dtype=torch.uint8, device=H.DEV), _zeros(C * C)
    torch.cuda.synchronize()
    code = lib.dsrl_seg_metrics_cm(logits.data_ptr(), C, target.data_ptr(), 64, C, 255, None, cm.data_ptr(), HF._stream())
    assert code == -2 and b'classes' in lib.dsrl_last_error()         # DSRL_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not cm.cpu().numpy().any()                                 # nothing was launched
    at = _zeros(limit * limit)
    lg = torch.zeros((64, limit), device=H.DEV)
    HF.call('dsrl_seg_metrics_cm', lg.data_ptr(), limit, target.data_ptr(), 64, limit, 255, None, at.data_ptr(), HF._stream())
    assert int(at[0]) == 64 and int(at.sum()) == 64                   # all-equal rows: class 0, target 0
    # ConfusionMatrix.update_from_logits / update on (N,C,H,W) logits and class maps
    rs = np.random.RandomState(71)
    L = rs.standard_normal((2, NC, 12, 20)).astype(np.float32)
    tg = _target(72, (2, 12, 20))
    a, b = ConfusionMatrix(NC), ConfusionMatrix(NC)
    a.update_from_logits(H.dev(L), H.dev(tg))
    pred = torch.from_numpy(L.argmax(1).astype(np.uint8)).to(H.DEV)
    b.update(pred, H.dev(tg), H.dev(tg) != IGNORE)
    want = _bincount_matrix(L.argmax(1), tg)
    assert a.matrix.is_cuda and tuple(a.matrix.shape) == (NC, NC)
    assert np.array_equal(a.result()['matrix'], want) and np.array_equal(b.result()['matrix'], want)
    a.merge(b)
    assert np.array_equal(a.result()['matrix'], 2 * want) and abs(a.result()['mIoU'] - _figures(want)[1]) <= 1e-12 * _figures(want)[1]
    a.reset()
    assert not a.result()['matrix'].any()


# ---------------------------------------------------------------------------------------------- 7. from class maps
def _maps(seed, P, C=NC):
    rs = np.random.RandomState(seed)
    tg = rs.randint(0, C, P)
    pr = np.where(rs.uniform(size=P) < 0.6, tg, rs.randint(0, C, P))
    u = rs.uniform(size=P)
    tg[u < 0.1] = 255
    tg[(u >= 0.1) & (u < 0.13)] = 200
    return pr.astype(np.uint8), tg.astype(np.uint8)


@pytest.mark.parametrize('offsets', [(0, 0), (1, 1), (3, 3), (1, 3), (0, 3)], ids=lambda o: 'pred+{}_target+{}'.format(*o))
def test_confusion_matrix_of_class_maps_at_any_byte(offsets):
    """P around the 16-pixel load and above one sweep of the grid (512 blocks x 256 threads x 16 pixels), buffers that start 0, 1 and 3 bytes past
    an aligned address (together and apart), ignored and foreign targets, three runs with identical results."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    for P in (1, 15, 16, 17, 4099, 512 * 256 * 16 + 4099):
        pr, tg = _maps(P % 1000 + 7, P)
        want = _bincount_matrix(pr, tg).reshape(-1)
        assert (pr < NC).all()
        bp = torch.zeros(P + 16, dtype=torch.uint8, device=H.DEV)[offsets[0]:offsets[0] + P]
        bt = torch.zeros(P + 16, dtype=torch.uint8, device=H.DEV)[offsets[1]:offsets[1] + P]
        assert bp.data_ptr() % 16 == offsets[0] and bt.data_ptr() % 16 == offsets[1]
        bp.copy_(torch.from_numpy(pr)); bt.copy_(torch.from_numpy(tg))
        runs = []
        for _ in range(3):
            cm, flag = _zeros(NC * NC), _flag()
            HF.call('dsrl_confusion_matrix', bp.data_ptr(), bt.data_ptr(), P, NC, 255, cm.data_ptr(), flag.data_ptr(), HF._stream())
            runs.append(cm.cpu().numpy())
            assert int(flag.item()) == 0
        assert np.array_equal(runs[0], want), f'P={P}'
        assert np.array_equal(runs[1], want) and np.array_equal(runs[2], want)


def test_confusion_matrix_predicted_class_outside_the_classes():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    P = 4099
    pr, tg = _maps(5, P)
    live = np.flatnonzero(tg < NC)
    dead = np.flatnonzero(tg == 255)
    cm, flag = _zeros(NC * NC), _flag()
    bad = pr.copy()
    bad[dead[:5]] = 77                            # on ignored pixels: nothing to report
    HF.confusion_matrix_(cm, H.dev(bad), H.dev(tg), NC, 255, flag)
    assert int(flag.item()) == 0 and np.array_equal(cm.cpu().numpy(), _bincount_matrix(pr, tg).reshape(-1))
    bad[live[3]] = NC                             # on a counted pixel: bit 1, not counted
    bad[live[-1]] = 255
    cm.zero_()
    HF.confusion_matrix_(cm, H.dev(bad), H.dev(tg), NC, 255, flag)
    assert int(flag.item()) == 2
    assert np.array_equal(cm.cpu().numpy(), _bincount_matrix(bad, tg).reshape(-1)) and int(cm.sum()) == live.size - 2
    HF.confusion_matrix_(cm, H.dev(bad), H.dev(tg), NC, 255)            # no flag: still not counted, and the buffer accumulates
    assert int(cm.sum()) == 2 * (live.size - 2)
    # skewed maps: one pair on 90 % of the pixels
    P = 300000
    rs = np.random.RandomState(9)
    pr, tg = _maps(6, P)
    same = rs.uniform(size=P) < 0.9
    pr[same], tg[same] = 0, 0
    cm.zero_()
    HF.confusion_matrix_(cm, H.dev(pr).reshape(3, 100, 1000), H.dev(tg).reshape(3, 100, 1000), NC)
    assert np.array_equal(cm.cpu().numpy(), _bincount_matrix(pr, tg).reshape(-1))


# ---------------------------------------------------------------------------------------------- the model: compiled predictor, benchmark, validation
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


def test_compiled_predictor_hands_each_tensor_its_batch(model):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    shape = (2, 3, 64, 128)
    batches = [(_image(200 + i, shape), H.dev(_target(210 + i, (2, 128, 256)))) for i in range(4)]
    eager = []
    for x, tg in batches:
        cm = _zeros(NC * NC)
        pred, counts, ce = model.predict(x, tg, confusion=cm)
        assert np.array_equal(cm.cpu().numpy().reshape(NC, NC), _bincount_matrix(pred.cpu().numpy(), tg.cpu().numpy()))
        eager.append((pred.cpu().numpy(), counts.cpu().numpy(), ce.cpu().numpy().tobytes(), cm.cpu().numpy()))
    plain = model.predict(*batches[0])
    assert np.array_equal(plain[0].cpu().numpy(), eager[0][0]) and np.array_equal(plain[1].cpu().numpy(), eager[0][1])
    cp = model.compile_predict()
    try:
        for _ in range(cp.GRAPH_WARMUP):              # the frozen eager path: the caller's tensor goes straight to the kernel
            cm = _zeros(NC * NC)
            cp(*batches[0], confusion=cm)
            assert np.array_equal(cm.cpu().numpy(), eager[0][3])
        assert cp.num_graphs == 0
        for i in (1, 2, 3):                           # the capture and two more replays: a fresh tensor and another batch every time
            cm, replays = _zeros(NC * NC), cp.replays
            pred, counts, ce = cp(*batches[i], confusion=cm)
            assert cp.replays == replays + 1 and cp.num_graphs == 1
            got = (pred.cpu().numpy(), counts.cpu().numpy(), ce.cpu().numpy().tobytes(), cm.cpu().numpy())
            for g, w, what in zip(got, eager[i], ('pred', 'counts', 'ce', 'confusion')):
                assert np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w, (i, what)
        # a tensor that already holds counts is added to, not overwritten
        cm = torch.from_numpy(eager[1][3].copy()).to(H.DEV)
        cp(*batches[2], confusion=cm)
        assert np.array_equal(cm.cpu().numpy(), eager[1][3] + eager[2][3])
        # without `confusion`: another key, today's outputs
        for _ in range(cp.GRAPH_WARMUP + 1):
            pred, counts, ce = cp(*batches[0])
        assert cp.num_graphs == 2
        assert np.array_equal(pred.cpu().numpy(), eager[0][0]) and np.array_equal(counts.cpu().numpy(), eager[0][1]) and ce.cpu().numpy().tobytes() == eager[0][2]
        with pytest.raises(HF.DsrlHipError):
            cp(*batches[0], confusion=_zeros(NC * NC, torch.int32))
        with pytest.raises(HF.DsrlHipError, match='needs a target'):
            cp(batches[0][0], confusion=_zeros(NC * NC))
    finally:
        cp.release()
    with pytest.raises(HF.DsrlHipError, match='needs a target'):
        model.predict(batches[0][0], confusion=_zeros(NC * NC))


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_benchmark_reports_the_dataset_level_figures(model, tmp_path, flip):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.metrices import Accuracy, AverageMeter, mIoU
    weights = str(tmp_path / 'final.weights')
    torch.save({'model_state_dict': model.state_dict()}, weights)
    batches = [((_image(10 + i, (n, 3, 64, 128)), None), (H.dev(_target(20 + i, (n, 128, 256))), None)) for i, n in enumerate((2, 2, 1))]
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda split, batch_size, device, rank, world: batches}
    out_dir = str(tmp_path / 'out')
    result = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=out_dir, flip=flip)
    # the parent's formulas from the per-batch tables, and the matrix from separate predict calls
    m, a, ce_avg = mIoU(NC, CS.IGNORE_CLASS_LABEL), Accuracy(NC, CS.IGNORE_CLASS_LABEL), AverageMeter()
    total = np.zeros((NC, NC), np.int64)
    for (img, _), (target, _) in batches:
        pred, counts, ce = model.predict(img, target, flip=flip)
        m.update_from_counts(counts.cpu()); a.update_from_counts(counts.cpu())
        ce_avg.update(float(ce.double().cpu()), 2)
        total += _bincount_matrix(pred.cpu().numpy(), target.cpu().numpy())
    assert result['CE'] == ce_avg() and result['mIoU'] == m() and result['accuracy'] == a()
    assert np.array_equal(np.array(result['confusion_matrix'], dtype=np.int64), total)
    iou, miou = _figures(total)
    assert abs(result['mIoU_dataset'] - miou) <= 1e-12 * miou and np.allclose(result['IoU_per_class'], iou, rtol=1e-12, atol=0, equal_nan=True)
    assert isinstance(result['IoU_per_class'], list) and len(result['IoU_per_class']) == NC
    assert abs(result['pixel_accuracy'] - 100. * np.trace(total) / total.sum()) <= 1e-10
    assert 0 <= result['mean_class_accuracy'] <= 100 and 0 <= result['fwIoU'] <= 100
    assert result['mIoU_dataset'] != result['mIoU']
    text = open(os.path.join(out_dir, 'benchmark.txt')).read()
    old = 'Avg. Cross Entropy Error: {:.3f}\nmIoU %: {:.2f}\nMean Accuracy %: {:.2f}\n'.format(result['CE'], result['mIoU'], result['accuracy'])
    assert old in text and 'Weights file: {:s}\n'.format(weights) in text
    assert ('flip' in text) == flip
    new = text[text.index(old) + len(old):]
    assert 'Dataset-level mIoU %: {:.2f}\n'.format(result['mIoU_dataset']) in new
    for k, name in enumerate(CS.CLASS_NAMES):
        row = [ln for ln in new.splitlines() if ln.startswith(name + '  ')]
        assert row and '{:.2f}'.format(result['IoU_per_class'][k]) in row[0], (name, row)
    saved = np.load(os.path.join(out_dir, 'confusion_matrix.npy'))
    assert saved.dtype == np.int64 and np.array_equal(saved, total)


def test_validation_appends_the_dataset_level_miou():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep, _do_train_val
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    from dualsuperreslearningforsemseg_amd.metrices import Accuracy, AverageMeter, mIoU
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    from dualsuperreslearningforsemseg_amd import functional as HF
    torch.manual_seed(77)
    model = DSRL(1, CS).to(H.DEV).to(memory_format=torch.channels_last)
    flat = FlatParams(model)
    step = TrainStep(model, flat, 1, 0.1, 1.0, IGNORE, graph=False)
    loader = []
    for i, n in enumerate((2, 1)):
        org = _image(300 + i, (n, 3, 128, 256))
        loader.append(((HF.upsample_bilinear_ac(org, (64, 128)), org), (H.dev(_target(310 + i, (n, 128, 256))), None)))

    class Recording:
        """the step, with the logits and the losses it hands out kept for the parent's formulas"""

        def __init__(self):
            self.logits, self.losses = [], []

        def __getattr__(self, name):
            return getattr(step, name)

        def enqueue(self, *args):
            outs = step.enqueue(*args)
            self.logits.append(outs[0].detach().clone())
            return outs

        def collect(self):
            vals = step.collect()
            self.losses.append(list(vals))
            return vals

    rec = Recording()
    try:
        details = {}
        got = _do_train_val(False, 1, model, rec, loader, 0.01, 0.9, 5e-4, False, True, details)
    finally:
        step.release()
    assert len(got) == 7 and len(rec.logits) == 2 and len(rec.losses) == 2
    meters = [AverageMeter() for _ in range(4)]
    m, a = mIoU(NC, IGNORE), Accuracy(NC, IGNORE)
    total = np.zeros((NC, NC), np.int64)
    for (_, (target, _)), logits, vals, n in zip(loader, rec.logits, rec.losses, (2, 1)):
        for mt, v in zip(meters, vals):
            mt.update(v, n)
        m.update_from_logits(logits, target); a.update_from_logits(logits, target)
        total += _bincount_matrix(torch.argmax(logits, dim=1).cpu().numpy(), target.cpu().numpy())
    assert got[:6] == [mt() for mt in meters] + [m(), a()]
    iou, miou = _figures(total)
    assert abs(got[6] - miou) <= 1e-12 * miou
    assert np.allclose(details['IoU_per_class'], iou, rtol=1e-12, atol=0, equal_nan=True)

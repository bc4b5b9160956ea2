"""CPU-only checks of the dataset-level evaluation: metrices.ConfusionMatrix on matrices given as host tensors against a plain numpy restatement
(a handful of fp64 operations on exact integers: 1e-12 relative), the NaN rules, the reason the class exists (the dataset-level mIoU is not the
per-batch one), and the argument errors of the `confusion=` surface that need no device."""
import numpy as np
import pytest
import torch

import predict_fixtures as PF

NC = 19


def _bincount_matrix(pred, target, C=NC, ignore=255):
    valid = (target != ignore) & (target < C)
    t, p = target[valid].astype(np.int64), pred[valid].astype(np.int64)
    return np.bincount(t * C + p, minlength=C * C).reshape(C, C)


def _restated(m):
    """the published figures, written out: sums over the split first, then per class, then the mean over the classes that exist"""
    m = m.astype(np.float64)
    C = m.shape[0]
    iou, recall = np.full(C, np.nan), np.full(C, np.nan)
    for c in range(C):
        inter, tgt, prd = m[c, c], m[c, :].sum(), m[:, c].sum()
        if tgt + prd - inter > 0:
            iou[c] = 100. * inter / (tgt + prd - inter)
        if tgt > 0:
            recall[c] = 100. * inter / tgt
    total = m.sum()
    fw = sum(m[c, :].sum() * iou[c] for c in range(C) if not np.isnan(iou[c])) / total
    return {'IoU': iou, 'mIoU': np.nanmean(iou), 'class_accuracy': recall, 'mean_class_accuracy': np.nanmean(recall),
            'pixel_accuracy': 100. * np.trace(m) / total, 'fwIoU': fw}


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= 1e-12 * np.abs(b[ok])), (a, b)


@pytest.fixture(scope='module')
def golden_matrices(golden):
    g = golden('pipeline_metrics')
    return g, [_bincount_matrix(g[f'metrics.pred{b}'], g[f'metrics.target{b}']) for b in range(3)]


def test_merge_and_result_against_numpy(golden_matrices):
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix
    _, mats = golden_matrices
    cm = ConfusionMatrix(NC)
    cm.merge(torch.from_numpy(mats[0]))                         # (C, C)
    cm.merge(torch.from_numpy(mats[1].reshape(-1)))             # flat, as the kernels see it
    other = ConfusionMatrix(NC)
    other.merge(torch.from_numpy(mats[2]))
    cm.merge(other)
    total = mats[0] + mats[1] + mats[2]
    assert cm.matrix.dtype == torch.int64 and tuple(cm.matrix.shape) == (NC, NC) and not cm.matrix.is_cuda
    res = cm.result()
    assert res['matrix'].dtype == np.int64 and np.array_equal(res['matrix'], total)
    want = _restated(total)
    for k, v in want.items():
        _close(res[k], v)
        assert np.asarray(res[k]).dtype == np.float64
    # the invariants every producer is tested against: rows = area_target, columns = area_pred, diagonal = area_inter
    g = golden_matrices[0]
    table = sum(PF.counts_table(g[f'metrics.pred{b}'], g[f'metrics.target{b}']) for b in range(3))
    assert np.array_equal(total.sum(axis=1), table[2 * NC:3 * NC]) and np.array_equal(total.sum(axis=0), table[:NC])
    assert np.array_equal(np.diag(total), table[NC:2 * NC]) and total.sum() == table[3 * NC + 1] and np.trace(total) == table[3 * NC]
    cm.reset()
    assert int(cm.matrix.sum()) == 0
    with pytest.raises(ValueError):
        cm.merge(torch.zeros(NC * NC, dtype=torch.int32))
    with pytest.raises(ValueError):
        cm.merge(torch.zeros(NC * NC - 1, dtype=torch.int64))


def test_a_class_without_pixels_is_nan_and_leaves_the_mean():
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix
    m = np.zeros((4, 4), np.int64)
    m[0, 0], m[0, 1], m[1, 1], m[3, 1] = 6, 2, 5, 3              # class 2: neither target nor predicted; class 3: target only
    cm = ConfusionMatrix(4)
    cm.merge(torch.from_numpy(m))
    res = cm.result()
    assert np.isnan(res['IoU'][2]) and np.isnan(res['class_accuracy'][2])
    assert res['IoU'][3] == 0.0 and res['class_accuracy'][3] == 0.0
    _close(res['IoU'], [100. * 6 / 8, 100. * 5 / 10, np.nan, 0.])
    _close(res['mIoU'], (75. + 50. + 0.) / 3)
    _close(res['class_accuracy'], [75., 100., np.nan, 0.])
    _close(res['mean_class_accuracy'], 175. / 3)
    _close(res['pixel_accuracy'], 100. * 11 / 16)
    _close(res['fwIoU'], (8 * 75. + 5 * 50. + 3 * 0.) / 16)


def test_the_empty_matrix_gives_nan_and_does_not_raise():
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix
    import warnings
    fresh, merged = ConfusionMatrix(NC), ConfusionMatrix(NC)
    merged.merge(torch.zeros((NC, NC), dtype=torch.int64))
    with warnings.catch_warnings():
        warnings.simplefilter('error')                          # neither a division warning nor a "mean of empty slice"
        for cm in (fresh, merged):
            res = cm.result()
            assert np.isnan(res['IoU']).all() and np.isnan(res['class_accuracy']).all()
            for k in ('mIoU', 'mean_class_accuracy', 'pixel_accuracy', 'fwIoU'):
                assert np.isnan(res[k]), k
            assert res['matrix'].shape == (NC, NC) and not res['matrix'].any()


def test_dataset_level_miou_is_not_the_per_batch_figure(golden_matrices):
    """Why the class exists: metrices.mIoU reproduces the reference's mean over batches of per-batch class means (the golden figure), which is not
    the mean over classes of the IoU of the summed intersections and unions."""
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix, mIoU
    g, mats = golden_matrices
    per_batch, whole = mIoU(NC), ConfusionMatrix(NC)
    for b in range(3):
        per_batch.update_from_counts(torch.from_numpy(PF.counts_table(g[f'metrics.pred{b}'], g[f'metrics.target{b}'])))
        whole.merge(torch.from_numpy(mats[b]))
    assert abs(per_batch() - float(g['metrics.miou'])) <= 1e-9 * abs(float(g['metrics.miou']))
    dataset = whole.result()['mIoU']
    _close(dataset, _restated(sum(mats))['mIoU'])
    print(f'per-batch mIoU {per_batch():.6f} %, dataset-level mIoU {dataset:.6f} %')
    assert abs(dataset - per_batch()) > 1e-6, (dataset, per_batch())


def test_argument_errors_without_a_device():
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    from dualsuperreslearningforsemseg_amd.metrices import ConfusionMatrix
    for name in ('dsrl_sssr_tail_predict_cm', 'dsrl_sssr_tail_predict_flip_cm', 'dsrl_seg_metrics_cm', 'dsrl_confusion_matrix'):
        assert name in _lib.PROTOTYPES
    assert 19 <= _lib.query('dsrl_seg_metrics_cm_max_classes') and 19 <= _lib.query('dsrl_confusion_matrix_max_classes')
    cpu = torch.device('cpu')
    with pytest.raises(HF.DsrlHipError, match='int64'):
        HF.check_confusion(torch.zeros(NC * NC, dtype=torch.int32), NC, cpu)
    with pytest.raises(HF.DsrlHipError, match='361 elements'):
        HF.check_confusion(torch.zeros(NC * NC + 1, dtype=torch.int64), NC, cpu)
    with pytest.raises(HF.DsrlHipError, match='contiguous'):
        HF.check_confusion(torch.zeros((NC * NC, 2), dtype=torch.int64)[:, 0], NC, cpu)
    with pytest.raises(HF.DsrlHipError, match='HIP device only'):
        HF.check_confusion(torch.zeros(NC * NC, dtype=torch.int64), NC, cpu)
    # confusion without a target: refused before anything else is looked at
    with pytest.raises(HF.DsrlHipError, match='needs a target'):
        HF.sssr_tail_predict(torch.zeros(1, NC, 2, 2), None, None, None, confusion=torch.zeros(NC * NC, dtype=torch.int64))
    # CPU tensors handed to the device paths
    pred = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(HF.DsrlHipError, match='HIP device only'):
        HF.confusion_matrix_(torch.zeros(NC * NC, dtype=torch.int64), pred, pred, NC)
    cm = ConfusionMatrix(NC)
    with pytest.raises(HF.DsrlHipError, match='HIP device only'):
        cm.update(pred, pred, pred == 0)
    with pytest.raises(HF.DsrlHipError, match='HIP device only'):
        cm.update_from_logits(torch.zeros(1, NC, 4, 4), pred)
    with pytest.raises(ValueError):
        cm.matrix                                   # nothing was fed: no device to allocate it on


def test_class_names_are_the_train_ids():
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    assert len(CS.CLASS_NAMES) == CS.NUM_CLASSES == len(set(CS.CLASS_NAMES))
    assert CS.CLASS_NAMES[0] == 'road' and CS.CLASS_NAMES[12] == 'rider' and CS.CLASS_NAMES[18] == 'bicycle'

"""On-device counterparts of the reference's metrices/ package (AverageMeter.py:16-27, mIoU.py:15-41, Accuracy.py:13-30), and the dataset-level
ConfusionMatrix the reference has no counterpart of."""
import numpy as np
import torch

from .. import functional as HF
from .._lib import call, query


class AverageMeter:
    """metrices/AverageMeter.py: running mean weighted by the batch size."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.sum, self.count = 0.0, 0

    def update(self, value, n=1):
        self.sum += float(value) * n
        self.count += n

    def __call__(self):
        return self.sum / self.count if self.count else 0.0


class _Counts:
    """Per-batch [area_pred | area_inter | area_target | correct, valid] counters produced by dsrl_seg_metrics, kept on the device
    until the metric is read (one readback per epoch instead of one host-side numpy pass per batch)."""

    def __init__(self, num_classes, ignore_index=255):
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.batches = []

    def add_logits(self, logits, target):
        logits, ld = HF.pm(logits)
        N, C, H, W = logits.shape
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        counts = torch.zeros(3 * C + 2, dtype=torch.int64, device=logits.device)
        call('dsrl_seg_metrics', logits.data_ptr(), ld, target.data_ptr(), N * H * W, C, self.ignore_index, counts.data_ptr(), HF._stream())
        self.batches.append(counts)

    def add_pred(self, pred, target, valid_labels_mask):
        """reference call shape: class maps + boolean mask (device tensors); routed through the same kernel via one-hot scores"""
        tgt = torch.where(valid_labels_mask.bool(), target.long(), torch.full_like(target.long(), self.ignore_index)).to(torch.uint8)
        scores = torch.nn.functional.one_hot(pred.long(), self.num_classes).permute(0, 3, 1, 2).float().contiguous(memory_format=torch.channels_last)
        self.add_logits(scores, tgt)

    def add_counts(self, counts):
        """a table some kernel already filled for one batch (dsrl_sssr_tail_predict); a host tensor is taken as it is"""
        if counts.numel() != 3 * self.num_classes + 2:
            raise ValueError(f'counts of {counts.numel()} elements, expected {3 * self.num_classes + 2}')
        self.batches.append(counts.reshape(-1).to(torch.int64))

    def table(self):
        return torch.stack(self.batches).cpu().double() if self.batches else torch.zeros((0, 3 * self.num_classes + 2), dtype=torch.float64)


class mIoU:
    """metrices/mIoU.py: per batch the nan-mean over classes of intersection/union, then the nan-mean over batches, in percent."""

    def __init__(self, num_classes, ignore_index=255):
        self.num_classes = num_classes
        self._c = _Counts(num_classes, ignore_index)

    def reset(self):
        self._c.batches = []

    def update(self, pred, target, valid_labels_mask):
        assert pred.shape == target.shape, "BUG CHECK: 'pred' and 'target' must be of the same shape of (B, H, W)."
        assert len(pred.shape) == 3, "BUG CHECK: 'target' and 'pred' must be (B, H, W) channel-order dimensions."
        self._c.add_pred(pred, target, valid_labels_mask)

    def update_from_logits(self, logits, target):
        self._c.add_logits(logits, target)

    def update_from_counts(self, counts):
        self._c.add_counts(counts)

    def __call__(self):
        t, C = self._c.table(), self.num_classes
        if t.shape[0] == 0:
            return 0.0
        inter, union = t[:, C:2 * C], t[:, :C] + t[:, 2 * C:3 * C] - t[:, C:2 * C]
        iou = inter / union                                     # 0/0 -> nan: classes absent from a batch are skipped (np.nanmean)
        return float(torch.nanmean(torch.nanmean(iou, dim=1)) * 100.)


class Accuracy:
    """metrices/Accuracy.py: mean over batches of correct / valid pixels, in percent."""

    def __init__(self, num_classes=19, ignore_index=255):
        self._c = _Counts(num_classes, ignore_index)

    def reset(self):
        self._c.batches = []

    def update(self, pred, target, valid_labels_mask):
        assert pred.shape == target.shape, "BUG CHECK: 'pred' and 'target' must be of the same shape of (B, H, W)."
        assert len(pred.shape) == 3, "BUG CHECK: 'target' and 'pred' must be (B, H, W) channel-order dimensions."
        self._c.add_pred(pred, target, valid_labels_mask)

    def update_from_logits(self, logits, target):
        self._c.add_logits(logits, target)

    def update_from_counts(self, counts):
        self._c.add_counts(counts)

    def __call__(self):
        t, C = self._c.table(), self._c.num_classes
        if t.shape[0] == 0:
            return 0.0
        return float((t[:, 3 * C] / t[:, 3 * C + 1]).mean() * 100.)


class ConfusionMatrix:
    """Dataset-level evaluation: one C x C matrix summed over a whole split, matrix[t, p] = pixels with target t and predicted class p (targets equal
    to `ignore_index` or >= C are not counted: the rule of the per-batch counters).  The figures are the published kind - intersections and unions
    summed over the split, then IoU per class, then the mean over the classes - where mIoU above is the reference's mean over batches of per-batch means.

    `.matrix` is the int64 (C, C) buffer, allocated on first use on the device of what it is fed; every producer adds to it and none clears it, so it
    can be handed to `DSRL.predict(confusion=cm.matrix)` batch after batch and read once."""

    def __init__(self, num_classes, ignore_index=255):
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self._matrix = None

    def _on(self, device):
        if self._matrix is None:
            self._matrix = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=device)
        elif self._matrix.device != torch.device(device):
            raise ValueError(f'ConfusionMatrix lives on {self._matrix.device}, fed from {device}')
        return self._matrix

    @property
    def matrix(self):
        if self._matrix is None:
            raise ValueError('ConfusionMatrix.matrix before first use: call on(device), update*() or merge() first')
        return self._matrix

    def on(self, device):
        """-> .matrix, allocated on `device` if nothing has been fed yet"""
        return self._on(torch.device(device))

    def reset(self):
        if self._matrix is not None:
            self._matrix.zero_()

    def update(self, pred, target, valid_labels_mask=None):
        """reference call shape: class maps (B, H, W) and a boolean mask of the pixels that count (device tensors) -> dsrl_confusion_matrix"""
        assert pred.shape == target.shape, "BUG CHECK: 'pred' and 'target' must be of the same shape of (B, H, W)."
        HF._need_gpu(pred, target, valid_labels_mask)
        if valid_labels_mask is not None:
            target = torch.where(valid_labels_mask.bool(), target.long(), torch.full_like(target.long(), self.ignore_index))
        HF.confusion_matrix_(self._on(pred.device), pred, target, self.num_classes, self.ignore_index)

    def update_from_logits(self, logits, target):
        """logits (N, C, H, W): the arg-max and the matrix in one pass over them (dsrl_seg_metrics_cm), no class map in memory"""
        HF._need_gpu(logits, target)
        logits, ld = HF.pm(logits)
        N, C, H, W = logits.shape
        if C != self.num_classes:
            raise ValueError(f'logits of {C} classes, expected {self.num_classes}')
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        cm = self._on(logits.device)
        call('dsrl_seg_metrics_cm', logits.data_ptr(), ld, target.data_ptr(), N * H * W, C, self.ignore_index, None, cm.data_ptr(), HF._stream())

    @staticmethod
    def max_classes_from_logits():
        """the largest class count update_from_logits takes (dsrl_seg_metrics_cm_max_classes)"""
        return int(query('dsrl_seg_metrics_cm_max_classes'))

    def merge(self, other):
        """adds another ConfusionMatrix or an int64 tensor of C*C elements; a host tensor is taken as it is (and so is its device)"""
        m = other.matrix if isinstance(other, ConfusionMatrix) else other
        if m.dtype != torch.int64 or m.numel() != self.num_classes ** 2:
            raise ValueError(f'merge: an int64 tensor of {self.num_classes ** 2} elements expected, got {m.dtype} of {m.numel()}')
        self._on(m.device).add_(m.reshape(self.num_classes, self.num_classes))

    def result(self):
        """The one device read -> dict of float64 figures (percent): IoU and class_accuracy (recall) per class, NaN where a class has no pixels to
        judge it by; mIoU and mean_class_accuracy their nan-means; pixel_accuracy = trace / total; fwIoU the frequency-weighted IoU; matrix the int64
        array.  An empty matrix gives NaN figures."""
        C = self.num_classes
        m = np.zeros((C, C), np.int64) if self._matrix is None else self._matrix.cpu().numpy().astype(np.int64)
        return figures(m)


def calibration_figures(record):
    """The figures of a calibration record [n_b | hit_b | q_b] (3 * bins integers; include/dsrl_hip.h "calibration"), float64, host only:
    acc_b = hit_b / n_b, conf_b = q_b / (2^24 n_b), ECE = sum_b (n_b / N) |acc_b - conf_b|, MCE the maximum of |acc_b - conf_b| over the non-empty
    bins, mean_confidence, accuracy (fractions in [0, 1]) and gap = mean_confidence - accuracy (> 0: over-confident).  -> dict with those and `bins`
    = {'n' int64, 'acc', 'conf'} per bin (NaN where a bin is empty), `pixels` = N.  An empty record gives NaN figures."""
    if isinstance(record, torch.Tensor):
        record = record.detach().cpu().numpy()
    rec = np.asarray(record)
    if rec.size == 0 or rec.size % 3:
        raise ValueError(f'calibration_figures: a record of 3 * bins integers expected, got {rec.size} elements')
    rec = rec.astype(np.int64).reshape(3, -1)
    n, hit, q = rec[0], rec[1], rec[2]
    total = int(n.sum())
    nf = n.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        acc = hit.astype(np.float64) / nf
        conf = q.astype(np.float64) / (16777216.0 * nf)
    bins = {'n': n.copy(), 'acc': acc, 'conf': conf}
    if total == 0:
        nan = float('nan')
        return {'ECE': nan, 'MCE': nan, 'mean_confidence': nan, 'accuracy': nan, 'gap': nan, 'pixels': 0, 'bins': bins}
    live = n > 0
    gap = np.abs(acc[live] - conf[live])
    mean_conf, accuracy = float(q.sum()) / (16777216.0 * total), float(hit.sum()) / total
    return {'ECE': float((nf[live] / total * gap).sum()), 'MCE': float(gap.max()), 'mean_confidence': mean_conf, 'accuracy': accuracy,
            'gap': mean_conf - accuracy, 'pixels': total, 'bins': bins}


class Calibration:
    """Expected / Maximum Calibration Error over a whole split (Guo et al. 2017): the reliability histogram of the maximum softmax probability over
    `bins` equal-width bins.  Shaped like ConfusionMatrix: `.record` is the int64 [n_b | hit_b | q_b] buffer of 3 * bins elements, allocated on first
    use on the device of what it is fed; every producer adds to it and none clears it, so it can be handed to `DSRL.predict(calibration=cal.record)`
    batch after batch; result() does the one read."""

    def __init__(self, bins=HF.CALIBRATION_DEFAULT_BINS, ignore_index=255):
        self.bins, self.ignore_index = HF.calibration_bins_value(bins, 'Calibration'), int(ignore_index)
        self._record = None

    def _on(self, device):
        if self._record is None:
            self._record = torch.zeros(3 * self.bins, dtype=torch.int64, device=device)
        elif self._record.device != torch.device(device):
            raise ValueError(f'Calibration lives on {self._record.device}, fed from {device}')
        return self._record

    @property
    def record(self):
        if self._record is None:
            raise ValueError('Calibration.record before first use: call on(device), update_from_logits() or merge() first')
        return self._record

    def on(self, device):
        """-> .record, allocated on `device` if nothing has been fed yet"""
        return self._on(torch.device(device))

    def reset(self):
        if self._record is not None:
            self._record.zero_()

    def update_from_logits(self, logits, target):
        """logits (N, C, H, W), target (N, H, W): one streaming pass (dsrl_calibration_from_logits), nothing read back"""
        HF._need_gpu(logits, target)
        HF.calibration_counts_(self._on(logits.device), logits, target, self.ignore_index, self.bins)

    def merge(self, other):
        """adds another Calibration or an int64 tensor of 3 * bins elements; a host tensor is taken as it is (and so is its device)"""
        r = other.record if isinstance(other, Calibration) else other
        if r.dtype != torch.int64 or r.numel() != 3 * self.bins:
            raise ValueError(f'merge: an int64 tensor of {3 * self.bins} elements expected, got {r.dtype} of {r.numel()}')
        self._on(r.device).add_(r.reshape(-1))

    def result(self):
        """The one device read -> calibration_figures(record); nothing fed: NaN figures"""
        return calibration_figures(np.zeros(3 * self.bins, np.int64) if self._record is None else self._record)


def temperature_figures(betas, record):
    """The figures of a temperature record (float64 [1 + 3 K]: live pixels, then the sums of L, G, H at each of the ascending `betas`;
    include/dsrl_hip.h "temperature"), host only: `beta` = the fitted 1 / T (functional.temperature_solve), `temperature` = 1 / beta, `at_bound`
    (the minimum lies at or beyond an end of the grid: the end is reported), `nll` = the mean NLL over the live pixels at each beta, `betas`,
    `pixels`.  An empty record gives NaN figures."""
    b, r = HF._temperature_record_value(betas, record, 'temperature_figures')
    n = int(r[0])
    if n == 0:
        nan = float('nan')
        return {'temperature': nan, 'beta': nan, 'at_bound': False, 'nll': np.full(b.size, nan), 'betas': b, 'pixels': 0}
    beta, at_bound = HF.temperature_solve(b, r)
    return {'temperature': 1.0 / beta, 'beta': beta, 'at_bound': bool(at_bound), 'nll': r[1::3] / float(n), 'betas': b, 'pixels': n}


class TemperatureFit:
    """One pass of a temperature fit over a whole split (Guo et al. 2017): the NLL of softmax(beta logits), beta = 1 / T, with its first and second
    derivative at the K <= 16 values `betas` (functional.temperature_grid).  Shaped like Calibration: `.record` is the float64 buffer of 1 + 3 K
    elements, allocated on first use on the device of what it is fed; update_from_logits adds to it and nothing clears it; result() does the one
    read.  The betas travel to the device once, beside the record."""

    def __init__(self, betas, ignore_index=255):
        self.betas, self.ignore_index = HF.temperature_betas_value(betas, 'TemperatureFit'), int(ignore_index)
        if np.any(np.diff(self.betas) <= 0.0):
            raise ValueError(f'TemperatureFit: the betas must ascend, got {self.betas.tolist()}')
        self._record = self._betas_dev = None

    def _on(self, device):
        if self._record is None:
            self._record = torch.zeros(1 + 3 * self.betas.size, dtype=torch.float64, device=device)
            self._betas_dev = torch.tensor(self.betas, dtype=torch.float32).to(device)
        elif self._record.device != torch.device(device):
            raise ValueError(f'TemperatureFit lives on {self._record.device}, fed from {device}')
        return self._record

    @property
    def record(self):
        if self._record is None:
            raise ValueError('TemperatureFit.record before first use: call on(device), update_from_logits() or merge() first')
        return self._record

    def on(self, device):
        """-> .record, allocated on `device` if nothing has been fed yet"""
        return self._on(torch.device(device))

    def reset(self):
        if self._record is not None:
            self._record.zero_()

    def update_from_logits(self, logits, target, nan_flag=None):
        """logits (N, C, H, W), target (N, H, W): one streaming pass and its finish (dsrl_temperature_stats), nothing read back"""
        HF._need_gpu(logits, target)
        rec = self._on(logits.device)
        HF.temperature_stats_(rec, logits, target, self._betas_dev if self._betas_dev.device.type != 'cpu' else self.betas, self.ignore_index, nan_flag)

    def merge(self, other):
        """adds another TemperatureFit over the same betas, or a float64 tensor of 1 + 3 K elements; a host tensor is taken as it is"""
        if isinstance(other, TemperatureFit) and not np.array_equal(other.betas, self.betas):
            raise ValueError('merge: the two fits are over different betas')
        r = other.record if isinstance(other, TemperatureFit) else other
        if r.dtype != torch.float64 or r.numel() != 1 + 3 * self.betas.size:
            raise ValueError(f'merge: a float64 tensor of {1 + 3 * self.betas.size} elements expected, got {r.dtype} of {r.numel()}')
        self._on(r.device).add_(r.reshape(-1))

    def result(self):
        """The one device read -> temperature_figures(betas, record); nothing fed: NaN figures"""
        return temperature_figures(self.betas, np.zeros(1 + 3 * self.betas.size) if self._record is None else self._record)


class SRQuality:
    """PSNR (dB, data range 1) and SSIM of super-resolved images against their originals over a whole split (functional.sr_quality): `mean` / `std`
    are the normalisation the tensors carry (dataset settings' MEAN / STD; None: values in [0, 1] already).  Every update leaves one (N, 2) float64
    record tensor on the device; result() does the one read."""

    def __init__(self, mean=None, std=None):
        self.mean, self.std = mean, std
        self.reset()

    def reset(self):
        self.batches = []           # [(records (N, 2), C, H, W)]

    def update(self, pred, ref):
        """pred, ref (N,C,H,W) device tensors -> dsrl_sr_quality; nothing is read back"""
        records = HF.sr_quality(pred, ref, self.mean, self.std)
        self.batches.append((records,) + tuple(int(v) for v in pred.shape[1:]))

    def update_from_records(self, records, C, H, W):
        """records (N, 2) {sse, ssim_sum} some call of functional.sr_quality already produced for (C, H, W) images; a host tensor is taken as it is"""
        if records.dim() != 2 or records.shape[1] != 2:
            raise ValueError(f'records of shape (N, 2) expected, got {tuple(records.shape)}')
        self.batches.append((records.to(torch.float64), int(C), int(H), int(W)))

    def result(self):
        """The one device read -> {'PSNR', 'SSIM', 'images', 'PSNR_per_image', 'SSIM_per_image'}: PSNR the mean over the images of their dB figures
        (the convention of super-resolution papers, not the dB of the mean error), SSIM the mean over the images.  Nothing fed: NaN figures and 0
        images.  An image identical to its original has PSNR +inf, and so has the mean."""
        if not self.batches:
            nan = float('nan')
            return {'PSNR': nan, 'SSIM': nan, 'images': 0, 'PSNR_per_image': np.zeros(0), 'SSIM_per_image': np.zeros(0)}
        devices = {b[0].device for b in self.batches}
        host = (torch.cat([b[0] for b in self.batches]).cpu() if len(devices) == 1 else torch.cat([b[0].cpu() for b in self.batches])).numpy()
        psnr, ssim, at = [], [], 0
        for rec, C, H, W in self.batches:
            p, s = HF.sr_quality_figures(host[at:at + rec.shape[0]], C, H, W)
            psnr.append(p); ssim.append(s)
            at += rec.shape[0]
        psnr, ssim = np.concatenate(psnr), np.concatenate(ssim)
        return {'PSNR': float(psnr.mean()), 'SSIM': float(ssim.mean()), 'images': int(psnr.size), 'PSNR_per_image': psnr, 'SSIM_per_image': ssim}


class BoundaryIoU:
    """Dataset-level Boundary IoU (Cheng et al., CVPR 2021): the IoU restricted to the pixels within `distance` of a class outline, `ratio` of each
    batch's image diagonal when `distance` is None (functional.boundary_counts_, dsrl_boundary_counts).  Shaped like ConfusionMatrix: `.counts` is the
    int64 [I | G | P] buffer of 3 * num_classes elements, allocated on first use on the device of what it is fed; every update adds to it, result()
    does the one read."""

    def __init__(self, num_classes, ignore_index=255, ratio=0.02, distance=None):
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self.ratio, self.distance = float(ratio), None if distance is None else int(distance)
        HF.boundary_distance(1, 1, self.ratio)          # a bad ratio is refused here
        if self.distance is not None and self.distance < 1:
            raise ValueError(f'BoundaryIoU: distance {self.distance} below 1')
        self._counts = None

    def _on(self, device):
        if self._counts is None:
            self._counts = torch.zeros(3 * self.num_classes, dtype=torch.int64, device=device)
        elif self._counts.device != torch.device(device):
            raise ValueError(f'BoundaryIoU lives on {self._counts.device}, fed from {device}')
        return self._counts

    @property
    def counts(self):
        if self._counts is None:
            raise ValueError('BoundaryIoU.counts before first use: call on(device), update() or merge() first')
        return self._counts

    def on(self, device):
        """-> .counts, allocated on `device` if nothing has been fed yet"""
        return self._on(torch.device(device))

    def reset(self):
        if self._counts is not None:
            self._counts.zero_()

    def update(self, pred, target, valid_labels_mask=None):
        """class maps (B, H, W) or (H, W) and an optional boolean mask of the pixels that count (device tensors) -> dsrl_boundary_counts"""
        assert pred.shape == target.shape, "BUG CHECK: 'pred' and 'target' must be of the same shape of (B, H, W)."
        HF._need_gpu(pred, target, valid_labels_mask)
        if valid_labels_mask is not None:
            target = torch.where(valid_labels_mask.bool(), target.long(), torch.full_like(target.long(), self.ignore_index))
        HF.boundary_counts_(self._on(pred.device), pred, target, self.num_classes, self.ignore_index, distance=self.distance, ratio=self.ratio)

    def merge(self, other):
        """adds another BoundaryIoU or an int64 tensor of 3 * C elements; a host tensor is taken as it is (and so is its device)"""
        m = other.counts if isinstance(other, BoundaryIoU) else other
        if m.dtype != torch.int64 or m.numel() != 3 * self.num_classes:
            raise ValueError(f'merge: an int64 tensor of {3 * self.num_classes} elements expected, got {m.dtype} of {m.numel()}')
        self._on(m.device).add_(m.reshape(-1))

    def result(self):
        """The one device read -> boundary_figures(counts); nothing fed gives NaN figures."""
        C = self.num_classes
        return boundary_figures(np.zeros(3 * C, np.int64) if self._counts is None else self._counts.cpu().numpy().astype(np.int64))


def boundary_figures(counts):
    """The figures of BoundaryIoU.result() from the [I | G | P] counters (3 * C integers): {'BIoU': per class I / (G + P - I) in percent, NaN where a
    class has no band pixel in either map; 'mBIoU': its nan-mean; 'I', 'G', 'P': the int64 counters}."""
    c = np.asarray(counts).astype(np.int64).reshape(3, -1)
    inter, union = c[0].astype(np.float64), (c[1] + c[2] - c[0]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        biou = np.where(union > 0, inter / union, np.nan)
    return {'BIoU': 100. * biou, 'mBIoU': 100. * _nanmean(biou), 'I': c[0].copy(), 'G': c[1].copy(), 'P': c[2].copy()}


def _nanmean(v):
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float('nan')


def figures(m):
    """The figures of ConfusionMatrix.result() from an int64 (C, C) array."""
    m = np.asarray(m, np.int64)
    inter = np.diag(m).astype(np.float64)
    tgt, prd = m.sum(axis=1).astype(np.float64), m.sum(axis=0).astype(np.float64)
    union, total = tgt + prd - inter, float(m.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = np.where(union > 0, inter / union, np.nan)
        recall = np.where(tgt > 0, inter / tgt, np.nan)
        pixel = inter.sum() / total if total > 0 else float('nan')
        fw = float(np.nansum(tgt * iou) / total) if total > 0 else float('nan')
    return {'IoU': 100. * iou, 'mIoU': 100. * _nanmean(iou), 'class_accuracy': 100. * recall, 'mean_class_accuracy': 100. * _nanmean(recall),
            'pixel_accuracy': 100. * float(pixel), 'fwIoU': 100. * fw, 'matrix': m}

"""Cross entropy, mIoU and accuracy of a weights file over a dataset split - counterpart of the reference's command_handlers/benchmark.py (same
`benchmark(...)` signature and figures).

What differs by design: the model runs `DSRL.predict` (the SSSR tail, the arg-max, the metric counters and the loss in one kernel; no logits in
memory), the batches come through the `loader_factory` protocol of train_or_resume (dataset['loader_factory'] when given, else the Cityscapes cache
without augmentation, every sample), and the host reads the device ONCE, after the last batch, instead of copying every batch's logits back.
`compiled_model=True` in other_args: `weights` names a file of the compile_model command and the batches run through inference.CompiledPredictor (the
full batch and the last short one are two of its graph keys); the figures are the same.
`flip=True` in other_args: every batch is evaluated as the horizontal-flip ensemble (`DSRL.predict(flip=True)`: the image and its mirror image, class
probabilities averaged); benchmark.txt then says so.
`scales=(0.5, 0.75, ...)` in other_args: every batch is evaluated as the multi-scale ensemble (`DSRL.predict(scales=...)`; combines with `flip`);
the value is validated before any device work, benchmark.txt names the scales and the view sizes, and with `compiled_model` the command raises
before it loads anything (graph replay of the multi-scale path is not built).
`ema=True` in other_args: `weights` names a checkpoint written with dataset['ema'] and its averaged weights ('ema_state_dict') are evaluated.
`sisr=True` in other_args: the super-resolution branch is measured too.  The model is built at stage 2 (a file without 'SISR_decoder' entries - a
stage-1 or pruned file - raises RuntimeError), every batch runs the backbone once and `DSRL.predict_head` and `DSRL.super_resolve_head` on its
features, and metrices.SRQuality compares the super-resolved image with the loader's original: the result gains 'PSNR' (dB, mean over the images)
and 'SSIM', benchmark.txt two lines; the records travel in the same single read.  Not with `flip`, `scales` or `compiled_model` (ValueError before
any device work): the SISR branch has no ensemble, and compiled files are stage-1.
`boundary=True` (ratio 0.02 of the image diagonal) or a positive ratio in other_args: every batch's class map - which every predict variant returns
anyway - also goes to `functional.boundary_counts_`, and the Boundary IoU counters (metrices.BoundaryIoU) ride in the same single read: the result
gains 'mBIoU_dataset' and 'BIoU_per_class', the per-class table of benchmark.txt a column and the file one summary line.  Combines with `flip`,
`scales`, `compiled_model`, `ema` and `sisr`; anything but True, False, None or a finite number > 0 is a ValueError before any device work.
`calibration=True` (15 bins) or a bin count in other_args: the kernel that writes every batch's class map also fills ONE reliability record over
the split (metrices.Calibration: the maximum softmax probability of every counted pixel binned against whether its class was right), which rides in
the same single read: the result gains 'ECE', 'MCE', 'mean_confidence' (fractions in [0, 1]) and 'reliability' (per bin: n, acc, conf),
benchmark.txt a reliability table and one summary line.  Combines with `flip`, `scales`, `ema`, `boundary` and `sisr`, not with `compiled_model`
(graphs are keyed on their outputs); anything but True, False, None or an integer from 1 to functional.calibration_max_bins() is a ValueError
before any device work.
`temperature=<number>`, `temperature=<path of a temperature.json>` (command_handlers.fit_temperature) or `temperature='fit'` in other_args:
temperature scaling - every batch is evaluated as `DSRL.predict(temperature=T)`, the model that reports softmax(logits / T).  'CE', 'ECE', 'MCE' and
'mean_confidence' are then those of the scaled model (the class maps and every figure counted from them do not change), the result gains
'temperature' and benchmark.txt one line naming T.  `'fit'` first fits T on the evaluated split itself (the two passes of fit_temperature), and
benchmark.txt says that the figure is in-sample.  Combines with `flip`, `ema`, `boundary`, `calibration` and `sisr`, not with `scales` or
`compiled_model`; a clash, a bad number or a file that is not a temperature.json is a ValueError before any device work.  Without the key the
command makes exactly the calls it makes without it.
`window=<side or (rows, columns)>` and optionally `stride=` in other_args, in pixels of `model_input_size`: sliding-window inference - every batch is
evaluated as `DSRL.predict(window=..., stride=...)`, overlapping windows of the training size whose class probabilities are averaged (a missing
stride is 2/3 of the window).  Validated against `model_input_size` before any device work; benchmark.txt gets one line naming the window, the
stride and the positions per axis.  Combines with `flip`, `ema`, `boundary`, `calibration` and `confusion`; with `scales`, `temperature`,
`compiled_model` or `sisr` it is a ValueError before any device work.  A window that is the whole input is "off".
Beside the reference's per-batch figures the command accumulates ONE confusion matrix over the split on the device (the kernel that writes the
class map fills it; it comes back in the same single read) and reports the dataset-level figures from it - intersections and unions summed over the
split, then IoU per class, then the mean over the classes, as Cityscapes results are published - with a per-class table in benchmark.txt and the
matrix itself in confusion_matrix.npy."""
import functools
import os
from datetime import datetime

import numpy as np
import torch as t

from .. import settings
from .._lib import DsrlHipError
from ..functional import (CALIBRATION_DEFAULT_BINS, boundary_counts_, boundary_distance, calibration_bins_value, multiscale_scales_value,
                          multiscale_sizes, nan_check_, temperature_value, window_plan, window_value)
from ..metrices import Accuracy, AverageMeter, BoundaryIoU, ConfusionMatrix, SRQuality, calibration_figures, mIoU
from ..models import DSRL
from ..utils import load_checkpoint_or_weights
from .train_or_resume import isCUDAdevice

NOT_GPU = "this build runs on the MI355X only: use device='gpu' (the reference's --device cpu path is its own)"


def load_eval_model(weights, dataset_settings, device_obj, ema=False, sisr=False):
    """Stage-1 DSRL in eval mode with the matching entries of the file's state dict (a stage-2/3 file carries more: strict=False, as the reference).
    `ema`: the averaged weights of a checkpoint written with dataset['ema'] (utils.load_checkpoint_or_weights).
    `sisr`: a stage-2 model, SISR decoder included; a file that does not carry the decoder raises RuntimeError naming the first missing key."""
    d = load_checkpoint_or_weights(weights, map_location='cpu', ema=ema)
    if d.get('format') is not None:
        raise RuntimeError(f"'{weights}' is a compiled model file (written by the compile_model command): pass compiled_model=True to read it")
    model = DSRL(stage=2 if sisr else 1, dataset_settings=dataset_settings).eval()
    loaded = model.load_state_dict(d['model_state_dict'], strict=False)
    missing = [k for k in loaded.missing_keys if k.startswith('SISR_decoder.')]
    if sisr and missing:
        raise RuntimeError(f"'{weights}' carries no '{missing[0]}': sisr=True needs a stage-2 or stage-3 weights file that was not pruned")
    return model.to(device_obj).to(memory_format=t.channels_last)


def split_loader(dataset, split, batch_size, device_obj, input_size):
    factory = dataset.get('loader_factory')
    if factory is None:
        os.makedirs(dataset['path'], exist_ok=True)
        if len(os.listdir(dataset['path'])) == 0:
            raise Exception("Cityscapes dataset was not found under '{:s}'.".format(dataset['path']))
        from ..datasets.Cityscapes.loader import loader_factory
        factory = loader_factory(dataset, input_size, settings.RANDOM_SEED)
    return factory(split, batch_size, device_obj, 0, 1)


def boundary_ratio_value(value):
    """other_args['boundary'] -> the band's share of the image diagonal, or None when the key is absent or off: True is the paper's 0.02, a finite
    number > 0 is itself; anything else is a ValueError"""
    if value is None or value is False:
        return None
    if value is True:
        return 0.02
    if isinstance(value, (int, float, np.integer, np.floating)):
        boundary_distance(1, 1, value)          # ValueError unless finite and > 0
        return float(value)
    raise ValueError(f'benchmark: boundary = {value!r} is neither True nor a positive ratio of the image diagonal')


def calibration_bins_arg(value):
    """other_args['calibration'] -> the bin count, or None when the key is absent or off: True is 15 bins, an integer from 1 to
    functional.calibration_max_bins() is itself; anything else is a ValueError"""
    if value is None or value is False:
        return None
    if value is True:
        return CALIBRATION_DEFAULT_BINS
    return calibration_bins_value(value, 'benchmark: calibration')


def temperature_arg(value):
    """other_args['temperature'] -> None when the key is absent, 'fit', or the temperature as a float: a number is itself (1 included: the model as
    it is), any other string names a temperature.json of fit_temperature, which is read here; anything else is a ValueError"""
    if value is None:
        return None
    if isinstance(value, (str, os.PathLike)):
        if value == 'fit':
            return 'fit'
        from .fit_temperature import read_temperature_file
        value = read_temperature_file(value)
    T = temperature_value(value, 'benchmark')
    return 1.0 if T is None else T


def benchmark(weights, dataset, device, num_workers, batch_size, **other_args):
    scales = multiscale_scales_value(other_args.get('scales'))          # ValueError on a bad value, before any device work
    boundary = boundary_ratio_value(other_args.get('boundary'))
    cal_bins = calibration_bins_arg(other_args.get('calibration'))
    temperature = temperature_arg(other_args.get('temperature'))
    if temperature is not None:
        clash = [k for k, on in (('scales', scales is not None), ('compiled_model', other_args.get('compiled_model'))) if on]
        if clash:
            raise ValueError(f"benchmark: temperature does not combine with {', '.join(clash)} (the multi-scale merge and compiled graphs take no temperature)")
    if cal_bins is not None and other_args.get('compiled_model'):
        raise ValueError('benchmark: calibration does not combine with compiled_model (compiled graphs are keyed on their outputs)')
    sisr = bool(other_args.get('sisr'))
    if sisr:
        clash = [k for k, on in (('flip', other_args.get('flip')), ('scales', scales is not None), ('compiled_model', other_args.get('compiled_model'))) if on]
        if clash:
            raise ValueError(f"benchmark: sisr=True does not combine with {', '.join(clash)} (the SISR branch has no ensemble; compiled files are stage-1)")
    window, positions = window_value(other_args.get('window'), other_args.get('stride')), None
    if window is not None:
        clash = [k for k, on in (('scales', scales is not None), ('temperature', temperature is not None), ('compiled_model', other_args.get('compiled_model')),
                                 ('sisr', sisr)) if on]
        if clash:
            raise ValueError(f"benchmark: window does not combine with {', '.join(clash)} (the windows run through the eager single-scale DSRL.predict)")
        size = tuple(other_args.get('model_input_size', settings.MODEL_INPUT_SIZE))
        positions = window_plan(size[0], size[1], *window)       # ValueError on a window the input cannot take; None: the whole input, "off"
        if positions is None:
            window = None
    if not isCUDAdevice(device):
        raise RuntimeError(NOT_GPU)
    if scales is not None and other_args.get('compiled_model'):
        from ..inference import MULTISCALE_NOT_COMPILED
        raise DsrlHipError(MULTISCALE_NOT_COMPILED)
    started = datetime.now()
    input_size = other_args.get('model_input_size', settings.MODEL_INPUT_SIZE)
    device_obj = t.device('cuda', t.cuda.current_device())
    ds = dataset['settings']
    split = dataset.get('split', 'val')
    predictor = None
    if other_args.get('compiled_model'):
        from ..inference import load_compiled_model
        model, predictor = load_compiled_model(weights, device_obj)          # frozen operands + hipGraph replay: the same class maps, counters and losses
    else:
        model = load_eval_model(weights, ds, device_obj, ema=other_args.get('ema', False), sisr=sisr)
    predict = model.predict if predictor is None else predictor
    flip = bool(other_args.get('flip'))
    if scales is not None:
        predict = functools.partial(predict, scales=scales)
    if window is not None:
        predict = functools.partial(predict, window=window[0], stride=window[1])
    fitted = None
    if temperature == 'fit':
        from .fit_temperature import fit_passes
        fitted = fit_passes(model, lambda: split_loader(dataset, split, batch_size, device_obj, input_size), ds.IGNORE_CLASS_LABEL, device_obj)
        temperature = fitted['temperature']
    temp_kw = {} if temperature is None or temperature == 1.0 else {'temperature': temperature}     # without the key: the calls of a command that does not know it
    loader = split_loader(dataset, split, batch_size, device_obj, input_size)

    nan_flag = t.zeros((), dtype=t.int32, device=device_obj)
    ces, tables = [], []
    nc = ds.NUM_CLASSES
    confusion = t.zeros(nc * nc, dtype=t.int64, device=device_obj)
    quality = SRQuality(ds.MEAN, ds.STD) if sisr else None
    band_counts = t.zeros(3 * nc, dtype=t.int64, device=device_obj) if boundary is not None else None
    band_distances = []
    cal_record = t.zeros(3 * cal_bins, dtype=t.int64, device=device_obj) if cal_bins is not None else None
    cal_kw = {} if cal_record is None else {'calibration': cal_record}          # without the key: the calls of a command that does not know it
    try:
        for (input_image, input_org), (target, _) in loader:
            if sisr:
                with t.no_grad():       # DSRL.predict with the trunk's features kept for the other branch
                    nan_check_(nan_flag, input_image)
                    features = model.feature_extractor['backbone'](input_image)
                    pred, counts, ce = model.predict_head(*features, target, ds.IGNORE_CLASS_LABEL, nan_flag, False, confusion, **cal_kw, **temp_kw)
                    quality.update(model.super_resolve_head(*features), input_org)
            else:
                pred, counts, ce = predict(input_image, target, ignore_index=ds.IGNORE_CLASS_LABEL, nan_flag=nan_flag, flip=flip, confusion=confusion,
                                          **cal_kw, **temp_kw)
            if boundary is not None:
                boundary_counts_(band_counts, pred, target, nc, ds.IGNORE_CLASS_LABEL, ratio=boundary, nan_flag=nan_flag)
                band_distances.append(boundary_distance(pred.shape[-2], pred.shape[-1], boundary))
            ces.append(ce)
            tables.append(counts)
        if not ces:
            raise RuntimeError(f"the '{split}' split yielded no batch")
        # the one device -> host read: losses, NaN flag, counters and the confusion matrix in a single float64 tensor (counters < 2^53: exact)
        nb = len(ces)
        parts = [t.stack(ces).double(), nan_flag.double().reshape(1), t.stack(tables).double().reshape(-1), confusion.double()]
        if boundary is not None:
            parts.append(band_counts.double())
        if sisr:
            parts += [b[0].reshape(-1) for b in quality.batches]
        if cal_record is not None:
            # n and hit are < 2^53; q (a sum of up to 2^24 per pixel) travels as its high and low 24-bit halves, each exact in float64
            q = cal_record[2 * cal_bins:]
            parts += [cal_record[:2 * cal_bins].double(), (q >> 24).double(), (q & 0xffffff).double()]
        host = t.cat(parts).cpu()
    finally:
        if predictor is not None:
            predictor.release()             # drops the graphs and restores the conv arithmetic the file selected
    bits = int(host[nb].item())
    if bits:
        raise RuntimeError('benchmark: ' + ' and '.join(m for b, m in ((1, 'NaN in the input or the logits'), (2, 'labels outside the classes')) if bits & b))
    CE_avg_loss = AverageMeter()
    miou, accuracy_mean = mIoU(num_classes=nc, ignore_index=ds.IGNORE_CLASS_LABEL), Accuracy(num_classes=nc, ignore_index=ds.IGNORE_CLASS_LABEL)
    host_tables = host[nb + 1:nb + 1 + nb * (3 * nc + 2)].reshape(nb, 3 * nc + 2).to(t.int64)
    for i in range(nb):
        CE_avg_loss.update(float(host[i]), batch_size)          # weighted by the nominal batch size, the last short batch included, as the reference
        miou.update_from_counts(host_tables[i])
        accuracy_mean.update_from_counts(host_tables[i])
    result = {'CE': CE_avg_loss(), 'mIoU': miou(), 'accuracy': accuracy_mean()}
    whole = ConfusionMatrix(nc, ds.IGNORE_CLASS_LABEL)
    at = nb + 1 + nb * (3 * nc + 2)
    whole.merge(host[at:at + nc * nc].to(t.int64))
    fig = whole.result()
    result.update({'mIoU_dataset': fig['mIoU'], 'IoU_per_class': [float(v) for v in fig['IoU']], 'pixel_accuracy': fig['pixel_accuracy'],
                   'mean_class_accuracy': fig['mean_class_accuracy'], 'fwIoU': fig['fwIoU'], 'confusion_matrix': fig['matrix'].tolist()})

    lines = ['Avg. Cross Entropy Error: {:.3f}'.format(result['CE']), 'mIoU %: {:.2f}'.format(result['mIoU']),
             'Mean Accuracy %: {:.2f}'.format(result['accuracy'])]
    names = list(getattr(ds, 'CLASS_NAMES', ()))
    names = [names[k] if k < len(names) else 'class {:d}'.format(k) for k in range(nc)]
    width = max(len(n) for n in names)
    lines += ['', 'Dataset-level mIoU %: {:.2f}'.format(result['mIoU_dataset']),
              'Dataset-level pixel accuracy %: {:.2f}, mean class accuracy %: {:.2f}, frequency-weighted IoU %: {:.2f}'.format(
                  result['pixel_accuracy'], result['mean_class_accuracy'], result['fwIoU']),
              '', '{:<{w}s}  {:>7s}  {:>8s}'.format('class', 'IoU %', 'recall %', w=width)]
    at += nc * nc
    if boundary is None:
        lines += ['{:<{w}s}  {:>7.2f}  {:>8.2f}'.format(n, i, r, w=width) for n, i, r in zip(names, fig['IoU'], fig['class_accuracy'])]
    else:
        band = BoundaryIoU(nc, ds.IGNORE_CLASS_LABEL, ratio=boundary)
        band.merge(host[at:at + 3 * nc].to(t.int64))
        at += 3 * nc
        bfig = band.result()
        result.update({'mBIoU_dataset': bfig['mBIoU'], 'BIoU_per_class': [float(v) for v in bfig['BIoU']]})
        lines[-1] += '  {:>15s}'.format('boundary IoU %')
        lines += ['{:<{w}s}  {:>7.2f}  {:>8.2f}  {:>15.2f}'.format(n, i, r, b, w=width)
                  for n, i, r, b in zip(names, fig['IoU'], fig['class_accuracy'], bfig['BIoU'])]
        lines.append('Dataset-level boundary mIoU %: {:.2f} (band of {:g} of the image diagonal: {:s} pixels)'.format(
            result['mBIoU_dataset'], boundary, ', '.join('{:d}'.format(d) for d in sorted(set(band_distances)))))
    if sisr:
        on_host = SRQuality()
        for records, C, H, W in quality.batches:
            on_host.update_from_records(host[at:at + records.numel()].reshape(-1, 2), C, H, W)
            at += records.numel()
        sr = on_host.result()
        result.update({'PSNR': sr['PSNR'], 'SSIM': sr['SSIM']})
        lines += ['Super-resolved image against the original, mean over {:d} images, PSNR dB: {:.2f}'.format(sr['images'], sr['PSNR']),
                  'Super-resolved image against the original, mean over {:d} images, SSIM: {:.4f}'.format(sr['images'], sr['SSIM'])]
    if cal_record is not None:
        B = cal_bins
        rec = host[at:at + 4 * B].to(t.int64)
        at += 4 * B
        cfig = calibration_figures(t.cat([rec[:2 * B], (rec[2 * B:3 * B] << 24) + rec[3 * B:]]))
        result.update({'ECE': cfig['ECE'], 'MCE': cfig['MCE'], 'mean_confidence': cfig['mean_confidence'],
                       'reliability': {'n': [int(v) for v in cfig['bins']['n']], 'acc': [float(v) for v in cfig['bins']['acc']],
                                       'conf': [float(v) for v in cfig['bins']['conf']]}})
        lines += ['', 'Reliability of the maximum softmax probability, {:d} bins over {:d} pixels'.format(B, cfig['pixels']),
                  '{:>15s}  {:>12s}  {:>10s}  {:>12s}'.format('confidence bin', 'pixels', 'accuracy', 'confidence')]
        lines += ['[{:5.3f}, {:5.3f}{:s}  {:>12d}  {:>10.4f}  {:>12.4f}'.format(b / B, (b + 1) / B, ']' if b == B - 1 else ')', int(n), a, c)
                  for b, (n, a, c) in enumerate(zip(cfig['bins']['n'], cfig['bins']['acc'], cfig['bins']['conf']))]
        lines.append('Expected calibration error: {:.4f}, maximum: {:.4f}, mean confidence: {:.4f} against accuracy {:.4f} ({:s})'.format(
            cfig['ECE'], cfig['MCE'], cfig['mean_confidence'], cfig['accuracy'],
            'over-confident' if cfig['gap'] > 0 else 'under-confident' if cfig['gap'] < 0 else 'no gap'))
    if temperature is not None:
        result['temperature'] = float(temperature)
        lines += ['', 'Temperature scaling: T = {:.4f}{:s}; cross entropy{:s} of softmax(logits / T)'.format(
            float(temperature),
            '' if fitted is None else ', fitted on this {:s} split itself (in-sample: NLL {:.4f} -> {:.4f} over {:d} pixels{:s})'.format(
                split, fitted['nll_before'], fitted['nll_after'], fitted['pixels'], ', at a bound of the search interval' if fitted['at_bound'] else ''),
            '' if cal_record is None else ', calibration errors and confidence')]
    print('-------- RESULTS --------')
    for ln in lines:
        print(ln)
    output_dir = other_args.get('output_dir', 'outputs')
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'benchmark.txt'), 'w') as f:
        f.write("Benchmarking results on the dataset's {:s} split\n\n".format(split))
        f.write('On: {:s}\n'.format(started.strftime('%c')))
        f.write('Weights file: {:s}\n'.format(str(weights)))
        if flip:
            f.write('Horizontal-flip ensemble: class probabilities of the image and its mirror image averaged\n')
        if scales is not None:
            f.write('Multi-scale ensemble: scales {:s} of the {:d} x {:d} input -> views of {:s}\n'.format(
                ', '.join('{:g}'.format(s) for s in scales), int(input_size[0]), int(input_size[1]),
                ', '.join('{:d} x {:d}'.format(h, w) for h, w in multiscale_sizes(input_size[0], input_size[1], scales))))
        if window is not None:
            f.write('Sliding-window ensemble: windows of {:d} x {:d} at stride {:d} x {:d} over the {:d} x {:d} input -> {:d} x {:d} positions, '
                    'class probabilities averaged where they overlap\n'.format(window[0][0], window[0][1], window[1][0], window[1][1], int(input_size[0]),
                                                                               int(input_size[1]), len(positions[0]), len(positions[1])))
        f.write('\n')
        f.write('\n'.join(lines) + '\n')
    np.save(os.path.join(output_dir, 'confusion_matrix.npy'), fig['matrix'])
    return result

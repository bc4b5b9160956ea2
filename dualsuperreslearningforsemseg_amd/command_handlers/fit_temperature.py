"""Temperature scaling (Guo et al. 2017), the fit: one scalar T for a weights file, fitted by minimising the NLL of softmax(logits / T) over a
held-out split.  `fit_temperature(...)` takes the arguments of `benchmark(...)` (the loader protocol, the model loading, `ema=True` honoured) and
returns {'temperature', 'beta' (= 1 / T), 'at_bound', 'nll_before' (T = 1), 'nll_after', 'pixels', 'passes'}; it writes `temperature.json` with the
same entries beside where benchmark writes benchmark.txt.  `benchmark(..., temperature=<that file>)` and `DSRL.predict(temperature=T)` apply it.

The fit takes two passes over the split, not one per optimiser iteration.  In each pass every batch's SSSR logits are written once
(`DSRL._eval_sssr_logits`) and one streaming kernel leaves the NLL with its first and second derivative in beta at 16 values of beta
(metrices.TemperatureFit, dsrl_temperature_stats); each pass ends with one device read.
    pass 1   16 log-spaced beta in [1/4, 4] -> the grid interval that brackets the root of dNLL/dbeta (the NLL is convex in beta)
    pass 2   16 linearly spaced beta across that bracket -> the root of the cubic Hermite interpolant of the derivative (functional.temperature_solve)
Pass 2 is skipped when pass 1 ends at a bound (T outside [1/4, 4]: the bound is reported, `at_bound` is True and `passes` is 1).
`nll_before`, the mean NLL at T = 1, and `nll_after`, at the fitted T, are not measured by a pass of their own: they are read off the cubic Hermite
interpolant of the NLL between the two grid points around them (the NLL sums as values, the derivative sums as slopes) - `nll_before` from pass 1,
whose grid is symmetric around beta = 1 in the logarithm, `nll_after` from the last pass."""
import json
import os

import torch as t

from .. import settings
from ..functional import temperature_bracket, temperature_grid, temperature_max_points, temperature_nll_at
from ..metrices import TemperatureFit, temperature_figures
from .benchmark import NOT_GPU, load_eval_model, split_loader
from .train_or_resume import isCUDAdevice

BETA_LO, BETA_HI = 0.25, 4.0            # pass 1: T in [1/4, 4]
FILE_NAME = 'temperature.json'


def fit_passes(model, batches, ignore_index, device_obj):
    """The two passes.  `batches()` -> a fresh iterable over the split per call, in the loader protocol ((image, _), (target, _)).  -> the result
    dict of fit_temperature.  A NaN logit or a label outside the classes raises RuntimeError after the pass that met it."""
    K = temperature_max_points()

    def one_pass(betas):
        fit = TemperatureFit(betas, ignore_index)
        flag = t.zeros((), dtype=t.int32, device=device_obj)
        seen = 0
        with t.no_grad():
            for (input_image, _), (target, _) in batches():
                fit.update_from_logits(model._eval_sssr_logits(input_image), target, nan_flag=flag)
                seen += 1
        if not seen:
            raise RuntimeError('fit_temperature: the split yielded no batch')
        host = t.cat([fit.record, flag.double().reshape(1)]).cpu()          # the one device read of the pass
        bits = int(host[-1].item())
        if bits:
            raise RuntimeError('fit_temperature: ' + ' and '.join(m for b, m in ((1, 'NaN in the logits'), (2, 'labels outside the classes')) if bits & b))
        return fit.betas, host[:-1].numpy()

    b1, r1 = one_pass(temperature_grid(BETA_LO, BETA_HI, K, log=True))
    fig = temperature_figures(b1, r1)
    if fig['pixels'] == 0:
        raise RuntimeError('fit_temperature: the split holds no labelled pixel')
    nll_before = temperature_nll_at(b1, r1, 1.0)
    passes, b, r = 1, b1, r1
    if not fig['at_bound']:
        i, _ = temperature_bracket(b1, r1)
        b, r = one_pass(temperature_grid(b1[i], b1[i + 1], K, log=False))
        fig = temperature_figures(b, r)
        passes = 2
    return {'temperature': float(fig['temperature']), 'beta': float(fig['beta']), 'at_bound': bool(fig['at_bound']), 'nll_before': float(nll_before),
            'nll_after': float(temperature_nll_at(b, r, fig['beta'])), 'pixels': int(fig['pixels']), 'passes': passes}


def read_temperature_file(path):
    """-> T of a temperature.json; ValueError when the file is not one"""
    try:
        with open(path) as f:
            d = json.load(f)
        return float(d['temperature'])
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise ValueError(f"'{path}' is not a temperature.json written by fit_temperature ({type(e).__name__}: {e})") from None


def fit_temperature(weights, dataset, device, num_workers, batch_size, **other_args):
    if not isCUDAdevice(device):
        raise RuntimeError(NOT_GPU)
    input_size = other_args.get('model_input_size', settings.MODEL_INPUT_SIZE)
    device_obj = t.device('cuda', t.cuda.current_device())
    ds = dataset['settings']
    split = dataset.get('split', 'val')
    model = load_eval_model(weights, ds, device_obj, ema=other_args.get('ema', False))
    result = fit_passes(model, lambda: split_loader(dataset, split, batch_size, device_obj, input_size), ds.IGNORE_CLASS_LABEL, device_obj)
    print('Temperature fitted on the {:s} split over {:d} pixels in {:d} pass{:s}: T = {:.4f}{:s}, NLL {:.4f} -> {:.4f}'.format(
        split, result['pixels'], result['passes'], '' if result['passes'] == 1 else 'es', result['temperature'],
        ' (at a bound of the search interval)' if result['at_bound'] else '', result['nll_before'], result['nll_after']))
    output_dir = other_args.get('output_dir', 'outputs')
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, FILE_NAME), 'w') as f:
        json.dump(dict(result, split=split, weights=str(weights)), f, indent=1)
        f.write('\n')
    return result

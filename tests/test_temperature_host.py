"""Host checks of temperature scaling: the reference restatement (tests/temperature_ref.py) against its own finite differences, the solver
(functional.temperature_solve / temperature_grid) on reference records against a float64 Newton solution, and every argument check that must
raise before any device work.  No GPU."""
import functools
import json

import numpy as np
import pytest
import torch

import temperature_ref as R

NC = 19


def _fit_case(T0, scale, C, P=20000, seed=1):
    """logits randn(P, C) * scale, labels drawn from softmax(logits / T0)"""
    rs = np.random.RandomState(seed + int(100 * T0) + C)
    z = rs.standard_normal((P, C)) * scale
    p = np.exp(z / T0 - (z / T0).max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    u = rs.uniform(size=(P, 1))
    labels = np.minimum((p.cumsum(1) < u).sum(1), C - 1).astype(np.uint8)
    return z, labels


@functools.lru_cache(maxsize=None)
def _fit_reference(T0, scale, C):
    z, labels = _fit_case(T0, scale, C)
    return z, labels, R.newton_beta(z, labels)


# ---------------------------------------------------------------------------------------------- the reference
def test_reference_derivatives_are_those_of_its_nll():
    """G and H of the reference are the first and second derivative of its L in beta: central differences of L and of G in float64.  Step h = 1e-5:
    truncation h^2 |L'''| / 6 ~ 1e-10 relative and rounding eps |L| / h ~ 1e-11 relative on sums of O(P) terms."""
    rs = np.random.RandomState(3)
    z = rs.standard_normal((500, NC)) * 3.0
    labels = rs.randint(0, NC, 500).astype(np.uint8)
    labels[::9] = 255
    rows, lab = R.live_rows(z, labels)
    assert rows.shape[0] == (labels != 255).sum()
    h = 1e-5
    for beta in (0.3, 1.0, 2.7):
        L, G, H = (x.sum() for x in R.terms(rows, lab, beta))
        Lp, Gp, _ = (x.sum() for x in R.terms(rows, lab, beta + h))
        Lm, Gm, _ = (x.sum() for x in R.terms(rows, lab, beta - h))
        assert abs((Lp - Lm) / (2 * h) - G) <= 1e-7 * max(abs(G), 1.0), beta
        assert abs((Gp - Gm) / (2 * h) - H) <= 1e-7 * abs(H), beta
        assert H > 0 and (R.terms(rows, lab, beta)[2] >= -1e-12).all()
    # the float32 restatement stays close to it, and the record lays the sums out as [n, (L, G, H) per beta]
    rec64, mag = R.record(z, labels, [0.5, 1.0])
    rec32, _ = R.record(z, labels, [0.5, 1.0], dtype=np.float32)
    assert rec64[0] == rec32[0] == rows.shape[0] and rec64.shape == (7,)
    assert np.array_equal(rec64[4:], [x.sum() for x in R.terms(rows, lab, 1.0)])
    assert (np.abs(rec32 - rec64)[1:] <= 1e-6 * mag[1:]).all() and (mag[1:] > 0).all()


# ---------------------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize('T0,scale,C', [(1, 3, 19), (2.5, 5, 19), (0.4, 2, 19), (1.7, 8, 2), (3.9, 4, 19)])
def test_two_passes_land_on_the_newton_solution(T0, scale, C):
    """Pass 1 (16 log-spaced beta in [1/4, 4]) within 5e-4 relative of the float64 Newton solution, pass 2 (16 linearly spaced beta across the bracket)
    within 1e-7 relative."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    z, labels, want = _fit_reference(T0, scale, C)
    assert abs(1.0 / want - T0) <= 0.05 * T0                   # the labels were drawn at T0: the fit finds it to sampling error
    b1 = HF.temperature_grid(0.25, 4.0, 16)
    assert b1.dtype == np.float64 and b1[0] == 0.25 and b1[-1] == 4.0 and np.array_equal(b1, b1.astype(np.float32).astype(np.float64))
    r1, _ = R.record(z, labels, b1)
    beta1, bound1 = HF.temperature_solve(b1, r1)
    assert not bound1
    e1 = abs(beta1 - want) / want
    i, at = HF.temperature_bracket(b1, r1)
    assert not at and b1[i] <= want <= b1[i + 1]
    b2 = HF.temperature_grid(b1[i], b1[i + 1], 16, log=False)
    r2, _ = R.record(z, labels, b2)
    beta2, bound2 = HF.temperature_solve(b2, r2)
    e2 = abs(beta2 - want) / want
    print(f'T0={T0} scale={scale} C={C}: newton beta {want:.12f}, pass 1 rel err {e1:.2e}, pass 2 rel err {e2:.2e}')
    assert not bound2 and e1 <= 5e-4 and e2 <= 1e-7
    # the NLL read off the interpolant: at a grid point its own value, between them close to the reference's
    rows, lab = R.live_rows(z, labels)
    n = rows.shape[0]
    assert HF.temperature_nll_at(b1, r1, b1[3]) == r1[1 + 9] / n
    assert abs(HF.temperature_nll_at(b1, r1, 1.0) - R.terms(rows, lab, 1.0)[0].sum() / n) <= 1e-4
    assert abs(HF.temperature_nll_at(b2, r2, beta2) - R.terms(rows, lab, beta2)[0].sum() / n) <= 1e-9
    assert np.isnan(HF.temperature_nll_at(b2, r2, 5.0))


def test_at_bound_at_both_ends_and_degenerate_records():
    from dualsuperreslearningforsemseg_amd import functional as HF
    z, labels, want = _fit_reference(1, 3, 19)             # beta close to 1
    low = HF.temperature_grid(0.05, 0.5, 8)                 # the minimum lies above the grid: G < 0 everywhere
    assert HF.temperature_solve(low, R.record(z, labels, low)[0]) == (0.5, True)
    high = HF.temperature_grid(2.0, 4.0, 8)                 # below it: G > 0 everywhere
    assert HF.temperature_solve(high, R.record(z, labels, high)[0]) == (2.0, True)
    assert HF.temperature_bracket(low, R.record(z, labels, low)[0]) == (7, True) and HF.temperature_bracket(high, R.record(z, labels, high)[0]) == (0, True)
    one = HF.temperature_grid(1.5, 1.5, 1)
    assert HF.temperature_solve(one, R.record(z, labels, one)[0]) == (1.5, True)
    # hand-made: G = beta - 1 exactly (H = 1): the root of the interpolant is 1
    b = np.array([0.5, 0.75, 1.25, 2.0])
    rec = np.concatenate([[10.0], np.stack([0.5 * (b - 1) ** 2, b - 1, np.ones(4)], 1).reshape(-1)])
    beta, at = HF.temperature_solve(b, rec)
    assert not at and abs(beta - 1.0) <= 1e-15
    assert abs(HF.temperature_nll_at(b, rec, 1.0)) <= 1e-16
    assert HF.temperature_solve(torch.tensor(b), torch.tensor(rec))[0] == beta          # tensors are read as they are
    with pytest.raises(ValueError, match='1 \\+ 3 K'):
        HF.temperature_solve(b, rec[:-1])
    with pytest.raises(ValueError, match='ascend'):
        HF.temperature_solve(b[::-1], rec)
    bad = rec.copy()
    bad[2] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        HF.temperature_solve(b, bad)


def test_figures_and_the_metric_class_on_the_host():
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.metrices import TemperatureFit, temperature_figures
    z, labels, want = _fit_reference(2.5, 5, 19)
    b = HF.temperature_grid(0.25, 4.0, 16)
    rec, _ = R.record(z, labels, b)
    f = temperature_figures(b, rec)
    assert set(f) == {'temperature', 'beta', 'at_bound', 'nll', 'betas', 'pixels'}
    assert f['pixels'] == 20000 and f['at_bound'] is False and f['temperature'] == 1.0 / f['beta'] and abs(f['beta'] - want) <= 5e-4 * want
    assert np.array_equal(f['nll'], rec[1::3] / 20000.0) and np.array_equal(f['betas'], b)
    fit = TemperatureFit(b)
    assert fit.ignore_index == 255 and np.array_equal(fit.betas, b)
    with pytest.raises(ValueError, match='before first use'):
        fit.record
    e = fit.result()
    assert e['pixels'] == 0 and np.isnan(e['temperature']) and np.isnan(e['nll']).all()
    fit.reset()
    fit.merge(torch.from_numpy(rec))
    fit.merge(fit.record.clone())
    g = fit.result()
    assert g['pixels'] == 40000 and g['beta'] == f['beta'] and np.allclose(g['nll'], f['nll'], rtol=1e-15)
    other = TemperatureFit(HF.temperature_grid(0.5, 2.0, 16))
    with pytest.raises(ValueError, match='different betas'):
        fit.merge(other)
    with pytest.raises(ValueError, match='49 elements'):
        fit.merge(torch.zeros(48, dtype=torch.float64))
    with pytest.raises(ValueError, match='49 elements'):
        fit.merge(torch.zeros(49, dtype=torch.float32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        TemperatureFit(b).update_from_logits(torch.zeros((1, NC, 4, 4)), torch.zeros((1, 4, 4), dtype=torch.uint8))
    for bad in ([], [1.0] * 17, [0.5, 0.0], [0.5, -1.0], [float('nan')], [float('inf')], 'abc', [1.0, 0.5], [1e-60]):
        with pytest.raises(ValueError):
            TemperatureFit(bad)


# ---------------------------------------------------------------------------------------------- argument checks, all before any device work
def test_temperature_value():
    from dualsuperreslearningforsemseg_amd.functional import temperature_beta, temperature_value as value
    assert value(None) is None and value(1) is None and value(1.0) is None and value(np.float32(1.0)) is None and value({}.get('temperature')) is None
    assert value(2) == 2.0 and type(value(2)) is float and value(0.5) == 0.5 and value(np.float64(1.7)) == 1.7 and value(np.int64(3)) == 3.0
    for bad in (0, 0.0, -1, -0.5, float('nan'), float('inf'), -float('inf'), True, False, '2', 'fit', (2.0,), [2.0], 1e-60, 1e60):
        with pytest.raises(ValueError, match='temperature'):
            value(bad, 'somewhere')
    assert temperature_beta(2.0) == 0.5 and temperature_beta(3.0) == float(np.float32(1.0 / 3.0))


def test_temperature_grid():
    from dualsuperreslearningforsemseg_amd import functional as HF
    assert HF.temperature_max_points() == 16
    g = HF.temperature_grid(0.25, 4.0, 16)
    assert g.shape == (16,) and (np.diff(g) > 0).all() and np.allclose(g[1:] / g[:-1], 16.0 ** (1 / 15), rtol=1e-6)
    assert abs(g[7] * g[8] - 1.0) <= 1e-6                  # symmetric around beta = 1 in the logarithm
    lin = HF.temperature_grid(1.0, 1.2, 5, log=False)
    assert np.allclose(lin, [1.0, 1.05, 1.1, 1.15, 1.2], rtol=1e-7) and np.array_equal(lin, lin.astype(np.float32).astype(np.float64))
    assert HF.temperature_grid(2.0, 2.0, 1).tolist() == [2.0]
    for lo, hi, K in ((0.25, 4.0, 0), (0.25, 4.0, 17), (0.25, 4.0, 16.0), (0.25, 4.0, True), (0.0, 4.0, 4), (-1.0, 4.0, 4), (4.0, 0.25, 4), (1.0, 1.0, 4),
                      (1.0, 2.0, 1), (float('nan'), 4.0, 4), (0.25, float('inf'), 4), ('a', 4.0, 4), (1.0, 1.0 + 1e-7, 16)):
        with pytest.raises(ValueError, match='temperature_grid'):
            HF.temperature_grid(lo, hi, K)


def test_stats_wrapper_refuses_before_the_device_check():
    from dualsuperreslearningforsemseg_amd import functional as HF
    L, tg = torch.zeros((1, NC, 4, 4)), torch.zeros((1, 4, 4), dtype=torch.uint8)
    for betas in ([], [1.0] * 17, [0.0], [-1.0], [float('nan')], [float('inf')]):
        with pytest.raises(ValueError, match='betas'):
            HF.temperature_stats_(torch.zeros(4, dtype=torch.float64), L, tg, betas)
    with pytest.raises(HF.DsrlHipError, match='7 elements'):
        HF.temperature_stats_(torch.zeros(4, dtype=torch.float64), L, tg, [0.5, 1.0])
    with pytest.raises(HF.DsrlHipError, match='7 elements'):
        HF.temperature_stats_(torch.zeros(7, dtype=torch.float32), L, tg, [0.5, 1.0])
    with pytest.raises(HF.DsrlHipError, match='4-D'):
        HF.temperature_stats_(torch.zeros(7, dtype=torch.float64), L[0], tg, [0.5, 1.0])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HF.temperature_stats_(torch.zeros(7, dtype=torch.float64), L, tg, [0.5, 1.0])
    # the size query and the point limit are host functions of the library
    q = HF.query
    assert q('dsrl_temperature_max_points') == 16
    assert q('dsrl_temperature_workspace_bytes', 265, 1) == 2 * 4 * 8 and q('dsrl_temperature_workspace_bytes', 265, 16) == 2 * 49 * 8
    assert q('dsrl_temperature_workspace_bytes', 10 ** 9, 16) == 1024 * 49 * 8
    assert q('dsrl_temperature_workspace_bytes', 0, 4) == 0 and q('dsrl_temperature_workspace_bytes', 100, 0) == 0 and q('dsrl_temperature_workspace_bytes', 100, 17) == 0


@pytest.mark.parametrize('value', [0, -2.0, float('nan'), float('inf'), True, (2.0,), [2.0]], ids=str)
def test_benchmark_refuses_a_bad_temperature_before_device_work(value, tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    asked = []
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda *a: asked.append(a) or []}
    with pytest.raises(ValueError, match='temperature'):
        benchmark(str(tmp_path / 'no.weights'), dataset, 'gpu', 0, 2, temperature=value, output_dir=str(tmp_path / 'out'))
    assert not asked and not (tmp_path / 'out').exists()


def test_benchmark_temperature_clashes_and_files(tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark, temperature_arg
    from dualsuperreslearningforsemseg_amd.command_handlers.fit_temperature import FILE_NAME, read_temperature_file
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    assert temperature_arg(None) is None and temperature_arg({}.get('temperature')) is None
    assert temperature_arg('fit') == 'fit' and temperature_arg(2) == 2.0 and temperature_arg(1) == 1.0 and temperature_arg(np.float32(0.5)) == 0.5
    good = tmp_path / FILE_NAME
    good.write_text(json.dumps({'temperature': 1.75, 'beta': 1 / 1.75}))
    assert FILE_NAME == 'temperature.json' and read_temperature_file(str(good)) == 1.75 and temperature_arg(str(good)) == 1.75 and temperature_arg(good) == 1.75
    asked = []
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda *a: asked.append(a) or []}
    kw = dict(output_dir=str(tmp_path / 'out'))
    for value in (2.0, 'fit', str(good)):
        with pytest.raises(ValueError, match='temperature does not combine with scales'):
            benchmark(str(tmp_path / 'no.weights'), dataset, 'gpu', 0, 2, temperature=value, scales=(0.5, 1.0), **kw)
        with pytest.raises(ValueError, match='temperature does not combine with compiled_model'):
            benchmark(str(tmp_path / 'no.weights'), dataset, 'gpu', 0, 2, temperature=value, compiled_model=True, **kw)
    # a file that is not there, is not JSON, or holds no (good) temperature
    (tmp_path / 'text.json').write_text('not json')
    (tmp_path / 'other.json').write_text(json.dumps({'T': 2.0}))
    (tmp_path / 'zero.json').write_text(json.dumps({'temperature': 0.0}))
    for name in ('missing.json', 'text.json', 'other.json', 'zero.json'):
        with pytest.raises(ValueError, match='temperature'):
            benchmark(str(tmp_path / 'no.weights'), dataset, 'gpu', 0, 2, temperature=str(tmp_path / name), **kw)
    # a good value gets as far as the device check (device='cpu' is refused there), "off" included
    for value in (2.0, 1, 'fit', str(good)):
        with pytest.raises(RuntimeError, match='MI355X only'):
            benchmark(str(tmp_path / 'no.weights'), dataset, 'cpu', 0, 2, temperature=value, **kw)
    assert not asked and not (tmp_path / 'out').exists()


def test_predict_refuses_bad_temperatures_and_scales_before_device_work():
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    model = DSRL(1, CS, init_weights=False).eval()
    x = torch.zeros(1, 3, 32, 32)
    for bad in (0, -1.0, float('nan'), float('inf'), True, '2'):
        with pytest.raises(ValueError, match='temperature'):
            model.predict(x, temperature=bad)
        with pytest.raises(ValueError, match='temperature'):
            model.predict_head(x, x, temperature=bad)
    with pytest.raises(ValueError, match='temperature does not combine with scales'):
        model.predict(x, temperature=2.0, scales=(0.5, 1.0))
    with pytest.raises(ValueError):
        model.predict(x, temperature=2.0, scales=(0.5, -1.0))          # a bad scale is refused as ever
    with pytest.raises(HF.DsrlHipError):
        model.predict(x, temperature=1.0, scales=(0.5, 1.0))           # 1 is "off": the multi-scale path, which wants a GPU tensor
    with pytest.raises(RuntimeError) as e:
        model.predict(x, temperature=2.0)                              # a good value gets as far as the device
    assert not isinstance(e.value, ValueError)
    # the tail wrapper and the logits kernel's wrapper: the value is checked first
    with pytest.raises(ValueError, match='temperature'):
        HF.sssr_tail_predict(x, None, None, None, temperature=-1.0)
    with pytest.raises(ValueError, match='temperature'):
        HF.calibration_counts_(torch.zeros(45, dtype=torch.int64), torch.zeros((1, NC, 4, 4)), torch.zeros((1, 4, 4), dtype=torch.uint8), temperature=0)


def test_compiled_predictor_refuses_the_keyword_first():
    """the check is the second statement of __call__ (behind the one on calibration / confidence): before the frozen-operand check and any device work"""
    import inspect
    from dualsuperreslearningforsemseg_amd.inference import CompiledPredictor
    sig = inspect.signature(CompiledPredictor.__call__)
    assert sig.parameters['temperature'].default is None
    body = inspect.getsource(CompiledPredictor.__call__).split('):', 1)[1].strip().splitlines()
    assert 'temperature_value(temperature' in body[3] and 'raise ValueError' in body[5]
    fake = object.__new__(CompiledPredictor)               # no frozen operands: the keyword is refused before anything is looked at
    with pytest.raises(ValueError, match='temperature'):
        fake(None, temperature=2.0)
    with pytest.raises(ValueError, match='temperature'):
        fake(None, temperature=-1.0)

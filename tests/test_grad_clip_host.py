"""The host side of gradient-norm clipping, without a GPU: the dataset['grad_clip'] parser, the record's host form, and the numpy
reference (tests/grad_clip_ref.py) against torch.nn.utils.clip_grad_norm_ on CPU tensors."""
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as R

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ dataset['grad_clip']
@pytest.mark.parametrize('given,expected', [
    (None, None), (False, None), (np.bool_(False), None),
    (1.0, 1.0), (1, 1.0), (0.25, 0.25), (np.float32(0.5), 0.5), (np.int64(3), 3.0), (1e-30, 1e-30), (float('inf'), float('inf')),
    ({'max_norm': 2.0}, 2.0), ({'max_norm': float('inf')}, float('inf')), ({'max_norm': np.float32(0.5)}, 0.5),
])
def test_grad_clip_value_accepts(given, expected):
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import check_grad_clip
    got = HF.grad_clip_value(given)
    assert got == expected and (got is None or type(got) is float)
    assert check_grad_clip({'grad_clip': given}) == expected
    assert check_grad_clip({}) is None


@pytest.mark.parametrize('given', [
    True, np.bool_(True), 0, 0.0, -0.0, -1.0, -float('inf'), float('nan'), 1e-60,       # a bool for the threshold; <= 0 (also once rounded to fp32); NaN
    {}, {'max_norm': 1.0, 'norm_type': 2}, {'norm': 1.0}, {'max_norm': True}, {'max_norm': 0}, {'max_norm': None}, {'max_norm': float('nan')},
    '1.0', (1.0,), [1.0], object(),
])
def test_grad_clip_value_refuses(given):
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import check_grad_clip
    with pytest.raises(ValueError):
        HF.grad_clip_value(given)
    with pytest.raises(ValueError):
        check_grad_clip({'grad_clip': given})


def test_train_or_resume_refuses_a_bad_grad_clip_before_any_device_work(tmp_path, monkeypatch):
    """A bad dataset['grad_clip'] ends train_or_resume with a ValueError before the device is selected, a model built or a directory made."""
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as T
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs

    def touched(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    monkeypatch.setattr(torch.cuda, 'current_device', touched)
    monkeypatch.setattr(T, 'DSRL', touched)
    kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
              dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': touched, 'grad_clip': -1.0}, val_interval=1, checkpoint_interval=1,
              checkpoint_history=2, init_weights=None, batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9,
              weights_decay=5e-4, poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / 'exp'),
              description='test', early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))
    with pytest.raises(ValueError, match='grad_clip'):
        T.train_or_resume(is_resuming_training=False, **kw)
    assert not (tmp_path / 'exp').exists() and not (tmp_path / 'data').exists()


def test_record_host_form():
    from dualsuperreslearningforsemseg_amd import functional as HF
    for m in (1.0, 0.1, float('inf'), 3.5e10):
        rec = HF.grad_clip_record(m, 'cpu')
        assert rec.dtype == torch.int32 and rec.numel() == HF.GRAD_CLIP_RECORD_WORDS == 16
        assert HF.grad_clip_record_read(rec) == R.new_record(m)
    w = np.zeros(16, np.int32)
    w[:4] = np.array([6.25, 7.5], F64).view(np.int32)
    w[4:8] = np.array([2.5, 0.4, 1.0, 3.0], F32).view(np.int32)
    w[8:11] = np.array([5, 2, 1], np.uint32).view(np.int32)
    assert HF.grad_clip_record_read(torch.from_numpy(w)) == {'sumsq': 6.25, 'norm_sum': 7.5, 'norm': 2.5, 'coef': float(F32(0.4)), 'max_norm': 1.0,
                                                             'norm_max': 3.0, 'steps': 5, 'clipped': 2, 'nonfinite': 1}


# ------------------------------------------------------------------------------------------------ the reference against torch
def _params(rs, scale):
    shapes = [(3, 5, 7), (1030,), (64, 33), (1,), (2, 1025)]
    return [(scale * rs.standard_normal(s)).astype(F32) for s in shapes]


@pytest.mark.parametrize('case,scale,max_norm', [('below', 1e-3, 1.0), ('above', 3.0, 1.0), ('above-small-threshold', 1.0, 0.01), ('zero', 0.0, 1.0)])
def test_reference_coefficient_matches_torch(case, scale, max_norm):
    """S, norm and coef of the reference on the flat arena against clip_grad_norm_ over the per-parameter tensors: the norm torch returns within
    float32 rounding of its own accumulation (n 2^-24 is far above what it shows; 1e-5 relative is asserted), and the clipped gradients - torch
    multiplies by its float32 coefficient only when it is below 1 - within 2 float32 ulps of g * reference coefficient."""
    rs = np.random.RandomState(len(case))
    gs_np = _params(rs, scale)
    flat = np.concatenate([g.ravel() for g in gs_np])
    S = R.total(R.tile_sums(flat))
    norm, coef = R.norm_coef(S, 1.0, max_norm)
    assert math.isclose(float(S), float((flat.astype(F64) ** 2).sum()), rel_tol=1e-13)
    ps = [torch.nn.Parameter(torch.zeros(g.shape)) for g in gs_np]
    for p, g in zip(ps, gs_np):
        p.grad = torch.from_numpy(g.copy())
    tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    assert abs(tn - float(norm)) <= 1e-5 * float(norm) + 1e-30, (tn, float(norm))
    if case == 'below' or case == 'zero':
        assert coef == 1.0 and R.grad_scale(1.0, coef) == F32(1.0)
        for p, g in zip(ps, gs_np):
            assert np.array_equal(p.grad.numpy(), g)
    else:
        assert coef < 1.0
        want = max_norm / (tn + 1e-6)
        assert abs(float(coef) - want) <= 1e-5 * want
        k = R.grad_scale(1.0, coef)
        for p, g in zip(ps, gs_np):
            ref = g.astype(F64) * F64(k)
            assert (np.abs(p.grad.numpy().astype(F64) - ref) <= 2 * 2.0 ** -23 * np.abs(ref) + 1e-45).all()
        clipped = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in ps))
        assert abs(clipped - max_norm) <= 1e-4 * max_norm


def test_reference_nonfinite_and_running_fields():
    """NaN stays NaN through the clamp, an infinite norm gives 0, inf / inf NaN (torch's clamp(max=1) on the same values); the running fields."""
    for S, m, want in ((float('nan'), 1.0, float('nan')), (float('inf'), 1.0, 0.0), (float('inf'), float('inf'), float('nan')), (4.0, float('inf'), 1.0)):
        coef = float(R.norm_coef(S, 1.0, m)[1])
        t = float(torch.clamp(torch.tensor(m, dtype=torch.float64) / (torch.tensor(S, dtype=torch.float64).sqrt() + 1e-6), max=1.0))
        assert (math.isnan(coef) and math.isnan(want) and math.isnan(t)) or coef == want == t, (S, m, coef, t)
    rec = R.new_record(1.0)
    rec, k1 = R.record_step(rec, 0.25, 1.0)           # norm 0.5: not clipped
    rec, k2 = R.record_step(rec, 16.0, 0.5)           # norm 2: clipped
    rec, k3 = R.record_step(rec, float('nan'), 1.0)
    rec, k4 = R.record_step(rec, float('inf'), 1.0)
    assert k1 == F32(1.0) and abs(float(k2) - 0.25) < 1e-6 and np.isnan(k3) and k4 == 0.0
    assert rec['steps'] == 4 and rec['clipped'] == 1 and rec['nonfinite'] == 2 and rec['norm_sum'] == 2.5 and rec['norm_max'] == 2.0
    assert rec['coef'] == 0.0 and rec['norm'] == float('inf') and rec['max_norm'] == 1.0

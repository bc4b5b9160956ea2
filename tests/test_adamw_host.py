"""AdamW without a device: tests/adamw_ref.py against torch.optim.AdamW, the accepted values of dataset['optimizer'], the
state_dict layout of ddp.FlatParams with AdamW enabled, and the refusal of the other optimiser's state."""
import math

import numpy as np
import pytest
import torch

import adamw_ref as R

F32, F64 = np.float32, np.float64


def _torch_adamw(inputs, hyper, steps, dtype, **kw):
    """`steps` steps of torch.optim.AdamW from the state (m, v, t - 1) on the constant gradient g * grad_scale -> [(p, m, v) after each]"""
    lr, b1, b2, eps, wd, gs, t = hyper
    p, g, m, v = (torch.from_numpy(np.asarray(a)).to(dtype) for a in inputs)
    param = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([param], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, **kw)
    sd = opt.state_dict()
    sd['state'] = {0: {'step': torch.tensor(float(t - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}}
    opt.load_state_dict(sd)
    out = []
    for _ in range(steps):
        param.grad = g * torch.tensor(gs, dtype=dtype)
        opt.step()
        st = opt.state[param]
        out.append(tuple(a.detach().numpy().copy() for a in (param, st['exp_avg'], st['exp_avg_sq'])))
    return out


# 2 x the largest gap measured below (1.77e-8, 4.65e-9 and 4.98e-9 u S on p, m and v after three steps: float64 rounding noise, 2^-53 / 2^-24 =
# 1.9e-9 per rounding, carried from step to step)
F64_GAP = (3.6e-8, 9.3e-9, 1.0e-8)


def test_ref_float64_against_torch_float64():
    """Three steps of the float64 restatement against torch.optim.AdamW(foreach=False) in float64, on every case: the gap, in the units of u S with
    u = 2^-24, is float64 rounding noise."""
    inputs = R.random_state(20000, 3)
    gap = [0.0, 0.0, 0.0]
    for hyper in R.CASES:
        lr, b1, b2, eps, wd, gs, t = hyper
        want = _torch_adamw(inputs, hyper, 3, torch.float64, foreach=False)
        p, g, m, v = (a.astype(F64) for a in inputs)
        for k in range(3):
            h = (lr, b1, b2, eps, wd, gs, t + k)
            s = R.scales(p, g, m, v, *h[-1:], *h[:-1])
            p, m, v = R.adamw_step(p, g, m, v, t + k, lr, b1, b2, eps, wd, gs, F64)
            for i, (a, b, sc) in enumerate(zip((p, m, v), want[k], s)):
                gap[i] = max(gap[i], R.worst(a, b, sc))
    print('float64 restatement against torch float64, u S units (p, m, v):', ['%.3g' % x for x in gap])
    assert all(x <= bound for x, bound in zip(gap, F64_GAP)), gap


def test_float32_restatement_and_torch_float32_errors():
    """The float32 restatement on one step of 10^6 elements: its worst errors are those of a handful of roundings (p: decay, lerp, moments, square
    root, division, sum, update: < 8; m: difference, product, sum: < 2; v: two products, sum, square: < 3), and torch's own float32 AdamW is no
    further from float64 on p than that."""
    inputs = R.random_state(10 ** 6, 1)
    top = [0.0, 0.0, 0.0]
    top_torch = 0.0
    for hyper in R.CASES:
        lr, b1, b2, eps, wd, gs, t = hyper
        e = R.errors(R.adamw_step(*inputs, t, lr, b1, b2, eps, wd, gs, F32), inputs, hyper)
        top = [max(a, b) for a, b in zip(top, e)]
        got = _torch_adamw(inputs, hyper, 1, torch.float32, foreach=False)[0]
        # (torch multiplies the gradient tensor by grad_scale in float32 too: the same inputs)
        top_torch = max(top_torch, R.errors(got, inputs, hyper)[0])
    print('float32 restatement, worst errors in u S (p, m, v):', ['%.2f' % x for x in top], ' torch float32 AdamW on p: %.2f' % top_torch)
    assert top[0] < 8 and top[1] < 2 and top[2] < 3, top
    assert top_torch < 8, top_torch


def test_zero_elements_are_exact_in_the_restatement():
    p, g, m, v = (np.array(a, F32) for a in ([1.5, -2.0, 0.0], [0, 0, 0], [0, 0, 0], [0, 0, 0]))
    for dt in (F32, F64):
        p1, m1, v1 = R.adamw_step(p, g, m, v, 3, 1e-3, .9, .999, 1e-8, 1e-2, 1.0, dt)
        assert np.array_equal(p1, p.astype(dt) * dt(1 - 1e-3 * 1e-2)) and not m1.any() and not v1.any()
        p1, _, _ = R.adamw_step(p, g, m, v, 3, 1e-3, .9, .999, 1e-8, 0.0, 1.0, dt)
        assert np.array_equal(p1, p.astype(dt))


# ------------------------------------------------------------------------------------------------ dataset['optimizer']
GOOD = [(None, None), ('sgd', None), ({'name': 'sgd'}, None), ('adamw', (0.9, 0.999, 1e-8)), ({'name': 'adamw'}, (0.9, 0.999, 1e-8)),
        ({'name': 'adamw', 'betas': (0.8, 0.99), 'eps': 1e-6}, (0.8, 0.99, 1e-6)), ({'name': 'adamw', 'betas': [0, 0]}, (0.0, 0.0, 1e-8)),
        ({'name': 'adamw', 'eps': 0}, (0.9, 0.999, 0.0)), ({'name': 'adamw', 'betas': (np.float32(0.5), 0.25)}, (0.5, 0.25, 1e-8))]
BAD = ['adam', 'AdamW', '', 0, True, ('adamw',), {'betas': (0.9, 0.999)}, {'name': 'lamb'}, {'name': 'sgd', 'eps': 1e-8}, {'name': 'adamw', 'lr': 1e-3},
       {'name': 'adamw', 'amsgrad': False}, {'name': 'adamw', 'betas': (0.9, 1.0)}, {'name': 'adamw', 'betas': (-0.1, 0.9)},
       {'name': 'adamw', 'betas': (0.9, 1 - 1e-12)},           # 1 as fp32
       {'name': 'adamw', 'betas': (float('nan'), 0.9)}, {'name': 'adamw', 'betas': 0.9}, {'name': 'adamw', 'betas': (0.9, 0.99, 0.999)},
       {'name': 'adamw', 'betas': (True, 0.9)}, {'name': 'adamw', 'betas': ('0.9', 0.9)}, {'name': 'adamw', 'eps': -1e-8},
       {'name': 'adamw', 'eps': float('nan')}, {'name': 'adamw', 'eps': float('inf')}, {'name': 'adamw', 'eps': None}, {'name': 'adamw', 'eps': False}]


def test_adamw_value_and_check_optimizer(monkeypatch):
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import check_optimizer

    def no_device(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'call', no_device)
    monkeypatch.setattr(HF, 'call', no_device)
    assert check_optimizer({}) is None
    for spec, want in GOOD:
        assert HF.adamw_value(spec) == want, spec
        assert check_optimizer({'optimizer': spec}) == want, spec
    for spec in BAD:
        with pytest.raises(ValueError):
            HF.adamw_value(spec)
        with pytest.raises(ValueError):
            check_optimizer({'optimizer': spec})


def test_train_or_resume_rejects_a_bad_optimizer_before_any_work(tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import train_or_resume
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    with pytest.raises(ValueError, match='optimizer'):
        train_or_resume(False, 'gpu', None, None, False, 0, {'path': str(tmp_path), 'settings': cs, 'optimizer': 'adam'}, 1, 1, 1, None, 2, 1, 0.01, 0.001,
                        0.9, 5e-4, 0.9, 3, 0.1, 1.0, False, str(tmp_path / 'exp'), 'test', False)
    assert not (tmp_path / 'exp').exists()


# ------------------------------------------------------------------------------------------------ FlatParams on a CPU model
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, bias=True)
        self.bn = torch.nn.BatchNorm2d(8)
        self.fc = torch.nn.Linear(8, 2)


def _tiny():
    from dualsuperreslearningforsemseg_amd import ddp
    torch.manual_seed(5)
    model = _Tiny().to(memory_format=torch.channels_last)
    return model, ddp.FlatParams(model)


def test_record_layout_on_the_host():
    from dualsuperreslearningforsemseg_amd import functional as HF
    rec = HF.adamw_record(0.9, 0.999, 1e-8, 'cpu')
    assert rec.dtype == torch.int32 and rec.numel() == 16
    w = rec.numpy()
    assert np.array_equal(w[:3].view(F32), np.array([0.9, 0.999, 1e-8], F32))
    assert np.array_equal(w[5:7].view(F32), np.array([1 - 0.9, 1 - 0.999], F32))           # of the double difference: 1 - float32(0.999) is 4.7e-5 off
    assert w[5:7].view(F32)[1] != F32(1) - F32(0.999)
    assert np.array_equal(w[10:14].view(F64), np.array([0.9, 0.999])) and not w[3:5].any() and not w[7:10].any() and not w[14:].any()
    assert HF.adamw_record_read(rec) == {'beta1': 0.9, 'beta2': 0.999, 'eps': float(F32(1e-8)), 'ss_factor': 0.0, 'isq': 0.0, 't': 0}


def test_state_dict_layout_is_torch_adamw():
    """FlatParams.state_dict() with AdamW enabled loads into a CPU torch.optim.AdamW over the model's parameters, as does a hand-built dict of the
    documented shape; the tensors are the arenas' in logical NCHW shape."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    model, flat = _tiny()
    flat.enable_adamw((0.8, 0.99), 1e-6)
    with pytest.raises(HF.DsrlHipError):
        flat.enable_adamw()
    assert flat.v_flat.shape == flat.p_flat.shape and not flat.v_flat.any() and not flat.m_flat.any()
    assert flat.v_flat.data_ptr() % 16 == 0 and flat.adamw_step_count() == 0
    with torch.no_grad():
        flat.m_flat.copy_(torch.arange(flat.numel, dtype=torch.float32))
        flat.v_flat.copy_(torch.arange(flat.numel, dtype=torch.float32) * 2)
    sd = flat.state_dict(lr=0.01, momentum=0.9, weight_decay=0.05, initial_lr=0.02)
    ps = [p for p in model.parameters() if p.requires_grad]
    assert list(sd) == ['state', 'param_groups'] and len(sd['param_groups']) == 1 and sorted(sd['state']) == list(range(len(ps)))
    group = sd['param_groups'][0]
    fresh = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=0.01, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)
    assert set(group) == set(fresh.state_dict()['param_groups'][0]) | {'initial_lr'}
    assert (group['lr'], group['betas'], group['eps'], group['weight_decay'], group['amsgrad']) == (0.01, (0.8, 0.99), 1e-6, 0.05, False)
    assert group['params'] == list(range(len(ps))) and 'momentum' not in group
    for i, p in enumerate(ps):
        st = sd['state'][i]
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and st['step'].dtype == torch.float32 and st['step'].dim() == 0 and float(st['step']) == 0.0
        o = flat.offsets[flat._index[id(p)]]
        for key, arena in (('exp_avg', flat.m_flat), ('exp_avg_sq', flat.v_flat)):
            assert tuple(st[key].shape) == tuple(p.shape) and st[key].is_contiguous() and st[key].device.type == 'cpu'
            assert torch.equal(st[key], arena.as_strided(p.shape, p.stride(), o))
    assert tuple(sd['state'][0]['exp_avg'].shape) == (8, 3, 3, 3)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.state[fresh.param_groups[0]['params'][0]]['exp_avg'], sd['state'][0]['exp_avg'])
    # a hand-built dict of the documented shape
    hand = {'state': {i: {'step': torch.tensor(4.0), 'exp_avg': torch.zeros(p.shape), 'exp_avg_sq': torch.ones(p.shape)} for i, p in enumerate(ps)},
            'param_groups': [{'lr': 0.01, 'betas': (0.8, 0.99), 'eps': 1e-6, 'weight_decay': 0.05, 'amsgrad': False,
                              **{k: v for k, v in fresh.state_dict()['param_groups'][0].items()
                                 if k not in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params')}, 'params': list(range(len(ps)))}]}
    fresh.load_state_dict(hand)
    fresh.zero_grad()
    for p in fresh.param_groups[0]['params']:
        p.grad = torch.ones_like(p)
    fresh.step()
    assert float(fresh.state[fresh.param_groups[0]['params'][0]]['step']) == 5.0


def test_state_mix_ups_raise():
    from dualsuperreslearningforsemseg_amd import ddp
    model, flat = _tiny()
    sgd_state = flat.state_dict(0.1, 0.9, 0.0)
    assert ddp.optimizer_state_kind(sgd_state) == 'sgd'
    model2, flat2 = _tiny()
    flat2.enable_adamw()
    adamw_state = flat2.state_dict(0.1, 0.9, 0.0)
    assert ddp.optimizer_state_kind(adamw_state) == 'adamw' and ddp.optimizer_state_kind({'state': {}, 'param_groups': []}) is None
    with pytest.raises(ValueError, match=r'(?s)SGD.*AdamW'):
        flat2.load_state_dict(sgd_state)
    with pytest.raises(ValueError, match=r'(?s)AdamW.*SGD'):
        flat.load_state_dict(adamw_state)
    with pytest.raises(ValueError, match=r'(?s)SGD.*AdamW'):
        flat2.load_state_dict({'momentum_arena': flat.m_flat, 'numel': flat.numel})
    assert not flat2.m_flat.any() and not flat2.v_flat.any()
    flat.load_state_dict(sgd_state)                     # its own state still loads
    # differing step counts cannot be one arena's
    bad = {'state': {k: dict(v) for k, v in adamw_state['state'].items()}, 'param_groups': adamw_state['param_groups']}
    bad['state'][1]['step'] = torch.tensor(3.0)
    with pytest.raises(ValueError, match='step'):
        flat2.load_state_dict(bad)
    assert math.isclose(float(adamw_state['state'][0]['step']), 0.0)

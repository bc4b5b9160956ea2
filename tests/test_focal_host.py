"""Host side of the focal cross entropy: what a gamma may be, what train_or_resume accepts as dataset['focal_gamma'], the five entry points in
the header and the ctypes table, and the float64 restatement the GPU tests compare with (tests/focal_ref.py) - nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as FR

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS

ENTRY_POINTS = ['dsrl_ce_fwd_f', 'dsrl_ce_bwd_f', 'dsrl_ce_fused_f', 'dsrl_convt2x2_fwd_ce_f', 'dsrl_convt2x2_bwd_ce_f']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsrl_hip.h')


@pytest.mark.parametrize('value,want', [(0, 0.0), (0.0, 0.0), (2, 2.0), (0.5, 0.5), (np.float32(1.5), 1.5), (np.int64(5), 5.0)])
def test_focal_gamma_value_accepts(value, want):
    got = HF.focal_gamma_value(value)
    assert type(got) is float and got == want


@pytest.mark.parametrize('value', [True, False, np.True_, '2', None, [2.0], float('nan'), float('inf'), -float('inf'), -1e-9, -2, 1e39])
def test_focal_gamma_value_rejects(value):
    with pytest.raises(ValueError):
        HF.focal_gamma_value(value)


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


def test_check_focal_gamma():
    assert TR.check_focal_gamma(_dataset()) == 0.0
    assert TR.check_focal_gamma(_dataset(focal_gamma=None)) == 0.0
    assert TR.check_focal_gamma(_dataset(focal_gamma=0)) == 0.0
    assert TR.check_focal_gamma(_dataset(focal_gamma=2)) == 2.0
    assert TR.check_focal_gamma(_dataset(focal_gamma=0.5)) == 0.5
    for bad in (True, 'two', float('nan'), float('inf'), -1.0, [2.0]):
        with pytest.raises(ValueError):
            TR.check_focal_gamma(_dataset(focal_gamma=bad))


@pytest.mark.parametrize('value', [-1.0, float('nan'), 'two', True])
def test_train_or_resume_refuses_a_bad_gamma_before_touching_a_device(value):
    args = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=_dataset(focal_gamma=value, loader_factory=lambda *a: []), val_interval=1, checkpoint_interval=1, checkpoint_history=1,
                init_weights=None, batch_size=1, epochs=1, learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4,
                poly_power=0.9, stage=1, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)
    with pytest.raises(ValueError, match='focal_gamma'):
        TR.train_or_resume(**args)


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_is_declared_and_registered(name):
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', text)
    assert m, f'{name} is not declared in include/dsrl_hip.h'
    params = [p.strip() for p in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
    k = [i for i, p in enumerate(params) if re.search(r'\bweights$', p)]
    assert k and params[k[0] + 1] == 'float gamma', f'{name}: `float gamma` does not follow `weights` ({params})'
    assert name in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[name]
    assert len(args) == len(params), f'{name}: {len(params)} parameters declared, {len(args)} registered'
    sib = _lib.PROTOTYPES[name[:-2] + '_w']                     # its _w sibling plus one float after the weights
    assert res is sib[0] and len(args) == len(sib[1]) + 1
    i = next(i for i in range(len(args)) if i >= len(sib[1]) or args[i] is not sib[1][i])
    assert args[:i] + args[i + 1:] == sib[1] and args[i] is _lib.f32


def _graded(C, seed, P=1000, ii=255):
    rs = np.random.RandomState(seed)
    lg, tg = FR.make_graded(P, C, rs, ii)
    w = rs.uniform(0.25, 8.0, C).astype(np.float32)
    w[rs.randint(C)] = 0.0
    return lg, tg, w


@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('gamma', [0.5, 1.0, 2.0, 5.0])
def test_closed_form_gradient_equals_autograd_on_graded(C, gamma):
    lg, tg, w = _graded(C, 40 + C)
    assert (FR.target_probability(lg, tg, 255) < 1.0).all()     # no pixel with q == 0: autograd is usable here
    L, g, D = FR.focal_loss_and_grad(lg, tg, 255, w, gamma)
    La, ga = FR.focal_autograd(lg, tg, 255, w, gamma)
    assert abs(L - La) <= 1e-12 * abs(La)
    assert np.all(g[tg == 255] == 0)
    assert np.abs(g - ga).max() <= 1e-12, np.abs(g - ga).max()


@pytest.mark.parametrize('C', [19, 3])
def test_graded_case_has_a_middle_and_moves_the_loss(C):
    for seed in (1, 2, 3):
        lg, tg, w = _graded(C, seed)
        p = FR.target_probability(lg, tg, 255)
        frac = float(((p > 0.1) & (p < 0.9)).mean())
        assert frac >= 0.25, frac
        ce = FR.focal_loss_and_grad(lg, tg, 255, w, 0.0)[0]
        fl = FR.focal_loss_and_grad(lg, tg, 255, w, 2.0)[0]
        assert abs(fl - ce) > 0.05 * abs(ce), (fl, ce)


@pytest.mark.parametrize('C', [19, 3])
def test_gamma_to_zero_is_the_weighted_cross_entropy(C):
    lg, tg, w = _graded(C, 7 + C)
    x = torch.tensor(lg.astype(np.float64), requires_grad=True)
    ref = F.cross_entropy(x, torch.tensor(tg.astype(np.int64)), weight=torch.tensor(w.astype(np.float64)), ignore_index=255)
    ref.backward()
    ref = ref.detach()
    L0, g0, _ = FR.focal_loss_and_grad(lg, tg, 255, w, 0.0)
    assert abs(L0 - float(ref)) <= 1e-12 * abs(float(ref))
    assert np.abs(g0 - x.grad.numpy()).max() <= 1e-12
    Le, ge, _ = FR.focal_loss_and_grad(lg, tg, 255, w, 1e-9)    # and continuously so
    assert abs(Le - float(ref)) <= 1e-7 * abs(float(ref)) and np.abs(ge - x.grad.numpy()).max() <= 1e-7


def test_limits_of_the_definition():
    # q == 0 in float64 (a margin of 800): term 0, gradient row 0, for gamma below and above 1; p == 0: mod = 1, the CE gradient
    lg = np.zeros((2, 3), np.float32); lg[0, 1] = 800.0; lg[1, 1] = 800.0
    tg = np.array([1, 0], np.uint8)
    w = np.ones(3, np.float32)
    for gamma in (0.5, 2.0):
        L, g, D = FR.focal_loss_and_grad(lg, tg, 255, w, gamma)
        assert np.isfinite(L) and np.all(g[0] == 0) and np.all(np.isfinite(g))
        assert abs(L - 800.0 / 2) < 1e-9                        # pixel 1: q = 1, nll = 800
        assert abs(g[1, 0] + 0.5) < 1e-12 and abs(g[1, 1] - 0.5) < 1e-12

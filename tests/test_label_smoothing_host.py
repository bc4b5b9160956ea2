"""Host side of the label-smoothed cross entropy: what a label_smoothing may be, what train_or_resume accepts as dataset['label_smoothing'], the
five entry points in the header and the ctypes table, the float64 restatement the GPU tests compare with (tests/label_smoothing_ref.py) against
torch on the CPU, and the float32 emulation of the kernels' pixel function against the two bounds - nothing here needs a GPU.

Emulation against the bounds, worst over every case below: error / bound 0.07 (loss) and 0.34 (gradient)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as FR
import label_smoothing_ref as SR
from test_class_weighted_ce_gpu import make_weights
from test_cross_entropy_edges import make_case

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS

ENTRY_POINTS = ['dsrl_ce_fwd_s', 'dsrl_ce_bwd_s', 'dsrl_ce_fused_s', 'dsrl_convt2x2_fwd_ce_s', 'dsrl_convt2x2_bwd_ce_s']
SIZE_QUERIES = ['dsrl_ce_s_workspace_bytes', 'dsrl_ce_fused_s_workspace_bytes', 'dsrl_convt2x2_fwd_ce_s_workspace_bytes']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsrl_hip.h')
REF_CASES = ['randn', 'offset_1e4', 'onehot', 'graded']
EPS = [0.1, 0.5, 1.0]
BAD = [True, False, np.True_, '0.1', None, [0.1], float('nan'), float('inf'), -float('inf'), -1e-30, 1.0000001, -1, 2, 1e39]


@pytest.mark.parametrize('value,want', [(0, 0.0), (0.0, 0.0), (1, 1.0), (1.0, 1.0), (0.1, 0.1), (np.float32(0.5), 0.5), (np.int64(1), 1.0), (1e-30, 1e-30)])
def test_label_smoothing_value_accepts(value, want):
    got = HF.label_smoothing_value(value)
    assert type(got) is float and got == want


@pytest.mark.parametrize('value', BAD)
def test_label_smoothing_value_rejects(value):
    with pytest.raises(ValueError, match='label_smoothing'):
        HF.label_smoothing_value(value)


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


def test_check_label_smoothing():
    assert TR.check_label_smoothing(_dataset()) == 0.0
    assert TR.check_label_smoothing(_dataset(label_smoothing=None)) == 0.0
    assert TR.check_label_smoothing(_dataset(label_smoothing=0)) == 0.0
    assert TR.check_label_smoothing(_dataset(label_smoothing=0.1)) == 0.1
    assert TR.check_label_smoothing(_dataset(label_smoothing=1)) == 1.0
    assert TR.check_label_smoothing(_dataset(label_smoothing=0.1, focal_gamma=0)) == 0.1
    assert TR.check_label_smoothing(_dataset(label_smoothing=0, focal_gamma=2.0)) == 0.0
    for bad in BAD:
        if bad is None:
            continue
        with pytest.raises(ValueError, match='label_smoothing'):
            TR.check_label_smoothing(_dataset(label_smoothing=bad))
    with pytest.raises(ValueError, match='focal_gamma'):
        TR.check_label_smoothing(_dataset(label_smoothing=0.1, focal_gamma=2.0))


def test_the_focal_combination_is_refused_everywhere():
    for f in (lambda: HF._focal_args(None, 2.0, 'cpu', 19, 0.1), lambda: HF.logits_target(None, 255, None, None, 2.0, 0.1)):
        with pytest.raises(ValueError, match='focal_gamma'):
            f()
    with pytest.raises(ValueError, match='label_smoothing'):
        HF.logits_target(None, 255, None, None, 0.0, 1.5)


@pytest.mark.parametrize('kw', [dict(label_smoothing=2), dict(label_smoothing=-1e-30), dict(label_smoothing=float('nan')), dict(label_smoothing='0.1'),
                                dict(label_smoothing=True), dict(label_smoothing=0.1, focal_gamma=2.0)])
def test_train_or_resume_refuses_a_bad_value_before_touching_a_device(kw):
    args = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=_dataset(loader_factory=lambda *a: [], **kw), val_interval=1, checkpoint_interval=1, checkpoint_history=1,
                init_weights=None, batch_size=1, epochs=1, learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4,
                poly_power=0.9, stage=1, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)
    with pytest.raises(ValueError, match='label_smoothing'):
        TR.train_or_resume(**args)


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_is_declared_and_registered(name):
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', text)
    assert m, f'{name} is not declared in include/dsrl_hip.h'
    params = [p.strip() for p in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]
    k = [i for i, p in enumerate(params) if re.search(r'\bweights$', p)]
    assert k and params[k[0] + 1] == 'float eps', f'{name}: `float eps` does not follow `weights` ({params})'
    assert name in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[name]
    assert len(args) == len(params), f'{name}: {len(params)} parameters declared, {len(args)} registered'
    sib = _lib.PROTOTYPES[name[:-2] + '_w']                     # its _w sibling plus one float after the weights
    assert res is sib[0] and len(args) == len(sib[1]) + 1
    i = next(i for i in range(len(args)) if i >= len(sib[1]) or args[i] is not sib[1][i])
    assert args[:i] + args[i + 1:] == sib[1] and args[i] is _lib.f32
    assert _lib.PROTOTYPES[name[:-2] + '_f'] == (res, args)     # and the shape of the focal family


@pytest.mark.parametrize('name', SIZE_QUERIES)
def test_size_query_is_declared_and_registered(name):
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r'\bsize_t\s+' + name + r'\s*\(', text), f'{name} is not declared in include/dsrl_hip.h'
    assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name.replace('_s_workspace', '_w_workspace')]


def _case(case, C, seed, P=300, ii=255, ones=False):
    rs = np.random.RandomState(seed)
    lg, tg = FR.make_graded(P, C, rs, ii) if case == 'graded' else make_case(case, P, C, rs, ii)
    w = np.ones(C, np.float32) if ones else make_weights(C, rs)
    return lg, tg, w


@pytest.mark.parametrize('ones', [False, True])
@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('case', REF_CASES)
def test_restatement_equals_torch_cpu_float64(case, C, ones):
    for eps in EPS:
        for ii in (255, 0, -1):
            lg, tg, w = _case(case, C, 11 + C + REF_CASES.index(case), ii=ii, ones=ones)
            L, g, D, ce_part, sm_part = SR.smooth_loss_and_grad(lg, tg, ii, w, eps)
            Lt, gt = SR.torch_reference(lg, tg, ii, w, eps)
            assert abs(L - (ce_part + sm_part)) <= 1e-15 * abs(L) and D > 0
            assert abs(L - Lt) <= 1e-12 * abs(Lt), (case, C, eps, ii, L, Lt)
            assert np.all(g[tg.astype(np.int64) == ii] == 0)
            assert np.abs(g - gt).max() <= 1e-12 * np.abs(gt).max(), (case, C, eps, ii, np.abs(g - gt).max())


@pytest.mark.parametrize('C', [19, 3])
def test_eps_to_zero_is_the_weighted_cross_entropy(C):
    lg, tg, w = _case('graded', C, 7 + C)
    x = torch.tensor(lg.astype(np.float64), requires_grad=True)
    ref = F.cross_entropy(x, torch.tensor(tg.astype(np.int64)), weight=torch.tensor(w.astype(np.float64)), ignore_index=255)
    ref.backward()
    ref = float(ref.detach())
    L0, g0, _, ce_part, sm_part = SR.smooth_loss_and_grad(lg, tg, 255, w, 0.0)
    assert abs(L0 - ref) <= 1e-12 * abs(ref) and sm_part == 0.0 and abs(ce_part - L0) <= 1e-15 * abs(L0)
    assert np.abs(g0 - x.grad.numpy()).max() <= 1e-12
    Le, ge = SR.smooth_loss_and_grad(lg, tg, 255, w, 1e-9)[:2]       # and continuously so
    assert abs(Le - ref) <= 1e-7 * abs(ref) and np.abs(ge - x.grad.numpy()).max() <= 1e-7


def _spread_with_zero_on_the_low_class(C, seed, P=300):
    """make_case's spread, the zero weight on the -3e38 class of its live spread pixels: the class that holds it most often, the other live spread
    pixels ignored (labels only: the logits stay make_case's)"""
    rs = np.random.RandomState(seed)
    lg, tg = make_case('spread', P, C, rs, 255)
    low = np.where((lg == np.float32(-3e38)).any(axis=1), (lg == np.float32(-3e38)).argmax(axis=1), -1)
    live = tg != 255
    z = int(np.bincount(low[live & (low >= 0)], minlength=C).argmax())
    tg = tg.copy()
    tg[live & (low >= 0) & (low != z)] = 255
    return lg, tg, make_weights(C, rs, zero=z), z


@pytest.mark.parametrize('C', [19, 3])
def test_a_zero_weight_class_adds_nothing_to_the_smoothing_sum(C):
    lg, tg, w, z = _spread_with_zero_on_the_low_class(C, 5 + C)
    assert ((lg == np.float32(-3e38)).any(axis=1) & (tg != 255)).any()
    L, g, D, ce_part, sm_part = SR.smooth_loss_and_grad(lg, tg, 255, w, 0.1)
    assert np.isfinite(L) and np.isfinite(g).all() and np.isfinite(np.float32(L))
    # where the class's nl is +inf (a -inf logit) torch forms 0 * inf = NaN and this definition does not
    lg2 = lg.copy(); lg2[lg2 == np.float32(-3e38)] = -np.inf
    L2, g2 = SR.smooth_loss_and_grad(lg2, tg, 255, w, 0.1)[:2]
    assert np.isfinite(L2) and np.isfinite(g2).all()
    assert np.isnan(SR.torch_reference(lg2, tg, 255, w, 0.1)[0])
    # and with a positive weight there the fp32 value is +inf (m - v_c overflows fp32), as the emulation has it
    w2 = w.copy(); w2[z] = 1.0
    assert np.isposinf(SR.emulate_fp32(lg, tg, 255, w2, 0.1)[0])


@pytest.mark.parametrize('ones', [False, True])
@pytest.mark.parametrize('C', [19, 3])
def test_smoothing_moves_the_loss_of_the_graded_case(C, ones):
    for seed in (1, 2, 3):
        lg, tg, w = _case('graded', C, seed, ones=ones)
        ce = SR.smooth_loss_and_grad(lg, tg, 255, w, 0.0)[0]
        sl = SR.smooth_loss_and_grad(lg, tg, 255, w, 0.1)[0]
        assert abs(sl - ce) > 0.05 * abs(ce), (sl, ce)


@pytest.mark.parametrize('ones', [False, True])
@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('case', REF_CASES + ['spread'])
def test_fp32_emulation_stays_inside_both_bounds(case, C, ones):
    worst = [0.0, 0.0]
    for eps in EPS:
        for P in (300, 1):
            for ii in (255, 0, -1):
                if case == 'spread':
                    if ones or ii != 255 or P == 1:
                        continue
                    lg, tg, w, _ = _spread_with_zero_on_the_low_class(C, 31 + C)
                else:
                    lg, tg, w = _case(case, C, 23 + C + REF_CASES.index(case), P=P, ii=ii, ones=ones)
                L, g, D = SR.smooth_loss_and_grad(lg, tg, ii, w, eps)[:3]
                if not D > 0:
                    continue
                Le, ge = SR.emulate_fp32(lg, tg, ii, w, eps)
                lb = SR.loss_bound(lg, tg, ii, w, eps)
                live = tg.astype(np.int64) != ii
                gb = SR.grad_bound(tg, ii, w, eps, D)
                rl = abs(float(Le) - L) / lb
                rg = float((np.abs(ge[live].astype(np.float64) - g[live]) / gb).max())
                worst = [max(worst[0], rl), max(worst[1], rg)]
                assert rl <= 1.0 and rg <= 1.0 and np.all(ge[~live] == 0), (case, C, eps, P, ii, rl, rg)
    print(f'{case} C={C} ones={ones}: emulation error / bound: loss {worst[0]:.3f}, gradient {worst[1]:.3f}')

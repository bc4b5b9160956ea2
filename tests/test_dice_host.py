"""Host side of the soft Dice term: tests/dice_ref.py against torch autograd in float64 and against central differences of its
own value, absent classes / all-ignored input / bad labels, what HF.dice_value and train_or_resume.check_dice accept, the combinations that are
refused before anything touches a device, and the argument errors and declarations of the new entry points (returned before any HIP call, so pinned
here) - nothing here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import dice_ref as DR

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS

BADARG, WORKSPACE = -1, -3                          # include/dsrl_hip.h: DSRL_E_BADARG, DSRL_E_WORKSPACE
ENTRY_POINTS = ['dsrl_dice_workspace_bytes', 'dsrl_dice_fwd', 'dsrl_dice_bwd', 'dsrl_convt2x2_bwd_ce_d']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsrl_hip.h')


# ------------------------------------------------------------------------------------------------------------------------------ the reference
def _dice_torch(x, t, ii, lam, smooth):
    """the definition on the softmax / one-hot composition, differentiable (float64 CPU tensors)"""
    C = x.shape[1]
    live = (t != ii) & (t < C)
    p = torch.softmax(x[live], dim=1)
    oh = torch.nn.functional.one_hot(t[live], C).to(p.dtype)
    I, Pc, G = (p * oh).sum(0), p.sum(0), oh.sum(0)
    present = G > 0
    if not bool(present.any()):
        return x.sum() * 0.0
    dice = (2 * I + smooth) / (Pc + G + smooth)
    return lam * (1.0 - dice[present].sum() / present.sum())


@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('scale', [1.0, 4.0, 12.0])
@pytest.mark.parametrize('lam,smooth', [(1.0, 1.0), (0.4, 0.0), (2.5, 1e-3)])
def test_reference_against_torch_autograd_in_float64(C, scale, lam, smooth):
    rs = np.random.RandomState(int(10 * scale) + C)
    P = 1536
    lg = (rs.standard_normal((P, C)) * scale).astype(np.float32)
    tg = rs.randint(0, C, P).astype(np.uint8)
    tg[rs.uniform(size=P) < 0.1] = 255
    tg[tg == 1] = 0                                  # class 1 is absent
    tg[5] = C + 3                                    # a bad label: takes no part
    x = torch.tensor(lg.astype(np.float64), requires_grad=True)
    loss = _dice_torch(x, torch.tensor(tg.astype(np.int64)), 255, lam, smooth)
    loss.backward()
    val, grad, K, a, b, G = DR.dice_loss_and_grad(lg, tg, 255, lam, smooth)
    assert K == C - 1 and G[1] == 0 and a[1] == 0.0 and b[1] == 0.0
    assert abs(val - float(loss.detach())) <= 1e-14
    assert np.abs(grad - x.grad.numpy()).max() <= 1e-16
    assert np.all(grad[tg == 255] == 0) and np.all(grad[5] == 0)


def test_gradient_against_central_differences_of_its_own_value():
    rs = np.random.RandomState(2)
    P, C = 40, 5
    lg, tg = DR.make_overlap(P, C, rs, 255)
    _, grad, *_ = DR.dice_loss_and_grad(lg, tg, 255, 1.5, 1.0)
    x = lg.astype(np.float64)
    h = 1e-5
    worst = 0.0
    for i in range(0, P, 3):
        for c in range(C):
            xp = x.copy(); xp[i, c] += h
            xm = x.copy(); xm[i, c] -= h
            num = (DR.value64(xp, tg, 255, 1.5, 1.0) - DR.value64(xm, tg, 255, 1.5, 1.0)) / (2 * h)
            worst = max(worst, abs(num - grad[i, c]))
    assert worst <= 1e-9, worst
    assert abs(DR.value64(x, tg, 255, 1.5, 1.0) - DR.dice_loss_and_grad(lg, tg, 255, 1.5, 1.0)[0]) <= 1e-15


def test_absent_classes_all_ignored_and_bad_labels():
    rs = np.random.RandomState(3)
    P, C = 200, 6
    lg = rs.standard_normal((P, C)).astype(np.float32)
    tg = rs.randint(0, 2, P).astype(np.uint8)                                   # classes 2..5 absent
    val, grad, K, a, b, G = DR.dice_loss_and_grad(lg, tg, 255)
    assert K == 2 and np.all(a[2:] == 0) and np.all(b[2:] == 0) and np.all(a[:2] < 0) and np.all(b[:2] > 0)
    I, Pc, Gc = DR.sums64(lg, tg, 255)
    want = 1.0 - 0.5 * sum((2 * I[c] + 1.0) / (Pc[c] + Gc[c] + 1.0) for c in (0, 1))   # the mean over the two present classes, not over six
    assert abs(val - want) <= 1e-15
    assert np.abs(grad.sum(axis=1)).max() <= 1e-16                             # every row of a softmax gradient sums to zero
    val, grad, K, a, b, G = DR.dice_loss_and_grad(lg, np.full(P, 255, np.uint8), 255)
    assert val == 0.0 and K == 0 and not grad.any() and not a.any() and not b.any()
    tb = tg.copy(); tb[:50] = 200                                               # bad labels: out of Dice altogether, as if ignored
    ti = tg.copy(); ti[:50] = 255
    rb, ri = DR.dice_loss_and_grad(lg, tb, 255), DR.dice_loss_and_grad(lg, ti, 255)
    assert rb[0] == ri[0] and np.array_equal(rb[1], ri[1]) and not rb[1][:50].any()
    e = DR.emulate_fp32(lg, tg, 255)                                            # the fp32 restatement is the same function to fp32 accuracy
    ref = DR.dice_loss_and_grad(lg, tg, 255)
    assert abs(float(e[0]) - ref[0]) <= 1e-6
    assert np.abs(e[1] - ref[1]).max() <= DR.GRAD_TOL * float((np.abs(ref[3]) + np.abs(ref[4])).max())


def test_overlap_case_meets_its_conditions():
    for C in (19, 3):
        for P in (1536, 1000):
            for seed in range(4):
                lg, tg = DR.make_overlap(P, C, np.random.RandomState(P + C + seed), 255)
                assert 0.05 < float((tg == 255).mean()) < 0.15
                DR.assert_overlap(lg, tg, 255)


# ------------------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('value,want', [(None, None), (False, None), (np.False_, None), (0, None), (0.0, None), ((0, 1.0), None), (True, (1.0, 1.0)),
                                        (0.5, (0.5, 1.0)), (2, (2.0, 1.0)), (np.float32(0.25), (0.25, 1.0)), ((0.5, 0), (0.5, 0.0)), ([2, 1e-3], (2.0, 1e-3)),
                                        ({'weight': 0.3}, (0.3, 1.0)), ({'smooth': 0.0}, (1.0, 0.0)), ({'weight': np.float64(3), 'smooth': 2}, (3.0, 2.0))])
def test_dice_value_accepts(value, want):
    got = HF.dice_value(value)
    assert got == want
    if got is not None:
        assert type(got[0]) is float and type(got[1]) is float


@pytest.mark.parametrize('value', ['on', (0.5,), (0.5, 1, 2), {}, {'weight': 1.0, 'eps': 1.0}, (True, 1.0), (1.0, True), (1.0, None), ('1', 1.0),
                                   -1.0, -1e-30, float('nan'), float('inf'), -float('inf'), 1e39, (1.0, -1.0), (1.0, float('nan')), (1.0, float('inf')),
                                   (float('nan'), 1.0), {'weight': -2}, {'smooth': float('inf')}, 1e-50])
def test_dice_value_rejects(value):
    with pytest.raises(ValueError, match='dice'):
        HF.dice_value(value)


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


def test_check_dice():
    assert TR.check_dice(_dataset()) is None
    for off in (None, False, 0, 0.0):
        assert TR.check_dice(_dataset(dice=off)) is None
    assert TR.check_dice(_dataset(dice=True)) == (1.0, 1.0)
    assert TR.check_dice(_dataset(dice=0.5)) == (0.5, 1.0)
    assert TR.check_dice(_dataset(dice=(2.0, 0.0))) == (2.0, 0.0)
    assert TR.check_dice(_dataset(dice={'weight': 0.6, 'smooth': 1e-5}, class_weights='enet')) == (0.6, 1e-5)
    assert TR.check_dice(_dataset(dice=True, focal_gamma=0, label_smoothing=0.0, ohem=False)) == (1.0, 1.0)
    for bad in ('on', -1.0, (1.0, -1), {'lambda': 1.0}, float('nan')):
        with pytest.raises(ValueError, match='dice'):
            TR.check_dice(_dataset(dice=bad))
    for other in (dict(focal_gamma=2.0), dict(label_smoothing=0.1), dict(ohem=True)):
        with pytest.raises(ValueError, match='dice.*together'):
            TR.check_dice(_dataset(dice=True, **other))
        assert TR.check_dice(_dataset(dice=False, **other)) is None              # off: nothing to refuse


@pytest.mark.parametrize('extra', [dict(dice=-1.0), dict(dice='on'), dict(dice=True, focal_gamma=2.0), dict(dice=True, label_smoothing=0.1),
                                   dict(dice=True, ohem=True)])
def test_train_or_resume_refuses_a_bad_dice_before_touching_a_device(extra):
    args = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=_dataset(loader_factory=lambda *a: [], **extra), val_interval=1, checkpoint_interval=1, checkpoint_history=1,
                init_weights=None, batch_size=1, epochs=1, learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4,
                poly_power=0.9, stage=1, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)
    with pytest.raises(ValueError, match='dice'):
        TR.train_or_resume(**args)


class _NoDevice:
    """stands in for a tensor: the refusals below must come before anything asks it for a device or a shape"""

    def __getattr__(self, name):
        raise AssertionError(f'touched .{name} before refusing the arguments')


@pytest.mark.parametrize('kw', [dict(focal_gamma=2.0), dict(label_smoothing=0.1), dict(ohem=True)])
def test_the_refused_combinations(kw, monkeypatch):
    def reached(name, *a):
        raise AssertionError(f'{name} reached the library')
    for fn in ('call', 'query', 'cquery'):
        monkeypatch.setattr(HF, fn, reached)
    nd = _NoDevice()
    with pytest.raises(ValueError, match='dice.*together'):
        HF.logits_target(None, 255, None, dice=True, **kw)
    with pytest.raises(ValueError, match='dice.*together'):
        HF.fused_losses((nd, nd, nd, nd), nd, nd, 255, 0.1, 1.0, 3, nd, dice=(1.0, 1.0), **kw)
    with pytest.raises(ValueError, match='dice.*together'):
        HF.cross_entropy(nd, nd, 255, dice=0.5, **kw)
    with pytest.raises(ValueError, match='dice.*together'):
        TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, dice=True, **kw)
    # off: nothing to refuse, and a bad value is refused as early
    assert HF._dice_args(None, kw.get('focal_gamma', 0.0), kw.get('label_smoothing', 0.0), HF.ohem_value(kw.get('ohem'))) is None
    for bad in (-1.0, float('nan'), (1.0, -1.0), 'on'):
        with pytest.raises(ValueError, match='dice'):
            HF.fused_losses((nd, nd, nd, nd), nd, nd, 255, 0.1, 1.0, 3, nd, dice=bad)
        with pytest.raises(ValueError, match='dice'):
            HF.logits_target(None, 255, None, dice=bad)
        with pytest.raises(ValueError, match='dice'):
            TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, dice=bad)
        with pytest.raises(ValueError, match='dice'):
            HF.dice_loss(nd, nd, 255, *((bad,) if not isinstance(bad, tuple) else bad))


def test_logits_target_with_dice_still_engages_the_forward():
    t = torch.zeros((1, 2, 2), dtype=torch.uint8)
    assert HF.logits_target(t, 255, torch.zeros(1, dtype=torch.int32), dice=True).new is None       # a CPU target engages nothing, with or without
    assert HF.logits_target(None, 255, None, dice=(0.5, 1.0)).new is None


# ------------------------------------------------------------------------------------------------------------------------------ entry points
def _params(name):
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r'\b(?:int|size_t)\s+' + name + r'\s*\(([^;]*)\)\s*;', text)
    assert m, f'{name} is not declared in include/dsrl_hip.h'
    return [re.sub(r'\[.*\]', '', p.strip()).split()[-1].lstrip('*') for p in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]


def _call(name, **named):
    """The entry point with every pointer null and every number 0 but for `named` (by the header's parameter names) -> (code, message)."""
    lib = _lib.load()
    names = _params(name)
    args = [None if t is _lib.fp else (0.0 if t is _lib.f32 else 0) for t in _lib.PROTOTYPES[name][1]]
    for k, v in named.items():
        args[names.index(k)] = v
    code = getattr(lib, name)(*args)
    return code, lib.dsrl_last_error().decode()


def _as_c_prints(v):
    return 'nan' if math.isnan(v) else (('-inf' if v < 0 else 'inf') if math.isinf(v) else '%g' % _lib.f32(v).value)


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_is_declared_and_registered(name):
    assert name in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[name]
    names = _params(name)
    assert len(args) == len(names), f'{name}: {len(names)} parameters declared, {len(args)} registered'
    kinds = {'P': _lib.i64, 'C': _lib.i32, 'ld': _lib.i32, 'lddl': _lib.i32, 'ignore_index': _lib.i32, 'accumulate': _lib.i32, 'ft_stride': _lib.i32,
             'N': _lib.i32, 'H': _lib.i32, 'W': _lib.i32, 'Cin': _lib.i32, 'Cout': _lib.i32, 'lambda': _lib.f32, 'smooth': _lib.f32,
             'ws_bytes': _lib.sz, 'stream': _lib.stream_t}
    for n, a in zip(names, args):
        assert a is kinds.get(n, _lib.fp), (name, n)
    assert res is (_lib.sz if name.endswith('_bytes') else _lib.i32)


OK_FWD = dict(logits=0x1000, target=0x2000, record=0x3000, ws=0x5000, P=10, C=19, ld=19, ws_bytes=1 << 30, smooth=1.0)
OK_FWD['lambda'] = 1.0


@pytest.mark.parametrize('lam,smooth', [(0.0, 1.0), (-1.0, 1.0), (float('nan'), 1.0), (float('inf'), 1.0), (1.0, -1e-30), (1.0, float('nan')),
                                        (1.0, float('inf')), (-float('inf'), 1.0)])
def test_a_bad_lambda_or_smooth_is_refused_first(lam, smooth):
    code, msg = _call('dsrl_dice_fwd', **dict(OK_FWD, **{'lambda': lam, 'smooth': smooth, 'logits': None}))
    assert code == BADARG
    assert msg == f'dice_fwd: lambda = {_as_c_prints(lam)} must be a finite number > 0 and smooth = {_as_c_prints(smooth)} a finite number >= 0', msg


def test_the_other_argument_errors():
    for bad in (dict(logits=None), dict(target=None), dict(record=None), dict(ws=None), dict(P=0), dict(P=-5), dict(C=0), dict(C=61), dict(ld=18),
                dict(record=0x3002)):
        code, msg = _call('dsrl_dice_fwd', **dict(OK_FWD, **bad))
        assert code == BADARG and msg.startswith('dice_fwd: bad arguments'), (bad, msg)
    code, msg = _call('dsrl_dice_fwd', **dict(OK_FWD, P=2 ** 31))
    assert code == BADARG and msg.startswith('dice_fwd: P = 2147483648'), msg
    need = _lib.query('dsrl_dice_workspace_bytes', 10)
    for bad in (dict(ws_bytes=need - 1), dict(ws=0x5004)):
        code, msg = _call('dsrl_dice_fwd', **dict(OK_FWD, **bad))
        assert code == WORKSPACE and msg == 'dice_fwd: workspace too small or misaligned', (bad, msg)
    ok = dict(logits=0x1000, target=0x2000, record=0x3000, dlogits=0x4000, P=10, C=19, ld=19, lddl=19)
    for bad in (dict(logits=None), dict(target=None), dict(record=None), dict(dlogits=None), dict(P=0), dict(C=61), dict(ld=18), dict(lddl=18),
                dict(accumulate=2), dict(accumulate=-1)):
        code, msg = _call('dsrl_dice_bwd', **dict(ok, **bad))
        assert code == BADARG and msg.startswith('dice_bwd: bad arguments'), (bad, msg)
    code, msg = _call('dsrl_convt2x2_bwd_ce_d')
    assert code == BADARG and msg.startswith('convt2x2_bwd_ce_d: bad arguments'), msg
    code, msg = _call('dsrl_convt2x2_bwd_ce_d', dice_record=0x3000)
    assert code == BADARG and msg.startswith('convt2x2_bwd_ce_d: bad arguments'), msg


def test_the_workspace_depends_on_P_alone():
    q = lambda P: _lib.query('dsrl_dice_workspace_bytes', P)     # noqa: E731
    assert q(0) == 0 and _lib.load().dsrl_last_error().decode().startswith('dice_workspace_bytes: bad arguments')
    assert q(-3) == 0 and q(2 ** 31) == 0
    row = 64 * (8 + 8 + 4)                                      # I and P in double, G in integers, 64 classes per row
    for P, chunks in ((1, 1), (256, 1), (257, 2), (1000, 4), (1536, 6), (256 * 1024, 1024), (8 * 512 * 1024, 1024)):
        assert q(P) == row * (1 + chunks), P                     # the totals, then one row per chunk: at most 1024 chunks

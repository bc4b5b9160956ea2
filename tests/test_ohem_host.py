"""Host side of OHEM: the exact select of tests/ohem_ref.py against a torch-CPU transcription of the rule, what HF.ohem_value and
train_or_resume.check_ohem accept, the combinations that are refused, the argument errors of the five entry points (returned before any HIP
call, so pinned here without a GPU) and their declarations - nothing here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import ohem_ref as OR

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS

BADARG = -1                                         # include/dsrl_hip.h: DSRL_E_BADARG
CALLS = ['dsrl_ohem_prob', 'dsrl_ohem_select', 'dsrl_ohem_apply', 'dsrl_ohem_target']
ENTRY_POINTS = CALLS + ['dsrl_ohem_workspace_bytes']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsrl_hip.h')


# ------------------------------------------------------------------------------------------------------------------------------ the reference
def _rule_torch(p, thresh, min_kept):
    """the rule, word for word, on a CPU tensor of candidates' probabilities -> (thr, keep mask)"""
    n = p.numel()
    k = min(min_kept, n - 1)
    v = torch.sort(p).values[k]
    thr = torch.maximum(v, torch.tensor(thresh, dtype=torch.float32))
    return thr, p < thr


@pytest.mark.parametrize('seed', range(6))
def test_select_is_the_rule_on_random_data(seed):
    rs = np.random.RandomState(seed)
    P = int(rs.randint(1, 3000))
    p = rs.uniform(0, 1, P).astype(np.float32) ** np.float32(rs.choice([0.3, 1.0, 4.0]))
    p[rs.uniform(size=P) < 0.3] = p[0]                                          # ties
    cand = rs.uniform(size=P) < 0.8
    cand[0] = True
    full = np.where(cand, p, OR.SENTINEL).astype(np.float32)
    for thresh in (0.0, 0.3, 0.7, 1.0):
        for min_kept in (0, 1, int(cand.sum()) // 3, int(cand.sum()) - 1, int(cand.sum()), 10 * P):
            bits, n, kept, below, keep = OR.select(full, thresh, min_kept)
            thr, k = _rule_torch(torch.tensor(p[cand]), np.float32(thresh), min_kept)
            assert n == int(cand.sum())
            assert bits == int(np.float32(thr).view(np.uint32))
            assert np.array_equal(keep[cand], k.numpy()) and keep[~cand].all()
            assert kept == int(k.sum()) and below == int((p[cand] < np.float32(thresh)).sum())


def test_select_edges():
    assert OR.select(np.full(5, 2.0, np.float32), 0.7, 3)[:4] == (int(np.float32(0.7).view(np.uint32)), 0, 0, 0)      # n == 0: thr = thresh
    bits, n, kept, below, keep = OR.select(np.array([0.25, 2.0], np.float32), 0.0, 100)                                 # n == 1: k = 0, nothing below v
    assert (bits, n, kept, below) == (int(np.float32(0.25).view(np.uint32)), 1, 0, 0) and keep.tolist() == [False, True]
    bits, n, kept, below, keep = OR.select(np.array([np.nan, -0.0, 0.5, 1e-42], np.float32), 0.5, 0)                    # NaN and -0 are 0
    assert (n, kept, below) == (4, 3, 3) and keep.tolist() == [True, True, False, True]
    assert OR.keys(np.array([np.nan, -0.0, -1.0, 1e-42, 1.0], np.float32)).tolist() == [0, 0, 0, 714, 0x3f800000]


def test_make_case_asserts_its_guard_and_that_mining_matters():
    for ii in (255, 0, 18):
        lg, tg, thresh, min_kept, _ = OR.make_case(700, 19, 5, ii)
        assert OR.guard_holds(lg, tg, ii, thresh, min_kept)
        out, thr, n, kept = OR.rewrite(lg, tg, ii, thresh, min_kept)
        assert np.all((out == tg) | (out == ii)) and (out != tg).sum() == n - kept >= n // 4
        p, cand = OR.target_probability64(lg, tg, ii)                               # the fp32 select on the rounded p agrees: what the guard is for
        assert np.array_equal(OR.select(p.astype(np.float32), thresh, min_kept)[4], (out == tg))


# ------------------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('value,want', [(None, None), (False, None), (np.False_, None), (True, (0.7, 100000)), ((0.5, 10), (0.5, 10)), ([1, 0], (1.0, 0)),
                                        ((0, np.int64(7)), (0.0, 7)), ({'thresh': 0.9}, (0.9, 100000)), ({'min_kept': 5}, (0.7, 5)),
                                        ({'thresh': np.float32(0.5), 'min_kept': 2}, (0.5, 2))])
def test_ohem_value_accepts(value, want):
    got = HF.ohem_value(value)
    assert got == want
    if got is not None:
        assert type(got[0]) is float and type(got[1]) is int


@pytest.mark.parametrize('value', [0.7, 1, 'on', (0.7,), (0.7, 1, 2), {}, {'thresh': 0.7, 'keep': 3}, (True, 3), (0.7, True), (0.7, 2.0), (0.7, -1),
                                   (-1e-30, 5), (1.0000001, 5), (float('nan'), 5), ('0.7', 5), (0.7, None), (0.7, 2 ** 63)])
def test_ohem_value_rejects(value):
    with pytest.raises(ValueError, match='ohem'):
        HF.ohem_value(value)


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


def test_check_ohem():
    assert TR.check_ohem(_dataset()) is None
    assert TR.check_ohem(_dataset(ohem=None)) is None
    assert TR.check_ohem(_dataset(ohem=False)) is None
    assert TR.check_ohem(_dataset(ohem=True)) == (0.7, 100000)
    assert TR.check_ohem(_dataset(ohem=(0.9, 50000))) == (0.9, 50000)
    assert TR.check_ohem(_dataset(ohem={'thresh': 0.6, 'min_kept': 1}, class_weights='enet')) == (0.6, 1)
    assert TR.check_ohem(_dataset(ohem=True, focal_gamma=0, label_smoothing=0.0)) == (0.7, 100000)
    for bad in (0.7, 'on', (0.7, -1), (2.0, 1), {'thresh': 'x'}):
        with pytest.raises(ValueError, match='ohem'):
            TR.check_ohem(_dataset(ohem=bad))
    with pytest.raises(ValueError, match='ohem.*together'):
        TR.check_ohem(_dataset(ohem=True, focal_gamma=2.0))
    with pytest.raises(ValueError, match='ohem.*together'):
        TR.check_ohem(_dataset(ohem=True, label_smoothing=0.1))
    assert TR.check_ohem(_dataset(ohem=False, focal_gamma=2.0)) is None             # off: nothing to refuse

    class Wide:
        IGNORE_CLASS_LABEL = 300
    with pytest.raises(ValueError, match='ignore_index'):
        TR.check_ohem({'settings': Wide, 'ohem': True})
    assert TR.check_ohem({'settings': Wide}) is None


@pytest.mark.parametrize('extra', [dict(ohem=(0.7, -1)), dict(ohem='on'), dict(ohem=True, focal_gamma=2.0), dict(ohem=True, label_smoothing=0.1)])
def test_train_or_resume_refuses_a_bad_ohem_before_touching_a_device(extra):
    args = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=_dataset(loader_factory=lambda *a: [], **extra), val_interval=1, checkpoint_interval=1, checkpoint_history=1,
                init_weights=None, batch_size=1, epochs=1, learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4,
                poly_power=0.9, stage=1, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)
    with pytest.raises(ValueError, match='ohem'):
        TR.train_or_resume(**args)


class _NoDevice:
    """stands in for a tensor: the refusals below must come before anything asks it for a device or a shape"""

    def __getattr__(self, name):
        raise AssertionError(f'touched .{name} before refusing the arguments')


@pytest.mark.parametrize('kw', [dict(focal_gamma=2.0), dict(label_smoothing=0.1)])
def test_the_refused_combinations(kw):
    with pytest.raises(ValueError, match='ohem.*together'):
        HF.logits_target(None, 255, None, ohem=True, **kw)
    with pytest.raises(ValueError, match='ohem.*together'):
        HF._ohem_args((0.7, 3), kw.get('focal_gamma', 0.0), kw.get('label_smoothing', 0.0), 255)
    assert HF._ohem_args(None, kw.get('focal_gamma', 0.0), kw.get('label_smoothing', 0.0), -1) is None     # off: nothing to refuse
    with pytest.raises(ValueError, match='ohem.*together'):
        TR.TrainStep(None, _NoDevice(), 3, 0.1, 1.0, 255, graph=False, ohem=True, **kw)


@pytest.mark.parametrize('ii', [-1, 256, 300, True, 2.0])
def test_an_ignore_index_that_is_no_byte_is_refused_with_ohem(ii):
    with pytest.raises(ValueError, match='ignore_index'):
        HF._ohem_args(True, 0.0, 0.0, ii)
    with pytest.raises(ValueError, match='ignore_index'):
        HF.logits_target(None, ii, None, ohem=True)
    with pytest.raises(ValueError, match='ignore_index'):
        HF.ohem_target(_NoDevice(), _NoDevice(), ii, 0.7, 3)
    with pytest.raises(ValueError, match='ignore_index'):
        TR.TrainStep(None, _NoDevice(), 3, 0.1, 1.0, ii, graph=False, ohem=True)


def test_logits_target_with_ohem_engages_nothing():
    assert HF.logits_target(None, 255, None, ohem=(0.7, 3)).new is None
    t = torch.zeros((1, 2, 2), dtype=torch.uint8)
    assert HF.logits_target(t, 255, torch.zeros(1, dtype=torch.int32), ohem=True).new is None


# ------------------------------------------------------------------------------------------------------------------------------ entry points
def _call(name, **named):
    """The entry point with every pointer null and every integer 0 but for `named` (by position in the header's parameter list) -> (code, message)."""
    lib = _lib.load()
    names = _params(name)
    args = [None if t is _lib.fp else (0.0 if t is _lib.f32 else 0) for t in _lib.PROTOTYPES[name][1]]
    for k, v in named.items():
        args[names.index(k)] = v
    code = getattr(lib, name)(*args)
    return code, lib.dsrl_last_error().decode()


def _params(name):
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r'\b(?:int|size_t)\s+' + name + r'\s*\(([^;]*)\)\s*;', text)
    assert m, f'{name} is not declared in include/dsrl_hip.h'
    return [re.sub(r'\[.*\]', '', p.strip()).split()[-1].lstrip('*') for p in re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')]


def _as_c_prints(v):
    return 'nan' if math.isnan(v) else ('inf' if math.isinf(v) else '%g' % _lib.f32(v).value)


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_is_declared_and_registered(name):
    assert name in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[name]
    names = _params(name)
    assert len(args) == len(names), f'{name}: {len(names)} parameters declared, {len(args)} registered'
    kinds = {'P': _lib.i64, 'min_kept': _lib.i64, 'thresh': _lib.f32, 'ignore_index': _lib.i32, 'C': _lib.i32, 'ld': _lib.i32, 'ws_bytes': _lib.sz,
             'stream': _lib.stream_t}
    for n, a in zip(names, args):
        assert a is kinds.get(n, _lib.fp), (name, n)
    assert res is (_lib.sz if name.endswith('_bytes') else _lib.i32)


@pytest.mark.parametrize('name', CALLS)
def test_a_null_call_is_a_bad_argument_in_the_entrys_own_name(name):
    code, msg = _call(name)
    assert code == BADARG
    assert msg.startswith(name[len('dsrl_'):] + ': bad arguments'), msg


@pytest.mark.parametrize('thresh', [-1e-30, 1.0000001, float('nan'), float('inf')])
@pytest.mark.parametrize('name', ['dsrl_ohem_select', 'dsrl_ohem_target'])
def test_a_bad_thresh_is_refused_first(name, thresh):
    code, msg = _call(name, thresh=thresh)
    assert code == BADARG
    assert msg == f'{name[len("dsrl_"):]}: thresh = {_as_c_prints(thresh)} is not a number in [0, 1]', msg


@pytest.mark.parametrize('min_kept', [-1, -2 ** 40])
@pytest.mark.parametrize('name', ['dsrl_ohem_select', 'dsrl_ohem_target'])
def test_a_negative_min_kept_is_refused(name, min_kept):
    code, msg = _call(name, min_kept=min_kept)
    assert code == BADARG
    assert msg == f'{name[len("dsrl_"):]}: min_kept = {min_kept} is negative', msg


@pytest.mark.parametrize('ii', [-1, 256, 300])
@pytest.mark.parametrize('name', ['dsrl_ohem_prob', 'dsrl_ohem_apply', 'dsrl_ohem_target'])
def test_an_ignore_index_that_is_no_byte_is_refused(name, ii):
    code, msg = _call(name, ignore_index=ii)
    assert code == BADARG
    assert msg == f'{name[len("dsrl_"):]}: ignore_index = {ii} is not a byte value 0..255', msg


def test_the_other_argument_errors_of_ohem_target():
    ok = dict(logits=0x1000, target=0x2000, target_out=0x3000, stats=0x4000, ws=0x5000, P=10, C=19, ld=19, ws_bytes=1 << 30)
    for bad in (dict(logits=None), dict(target=None), dict(target_out=None), dict(stats=None), dict(ws=None), dict(P=0), dict(P=-5), dict(C=0), dict(C=61),
                dict(ld=18), dict(stats=0x4002)):
        code, msg = _call('dsrl_ohem_target', **dict(ok, **bad))
        assert code == BADARG and msg.startswith('ohem_target: bad arguments'), (bad, msg)
    code, msg = _call('dsrl_ohem_target', **dict(ok, P=2 ** 31))
    assert code == BADARG and msg.startswith('ohem_target: P = 2147483648'), msg
    need = _lib.query('dsrl_ohem_workspace_bytes', 10)
    for bad in (dict(ws_bytes=need - 1), dict(ws=0x5004)):
        code, msg = _call('dsrl_ohem_target', **dict(ok, **bad))
        assert code == -3 and msg == 'ohem_target: workspace too small or misaligned', (bad, msg)
    code, msg = _call('dsrl_ohem_select', p=0x1000, P=10, stats=0x4000, ws=0x5000, ws_bytes=16)
    assert code == -3 and msg == 'ohem_select: workspace too small or misaligned', msg


def test_the_workspace_depends_on_P_alone():
    q = lambda P: _lib.query('dsrl_ohem_workspace_bytes', P)     # noqa: E731
    assert q(0) == 0 and _lib.load().dsrl_last_error().decode().startswith('ohem_workspace_bytes: bad arguments')
    assert q(-3) == 0 and q(2 ** 31) == 0
    fixed = q(1) - 16
    assert fixed >= (256 * 256 + 256) * 4 and fixed % 16 == 0                    # the partial histograms [256][256], a count per block, the state
    for P in (2, 255, 4097, 70001, 8 * 512 * 1024):
        assert q(P) == fixed + (4 * P + 15) // 16 * 16

"""Host side of the Lovasz-Softmax term: the closed form of tests/lovasz_ref.py against the Lovasz extension itself, the 1 / (2 K)
bound against the sorted loss, the cases the GPU test relies on (borderline shares, the seeds without a borderline element), what HF.lovasz_value and
train_or_resume.check_lovasz accept, the combinations that are refused before anything touches a device, and the size queries, argument errors and
declarations of the new entry points (returned before any HIP call, so pinned here) - nothing here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import lovasz_ref as LR

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS

BADARG, WORKSPACE = -1, -3                          # include/dsrl_hip.h: DSRL_E_BADARG, DSRL_E_WORKSPACE
ENTRY_POINTS = ['dsrl_lovasz_workspace_bytes', 'dsrl_lovasz_record_floats', 'dsrl_lovasz_fwd', 'dsrl_lovasz_bwd', 'dsrl_convt2x2_bwd_ce_l']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsrl_hip.h')


# ------------------------------------------------------------------------------------------------------------------------------ the reference
def _cases(C):
    """(logits, labels): the generator of the GPU test, every class in play at three spreads, and a confident model"""
    yield LR.make_case(3000, C, 7 + C)
    for scale in (1.0, 4.0, 12.0):
        rs = np.random.RandomState(int(scale) + C)
        lg = (scale * rs.standard_normal((1536, C))).astype(np.float32)
        tg = rs.randint(0, C, 1536).astype(np.uint8)
        tg[rs.uniform(size=1536) < 0.1] = 255
        tg[tg == 1] = 0                             # class 1 is absent
        tg[5] = C + 3                               # a bad label: takes no part
        yield lg, tg


@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('K', [16, 64, 1024])
def test_the_closed_form_is_the_lovasz_extension_at_the_level_centres(K, C):
    for lg, tg in _cases(C):
        r = LR.binned(lg, tg, 255, 1.0, K)
        err, fg, live = LR.errors(lg, tg, 255)
        e_hat = (LR.bins_of(err, K) + 0.5) / K
        per_class = [LR.lovasz_extension(e_hat[live, c], fg[live, c], fg_first=True) for c in range(C) if fg[live, c].any()]
        assert r['present'] == len(per_class) < C                           # an absent class is not counted
        assert abs(r['value'] - float(np.mean(per_class))) <= 1e-12
        # the extension is monotone and 1-Lipschitz in the sup norm (J(V) = 1) and |e_hat - err| <= 1 / (2 K)
        assert abs(r['value'] - r['exact']) <= 1.0 / (2 * K), (K, C, r['value'], r['exact'])
        assert r['exact'] > 0.05                                            # not a degenerate case
        # histogram sums, and a subgradient: every row of a softmax gradient sums to zero; nothing on a pixel that is not live
        assert np.array_equal(r['nf'].sum(axis=1), r['G']) and (r['nf'] + r['nb']).sum(axis=1).tolist() == [int(live.sum())] * C
        assert np.abs(r['rows'].sum(axis=1)).max() <= 1e-15 and not r['rows'][~live].any()
        assert not r['gf'][r['G'] == 0].any() and not r['gb'][r['G'] == 0].any()
        assert np.all(r['gf'][r['G'] > 0] < 0) and np.all(r['gb'] >= 0)


def test_the_value_scales_with_lambda_and_all_ignored_is_zero():
    lg, tg = LR.make_case(500, 5, 3)
    a, b = LR.binned(lg, tg, 255, 1.0, 64), LR.binned(lg, tg, 255, 2.5, 64)
    assert abs(b['value'] - 2.5 * a['value']) <= 1e-15 and np.allclose(b['rows'], 2.5 * a['rows'], rtol=1e-14, atol=0)
    r = LR.binned(lg, np.full(500, 255, np.uint8), 255, 1.0, 64)
    assert r['value'] == 0.0 and r['present'] == 0 and r['exact'] == 0.0 and not r['rows'].any() and not r['gf'].any() and not r['gb'].any()
    tb = tg.copy(); tb[:50] = 200                   # labels >= C: out of the term altogether, as if ignored
    ti = tg.copy(); ti[:50] = 255
    rb, ri = LR.binned(lg, tb, 255, 1.0, 64), LR.binned(lg, ti, 255, 1.0, 64)
    assert rb['value'] == ri['value'] and np.array_equal(rb['rows'], ri['rows']) and np.array_equal(rb['nb'], ri['nb'])


def test_the_gradient_is_the_derivative_of_the_sorted_loss_where_the_ranking_holds():
    """With K so large that no two errors share a level, the tables are Berman's Jaccard increments and the row is autograd's (ranking constant)."""
    rs = np.random.RandomState(4)
    P, C, K = 30, 4, 1 << 20                        # (the reference takes any K)
    lg = rs.standard_normal((P, C)).astype(np.float32)
    tg = rs.randint(0, C, P).astype(np.uint8)
    r = LR.binned(lg, tg, 255, 1.0, K)
    assert (r['nf'] + r['nb']).max() == 1
    x = torch.tensor(lg.astype(np.float64), requires_grad=True)
    p = torch.softmax(x, dim=1)
    t = torch.tensor(tg.astype(np.int64))
    loss = 0.0
    for c in range(C):
        fg = (t == c).to(p.dtype)
        e = (fg - p[:, c]).abs()
        es, perm = torch.sort(e, descending=True)
        loss = loss + torch.dot(es, torch.tensor(LR.jaccard_increments(fg[perm].numpy().astype(bool))))
    (loss / C).backward()
    assert np.abs(r['rows'] - x.grad.numpy()).max() <= 1e-15


def test_the_cases_of_the_gpu_test():
    """Decided by the reference alone: fewer than a quarter of the live pixels of every combination carry a borderline element, the two K = 16 seeds
    have none at all, the single pixel is live, and class C - 1 is absent everywhere."""
    for C in LR.CS:
        for K in LR.KS:
            for P in LR.PS:
                for layout in LR.LAYOUTS:
                    lg, tg = LR.make_case(P, C, LR.case_seed(C, K, P, layout))
                    live = LR.live_mask(tg, C, 255)
                    bl = LR.borderline(lg, tg, 255, K)
                    assert live.sum() >= 1 and not (tg == C - 1).any()
                    assert bl.any(axis=1).sum() < 0.25 * live.sum(), (C, K, P, layout)
                    if K == 16 and P == 2048:
                        assert not bl.any(), (C, layout)
    lg, tg = LR.make_case(2048, 19, LR.EXACT_SEED[19])
    assert 0.05 < float((tg == 255).mean()) < 0.15
    r = LR.binned(lg, tg, 255, 1.0, 1024)
    assert 0.2 < r['exact'] < 0.9 and r['nb'][:, 0].sum() > 0.7 * r['nb'].sum()       # most background errors sit in level 0: the contended case


def test_the_fp32_restatement_is_the_same_row_to_fp32_accuracy():
    lg, tg = LR.make_case(2048, 19, 11)
    r = LR.binned(lg, tg, 255, 1.0, 1024)
    ok = ~r['borderline'].any(axis=1)
    g32 = LR.rows_fp32(lg, tg, 255, r['gf'].astype(np.float32), r['gb'].astype(np.float32), 1024)
    g64 = LR.rows_from_tables(lg, tg, 255, r['gf'].astype(np.float32), r['gb'].astype(np.float32), 1024)
    err = np.abs(g32[ok] - g64[ok]).max()
    assert 0 < err <= 2.0 ** -20 * float(max(np.abs(r['gf']).max(), np.abs(r['gb']).max()))


# ------------------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('value,want', [(None, None), (False, None), (np.False_, None), (0, None), (0.0, None), ((0, 64), None), (True, (1.0, 1024)),
                                        (0.5, (0.5, 1024)), (2, (2.0, 1024)), (np.float32(0.25), (0.25, 1024)), ((0.5, 16), (0.5, 16)),
                                        ([2, np.int64(4096)], (2.0, 4096)), ({'weight': 0.3}, (0.3, 1024)), ({'bins': 256}, (1.0, 256)),
                                        ({'weight': np.float64(3), 'bins': 64}, (3.0, 64))])
def test_lovasz_value_accepts(value, want):
    got = HF.lovasz_value(value)
    assert got == want
    if got is not None:
        assert type(got[0]) is float and type(got[1]) is int


@pytest.mark.parametrize('value', ['on', (0.5,), (0.5, 64, 2), {}, {'weight': 1.0, 'smooth': 1.0}, (True, 64), (1.0, True), (1.0, None), ('1', 64),
                                   -1.0, -1e-30, float('nan'), float('inf'), -float('inf'), 1e39, (1.0, 8), (1.0, 8192), (1.0, 100), (1.0, 64.0),
                                   (1.0, 0), (1.0, -16), (float('nan'), 64), {'weight': -2}, {'bins': 1000}, 1e-50])
def test_lovasz_value_rejects(value):
    with pytest.raises(ValueError, match='lovasz'):
        HF.lovasz_value(value)


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


def test_check_lovasz():
    assert TR.check_lovasz(_dataset()) is None
    for off in (None, False, 0, 0.0):
        assert TR.check_lovasz(_dataset(lovasz=off)) is None
    assert TR.check_lovasz(_dataset(lovasz=True)) == (1.0, 1024)
    assert TR.check_lovasz(_dataset(lovasz=0.5)) == (0.5, 1024)
    assert TR.check_lovasz(_dataset(lovasz=(2.0, 256))) == (2.0, 256)
    assert TR.check_lovasz(_dataset(lovasz={'weight': 0.6, 'bins': 4096}, class_weights='enet')) == (0.6, 4096)
    assert TR.check_lovasz(_dataset(lovasz=True, focal_gamma=0, label_smoothing=0.0, ohem=False, dice=None)) == (1.0, 1024)
    for bad in ('on', -1.0, (1.0, 100), {'lambda': 1.0}, float('nan')):
        with pytest.raises(ValueError, match='lovasz'):
            TR.check_lovasz(_dataset(lovasz=bad))
    for other in (dict(focal_gamma=2.0), dict(label_smoothing=0.1), dict(ohem=True), dict(dice=True)):
        with pytest.raises(ValueError, match='lovasz.*together'):
            TR.check_lovasz(_dataset(lovasz=True, **other))
        assert TR.check_lovasz(_dataset(lovasz=False, **other)) is None            # off: nothing to refuse


@pytest.mark.parametrize('extra', [dict(lovasz=-1.0), dict(lovasz='on'), dict(lovasz=True, focal_gamma=2.0), dict(lovasz=True, label_smoothing=0.1),
                                   dict(lovasz=True, ohem=True), dict(lovasz=True, dice=True)])
def test_train_or_resume_refuses_a_bad_lovasz_before_touching_a_device(extra):
    args = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=_dataset(loader_factory=lambda *a: [], **extra), val_interval=1, checkpoint_interval=1, checkpoint_history=1,
                init_weights=None, batch_size=1, epochs=1, learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4,
                poly_power=0.9, stage=1, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)
    with pytest.raises(ValueError, match='lovasz'):
        TR.train_or_resume(**args)


class _NoDevice:
    """stands in for a tensor: the refusals below must come before anything asks it for a device or a shape"""

    def __getattr__(self, name):
        raise AssertionError(f'touched .{name} before refusing the arguments')


@pytest.mark.parametrize('kw', [dict(focal_gamma=2.0), dict(label_smoothing=0.1), dict(ohem=True), dict(dice=True)])
def test_the_refused_combinations(kw, monkeypatch):
    def reached(name, *a):
        raise AssertionError(f'{name} reached the library')
    for fn in ('call', 'query', 'cquery'):
        monkeypatch.setattr(HF, fn, reached)
    nd = _NoDevice()
    with pytest.raises(ValueError, match='lovasz.*together'):
        HF.logits_target(None, 255, None, lovasz=True, **kw)
    with pytest.raises(ValueError, match='lovasz.*together'):
        HF.fused_losses((nd, nd, nd, nd), nd, nd, 255, 0.1, 1.0, 3, nd, lovasz=(1.0, 64), **kw)
    with pytest.raises(ValueError, match='lovasz.*together'):
        HF.cross_entropy(nd, nd, 255, lovasz=0.5, **kw)
    with pytest.raises(ValueError, match='lovasz.*together'):
        TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, lovasz=True, **kw)
    # off: nothing to refuse, and a bad value is refused as early
    assert HF._lovasz_args(None, kw.get('focal_gamma', 0.0), kw.get('label_smoothing', 0.0), HF.ohem_value(kw.get('ohem')), HF.dice_value(kw.get('dice'))) is None
    for bad in (-1.0, float('nan'), (1.0, 100), 'on'):
        with pytest.raises(ValueError, match='lovasz'):
            HF.fused_losses((nd, nd, nd, nd), nd, nd, 255, 0.1, 1.0, 3, nd, lovasz=bad)
        with pytest.raises(ValueError, match='lovasz'):
            HF.logits_target(None, 255, None, lovasz=bad)
        with pytest.raises(ValueError, match='lovasz'):
            TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, lovasz=bad)
        with pytest.raises(ValueError, match='lovasz'):
            HF.lovasz_softmax_loss(nd, nd, 255, *((bad,) if not isinstance(bad, tuple) else bad))


def test_logits_target_with_lovasz_still_engages_the_forward():
    t = torch.zeros((1, 2, 2), dtype=torch.uint8)
    assert HF.logits_target(t, 255, torch.zeros(1, dtype=torch.int32), lovasz=True).new is None     # a CPU target engages nothing, with or without
    assert HF.logits_target(None, 255, None, lovasz=(0.5, 64)).new is None


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


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_is_declared_and_registered(name):
    assert name in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES[name]
    names = _params(name)
    assert len(args) == len(names), f'{name}: {len(names)} parameters declared, {len(args)} registered'
    kinds = {'P': _lib.i64, 'C': _lib.i32, 'ld': _lib.i32, 'lddl': _lib.i32, 'ignore_index': _lib.i32, 'accumulate': _lib.i32, 'ft_stride': _lib.i32,
             'N': _lib.i32, 'H': _lib.i32, 'W': _lib.i32, 'Cin': _lib.i32, 'Cout': _lib.i32, 'lambda': _lib.f32, 'bins': _lib.i32,
             'ws_bytes': _lib.sz, 'stream': _lib.stream_t}
    for n, a in zip(names, args):
        assert a is kinds.get(n, _lib.fp), (name, n)
    assert res is (_lib.sz if name.endswith(('_bytes', '_floats')) else _lib.i32)


OK_FWD = dict(logits=0x1000, target=0x2000, record=0x3000, ws=0x5000, P=10, C=19, ld=19, ws_bytes=1 << 30, bins=1024)
OK_FWD['lambda'] = 1.0
OK_BWD = dict(logits=0x1000, target=0x2000, record=0x3000, dlogits=0x4000, P=10, C=19, ld=19, lddl=19, bins=1024)


def test_the_size_queries_are_the_layout():
    ws = lambda P, C, K: _lib.query('dsrl_lovasz_workspace_bytes', P, C, K)     # noqa: E731
    rf = lambda C, K: _lib.query('dsrl_lovasz_record_floats', C, K)             # noqa: E731
    tail = 64 * (8 + 4) + 16                        # double L_c[64], uint32 G_c[64], the NaN word padded to 16 bytes
    for C in (1, 3, 19, 60):
        for K in (16, 64, 1024, 4096):
            assert rf(C, K) == 4 + 2 * C * K        # {lambda L, |Present|, padding to 16 bytes, gf[C][K], gb[C][K]}
            for P in (1, 63, 70001, 8 * 512 * 1024, 2 ** 31 - 257):            # the arguments alone: P bounds the counts, not the size
                assert ws(P, C, K) == 2 * C * K * 4 + tail, (P, C, K)
    for bad in ((0, 19, 1024), (-3, 19, 1024), (2 ** 31 - 256, 19, 1024), (10, 0, 1024), (10, 61, 1024), (10, 19, 8), (10, 19, 8192), (10, 19, 100)):
        assert ws(*bad) == 0 and _lib.load().dsrl_last_error().decode().startswith('lovasz_workspace_bytes: bad arguments'), bad
    for bad in ((0, 1024), (61, 1024), (19, 8), (19, 8192), (19, 48)):
        assert rf(*bad) == 0 and _lib.load().dsrl_last_error().decode().startswith('lovasz_record_floats: bad arguments'), bad


@pytest.mark.parametrize('lam', [0.0, -1.0, float('nan'), float('inf'), -float('inf'), -1e-30])
def test_a_bad_lambda_is_refused_first(lam):
    code, msg = _call('dsrl_lovasz_fwd', **dict(OK_FWD, **{'lambda': lam, 'logits': None}))
    want = 'nan' if math.isnan(lam) else (('-inf' if lam < 0 else 'inf') if math.isinf(lam) else '%g' % _lib.f32(lam).value)
    assert code == BADARG and msg == f'lovasz_fwd: lambda = {want} must be a finite number > 0', msg


def test_the_other_argument_errors():
    for bad in (dict(logits=None), dict(target=None), dict(record=None), dict(ws=None), dict(ld=18), dict(record=0x3002)):
        code, msg = _call('dsrl_lovasz_fwd', **dict(OK_FWD, **bad))
        assert code == BADARG and msg.startswith('lovasz_fwd: bad arguments'), (bad, msg)
    for bad in (dict(P=0), dict(P=-5), dict(P=2 ** 31 - 256), dict(P=2 ** 31), dict(C=0), dict(C=61), dict(bins=0), dict(bins=8), dict(bins=8192),
                dict(bins=1000), dict(bins=-1024)):
        for name, ok in (('dsrl_lovasz_fwd', OK_FWD), ('dsrl_lovasz_bwd', OK_BWD)):
            code, msg = _call(name, **dict(ok, **bad))
            assert code == BADARG and msg.startswith(name[5:] + ': P = '), (name, bad, msg)
    assert _call('dsrl_lovasz_fwd', **dict(OK_FWD, P=2 ** 31 - 257, ws_bytes=0))[0] == WORKSPACE       # the largest P passes the argument check
    need = _lib.query('dsrl_lovasz_workspace_bytes', 10, 19, 1024)
    for bad in (dict(ws_bytes=need - 1), dict(ws=0x5008)):
        code, msg = _call('dsrl_lovasz_fwd', **dict(OK_FWD, **bad))
        assert code == WORKSPACE and msg == 'lovasz_fwd: workspace too small or misaligned', (bad, msg)
    for bad in (dict(logits=None), dict(target=None), dict(record=None), dict(dlogits=None), dict(ld=18), dict(lddl=18), dict(accumulate=2),
                dict(accumulate=-1), dict(record=0x3001)):
        code, msg = _call('dsrl_lovasz_bwd', **dict(OK_BWD, **bad))
        assert code == BADARG and msg.startswith('lovasz_bwd: bad arguments'), (bad, msg)
    code, msg = _call('dsrl_convt2x2_bwd_ce_l')
    assert code == BADARG and msg.startswith('convt2x2_bwd_ce_l: bad arguments'), msg
    for bins in (0, 8, 100, 8192):
        code, msg = _call('dsrl_convt2x2_bwd_ce_l', lovasz_record=0x3000, bins=bins)
        assert code == BADARG and msg.startswith('convt2x2_bwd_ce_l: bad arguments (no Lovasz record'), msg
    code, msg = _call('dsrl_convt2x2_bwd_ce_l', lovasz_record=0x3000, bins=1024)
    assert code == BADARG and msg.startswith('convt2x2_bwd_ce_l: bad arguments'), msg


def test_lovasz_bin_is_in_range_for_every_bit_pattern():
    """The arithmetic of lovasz_bin (csrc/common.h) restated in numpy float32 on special values and a sweep of bit patterns: fmaxf(x, 0) of a NaN is
    0, the clamp bounds +-inf, the mask holds the range whatever came before"""
    bits = np.concatenate([np.array([0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000, 0x7f800001, 0x00000001, 0x80000000, 0x3f800000, 0x3f7fffff,
                                     0x7f7fffff, 0xff7fffff], np.uint32), np.arange(0, 2 ** 32, 65521, dtype=np.uint64).astype(np.uint32)])
    err = bits.view(np.float32)
    for K in (16, 1024, 4096):
        with np.errstate(all='ignore'):
            x = np.fmin(np.fmax(err * np.float32(K), np.float32(0)), np.float32(K - 1))
        b = x.astype(np.int64) & (K - 1)
        assert b.min() >= 0 and b.max() <= K - 1
        assert b[0] == 0 and b[2] == K - 1 and b[3] == 0 and b[7] == K - 1 and b[8] == K - 1
        fin = np.isfinite(err) & (err >= 0) & (err <= 1)
        assert np.array_equal(b[fin], LR.bins_of(err[fin].astype(np.float64), K))

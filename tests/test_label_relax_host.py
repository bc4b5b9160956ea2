"""Host side of boundary label relaxation: what HF.label_relax_value and train_or_resume.check_label_relax accept, the
combinations that are refused before anything touches a device, the argument errors, declarations and size queries of the new entry points
(returned before any HIP call, so pinned here), and the reference of tests/label_relax_ref.py checked against itself - the two mask formulations,
the singleton identity with the weighted loss, finite differences, the fp32 restatement and the set-size shares the GPU test's inputs must have.
Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import label_relax_ref as RR

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS

BADARG = -1                                         # include/dsrl_hip.h: DSRL_E_BADARG
FAMILIES = ['dsrl_ce_fwd', 'dsrl_ce_bwd', 'dsrl_ce_fused', 'dsrl_convt2x2_fwd_ce', 'dsrl_convt2x2_bwd_ce']
AFTER_IGNORE_INDEX = {'dsrl_ce_fwd': 6, 'dsrl_ce_bwd': 6, 'dsrl_ce_fused': 6, 'dsrl_convt2x2_fwd_ce': 11, 'dsrl_convt2x2_bwd_ce': 5}
QUERIES = ['dsrl_ce%s_workspace_bytes', 'dsrl_ce_fused%s_workspace_bytes', 'dsrl_convt2x2_fwd_ce%s_workspace_bytes']
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dsrl_hip.h')


# ------------------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('value,want', [(None, None), (False, None), (np.False_, None), (0, None), (0.0, None), (True, 1), (np.True_, 1), (1, 1), (2, 2),
                                        (4, 4), (3.0, 3), (np.int64(2), 2), (np.float32(4), 4), ({'radius': 1}, 1), ({'radius': 4.0}, 4)])
def test_label_relax_value_accepts(value, want):
    got = HF.label_relax_value(value)
    assert got == want and (got is None or type(got) is int)


@pytest.mark.parametrize('value', [5, -1, 1.5, float('nan'), float('inf'), 'on', '1', (1,), [2], {}, {'r': 1}, {'radius': 1, 'shape': 'box'},
                                   {'radius': True}, {'radius': None}, {'radius': 0}, {'radius': 5}, {'radius': 2.5}, 1e39])
def test_label_relax_value_rejects(value):
    with pytest.raises(ValueError, match='label_relax'):
        HF.label_relax_value(value)


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


OTHERS = [dict(focal_gamma=2.0), dict(label_smoothing=0.1), dict(ohem=True), dict(dice=True), dict(lovasz=True)]


def test_check_label_relax():
    assert TR.check_label_relax(_dataset()) is None
    for off in (None, False, 0):
        assert TR.check_label_relax(_dataset(label_relax=off)) is None
    assert TR.check_label_relax(_dataset(label_relax=True)) == 1
    assert TR.check_label_relax(_dataset(label_relax=3, class_weights='enet')) == 3
    assert TR.check_label_relax(_dataset(label_relax={'radius': 2}, focal_gamma=0, label_smoothing=0.0, ohem=False, dice=None, lovasz=None)) == 2
    for bad in ('on', 5, 1.5, {'r': 1}, torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match='label_relax'):
            TR.check_label_relax(_dataset(label_relax=bad))
    for other in OTHERS:
        with pytest.raises(ValueError, match='label_relax.*together'):
            TR.check_label_relax(_dataset(label_relax=True, **other))
        assert TR.check_label_relax(_dataset(label_relax=False, **other)) is None          # off: nothing to refuse


@pytest.mark.parametrize('extra', [dict(label_relax=5), dict(label_relax='on')] + [dict(label_relax=True, **o) for o in OTHERS])
def test_train_or_resume_refuses_a_bad_label_relax_before_touching_a_device(extra):
    args = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=_dataset(loader_factory=lambda *a: [], **extra), val_interval=1, checkpoint_interval=1, checkpoint_history=1,
                init_weights=None, batch_size=1, epochs=1, learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4,
                poly_power=0.9, stage=1, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)
    with pytest.raises(ValueError, match='label_relax'):
        TR.train_or_resume(**args)


class _NoDevice:
    """stands in for a tensor: the refusals below must come before anything asks it for a device or a shape"""

    def __getattr__(self, name):
        raise AssertionError(f'touched .{name} before refusing the arguments')


@pytest.mark.parametrize('kw', OTHERS)
def test_the_refused_combinations(kw, monkeypatch):
    def reached(name, *a):
        raise AssertionError(f'{name} reached the library')
    for fn in ('call', 'query', 'cquery'):
        monkeypatch.setattr(HF, fn, reached)
    nd = _NoDevice()
    ready = torch.zeros((1, 2, 2), dtype=torch.int32)               # a ready mask is refused in the same combinations
    for value in (True, 2, {'radius': 1}, ready):
        with pytest.raises(ValueError, match='label_relax.*together'):
            HF.logits_target(None, 255, None, label_relax=value, **kw)
        with pytest.raises(ValueError, match='label_relax.*together'):
            HF.fused_losses((nd, nd, nd, nd), nd, nd, 255, 0.1, 1.0, 3, nd, label_relax=value, **kw)
        with pytest.raises(ValueError, match='label_relax.*together'):
            HF.cross_entropy(nd, nd, 255, label_relax=value, **kw)
    with pytest.raises(ValueError, match='label_relax.*together'):
        TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, label_relax=True, **kw)
    args = (kw.get('focal_gamma', 0.0), kw.get('label_smoothing', 0.0), HF.ohem_value(kw.get('ohem')), HF.dice_value(kw.get('dice')),
            HF.lovasz_value(kw.get('lovasz')))
    with pytest.raises(ValueError, match='label_relax.*together'):
        HF._label_relax_args(1, *args)
    assert HF._label_relax_args(None, *args) is None and HF._label_relax_args(0, *args) is None      # off: nothing to refuse
    for bad in (5, 1.5, 'on', {'r': 1}, torch.zeros(2, dtype=torch.float32)):
        with pytest.raises(ValueError, match='label_relax'):
            HF.fused_losses((nd, nd, nd, nd), nd, nd, 255, 0.1, 1.0, 3, nd, label_relax=bad)
        with pytest.raises(ValueError, match='label_relax'):
            HF.logits_target(None, 255, None, label_relax=bad)
        with pytest.raises(ValueError, match='label_relax'):
            HF.cross_entropy(nd, nd, 255, label_relax=bad)
        with pytest.raises(ValueError, match='label_relax'):
            TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, label_relax=bad)
    with pytest.raises(ValueError, match='label_relax'):
        TR.TrainStep(None, nd, 3, 0.1, 1.0, 255, graph=False, label_relax=ready)        # a step takes the setting, never a mask


def test_alone_or_with_class_weights_it_is_accepted():
    assert HF._label_relax_args(True, 0.0, 0.0, None, None, None) == 1
    assert HF._label_relax_args({'radius': 4}, 0.0, 0.0, None, None, None) == 4
    ready = torch.zeros((1, 2, 2), dtype=torch.int32)
    assert HF._label_relax_args(ready, 0.0, 0.0, None, None, None) is ready
    assert HF.logits_target(torch.zeros((1, 2, 2), dtype=torch.uint8), 255, torch.zeros(1, dtype=torch.int32), label_relax=2).new is None    # a CPU target engages nothing
    assert HF.logits_target(None, 255, None, label_relax=True).new is None


class _Table:
    def data_ptr(self):
        return 0x1000


class _Mask:
    def data_ptr(self):
        return 0x2000


def test_the_variant_helper_keeps_its_four_answers_and_gains_the_fifth():
    t = _Table()
    assert HF._ce_variant(None, 0.0, 0.0) == ('', ())
    assert HF._ce_variant(t, 0.0, 0.0) == ('_w', (0x1000,))
    assert HF._ce_variant(t, 2.0, 0.0) == ('_f', (0x1000, 2.0))
    assert HF._ce_variant(t, 0.0, 0.25) == ('_s', (0x1000, 0.25))
    assert HF._ce_variant(t, 0.0, 0.0, None) == ('_w', (0x1000,))
    assert HF._ce_variant(t, 0.0, 0.0, _Mask()) == ('_r', (0x1000, 0x2000))
    assert 'relax' in HF.LogitsGrad.__slots__ and HF.LogitsGrad().relax is None


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
    args = [None if t is _lib.fp else 0 for t in _lib.PROTOTYPES[name][1]]
    for k, v in named.items():
        args[names.index(k)] = v
    code = getattr(lib, name)(*args)
    return code, lib.dsrl_last_error().decode()


@pytest.mark.parametrize('family', FAMILIES)
def test_the_relaxed_prototype_is_the_plain_one_plus_two_pointers_after_ignore_index(family):
    plain, relaxed = _lib.PROTOTYPES[family][1], _lib.PROTOTYPES[family + '_r'][1]
    k = AFTER_IGNORE_INDEX[family]
    assert len(relaxed) == len(plain) + 2
    assert relaxed[:k] + relaxed[k + 2:] == plain and relaxed[k:k + 2] == [_lib.fp, _lib.fp]
    assert relaxed == _lib.PROTOTYPES[family + '_w'][1][:k + 1] + [_lib.fp] + _lib.PROTOTYPES[family + '_w'][1][k + 1:]
    names = _params(family + '_r')
    assert len(names) == len(relaxed) and names[k - 1] == 'ignore_index' and names[k:k + 2] == ['weights', 'mask']


@pytest.mark.parametrize('name', [f + '_r' for f in FAMILIES])
def test_null_pointers_are_a_bad_argument_in_the_entrys_own_name(name):
    code, msg = _call(name)
    assert code == BADARG and msg.startswith(name[len('dsrl_'):] + ': bad arguments'), msg
    # everything of the weighted form in place but the mask: still refused
    w = _call(name, weights=0x3000)
    assert w[0] == BADARG and w[1].startswith(name[len('dsrl_'):] + ': bad arguments'), w


def test_more_than_32_classes_are_refused():
    ok = dict(logits=0x1000, target=0x2000, weights=0x3000, mask=0x4000, loss_out=0x5000, ws=0x6000, P=10, ld=40, ws_bytes=1 << 30)
    for C in (33, 60):
        code, msg = _call('dsrl_ce_fwd_r', C=C, **ok)
        assert code == BADARG and msg.startswith('ce_fwd_r: bad arguments'), msg
        code, msg = _call('dsrl_ce_fused_r', C=C, **ok)
        assert code == BADARG and msg.startswith('ce_fused_r: bad arguments'), msg


def test_relax_mask_argument_errors():
    assert _lib.PROTOTYPES['dsrl_relax_mask'] == (_lib.i32, [_lib.fp, _lib.i32, _lib.i32, _lib.i32, _lib.i32, _lib.i32, _lib.i32, _lib.fp, _lib.fp, _lib.stream_t])
    assert _params('dsrl_relax_mask') == ['target', 'N', 'H', 'W', 'C', 'ignore_index', 'radius', 'mask', 'stats', 'stream']
    ok = dict(target=0x1000, mask=0x2000, N=1, H=4, W=4, C=19, ignore_index=255, radius=1)
    code, msg = _call('dsrl_relax_mask', **dict(ok, target=None))
    assert code == BADARG and msg.startswith('relax_mask: bad arguments'), msg
    for bad in (dict(mask=None), dict(N=0), dict(H=0), dict(W=-1), dict(mask=0x2002), dict(stats=0x3004)):
        code, msg = _call('dsrl_relax_mask', **dict(ok, **bad))
        assert code == BADARG and msg.startswith('relax_mask: bad arguments'), (bad, msg)
    for radius in (0, -1, 5, 100):                                      # refused first: with every pointer null as well
        for base in (ok, dict(C=19)):
            code, msg = _call('dsrl_relax_mask', **dict(base, radius=radius))
            assert code == BADARG and msg == f'relax_mask: radius = {radius} is not in [1, 4]', msg
    for C in (0, -3, 33, 60):
        for base in (ok, dict(radius=1)):
            code, msg = _call('dsrl_relax_mask', **dict(base, C=C))
            assert code == BADARG and msg == f'relax_mask: C = {C} is not in [1, 32]', msg


def test_the_workspace_queries_are_those_of_the_weighted_form():
    for q in QUERIES:
        assert _lib.PROTOTYPES[q % '_r'] == _lib.PROTOTYPES[q % '_w']
    for P in (1, 63, 2048, 70001, 8 * 512 * 1024):
        assert _lib.query('dsrl_ce_r_workspace_bytes', P) == _lib.query('dsrl_ce_w_workspace_bytes', P) > 0
        assert _lib.query('dsrl_ce_fused_r_workspace_bytes', P) == _lib.query('dsrl_ce_fused_w_workspace_bytes', P) > 0
    for shape in ((1, 3, 200), (2, 5, 128), (8, 256, 512)):
        assert _lib.query('dsrl_convt2x2_fwd_ce_r_workspace_bytes', *shape) == _lib.query('dsrl_convt2x2_fwd_ce_w_workspace_bytes', *shape) > 0


# ------------------------------------------------------------------------------------------------------------------------------ the reference
W19 = np.linspace(0.5, 2.0, 19)


@pytest.mark.parametrize('r', [1, 2, 4])
@pytest.mark.parametrize('C,ii', [(19, 255), (3, 0), (32, -1)])
def test_the_two_mask_formulations_agree(C, ii, r):
    for shape, b in (((1, 1, 1), 4), ((1, 3, 5), 2), ((2, 37, 130), 8), ((3, 5, 131), 4)):
        tg = RR.block_labels(*shape, C, b, 11 + r, ii if ii >= 0 else 255, p_bad=0.05 if C < 32 else 0.0)
        a, sa = RR.mask_ref(tg, C, ii, r, 'window')
        s, ss = RR.mask_ref(tg, C, ii, r, 'separable')
        assert np.array_equal(a, s) and sa == ss
        t64 = tg.astype(np.int64)
        dead = (t64 == ii) | (t64 >= C)
        assert not a[dead].any()
        own = np.left_shift(np.uint64(1), np.where(dead, 0, t64).astype(np.uint64)).astype(np.uint32)
        assert np.all((a[~dead] & own[~dead]) != 0)                    # a live pixel's set holds its own label
        assert not (a >> np.uint32(C)).any() if C < 32 else True


def test_sets_do_not_cross_an_image_or_wrap_a_row():
    tg = np.zeros((2, 6, 7), np.uint8); tg[1] = 5
    for r in (1, 2, 4):
        m, (live, multi) = RR.mask_ref(tg, 19, 255, r)
        assert multi == 0 and live == tg.size and np.all(m[0] == 1) and np.all(m[1] == 32)
    tg = np.zeros((1, 4, 6), np.uint8); tg[0, :, -1] = 3                # the last column: its class reaches r columns back, never the next row's start
    m, _ = RR.mask_ref(tg, 19, 255, 1)
    assert np.all(m[0, :, 0] == 1) and np.all(m[0, :, -2] == 9)


@pytest.mark.parametrize('b,r', [(4, 1), (8, 1), (8, 2)])
def test_the_generators_set_size_shares(b, r):
    """every input of the accuracy checks has >= 20 % one-class sets, >= 20 % larger ones, a set of three and a set of four or more"""
    for C in (19, 3):
        if C == 3 and (b, r) == (8, 1):
            continue                # three classes on the 8-grid at radius 1: neighbouring blocks agree too often (18 % larger sets); the GPU test uses b = 4 there
        for P in (2048, 70001):
            lg, tg, mk = RR.make_case(P, C, 5 + C, b=b, r=r)
            s = RR.set_size_shares(mk, tg, C, 255)
            assert s[0] >= 0.2 and s[1] + s[2] + s[3] >= 0.2, (b, r, C, P, s)
            if C >= 4:
                assert s[2] > 0 and s[3] > 0, (b, r, C, P, s)
            else:
                assert s[2] > 0, (b, r, C, P, s)                        # three classes: the full set is the largest there is
    tg = RR.block_labels(2, 64, 256, 19, b, 3)
    mk, (live, multi) = RR.mask_ref(tg, 19, 255, r)
    s = RR.set_size_shares(mk, tg, 19, 255)
    assert s[0] >= 0.2 and 1.0 - s[0] >= 0.2 and s[2] > 0 and s[3] > 0 and abs(multi / live - (1.0 - s[0])) < 1e-12


@pytest.mark.parametrize('C', [19, 3])
def test_singleton_masks_give_the_weighted_loss_and_row_exactly(C):
    w = W19[:C]
    lg, tg, _ = RR.make_case(1500, C, 21)
    zero = np.zeros(len(tg), np.uint32)
    own = RR.clean(zero, np.where(tg == 255, C, tg), C)
    for mk in (zero, own, own | np.uint32(1 << C)):                     # no bits, the own label's bit, and a bit of a class that does not exist
        L, G, D = RR.relaxed_loss_and_grad(lg, tg, 255, w, mk)
        Lw, Gw, Dw = RR.weighted_loss_and_grad(lg, tg, 255, w)
        assert L == Lw and D == Dw and np.array_equal(G, Gw)
    L32, G32, D32 = RR.emulate_fp32(lg, tg, 255, w, zero)
    f = np.float32
    v = lg.astype(f); live = tg != 255; t = np.where(live, tg, 0)
    m = v.max(axis=1); e = np.exp(v - m[:, None]).astype(f)
    s = np.zeros(len(t), f)
    for c in range(C):
        s = (s + e[:, c]).astype(f)
    sc = (np.where(live, w.astype(f)[t], f(0)) * (f(1) / D32)).astype(f)
    onehot = np.zeros_like(e); onehot[np.arange(len(t)), t] = 1
    row = ((e * (sc / s).astype(f)[:, None]).astype(f) - (onehot * sc[:, None]).astype(f)).astype(f)
    assert np.array_equal(G32[live], row[live])                         # e_c (sc / s) - [c == t] sc, bit for bit


@pytest.mark.parametrize('C', [19, 3])
def test_finite_differences_and_the_fp32_restatement(C):
    w = W19[:C]
    lg, tg, mk = RR.make_case(300, C, 33, b=4)
    lg64 = lg.astype(np.float64)
    L, G, D = RR.relaxed_loss_and_grad(lg64, tg, 255, w, mk)
    rs = np.random.RandomState(1)
    h = 1e-6
    worst = 0.0
    for _ in range(40):
        p, c = rs.randint(0, 300), rs.randint(0, C)
        up = lg64.copy(); up[p, c] += h
        dn = lg64.copy(); dn[p, c] -= h
        fd = (RR.relaxed_loss_and_grad(up, tg, 255, w, mk)[0] - RR.relaxed_loss_and_grad(dn, tg, 255, w, mk)[0]) / (2 * h)
        worst = max(worst, abs(fd - G[p, c]))
    assert worst < 1e-8, worst
    assert np.abs(G.sum(axis=1)).max() < 1e-15                          # both softmaxes sum to one: every row sums to zero
    L32, G32, D32 = RR.emulate_fp32(lg, tg, 255, w, mk)
    assert abs(float(L32) - L) <= RR.loss_bound(lg, tg, 255, L)
    assert np.all(np.abs(G32.astype(np.float64) - G) <= RR.grad_bound(tg, 255, w, mk, C))


def test_the_set_softmax_is_relative_to_its_own_maximum():
    """a pixel whose set classes all lie 200 below its largest logit: finite value and row, in float64 and in the fp32 restatement, where a
    -log(sum_S e_c / s) on the shared terms would be infinite; and a seventh of the pixels scaled by 40 stays finite"""
    C = 5
    lg = np.array([[0.0, -200.0, -201.0, 3.0, -5.0]], np.float32)
    tg = np.array([1], np.uint8); mk = np.array([0b110], np.uint32)
    w = np.ones(C)
    L, G, _ = RR.relaxed_loss_and_grad(lg, tg, 255, w, mk)
    L32, G32, _ = RR.emulate_fp32(lg, tg, 255, w, mk)
    assert np.isfinite(L) and 200 < L < 204 and np.isfinite(L32) and abs(float(L32) - L) <= RR.loss_bound(lg, tg, 255, L)
    assert np.all(np.isfinite(G32)) and np.all(np.abs(G32 - G) <= RR.grad_bound(tg, 255, w, mk, C))
    lg, tg, mk = RR.make_case(700, 19, 4, b=4)
    lg[::7] *= 40
    L, G, _ = RR.relaxed_loss_and_grad(lg, tg, 255, W19, mk)
    L32, G32, _ = RR.emulate_fp32(lg, tg, 255, W19, mk)
    assert np.isfinite(L) and np.isfinite(L32) and np.all(np.isfinite(G32))

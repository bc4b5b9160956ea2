"""CPU-only checks of sliding-window inference: the planner (functional.window_value / window_plan) against brute force, the store-or-add rule the
merge launches rest on, the host part of the dsrl_window_merge ABI, every refusal that must come before any device work, and self-checks of the fp64
restatement (window_ref) with the condition the GPU class-map tests rest on (few near-ties of the ensemble in every fixture)."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import multiscale_ref as MR
import predict_fixtures as PF
import predict_flip_ref as PFR
import window_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('dsrl_window_merge_supported', 'dsrl_window_merge_workspace_bytes', 'dsrl_window_merge', 'dsrl_window_merge_finish',
                'dsrl_window_merge_finish_ex')
AXES = [(64, 32, 21), (96, 48, 32), (70, 33, 12), (1024, 512, 341), (48, 16, 16), (160, 96, 32), (33, 33, 5), (40, 7, 1), (100, 30, 30)]


# ---------------------------------------------------------------------------------------------- the planner
def test_the_four_plans_of_the_definition():
    from dualsuperreslearningforsemseg_amd.functional import window_positions
    assert window_positions(64, 32, 21) == (0, 21, 32)
    assert window_positions(96, 48, 32) == (0, 32, 48)
    assert window_positions(70, 33, 12) == (0, 12, 24, 36, 37)
    assert window_positions(1024, 512, 341) == (0, 341, 512)
    for S, w, s in AXES:
        assert window_positions(S, w, s) == WR.positions(S, w, s)


@pytest.mark.parametrize('S, w, s', AXES)
def test_positions_cover_the_axis_and_increase(S, w, s):
    from dualsuperreslearningforsemseg_amd.functional import window_positions
    a = window_positions(S, w, s)
    assert len(a) == max(S - w + s - 1, 0) // s + 1 and a[0] == 0 and a[-1] + w == S
    assert all(q > p for p, q in zip(a, a[1:])) and all(q <= p + w for p, q in zip(a, a[1:]))
    cnt = np.zeros(S, np.int64)
    for p in a:
        cnt[p:p + w] += 1
    assert cnt.min() >= 1                                       # brute-force cover count: no pixel is left out


def test_window_value():
    from dualsuperreslearningforsemseg_amd.functional import window_value as value
    assert value(None) is None and value(None, None) is None
    assert value((256, 512)) == ((256, 512), (171, 342)) and value(32) == ((32, 32), (22, 22))          # ceil(2 side / 3)
    assert value((32, 48), (21, 32)) == ((32, 48), (21, 32)) and value([32, 48], 16) == ((32, 48), (16, 16))
    assert value((np.int64(32), np.int32(48))) == ((32, 48), (22, 32)) and all(type(v) is int for pair in value(np.array([32, 48])) for v in pair)
    for bad in (True, (True, 32), '32', ('32', '48'), torch.tensor([32, 48]), 32.0, (32.0, 48), (32,), (32, 48, 64), 0, (0, 32), (32, -16), object(),
                (None, 32), b'32'):
        with pytest.raises(ValueError, match='window'):
            value(bad)
        with pytest.raises(ValueError, match='stride'):
            value((32, 48), bad)
    with pytest.raises(ValueError, match='stride'):
        value(None, 16)                                         # a stride without a window


def test_window_plan():
    from dualsuperreslearningforsemseg_amd.functional import window_plan as plan
    assert plan(64, 96, (32, 48), (21, 32)) == ((0, 21, 32), (0, 32, 48))
    assert plan(512, 1024, (256, 512)) == ((0, 171, 256), (0, 342, 512))
    assert plan(64, 96, None) is None and plan(64, 96, (64, 96)) is None and plan(64, 96, (64, 96), (8, 8)) is None       # the whole image is "off"
    assert plan(64, 96, 32, 32) == ((0, 32), (0, 32, 64))
    assert len(plan(512, 512, 16, 16)[0]) == 32
    with pytest.raises(ValueError, match='larger than the image'):
        plan(64, 96, (80, 96))
    with pytest.raises(ValueError, match='larger than the image'):
        plan(64, 96, (64, 112))
    with pytest.raises(ValueError, match='uncovered'):
        plan(64, 96, (32, 48), (33, 48))
    with pytest.raises(ValueError, match='uncovered'):
        plan(64, 96, (32, 48), (32, 49))
    for H, W, win in ((64, 96, (24, 48)), (64, 96, (32, 40)), (72, 96, (32, 48)), (64, 100, (32, 48))):
        with pytest.raises(ValueError, match='multiple of 16'):
            plan(H, W, win)
    with pytest.raises(ValueError, match='32'):
        plan(528, 512, 16, 16)                                  # 33 positions
    with pytest.raises(ValueError, match='32'):
        plan(64, 1024, (16, 16), (16, 1))
    with pytest.raises(ValueError, match='window'):
        plan(64, 96, 'all')


@pytest.mark.parametrize('ay, ax', [((64, 32, 21), (96, 48, 32)), ((70, 33, 12), (64, 32, 21)), ((48, 16, 16), (70, 33, 12)), ((33, 33, 5), (160, 96, 32)),
                                    ((40, 7, 1), (100, 30, 30))])
def test_fresh_rule_against_brute_force(ay, ax):
    """Positions visited row-major: pixel (wy, wx) of window (i, j) has NOT been covered by an earlier window iff wy >= fresh_y and wx >= fresh_x."""
    from dualsuperreslearningforsemseg_amd.functional import window_fresh, window_positions
    ys, xs = window_positions(*ay), window_positions(*ax)
    h, w = ay[1], ax[1]
    seen = np.zeros((ay[0], ax[0]), bool)
    for i, y0 in enumerate(ys):
        for j, x0 in enumerate(xs):
            fy, fx = window_fresh(ys, h, i), window_fresh(xs, w, j)
            assert 0 <= fy < h + (i == 0) and 0 <= fx < w + (j == 0)
            want = np.zeros((h, w), bool)
            want[fy:, fx:] = True
            assert np.array_equal(~seen[y0:y0 + h, x0:x0 + w], want), (i, j)
            seen[y0:y0 + h, x0:x0 + w] = True
    assert seen.all()


# ---------------------------------------------------------------------------------------------- the ABI
def test_window_entry_points_are_exported_prototyped_and_declared():
    from dualsuperreslearningforsemseg_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dsrl_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), name
    assert len(_lib.PROTOTYPES['dsrl_window_merge'][1]) == 15 and len(_lib.PROTOTYPES['dsrl_window_merge_finish'][1]) == 22
    assert len(_lib.PROTOTYPES['dsrl_window_merge_finish_ex'][1]) == 25
    assert re.search(r'\bint\s+dsrl_window_merge\s*\(const float\* logits, int ld, int N, int hw, int ww, int C, int mirror, float\* acc, int Ho, int Wo, '
                     r'int oy, int ox, int fresh_y,\s+int fresh_x,', header)
    assert 'sliding-window ensemble' in header
    assert 'window.hip' in open(os.path.join(ROOT, 'dualsuperreslearningforsemseg_amd', 'csrc', 'Makefile')).read()


def test_supported_and_size_queries_are_pure_host_code():
    from dualsuperreslearningforsemseg_amd import _lib
    q = _lib.query
    for _, n, ho, wo, (wh, ww), _, _, _ in WR.FIXTURES:
        assert q('dsrl_window_merge_supported', n, wh, ww, ho, wo, 19) == 1
        ws = q('dsrl_window_merge_workspace_bytes', n, ho, wo)
        assert ws >= 16 and ws % 16 == 0 and ws == q('dsrl_prob_merge_workspace_bytes', n, ho, wo)
    assert q('dsrl_window_merge_supported', 1, 8, 8, 8, 8, 32) == 1 and q('dsrl_window_merge_supported', 1, 8, 8, 8, 8, 1) == 1
    assert q('dsrl_window_merge_supported', 1, 8, 8, 8, 8, 33) == 0 and q('dsrl_window_merge_supported', 1, 8, 8, 8, 8, 0) == 0
    assert q('dsrl_window_merge_supported', 1, 9, 8, 8, 8, 19) == 0 and q('dsrl_window_merge_supported', 1, 8, 9, 8, 8, 19) == 0       # window outside the grid
    for bad in ((0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 0, 8, 8)):
        assert q('dsrl_window_merge_supported', *bad, 19) == 0
    assert q('dsrl_window_merge_supported', 8, 512, 1024, 1024, 2048, 19) == 1
    assert q('dsrl_window_merge_supported', 64, 512, 1024, 1024, 2048, 19) == 0             # the Python side splits by image
    assert q('dsrl_window_merge_supported', 1, 512, 1024, 1024, 2048, 19) == 1
    assert q('dsrl_window_merge_workspace_bytes', 0, 4, 4) == 0


def test_argument_errors_come_before_any_launch():
    """null pointers reach no kernel: every one of these is refused by the host checks, with a message"""
    from dualsuperreslearningforsemseg_amd import _lib
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)           # noqa: E731
    fake = 4096                                             # a non-null, aligned address that is never dereferenced
    assert lib.dsrl_window_merge(None, 19, 1, 8, 8, 19, 0, fake, 8, 8, 0, 0, 0, 0, None) == -1 and b'null' in lib.dsrl_last_error()
    assert lib.dsrl_window_merge(fake, 19, 1, 8, 8, 19, 0, fake, 12, 12, 5, 0, 0, 0, None) == -1 and b'leaves' in lib.dsrl_last_error()
    assert lib.dsrl_window_merge(fake, 19, 1, 8, 8, 19, 0, fake, 12, 12, 0, -1, 0, 0, None) == -1 and b'leaves' in lib.dsrl_last_error()
    assert lib.dsrl_window_merge(fake, 19, 1, 8, 8, 19, 0, fake, 12, 12, 0, 0, 9, 0, None) == -1 and b'fresh' in lib.dsrl_last_error()
    assert lib.dsrl_window_merge(fake, 19, 1, 8, 8, 40, 0, fake, 12, 12, 0, 0, 0, 0, None) == -2 and b'C <= 32' in lib.dsrl_last_error()
    assert lib.dsrl_window_merge(fake, 18, 1, 8, 8, 19, 0, fake, 12, 12, 0, 0, 0, 0, None) == -1 and b'ld < C' in lib.dsrl_last_error()

    def finish(ys, xs, hw=8, ww=8, ho=12, wo=12, ny=None, nx=None, ce=None, ws=None, ws_bytes=0, target=None, counts=None):
        return lib.dsrl_window_merge_finish(fake, 1, 19, ho, wo, ints(*ys), len(ys) if ny is None else ny, ints(*xs), len(xs) if nx is None else nx, hw, ww, 1,
                                            fake, target, 255, counts, ce, None, ws, ws_bytes, None, None)
    for ys, xs in (((0, 3), (0, 4)),            # ends at 11
                   ((0, 4), (0, 5)),            # ends at 13
                   ((1, 4), (0, 4)),            # does not start at 0
                   ((0, 4, 4), (0, 4)),         # not increasing
                   ((0, 4, 2, 4), (0, 4))):
        assert finish(ys, xs) == -1 and b'positions' in lib.dsrl_last_error(), (ys, xs)
    assert finish((0, 9), (0, 1), hw=3, ww=11) == -1            # a gap: rows 3 .. 8 uncovered
    assert finish(tuple(range(33)), (0, 4), hw=8, ho=40) == -1 and b'positions' in lib.dsrl_last_error()         # 33 positions
    assert finish((0, 4), (0, 4), ny=0) == -1
    assert finish((0, 4), (0, 4), counts=fake) == -1 and b'need a target' in lib.dsrl_last_error()
    assert finish((0, 4), (0, 4), target=fake, ce=fake, ws=fake, ws_bytes=8) == -3 and b'workspace' in lib.dsrl_last_error()


# ---------------------------------------------------------------------------------------------- refusals of the Python layers
def test_window_merge_refuses_bad_positions_and_cpu_tensors():
    from dualsuperreslearningforsemseg_amd import functional as HF
    dev = torch.device('cpu')
    for ys, xs in (((0, 3), (0, 4)), ((1, 4), (0, 4)), ((0, 4, 4), (0, 4)), ((0, 4.0), (0, 4)), ('04', (0, 4)), ((), (0, 4)), ((0, 4), tuple(range(33)))):
        with pytest.raises(ValueError):
            HF.WindowMerge(ys, xs, (8, 8), 1, 19, (12, 12), dev)
    with pytest.raises(ValueError):
        HF.WindowMerge((0,), (0,), (16, 8), 1, 19, (12, 12), dev)
    with pytest.raises(HF.DsrlHipError):
        HF.window_merge([torch.zeros(1, 19, 8, 8)] * 4, (0, 4), (0, 4), (12, 12))
    with pytest.raises(HF.DsrlHipError, match='no views'):
        HF.window_merge([], (0, 4), (0, 4), (12, 12))


def test_predict_refuses_before_any_device_work():
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    model = DSRL(1, CS, init_weights=False).eval()
    x = torch.zeros(1, 3, 64, 96)                           # a CPU tensor: anything that reached the device path would raise DsrlHipError
    for kw in ({'window': (32, 48), 'scales': (0.5, 1.0)}, {'window': (32, 48), 'temperature': 2.0}, {'window': 'all'}, {'window': (32.0, 48)},
               {'window': True}, {'window': (32, 48), 'stride': 0}, {'stride': 16}, {'window': (80, 96)}, {'window': (32, 48), 'stride': (33, 48)},
               {'window': (24, 48)}, {'window': (16, 16), 'stride': (1, 1)}):
        with pytest.raises(ValueError):
            model.predict(x, **kw)
    with pytest.raises(HF.DsrlHipError):
        model.predict(x, window=(32, 48))                   # a good value gets as far as the device check
    with pytest.raises(HF.DsrlHipError, match='eval'):
        model.train().predict(x, window=(32, 48))


def test_compiled_predictor_refuses_the_keyword():
    from dualsuperreslearningforsemseg_amd.inference import CompiledPredictor
    sig = inspect.signature(CompiledPredictor.__call__)
    assert list(sig.parameters)[-2:] == ['window', 'stride'] and sig.parameters['window'].default is None and sig.parameters['stride'].default is None
    fake = object.__new__(CompiledPredictor)                # no frozen operands: the keyword is refused before anything is looked at
    with pytest.raises(ValueError, match='window'):
        fake(None, window=(32, 48))
    with pytest.raises(ValueError, match='window'):
        fake(None, window=32, stride=16)
    with pytest.raises(ValueError, match='window'):
        fake(None, window='all')
    with pytest.raises(AttributeError):
        fake(None, window=None)                             # "off" goes on to the frozen operands, which this instance does not have


def test_commands_refuse_before_touching_a_device(tmp_path):
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    ds = dict(settings.DATASETS['cityscapes'], split='val')
    weights = str(tmp_path / 'final.weights')               # does not exist: nothing may get as far as reading it
    run_test = lambda **kw: test_command(None, str(tmp_path), None, str(tmp_path / 'out'), weights, kw.pop('device', 'cpu'), kw.pop('compiled', False), **kw)   # noqa: E731
    for bad in ({'window': 'all'}, {'window': (32.5, 48)}, {'window': True}, {'window': (32, 48), 'stride': (0, 1)}, {'stride': 8},
                {'window': (80, 96)}, {'window': (32, 48), 'stride': (48, 48)}, {'window': (24, 48)}, {'window': 16, 'stride': 1}):
        # device='cpu' would raise RuntimeError('MI355X only'): the value is refused first
        with pytest.raises(ValueError):
            benchmark(weights, ds, 'cpu', 0, 2, model_input_size=(64, 96), **bad)
        with pytest.raises(ValueError):
            run_test(model_input_size=(64, 96), **bad)
    # clashes, device='gpu': raised before a model is built or a file read
    for clash in ({'scales': (0.5, 1.0)}, {'temperature': 2.0}, {'compiled_model': True}, {'sisr': True}):
        with pytest.raises(ValueError, match='window does not combine'):
            benchmark(weights, ds, 'gpu', 0, 2, model_input_size=(64, 96), window=(32, 48), **clash)
    with pytest.raises(ValueError, match='window does not combine'):
        run_test(device='gpu', model_input_size=(64, 96), window=(32, 48), scales=(0.5, 1.0))
    with pytest.raises(ValueError, match='window does not combine'):
        run_test(device='gpu', compiled=True, model_input_size=(64, 96), window=(32, 48))
    # a good value gets as far as the device check, "off" spellings included, and combines with flip, ema, boundary and calibration
    for good in ({'window': (32, 48)}, {'window': (32, 48), 'stride': (21, 32)}, {'window': None}, {'window': (64, 96)}):
        with pytest.raises(RuntimeError, match='MI355X only'):
            benchmark(weights, ds, 'cpu', 0, 2, model_input_size=(64, 96), flip=True, ema=True, boundary=True, calibration=True, **good)
        with pytest.raises(RuntimeError, match='MI355X only'):
            run_test(model_input_size=(64, 96), flip=True, **good)


# ---------------------------------------------------------------------------------------------- the fp64 restatement
BAND_PIXELS = {181: 0, 182: 0, 183: 0, 184: 0, 185: 9}          # of the fp64 reference alone


@pytest.mark.parametrize('fixture', WR.FIXTURES, ids=WR.fixture_id)
def test_fixtures_cover_counts_and_near_ties(fixture):
    views, P, cnt = WR.fixture(fixture)
    seed, n, ho, wo, win, ys, xs, flip = fixture
    assert len(views) == len(ys) * len(xs) * (2 if flip else 1) and all(L.shape == (n, WR.NC) + win for L in views)
    assert P.shape == (n, WR.NC, ho, wo) and np.abs(P.sum(axis=1) - 1).max() < 1e-12
    assert set(np.unique(cnt).tolist()) == WR.COVER_COUNTS[seed]
    # the separable count the kernel forms is the brute-force one
    cy = np.array([sum(y <= r < y + win[0] for y in ys) for r in range(ho)])
    cx = np.array([sum(x <= c < x + win[1] for x in xs) for c in range(wo)])
    assert np.array_equal(cnt, np.outer(cy, cx) * (2 if flip else 1))
    _, _, band = MR.band_of(P)
    print(f'{WR.fixture_id(fixture)}: {int(band.sum())} of {band.size} pixels ({100 * band.mean():.5f} %) inside the band')
    assert band.mean() <= PF.MAX_BAND_SHARE
    assert int(band.sum()) == BAND_PIXELS[seed]


def test_one_whole_image_window_with_flip_is_the_flip_ensemble():
    """fixture 184 against predict_flip_ref (the log of the two views' averaged probabilities) and multiscale_ref.merge on the same two views"""
    f = WR.FIXTURES[3]
    views, P, cnt = WR.fixture(f)
    assert (cnt == 2).all()
    E = PFR.ensemble(views[0], views[1])
    assert np.abs(np.log(P) - E).max() < 1e-12
    assert np.abs(P - MR.merge([(views[0], False), (views[1], True)], (6, 6))).max() < 1e-15
    target = PFR.make_target(5, (1, 6, 6))
    assert abs(WR.ce(P, target) - PFR.ce(E, target)) < 1e-12


def test_equal_views_give_the_single_softmax_wherever_they_overlap():
    L = np.random.RandomState(9).standard_normal((1, 19, 12, 20)) * 2
    ys, xs, win = (0, 4), (0, 8), (8, 12)
    views = [L[:, :, y:y + 8, x:x + 12] for y, x in itertools.product(ys, xs)]
    P, _ = WR.merge(views, ys, xs, (12, 20))
    assert np.abs(P - MR.softmax(L)).max() < 1e-15
    # with flip: the mirrored-frame view of a crop is the crop's mirror image
    both = [v for c in views for v in (c, c[:, :, :, ::-1])]
    P2, cnt = WR.merge(both, ys, xs, (12, 20), flip=True)
    assert np.abs(P2 - MR.softmax(L)).max() < 1e-15 and set(np.unique(cnt).tolist()) == {2, 4, 8}

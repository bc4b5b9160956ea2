"""CPU-only checks of multi-scale inference: the host part of the dsrl_prob_merge ABI, the argument rules of functional.multiscale_scales_value /
multiscale_sizes, the loud failures without a GPU, self-checks of the fp64 restatement (multiscale_ref) and the condition the GPU class-map tests rest
on (few near-ties of the ensemble in every fixture)."""
import os
import re

import numpy as np
import pytest
import torch

import multiscale_ref as MR
import predict_fixtures as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('dsrl_prob_merge_supported', 'dsrl_prob_merge_acc_bytes', 'dsrl_prob_merge_workspace_bytes', 'dsrl_prob_merge', 'dsrl_prob_merge_finish')


def test_merge_entry_points_are_exported_prototyped_and_declared():
    from dualsuperreslearningforsemseg_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dsrl_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), name
    assert len(_lib.PROTOTYPES['dsrl_prob_merge'][1]) == 12 and len(_lib.PROTOTYPES['dsrl_prob_merge_finish'][1]) == 21
    assert re.search(r'\bint\s+dsrl_prob_merge\s*\(const float\* logits, int ld, int N, int Hs, int Ws, int C, int mirror, float\* acc, int Ho, int Wo, '
                     r'int first,', header)
    assert re.search(r'\bint\s+dsrl_prob_merge_finish\s*\(const float\* logits, int ld, int N, int Hs, int Ws, int C, int mirror, const float\* acc', header)
    assert 'merge.hip' in open(os.path.join(ROOT, 'dualsuperreslearningforsemseg_amd', 'csrc', 'Makefile')).read()


def test_supported_and_size_queries_are_pure_host_code():
    from dualsuperreslearningforsemseg_amd import _lib
    q = _lib.query
    for _, n, ho, wo, sizes, _ in MR.FIXTURES:
        for h, w in sizes:
            assert q('dsrl_prob_merge_supported', n, h, w, ho, wo, 19) == 1
        assert q('dsrl_prob_merge_acc_bytes', n, ho, wo, 19) == n * 19 * ho * wo * 4
        ws = q('dsrl_prob_merge_workspace_bytes', n, ho, wo)
        assert ws >= 16 and ws % 16 == 0 and ws == q('dsrl_prob_merge_workspace_bytes', n, ho, wo)
    assert q('dsrl_prob_merge_supported', 1, 8, 8, 8, 8, 32) == 1 and q('dsrl_prob_merge_supported', 1, 8, 8, 8, 8, 1) == 1
    assert q('dsrl_prob_merge_supported', 1, 8, 8, 8, 8, 33) == 0 and q('dsrl_prob_merge_supported', 1, 8, 8, 8, 8, 0) == 0
    for bad in ((0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, 0, 8, 8), (1, 8, 8, 0, 8), (1, 8, 8, 8, 0)):
        assert q('dsrl_prob_merge_supported', *bad, 19) == 0
    # N * Ho * Wo * C: 8 * 1024 * 2048 * 19 = 3.2e8 fits, 64 images of it do not; one image of them does (the Python side splits by image)
    assert q('dsrl_prob_merge_supported', 8, 512, 1024, 1024, 2048, 19) == 1
    assert q('dsrl_prob_merge_supported', 64, 512, 1024, 1024, 2048, 19) == 0
    assert q('dsrl_prob_merge_supported', 1, 512, 1024, 1024, 2048, 19) == 1
    # N * Hs * Ws * C of the source, and o * (S - 1) on one axis
    assert q('dsrl_prob_merge_supported', 1, 16384, 16384, 8, 8, 19) == 0
    assert q('dsrl_prob_merge_supported', 1, 60000, 1, 60000, 1, 1) == 0 and q('dsrl_prob_merge_supported', 1, 40000, 1, 40000, 1, 1) == 1
    # the workspace depends on the shape only and is bounded by the block cap
    assert q('dsrl_prob_merge_workspace_bytes', 8, 1024, 2048) == q('dsrl_prob_merge_workspace_bytes', 64, 1024, 2048)
    assert q('dsrl_prob_merge_workspace_bytes', 0, 4, 4) == 0 and q('dsrl_prob_merge_acc_bytes', 1, 4, 4, 0) == 0


def test_multiscale_scales_value():
    from dualsuperreslearningforsemseg_amd.functional import multiscale_scales_value as value
    assert value(None) is None and value(()) is None and value([]) is None and value((1.0,)) is None and value([1]) is None
    assert value((0.5, 1, 1.5)) == (0.5, 1.0, 1.5) and all(type(v) is float for v in value((0.5, 1, np.float32(1.5), np.int64(2))))
    assert value((1.0, 1.0)) == (1.0, 1.0)                  # only the exact "off" spellings are off: duplicates are multiscale_sizes' to refuse
    assert value([0.75]) == (0.75,) and value(np.array([0.5, 2.0])) == (0.5, 2.0)
    assert len(value(tuple(0.5 + 0.1 * i for i in range(16)))) == 16
    for bad in ((True,), (0.5, False), ('1.0',), '0.5', (None,), ([1.0],), (float('nan'),), (float('inf'),), (-float('inf'),), (0,), (0.0,), (-0.5,),
                (1.0, -1e-30), tuple(0.5 + 0.1 * i for i in range(17)), 1.5, object(), (np.bool_(True),), (1 + 2j,)):
        with pytest.raises(ValueError):
            value(bad)


def test_multiscale_sizes():
    from dualsuperreslearningforsemseg_amd.functional import multiscale_sizes as sizes
    assert sizes(256, 512, (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)) == [(128, 256), (192, 384), (256, 512), (320, 640), (384, 768), (448, 896)]
    assert sizes(64, 96, (0.5, 1.0, 1.5)) == [(32, 48), (64, 96), (96, 144)]
    assert sizes(64, 96, (1.5, 0.5)) == [(96, 144), (32, 48)]                   # the given order is kept
    with pytest.raises(ValueError, match='same'):
        sizes(64, 96, (0.5, 0.55))                                                # 32 x 48 and 35.2 x 52.8 -> 32 x 48
    with pytest.raises(ValueError, match='same'):
        sizes(64, 96, (1.0, 1.0))
    assert sizes(64, 96, (0.01,)) == [(16, 16)] and sizes(16, 16, (0.3, 1.6)) == [(16, 16), (32, 32)]
    assert sizes(64, 96, (0.625,)) == [(48, 64)]                                  # 2.5 and 3.75 sixteens: halves round up


@pytest.mark.parametrize('shape, size', [((2, 3, 5, 7), (10, 14)), ((2, 3, 5, 7), (13, 9)), ((1, 2, 9, 16), (5, 7)), ((1, 2, 9, 16), (9, 16)),
                                         ((1, 2, 1, 1), (4, 3)), ((1, 2, 3, 2), (1, 1)), ((1, 1, 1, 5), (1, 9)), ((1, 1, 6, 1), (3, 1))])
def test_resize_ac_is_torchs_align_corners_interpolation(shape, size):
    L = np.random.RandomState(7).standard_normal(shape) * 3
    want = torch.nn.functional.interpolate(torch.from_numpy(L), size=size, mode='bilinear', align_corners=True).numpy()
    got = MR.resize_ac(L, size)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-12


# ---------------------------------------------------------------------------------------------- near-tie guard (passes on any commit)
BAND_PIXELS = {81: 0, 82: 0, 83: 0, 84: 0, 85: 11, 86: 0}          # of the fp64 reference alone


@pytest.mark.parametrize('fixture', MR.FIXTURES, ids=MR.fixture_id)
def test_fixtures_have_few_near_ties(fixture):
    views, P = MR.fixture(fixture)
    assert len(views) == len(fixture[4]) * (2 if fixture[5] else 1) and [m for _, m in views] == [bool(fixture[5]) and i % 2 == 1 for i in range(len(views))]
    assert P.shape == (fixture[1], MR.NC, fixture[2], fixture[3]) and np.abs(P.sum(axis=1) - 1).max() < 1e-12
    _, _, band = MR.band_of(P)
    print(f'{MR.fixture_id(fixture)}: {int(band.sum())} of {band.size} pixels ({100 * band.mean():.3f} %) inside the band; max |L| '
          f'{max(np.abs(L).max() for L, _ in views):.2f}, max P {P.max():.3f}')
    assert band.mean() <= PF.MAX_BAND_SHARE
    assert int(band.sum()) == BAND_PIXELS[fixture[0]]


# ---------------------------------------------------------------------------------------------- self-checks of the fp64 restatement
def test_one_identity_view_gives_softmax():
    L = np.random.RandomState(3).standard_normal((2, 19, 6, 9)) * 3
    P = MR.merge([(L, False)], (6, 9))
    assert np.abs(P - MR.softmax(L)).max() < 1e-15 and np.array_equal(P.argmax(1), L.argmax(1))
    target = np.random.RandomState(4).randint(0, 19, (2, 6, 9)).astype(np.uint8)
    target[0, :2] = 255
    want = float(torch.nn.functional.cross_entropy(torch.from_numpy(L), torch.from_numpy(target.astype(np.int64)), ignore_index=255))
    assert abs(MR.ce(P, target) - want) < 1e-12
    assert np.isnan(MR.ce(P, np.full_like(target, 255)))
    bad = target.copy()
    bad[1, 3, 3] = 19
    assert np.isnan(MR.ce(P, bad))


def test_two_equal_views_give_the_single_view():
    L = np.random.RandomState(5).standard_normal((1, 19, 5, 8)) * 2
    one = MR.merge([(L, False)], (10, 16))
    assert np.abs(MR.merge([(L, False), (L, False)], (10, 16)) - one).max() < 1e-15
    # a view handed over in the mirrored frame is the same view
    assert np.abs(MR.merge([(L, False), (L[:, :, :, ::-1], True)], (10, 16)) - one).max() < 1e-13


def test_swapping_every_view_for_its_mirror_image_mirrors_the_ensemble():
    rs = np.random.RandomState(6)
    views = [(rs.standard_normal((2, 19, 4, 7)) * 2, False), (rs.standard_normal((2, 19, 9, 5)) * 2, True), (rs.standard_normal((2, 19, 6, 11)) * 2, False)]
    P = MR.merge(views, (8, 13))
    swapped = MR.merge([(L, not m) for L, m in views], (8, 13))
    assert np.abs(swapped - P[:, :, :, ::-1]).max() < 1e-13
    assert (swapped.argmax(1) != P.argmax(1)).mean() > 0.3                  # and the mirroring matters


# ---------------------------------------------------------------------------------------------- loud failures without a GPU
def test_merge_and_predict_on_cpu_tensors_raise():
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    with pytest.raises(HF.DsrlHipError):
        HF.multiscale_merge([(torch.zeros(1, 19, 4, 4), False), (torch.zeros(1, 19, 8, 8), True)], (8, 8))
    with pytest.raises(HF.DsrlHipError, match='no views'):
        HF.multiscale_merge([], (8, 8))
    with pytest.raises(HF.DsrlHipError):
        HF.resize_image_ac(torch.zeros(1, 3, 16, 16), (32, 32))
    model = DSRL(1, CS, init_weights=False).eval()
    with pytest.raises(HF.DsrlHipError):
        model.predict(torch.zeros(1, 3, 32, 32), scales=(0.5, 1.0))
    with pytest.raises(ValueError):
        model.predict(torch.zeros(1, 3, 32, 32), scales=(0.5, -1.0))
    with pytest.raises(HF.DsrlHipError, match='eval'):
        model.train().predict(torch.zeros(1, 3, 32, 32), scales=(0.5, 1.0))


def test_commands_refuse_bad_scales_before_touching_a_device(tmp_path):
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd._lib import DsrlHipError
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    ds = dict(settings.DATASETS['cityscapes'], split='val')
    weights = str(tmp_path / 'final.weights')               # does not exist: nothing may get as far as reading it
    for bad in ((0.5, -1.0), (True,), 'all', (float('nan'),), tuple([0.5] * 17)):
        # device='cpu' would raise RuntimeError('MI355X only'): the value is refused first
        with pytest.raises(ValueError, match='scales'):
            benchmark(weights, ds, 'cpu', 0, 2, scales=bad)
        with pytest.raises(ValueError, match='scales'):
            test_command(None, str(tmp_path), None, str(tmp_path / 'out'), weights, 'cpu', False, scales=bad)
    # a good value gets as far as the device check, "off" spellings included
    for good in ((0.5, 1.0), (1.0,), None):
        with pytest.raises(RuntimeError, match='MI355X only'):
            benchmark(weights, ds, 'cpu', 0, 2, scales=good, flip=True)
        with pytest.raises(RuntimeError, match='MI355X only'):
            test_command(None, str(tmp_path), None, str(tmp_path / 'out'), weights, 'cpu', False, scales=good)
    # with a compiled model the commands refuse before they load the file
    with pytest.raises(DsrlHipError, match='eager'):
        benchmark(weights, ds, 'gpu', 0, 2, scales=(0.5, 1.0), compiled_model=True)
    with pytest.raises(DsrlHipError, match='eager'):
        test_command(None, str(tmp_path), None, str(tmp_path / 'out'), weights, 'gpu', True, scales=(0.5, 1.0))

"""CPU-only checks of flip-averaged inference: the host part of the dsrl_sssr_tail_predict_flip ABI, the loud failures without a GPU, self-checks of the
fp64 restatement (predict_flip_ref) and the condition the GPU class-map tests rest on (few near-ties of the ensemble in every fixture)."""
import os
import re

import numpy as np
import pytest
import torch

import predict_fixtures as PF
import predict_flip_ref as PFR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flip_entry_point_is_exported_prototyped_and_declared():
    from dualsuperreslearningforsemseg_amd import _lib
    assert 'dsrl_sssr_tail_predict_flip' in _lib.PROTOTYPES
    assert _lib.PROTOTYPES['dsrl_sssr_tail_predict_flip'] == _lib.PROTOTYPES['dsrl_sssr_tail_predict']        # "...same tail as dsrl_sssr_tail_predict"
    assert hasattr(_lib.load(), 'dsrl_sssr_tail_predict_flip')
    header = open(os.path.join(ROOT, 'include', 'dsrl_hip.h')).read()
    assert re.search(r'\bint\s+dsrl_sssr_tail_predict_flip\s*\(const float\* x, int ldx, int N, int H, int W, int Cin, int Cmid, int Cout,', header)


def test_flip_on_cpu_tensors_raises():
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.nn_modules import HipBatchNorm2d, HipConvTranspose2d
    mods = [HipConvTranspose2d(19, 19, kernel_size=2, stride=2, padding=0, bias=False).eval(), HipBatchNorm2d(19).eval(),
            HipConvTranspose2d(19, 19, kernel_size=2, stride=2, padding=0, bias=True).eval()]
    with pytest.raises(HF.DsrlHipError):
        HF.sssr_tail_predict(torch.zeros(2, 19, 4, 4), *mods, flip=True)


def test_commands_refuse_other_devices_with_flip(tmp_path):
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    ds = dict(settings.DATASETS['cityscapes'], split='val')
    with pytest.raises(RuntimeError, match='MI355X only'):
        benchmark(str(tmp_path / 'final.weights'), ds, 'cpu', 0, 2, flip=True)
    with pytest.raises(RuntimeError, match='MI355X only'):
        test_command(None, str(tmp_path), None, str(tmp_path / 'out'), str(tmp_path / 'final.weights'), 'cpu', False, flip=True)


# ---------------------------------------------------------------------------------------------- self-checks of the fp64 restatement
def test_two_identical_views_give_the_single_view():
    rs = np.random.RandomState(3)
    L = rs.standard_normal((2, 19, 8, 12)) * 3
    target = PFR.make_target(4, (2, 8, 12))
    E = PFR.ensemble(L, L[:, :, :, ::-1])               # the second view IS the first one, handed over in the mirrored frame
    assert np.array_equal(E.argmax(1), L.argmax(1))
    assert np.abs(E - PFR.log_softmax(L)).max() < 1e-13
    want = float(torch.nn.functional.cross_entropy(torch.from_numpy(L), torch.from_numpy(target.astype(np.int64)), ignore_index=255))
    assert abs(PFR.ce(E, target) - want) < 1e-12
    assert np.isnan(PFR.ce(E, np.full_like(target, 255)))
    bad = target.copy()
    bad[0, 0, 0] = 200
    assert np.isnan(PFR.ce(E, bad))


def test_swapping_the_views_mirrors_the_ensemble():
    rs = np.random.RandomState(5)
    La, Lb = rs.standard_normal((2, 19, 4, 7)) * 2, rs.standard_normal((2, 19, 4, 7)) * 2
    E, swapped = PFR.ensemble(La, Lb), PFR.ensemble(Lb, La)
    assert np.abs(swapped - E[:, :, :, ::-1]).max() < 1e-13
    # and the un-mirroring matters: without it the class map is another one
    unmirrored = PFR.ensemble(La, Lb[:, :, :, ::-1])
    assert (unmirrored.argmax(1) != E.argmax(1)).mean() > 0.3


# ---------------------------------------------------------------------------------------------- near-tie guards (pass on any commit)
@pytest.mark.parametrize('fixture', PFR.TAIL_FIXTURES, ids=PFR.tail_fixture_id)
def test_tail_fixtures_have_few_near_ties(fixture):
    """The share of pixels whose top-two margin of the fp64 ensemble is below PF.BAND * max |L| (both views' logits) is at most 0.5 %; the ensemble
    differs from view a's own arg-max and from an ensemble without the un-mirroring at a large share of the pixels (W > 1), so that a missing or wrong
    mirror cannot pass the GPU tests."""
    _, _, L, E = PFR.tail_fixture(fixture)
    n = L.shape[0] // 2
    best, _, band = PFR.band_of(E, L)
    vs_a = (best != L[:n].argmax(1)).mean()
    vs_unmirrored = (best != PFR.ensemble(L[:n], L[n:, :, :, ::-1]).argmax(1)).mean()
    print(f'{PFR.tail_fixture_id(fixture)}: {100 * band.mean():.3f} % ({int(band.sum())} of {band.size} pixels) inside the band; ensemble != view a at '
          f'{100 * vs_a:.1f} %, != un-mirrored ensemble at {100 * vs_unmirrored:.1f} %')
    assert band.mean() <= PF.MAX_BAND_SHARE
    if fixture[4] > 1 and band.size >= 1000:
        assert vs_a > 0.3 and vs_unmirrored > 0.3


@pytest.mark.parametrize('fixture', PF.HEAD_FIXTURES, ids=PF.fixture_id)
def test_head_fixtures_have_few_near_ties(fixture):
    _, _, _, _, L, E = PFR.head_fixture(fixture)
    _, _, band = PFR.band_of(E, L)
    print(f'{PF.fixture_id(fixture)}: {100 * band.mean():.3f} % of {band.size} pixels inside the band')
    assert band.mean() <= PF.MAX_BAND_SHARE

"""CPU-only checks of the inference surface: the host part of the dsrl_sssr_tail_predict ABI, the visualisation helper, the palette, the loud
failures of the two commands without a GPU, and the condition the GPU class-map test rests on (few near-ties in the fixtures)."""
import numpy as np
import pytest

import predict_fixtures as PF


def test_supported_is_exported_and_answers_without_a_gpu():
    from dualsuperreslearningforsemseg_amd import _lib
    for name in ('dsrl_sssr_tail_predict_supported', 'dsrl_sssr_tail_predict_workspace_bytes', 'dsrl_sssr_tail_predict'):
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.dsrl_sssr_tail_predict_supported(1, 128, 256, 19, 19, 19) == 1
    assert lib.dsrl_sssr_tail_predict_supported(3, 5, 7, 19, 19, 19) == 1
    assert lib.dsrl_sssr_tail_predict_supported(1, 128, 256, 8, 8, 8) == 0
    assert lib.dsrl_sssr_tail_predict_supported(0, 128, 256, 19, 19, 19) == 0
    assert lib.dsrl_sssr_tail_predict_supported(64, 2048, 2048, 19, 19, 19) == 0        # 2^32 output pixels: beyond what the kernel indexes
    # the workspace depends on the shape only, and never on the number of classes: a few KiB of per-block partials
    assert 0 < lib.dsrl_sssr_tail_predict_workspace_bytes(8, 128, 256) <= 16384
    assert lib.dsrl_sssr_tail_predict_workspace_bytes(8, 256, 512) <= 16384


def test_visualization_equals_the_literal_formula():
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.utils import make_input_output_visualization
    palette = CS.CLASS_RGB_COLOR
    labels = sorted(palette)
    # every input byte 0..255 under every palette entry, in each channel: rows = labels, columns = bytes; channels shifted against each other
    H, W = len(labels), 256
    image = np.stack([(np.arange(W) + 85 * c) % 256 for c in range(3)]).astype(np.uint8)[:, None, :].repeat(H, axis=1)
    for c in range(3):
        assert set(image[c, 0].tolist()) == set(range(256))
    label_map = np.array(labels)[:, None].repeat(W, axis=1)
    b = 0.4
    vis = make_input_output_visualization(image, label_map, palette, blend_factor=b)
    assert vis.shape == (3, H, 3 * W) and vis.dtype == np.uint8
    assert np.array_equal(vis[:, :, :W], image)
    for c in range(3):
        for y in range(H):
            colour = palette[labels[y]][c]
            assert (vis[c, y, W:2 * W] == colour).all()
            for x in range(W):
                want = int(min((1. - b) * float(image[c, y, x]) + b * float(colour), 255))
                assert vis[c, y, 2 * W + x] == want, (c, y, x, vis[c, y, 2 * W + x], want)


def test_palette_covers_the_train_ids_and_the_ignore_label():
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    assert sorted(CS.CLASS_RGB_COLOR) == list(range(19)) + [CS.IGNORE_CLASS_LABEL]
    for rgb in CS.CLASS_RGB_COLOR.values():
        assert len(rgb) == 3 and all(isinstance(v, int) and 0 <= v <= 255 for v in rgb)
    assert CS.CLASS_RGB_COLOR[CS.IGNORE_CLASS_LABEL] == (0, 0, 0)
    assert len(set(CS.CLASS_RGB_COLOR.values())) == 20


def test_commands_refuse_other_devices_and_compiled_models(tmp_path):
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    ds = dict(settings.DATASETS['cityscapes'], split='val')
    with pytest.raises(RuntimeError, match='MI355X only'):
        benchmark(str(tmp_path / 'final.weights'), ds, 'cpu', 0, 2)
    with pytest.raises(RuntimeError, match='MI355X only'):
        test_command(None, str(tmp_path), None, str(tmp_path / 'out'), str(tmp_path / 'final.weights'), 'cpu', False)
    with pytest.raises(RuntimeError, match='compiled_model'):
        test_command(None, str(tmp_path), None, str(tmp_path / 'out'), str(tmp_path / 'final.weights'), 'gpu', True)


def test_metrics_take_a_counts_table():
    import torch
    from dualsuperreslearningforsemseg_amd.metrices import Accuracy, mIoU
    import oracle as O
    rs = np.random.RandomState(5)
    m, a = mIoU(19), Accuracy(19)
    want_m, want_a = [], []
    for _ in range(2):
        pred = rs.randint(0, 19, (2, 8, 16)).astype(np.uint8)
        target = np.where(rs.uniform(size=pred.shape) < 0.5, pred, rs.randint(0, 19, pred.shape)).astype(np.uint8)
        target[rs.uniform(size=pred.shape) < 0.1] = 255
        table = torch.from_numpy(PF.counts_table(pred, target))
        m.update_from_counts(table); a.update_from_counts(table)
        mi, ac = O.seg_metrics_batch(pred, target)
        want_m.append(mi); want_a.append(ac)
    assert abs(m() - 100 * np.mean(want_m)) < 1e-9 and abs(a() - 100 * np.mean(want_a)) < 1e-9
    with pytest.raises(ValueError):
        m.update_from_counts(torch.zeros(7, dtype=torch.int64))


@pytest.mark.parametrize('fixture', PF.HEAD_FIXTURES, ids=PF.fixture_id)
def test_fixtures_have_few_near_ties(fixture):
    """Guards the GPU class-map test (passes on any commit): the share of pixels whose fp64 top-two margin is below 1e-4 * max |L| is at most 0.5 %."""
    P, x16, x4, _ = PF.head_fixture(fixture)
    _, _, band = PF.band_of(PF.oracle_logits(P, x16, x4))
    print(f'{PF.fixture_id(fixture)}: {100 * band.mean():.3f} % of {band.size} pixels inside the band')
    assert band.mean() <= PF.MAX_BAND_SHARE

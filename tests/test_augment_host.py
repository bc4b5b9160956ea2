"""CPU checks of the training augmentations and the Cityscapes loader: the numpy restatement of the Pillow geometry against Pillow itself, the
committed fixture against its generator, the parameter draws, the uint8 cache and the rank partition."""
import os

import numpy as np
import pytest

import augment_ref as R
from dualsuperreslearningforsemseg_amd.models.transforms import augment as A
from dualsuperreslearningforsemseg_amd.models.transforms import DeviceJointAugmentation
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L


def _aug():
    return DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, (256, 512), seed=54321)


@pytest.mark.parametrize('H,W,cases', [
    (48, 96, [(0.0, 1.0), (15.0, 3.45), (-15.0, 1.0), (7.3, 2.2), (-11.9, 3.3), (0.01, 1.5)]),
    (1024, 2048, [(15.0, 3.49), (-8.25, 1.7)]),
])
def test_numpy_restatement_matches_pillow(H, W, cases):
    pytest.importorskip('PIL')
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, 34, (H, W), dtype=np.uint8)
    for k, (angle, scale) in enumerate(cases):
        p = A.AugmentParams(angle, scale, A.crop_box(scale, 0.37 * k % 1, 0.71 * k % 1, W, H), False, False, 1.0, False)
        a, al = R.geometry_numpy(img, lab, p)
        b, bl = R.geometry_pillow(img, lab, p)
        assert np.array_equal(a, b), (angle, p.box, int((a != b).sum()))
        assert np.array_equal(al, bl), (angle, p.box, int((al != bl).sum()))


def test_generator_reproduces_committed_fixture(golden):
    pytest.importorskip('PIL')
    import make_augment_golden as M
    g, fresh = golden('augment'), M.make()
    assert sorted(g.files) == sorted(fresh)
    for k in fresh:
        if fresh[k].dtype.kind == 'f' and k in ('img_in', 'img_org'):
            np.testing.assert_allclose(g[k], fresh[k], rtol=0, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(g[k], fresh[k]), k
    # the geometry of the fixture is also what the numpy restatement gives
    for i, p in enumerate(M.params_of(g)):
        a, al = R.geometry_numpy(g['rgb'][i], g['labels'][i], p)
        assert np.array_equal(a, g['geo_rgb'][i]) and np.array_equal(al, g['geo_labels'][i]), i


def test_draws_are_deterministic_and_independent_of_the_batch():
    aug = _aug()
    a = aug.draw(3, [5, 9, 11])
    assert a == aug.draw(3, [5, 9, 11])
    assert a[1:] == aug.draw(3, [9, 11]) and a[0] == aug.draw(3, [5])[0]
    assert a != aug.draw(4, [5, 9, 11])
    assert _aug().draw(3, [5]) == [a[0]]
    other = DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, (256, 512), seed=1)
    assert other.draw(3, [5]) != [a[0]]


def test_draws_stay_in_range_and_have_the_reference_frequencies():
    aug = _aug()
    H, W = 1024, 2048
    n = 20000
    ps = aug.draw(0, range(n), (H, W))
    ang = np.array([p.angle for p in ps]); sc = np.array([p.scale for p in ps]); sg = np.array([p.sigma for p in ps])
    assert ang.min() >= -15 and ang.max() <= 15 and ang.min() < -14.9 and ang.max() > 14.9
    assert sc.min() >= 1.0 and sc.max() <= 3.5 and sc.max() > 3.49
    assert sg.min() >= 0.1 and sg.max() <= 2.0
    frac_x, frac_y = [], []
    for p in ps:
        x, y, cw, ch = p.box
        assert (cw, ch) == (int(1.0 / p.scale * W), int(1.0 / p.scale * H))
        # the reference's offsets span only the top-left half of the admissible range
        assert 0 <= x <= (W - cw) // 2 and 0 <= y <= (H - ch) // 2 and x + cw <= W and y + ch <= H
        if (W - cw) // 2 > 0:
            frac_x.append(x / ((W - cw) // 2))
        if (H - ch) // 2 > 0:
            frac_y.append(y / ((H - ch) // 2))
    assert max(frac_x) > 0.99 and max(frac_y) > 0.99 and 0.45 < np.mean(frac_x) < 0.55
    for name, prob in (('flip', 0.5), ('blur', 0.5), ('gray', 0.1)):
        k = sum(getattr(p, name) for p in ps)
        assert abs(k - n * prob) <= 4 * np.sqrt(n * prob * (1 - prob)), (name, k)


def test_parameter_rows_follow_pillow_and_torchvision():
    p = A.AugmentParams(-15.0, 2.0, (10, 20, 30, 15), True, True, 0.8, True)
    row = A.pack([p], 96, 48)[0]
    assert row['flags'] == A.AUG_HFLIP | A.AUG_BLUR | A.AUG_GRAY and tuple(row['box']) == (10, 20, 30, 15)
    # Image.rotate works on angle % 360
    m = A.rotate_matrix(345.0, 96, 48)
    assert list(row['rot']) == m
    k = row['blur'].reshape(3, 3)
    assert abs(float(k.sum()) - 1) < 1e-6 and np.allclose(k, k.T) and k[1, 1] == k.max()
    assert A.pack([A.identity_params()], 96, 48)[0]['flags'] == 0


def _write_tree(root, split, n, H, W, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        city = ('aachen', 'bochum')[i % 2]
        stem = f'{city}_{i:06d}_000019'
        for d in (os.path.join(root, 'leftImg8bit', split, city), os.path.join(root, 'gtFine', split, city)):
            os.makedirs(d, exist_ok=True)
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        lab = rng.integers(0, 34, (H, W), dtype=np.uint8)
        Image.fromarray(rgb).save(os.path.join(root, 'leftImg8bit', split, city, stem + '_leftImg8bit.png'))
        Image.fromarray(lab).save(os.path.join(root, 'gtFine', split, city, stem + '_gtFine_labelIds.png'))
        Image.fromarray(lab).save(os.path.join(root, 'gtFine', split, city, stem + '_gtFine_color.png'))      # not a label-id map: ignored
        out.append((stem, rgb, lab))
    return out


def test_cache_round_trips_a_png_tree(tmp_path):
    pytest.importorskip('PIL')
    root, cache = str(tmp_path / 'cityscapes'), str(tmp_path / 'cache')
    written = {s: _write_tree(root, s, n, 12, 20, k) for k, (s, n) in enumerate((('train', 5), ('val', 2)))}
    assert L.has_tree(root) and not L.has_cache(cache)
    L.build_cache(root, cache)
    assert L.has_cache(cache)
    for split, items in written.items():
        c = L.CityscapesCache(cache, split)
        order = sorted(range(len(items)), key=lambda i: (items[i][0].split('_')[0], items[i][0]))      # city folder, then file name
        assert len(c) == len(items) and (c.height, c.width) == (12, 20)
        for j, i in enumerate(order):
            assert c.images[j].endswith(items[i][0] + '_leftImg8bit.png')
            assert np.array_equal(c.rgb[j], items[i][1]) and np.array_equal(c.labels[j], items[i][2])


@pytest.mark.parametrize('n,world', [(10, 1), (10, 3), (11, 4), (2975, 8)])
def test_rank_partition_is_disjoint_and_even(n, world):
    parts = [L.rank_indices(n, 7, 54321, r, world) for r in range(world)]
    assert len({len(p) for p in parts}) == 1 and len(parts[0]) == (n // world if n % world == 0 else -(-(n - world) // world))
    allidx = np.concatenate(parts)
    assert len(set(allidx.tolist())) == len(allidx) and allidx.min() >= 0 and allidx.max() < n
    assert not np.array_equal(L.rank_indices(n, 8, 54321, 0, world), parts[0]) or n < 3
    assert np.array_equal(L.rank_indices(n, 7, 54321, 0, world), parts[0])

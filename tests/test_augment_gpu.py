"""The training augmentations on the MI355X: dsrl_augment_geometry against Pillow (tests/golden/augment.npz) bit for bit, the whole augmented
preparation against Pillow + torch, the identity and flip-only cases against dsrl_prepare_batch, argument checks, and train_or_resume fed by the
Cityscapes loader with no loader_factory."""
import os

import numpy as np
import pytest
import torch

import make_augment_golden as M
from hip_helpers import check, host
from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
from dualsuperreslearningforsemseg_amd.models.transforms import DeviceBatchPreparation, DeviceJointAugmentation
from dualsuperreslearningforsemseg_amd.models.transforms import augment as A

pytestmark = pytest.mark.gpu


def _u8(a):
    return torch.from_numpy(np.array(a)).cuda()


def _aug(size=M.MODEL_INPUT):
    return DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL)


def test_geometry_matches_pillow_bit_for_bit(golden):
    g = golden('augment')
    aug = _aug()
    ps = M.params_of(g)
    N, H, W, _ = g['rgb'].shape
    table = aug.table(ps, W, H, torch.device('cuda'))
    rgb, lab = aug.geometry(_u8(g['rgb']), _u8(g['labels']), table)
    torch.cuda.synchronize()
    r, l_ = rgb.cpu().numpy(), lab.cpu().numpy()
    for i in range(N):
        assert np.array_equal(r[i], g['geo_rgb'][i]), (i, int((r[i] != g['geo_rgb'][i]).sum()))
        assert np.array_equal(l_[i], g['geo_labels'][i]), (i, int((l_[i] != g['geo_labels'][i]).sum()))


def test_augmented_batch_matches_pillow_and_torch(golden):
    g = golden('augment')
    aug = _aug()
    (img_in, img_org), (target, aux) = aug(_u8(g['rgb']), _u8(g['labels']), M.params_of(g))
    assert aux is None and img_in.shape == (5, 3, 16, 32) and img_org.shape == (5, 3, 32, 64)
    check(host(img_in), g['img_in'], 1e-5, 'img_in')
    check(host(img_org), g['img_org'], 1e-5, 'img_org')
    assert np.array_equal(target.cpu().numpy(), g['target'])


def _rand_batch(N, H, W, seed):
    rng = np.random.default_rng(seed)
    ids = np.array(sorted(k for k in cs.LABEL_MAPPING_DICT if 0 <= k < 256), dtype=np.uint8)
    return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), ids[rng.integers(0, len(ids), (N, H, W))]


@pytest.mark.parametrize('H,W,size', [(48, 96, (16, 32)), (256, 512, (64, 128)), (100, 150, (37, 61))])
def test_identity_parameters_are_prepare_batch_bit_for_bit(H, W, size):
    rgb, lab = _rand_batch(3, H, W, H)
    aug, prep = _aug(size), DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL)
    (a_in, a_org), (a_t, _) = aug(_u8(rgb), _u8(lab), [A.identity_params()] * 3)
    (b_in, b_org), (b_t, _) = prep(_u8(rgb), _u8(lab))
    assert torch.equal(a_in, b_in) and torch.equal(a_org, b_org) and torch.equal(a_t, b_t)


def test_flip_only_is_prepare_batch_of_the_mirrored_input():
    rgb, lab = _rand_batch(2, 64, 128, 7)
    size = (24, 40)
    aug, prep = _aug(size), DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL)
    flip = A.identity_params()._replace(flip=True)
    (a_in, a_org), (a_t, _) = aug(_u8(rgb), _u8(lab), [flip, A.identity_params()])
    (b_in, b_org), (b_t, _) = prep(_u8(rgb[0:1, :, ::-1]), _u8(lab[0:1, :, ::-1]))
    (c_in, c_org), (c_t, _) = prep(_u8(rgb[1:2]), _u8(lab[1:2]))
    assert torch.equal(a_in[0:1], b_in) and torch.equal(a_org[0:1], b_org) and torch.equal(a_t[0:1], b_t)
    assert torch.equal(a_in[1:2], c_in) and torch.equal(a_org[1:2], c_org) and torch.equal(a_t[1:2], c_t)


def test_drawn_batches_are_reproducible_and_finite():
    rgb, lab = _rand_batch(4, 128, 256, 3)
    aug = _aug((32, 64))
    ps = aug.draw(1, range(4), (128, 256))
    (x1, o1), (t1, _) = aug(_u8(rgb), _u8(lab), ps)
    (x2, o2), (t2, _) = aug(_u8(rgb), _u8(lab), ps)
    assert torch.equal(x1, x2) and torch.equal(o1, o2) and torch.equal(t1, t2)
    assert torch.isfinite(o1).all()


def test_bad_arguments_are_refused():
    aug = _aug()
    rgb, lab = _rand_batch(2, 8, 16, 1)
    r, l_ = _u8(rgb), _u8(lab)
    table = aug.table([A.identity_params()] * 2, 16, 8, torch.device('cuda'))
    out, lout = torch.empty_like(r), torch.empty_like(l_)
    src = table.data_ptr() + 2 * 128
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.DsrlHipError):           # no parameter table
        _lib.call('dsrl_augment_geometry', r.data_ptr(), l_.data_ptr(), None, src, out.data_ptr(), lout.data_ptr(), 2, 8, 16, s)
    with pytest.raises(_lib.DsrlHipError):           # labels without label indices
        _lib.call('dsrl_augment_geometry', r.data_ptr(), l_.data_ptr(), table.data_ptr(), None, out.data_ptr(), lout.data_ptr(), 2, 8, 16, s)
    with pytest.raises(_lib.DsrlHipError):           # misaligned table
        _lib.call('dsrl_augment_geometry', r.data_ptr(), None, table.data_ptr() + 4, None, out.data_ptr(), None, 2, 8, 16, s)
    with pytest.raises(_lib.DsrlHipError):           # in place
        _lib.call('dsrl_augment_geometry', r.data_ptr(), None, table.data_ptr(), None, r.data_ptr(), None, 2, 8, 16, s)
    with pytest.raises(_lib.DsrlHipError):           # empty batch
        _lib.call('dsrl_augment_geometry', r.data_ptr(), None, table.data_ptr(), None, out.data_ptr(), None, 0, 8, 16, s)
    prep = aug.prep
    lut = prep.lut_host.cuda()
    img_in = torch.empty((2, 4, 8, 4), device='cuda'); img_org = torch.empty((2, 8, 16, 3), device='cuda')
    tgt = torch.empty((2, 8, 16), dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.DsrlHipError):           # a 1-pixel-high sample cannot be blurred with reflect padding
        _lib.call('dsrl_prepare_batch_augmented', r.data_ptr(), l_.data_ptr(), lut.data_ptr(), prep.mean, prep.std, img_in.data_ptr(), img_org.data_ptr(),
                  tgt.data_ptr(), 2, 1, 16, 4, 8, table.data_ptr(), s)
    with pytest.raises(_lib.DsrlHipError):           # labels without a target
        _lib.call('dsrl_prepare_batch_augmented', r.data_ptr(), l_.data_ptr(), lut.data_ptr(), prep.mean, prep.std, img_in.data_ptr(), img_org.data_ptr(),
                  None, 2, 8, 16, 4, 8, table.data_ptr(), s)
    with pytest.raises(_lib.DsrlHipError):           # no parameter table
        _lib.call('dsrl_prepare_batch_augmented', r.data_ptr(), l_.data_ptr(), lut.data_ptr(), prep.mean, prep.std, img_in.data_ptr(), img_org.data_ptr(),
                  tgt.data_ptr(), 2, 8, 16, 4, 8, None, s)
    with pytest.raises(ValueError):                  # a table of another batch size
        aug(r, l_, table[:128 + 4 * 24])
    torch.cuda.synchronize()


def _write_tree(root, split, n, H, W, seed):
    from PIL import Image
    rgb, lab = _rand_batch(n, H, W, seed)
    for i in range(n):
        city = 'aachen'
        for d in ('leftImg8bit', 'gtFine'):
            os.makedirs(os.path.join(root, d, split, city), exist_ok=True)
        stem = f'{city}_{i:06d}_000019'
        Image.fromarray(rgb[i]).save(os.path.join(root, 'leftImg8bit', split, city, stem + '_leftImg8bit.png'))
        Image.fromarray(lab[i]).save(os.path.join(root, 'gtFine', split, city, stem + '_gtFine_labelIds.png'))


def _cache_tree(tmp_path):
    """4 train + 2 val images at 64x128: a PNG tree, or without PIL the pre-decoded cache written directly."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L
    data = str(tmp_path / 'data')
    try:
        import PIL  # noqa: F401
        _write_tree(data, 'train', 4, 64, 128, 1)
        _write_tree(data, 'val', 2, 64, 128, 2)
        return data, None
    except ImportError:
        cache = os.path.join(data, 'dsrl_u8_cache')
        os.makedirs(cache)
        index = {'version': L.CACHE_VERSION, 'splits': {}}
        for split, n, seed in (('train', 4, 1), ('val', 2, 2)):
            rgb, lab = _rand_batch(n, 64, 128, seed)
            np.save(os.path.join(cache, f'{split}_rgb.npy'), rgb)
            np.save(os.path.join(cache, f'{split}_labels.npy'), lab)
            index['splits'][split] = {'count': n, 'height': 64, 'width': 128, 'images': [f'{split}{i}' for i in range(n)],
                                      'labels': [f'{split}{i}' for i in range(n)]}
        import json
        with open(os.path.join(cache, L.INDEX), 'w') as f:
            json.dump(index, f)
        return data, cache


def test_train_or_resume_reads_cityscapes_without_a_loader_factory(tmp_path):
    from dualsuperreslearningforsemseg_amd import functional as HF, settings
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import train_or_resume
    data, _ = _cache_tree(tmp_path)

    def run(tag):
        torch.manual_seed(1234)
        HF.set_dropout_seed(77)
        kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                  dataset={'path': data, 'settings': cs}, val_interval=1, checkpoint_interval=1, checkpoint_history=2, init_weights=None,
                  batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9, weights_decay=5e-4, poly_power=0.9, stage=3,
                  w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / tag), description='test', early_stopping=False,
                  pretrained_backbone=False, model_input_size=(32, 64))
        return train_or_resume(is_resuming_training=False, **kw)

    h1 = run('a')
    assert os.path.isfile(os.path.join(data, 'dsrl_u8_cache', 'index.json'))
    assert all(np.isfinite(v) for v in h1[0]['train'][:4]) and h1[0]['train'][0] > 0
    assert 'val' in h1[0] and 0 <= h1[0]['val'][4] <= 100 and np.isfinite(h1[0]['val'][3])
    ckdir = os.path.join(str(tmp_path / 'a'), settings.CHECKPOINTS_DIR.format(stage=3))
    assert os.path.isfile(os.path.join(ckdir, settings.CHECKPOINT_FILE.format(epoch=1)))
    assert os.path.isfile(os.path.join(str(tmp_path / 'a'), settings.WEIGHTS_DIR.format(stage=3), settings.FINAL_WEIGHTS_FILE))
    h2 = run('b')
    assert h2[0]['train'][:4] == h1[0]['train'][:4]


def test_loader_yields_the_rank_share_of_augmented_batches(tmp_path):
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L
    data, _ = _cache_tree(tmp_path)
    ds = {'path': data, 'settings': cs}
    factory = L.loader_factory(ds, (16, 32), 54321)
    tr = factory('train', 1, torch.device('cuda'), 1, 2)
    va = factory('val', 3, torch.device('cuda'), 0, 1)
    assert len(tr) == 2 and len(va) == 1
    tr.set_epoch(5)
    got = list(tr)
    assert len(got) == 2 and got[0][0][0].shape == (1, 3, 16, 32) and got[0][1][0].shape == (1, 32, 64)
    tr.set_epoch(5)
    again = list(tr)
    for (a, b) in zip(got, again):
        assert torch.equal(a[0][1], b[0][1]) and torch.equal(a[1][0], b[1][0])
    vb = list(va)
    assert len(vb) == 1 and vb[0][0][1].shape == (2, 3, 32, 64)
    # validation batches are DeviceBatchPreparation of the cached samples in file order
    c = L.CityscapesCache(L.cache_dir_of(ds), 'val')
    prep = DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, (16, 32), cs.IGNORE_CLASS_LABEL)
    (pi, po), (pt, _) = prep(_u8(np.asarray(c.rgb)), _u8(np.asarray(c.labels)))
    assert torch.equal(vb[0][0][1], po) and torch.equal(vb[0][1][0], pt)

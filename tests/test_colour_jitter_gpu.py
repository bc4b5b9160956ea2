"""The colour jitter on the MI355X: dsrl_colour_jitter_means and dsrl_prepare_batch_jittered against the torch restatement of the specification
(colour_jitter_ref) at the tolerance of the float tail (test_augment_gpu: 1e-5 of the range; the float32 and float64 restatements of the jitter
differ by at most 7e-7 of the range over all 24 orders at the extreme factors; the library is built without FMA contraction, so the margin is
for the 0..255 scale the kernel works in and the order of its sums), jitter switched off against the code path without it bit for bit,
argument refusals, and the Cityscapes loader with dataset['color_jitter']."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import augment_ref as R
import colour_jitter_ref as J
import make_augment_golden as M
from hip_helpers import check, host, rel_err
from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
from dualsuperreslearningforsemseg_amd.models.transforms import DeviceBatchPreparation, DeviceJointAugmentation
from dualsuperreslearningforsemseg_amd.models.transforms import augment as A

pytestmark = pytest.mark.gpu

TOL = 1e-5
REFERENCE_VALUES = (0.4, 0.4, 0.4, 0.4)
LUT = R.lut_of(cs.LABEL_MAPPING_DICT)
ORDERS = list(itertools.permutations(range(4)))


def _u8(a):
    return torch.from_numpy(np.array(a)).cuda()


def _aug(size=M.MODEL_INPUT, color_jitter=REFERENCE_VALUES, **kw):
    return DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL, color_jitter=color_jitter, **kw)


def _rand_batch(N, H, W, seed):
    rng = np.random.default_rng(seed)
    ids = np.array(sorted(k for k in cs.LABEL_MAPPING_DICT if 0 <= k < 256), dtype=np.uint8)
    return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), ids[rng.integers(0, len(ids), (N, H, W))]


def _with(j, **kw):
    return A.identity_params()._replace(jitter=j, **kw)


def _compare(aug, rgb, lab, params, size, geometry):
    """Runs the batch on the device and checks every sample against the float32 restatement; returns the reference."""
    (img_in, img_org), (target, aux) = aug(_u8(rgb), _u8(lab), params)
    ref = J.batch(rgb, lab, params, LUT, cs.MEAN, cs.STD, size, geometry=geometry)
    a, b, t = host(img_in), host(img_org), target.cpu().numpy()
    assert aux is None
    for i in range(len(params)):
        e1, e2 = rel_err(a[i], ref[0][i]), rel_err(b[i], ref[1][i])
        print(f'sample {i} {params[i].jitter}: img_in {e1:.2e} img_org {e2:.2e}')
    for i in range(len(params)):
        check(a[i], ref[0][i], TOL, f'img_in[{i}] {params[i].jitter}')
        check(b[i], ref[1][i], TOL, f'img_org[{i}] {params[i].jitter}')
        assert np.array_equal(t[i], ref[2][i]), i
    return ref


# ---------------------------------------------------------------------------------------------- 1. each operation alone
def test_each_operation_alone():
    one = lambda **kw: A.ColourJitterParams((0, 1, 2, 3), **{**dict(brightness=None, contrast=None, saturation=None, hue=None), **kw})
    js = [one(brightness=0.6), one(brightness=1.4), one(contrast=0.6), one(contrast=1.4), one(saturation=0.6), one(saturation=1.4),
          one(saturation=0.0), one(hue=-0.4), one(hue=0.4), one(hue=-0.5), one(hue=0.5)]
    rgb, lab = _rand_batch(len(js), 48, 96, 11)
    _compare(_aug(), rgb, lab, [_with(j) for j in js], M.MODEL_INPUT, geometry=False)


# ---------------------------------------------------------------------------------------------- 2. all 24 orders in one batch
@pytest.mark.parametrize('factors', [(1.4, 1.4, 1.4, 0.4), (0.6, 0.6, 0.6, -0.4)])
def test_all_24_orders_in_one_batch(factors):
    rgb, lab = _rand_batch(24, 48, 96, 24)
    params = [_with(A.ColourJitterParams(o, *factors)) for o in ORDERS]
    ref = _compare(_aug(), rgb, lab, params, M.MODEL_INPUT, geometry=False)
    # On one image (reference only), how far apart are the outputs of two different orders, in normalised units (range about 4.5)?
    same = [J.sample(rgb[0], lab[0], p, LUT, cs.MEAN, cs.STD, M.MODEL_INPUT, geometry=False)[1] for p in params]
    pairs = [(float(np.abs(same[a] - same[b]).max()), ORDERS[a], ORDERS[b]) for a in range(24) for b in range(a)]
    gaps = [g for g, _, _ in pairs]
    print(f'factors {factors}: smallest difference between two orders {min(gaps):.2e}, {sum(g < 0.08 for g in gaps)} of {len(gaps)} pairs below 0.08')
    if factors[0] > 1.0:
        # every operation reaches its clamp: all 276 pairs of orders are told apart (smallest gap 0.16), so a wrong order or a mean taken at the
        # wrong point misses the tolerance by four orders of magnitude
        assert min(gaps) >= 0.08
        # the inputs exercise the clamps: the specification without them misses the tolerance
        free = J.batch(rgb, lab, params, LUT, cs.MEAN, cs.STD, M.MODEL_INPUT, geometry=False, clamp=False)
        assert rel_err(free[1], ref[1]) > TOL
    else:
        # At 0.6 brightness, contrast and saturation never reach a clamp: they are affine and commute with each other, and with the hue rotation
        # wherever that stays inside the unit cube.  What does not commute even then is gray: the rotation keeps (R + G + B) / 3, not
        # 0.2989 R + 0.587 G + 0.114 B, so contrast's mean and saturation's gray change when they move across hue.  Hence, of the 276 pairs:
        #   52 compute the same thing (they agree to float32 rounding, <= 1e-5 absolute),
        #   every other pair differs by >= 0.05 (smallest 0.053: 5000 x the tolerance), 36 of them by less than 0.08,
        #   and every pair that places hue differently relative to contrast or to saturation (208 pairs) is among those.
        across = lambda o: (o.index(A.JITTER_CONTRAST) < o.index(A.JITTER_HUE), o.index(A.JITTER_SATURATION) < o.index(A.JITTER_HUE))
        coincide = [x for x in pairs if x[0] <= 1e-5]
        apart = [x for x in pairs if x[0] > 1e-5]
        assert len(coincide) == 52 and min(g for g, _, _ in apart) >= 0.05 and sum(g < 0.08 for g, _, _ in apart) == 36
        moved = [g for g, a, b in pairs if across(a) != across(b)]
        assert len(moved) == 208 and min(moved) >= 0.05
        assert all(across(a) == across(b) for _, a, b in coincide)

# ---------------------------------------------------------------------------------------------- 3. with everything else
def test_jitter_with_rotation_crop_flip_blur_and_gray(golden):
    g = golden('augment')
    js = [A.ColourJitterParams((1, 3, 0, 2), 1.4, 0.6, 1.4, 0.4), A.ColourJitterParams((3, 2, 1, 0), 0.6, 1.4, 0.0, -0.5),
          A.ColourJitterParams((0, 2, 3, 1), 1.3, 1.4, 0.7, 0.1), A.ColourJitterParams((2, 0, 1, 3), 0.8, None, 1.2, None),
          A.ColourJitterParams((2, 1, 3, 0), 1.4, 1.4, 1.4, -0.4)]
    params = [p._replace(jitter=j) for p, j in zip(M.params_of(g), js)]
    rgb, lab = np.array(g['rgb']), np.array(g['labels'])
    (img_in, img_org), (target, _) = _aug()(_u8(rgb), _u8(lab), params)
    ref = J.batch(rgb, lab, params, LUT, cs.MEAN, cs.STD, M.MODEL_INPUT)
    for i in range(5):
        print(f'sample {i}: img_in {rel_err(host(img_in)[i], ref[0][i]):.2e} img_org {rel_err(host(img_org)[i], ref[1][i]):.2e}')
    check(host(img_in), ref[0], TOL, 'img_in')
    check(host(img_org), ref[1], TOL, 'img_org')
    assert np.array_equal(target.cpu().numpy(), g['target'])                   # the jitter does not touch the labels
    assert rel_err(ref[1], g['img_org']) > 0.05                                # and it is not a no-op on these images


# ---------------------------------------------------------------------------------------------- 4. the mean kernel on its own
def _means(rgb_d, rows_d, N, H, W, fill=-7.0):
    ws_bytes = _lib.query('dsrl_colour_jitter_workspace_bytes', N, H, W)
    assert ws_bytes >= 8 * N
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device='cuda')
    means = torch.full((N,), fill, dtype=torch.float32, device='cuda')
    _lib.call('dsrl_colour_jitter_means', rgb_d.data_ptr(), rows_d.data_ptr(), means.data_ptr(), ws.data_ptr(), ws_bytes, N, H, W,
              torch.cuda.current_stream().cuda_stream)
    return means.cpu().numpy()


@pytest.mark.parametrize('order', [(1, 0, 2, 3), (0, 2, 3, 1), (3, 0, 1, 2)], ids=['first', 'last', 'middle'])
@pytest.mark.parametrize('H,W', [(2, 2), (3, 67), (100, 150), (256, 512)])
def test_contrast_mean(H, W, order):
    rgb, _ = _rand_batch(3, H, W, H + W)
    on = A.ColourJitterParams(order, 1.4, 1.3, 1.4, 0.4)
    js = [on, on._replace(contrast=None), on._replace(brightness=0.7, saturation=0.2, hue=-0.3)]
    rows = A.pack_jitter([_with(j) for j in js])
    rgb_d, rows_d = _u8(rgb), torch.from_numpy(rows.view(np.uint8).ravel()).cuda()
    m1 = _means(rgb_d, rows_d, 3, H, W)
    m2 = _means(rgb_d, rows_d, 3, H, W)
    torch.cuda.synchronize()
    for i in (0, 2):                                                           # sample 1 has no contrast: its entry is nobody's business
        want = J.prefix_mean(rgb[i], js[i])
        print(f'{H}x{W} order {order} sample {i}: mean {m1[i]:.7f} reference {want:.7f}')
        check(np.array([m1[i]]), np.array([want]), TOL, f'mean[{i}]')
    assert m1[[0, 2]].tobytes() == m2[[0, 2]].tobytes()


# ---------------------------------------------------------------------------------------------- 5. off means off
@pytest.mark.parametrize('H,W,size', [(48, 96, (16, 32)), (256, 512, (64, 128)), (100, 150, (37, 61))])
def test_jitter_off_is_the_path_without_it_bit_for_bit(H, W, size):
    rgb, lab = _rand_batch(3, H, W, H)
    today = DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL)
    ps = today.draw(1, range(3), (H, W))
    (a_in, a_org), (a_t, _) = today(_u8(rgb), _u8(lab), ps)
    for cj in (None, (0, 0, 0, 0), {'brightness': (1.0, 1.0), 'hue': (0.0, 0.0)}):
        off = _aug(size, cj)
        assert off.draw(1, range(3), (H, W)) == ps and not off.jitter
        (b_in, b_org), (b_t, _) = off(_u8(rgb), _u8(lab), off.draw(1, range(3), (H, W)))
        assert torch.equal(a_in, b_in) and torch.equal(a_org, b_org) and torch.equal(a_t, b_t), cj
    # dsrl_prepare_batch_augmented itself, under identity parameters, is still dsrl_prepare_batch
    prep = DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL)
    table = today.table([A.identity_params()] * 3, W, H, torch.device('cuda'))
    (c_in, c_org), (c_t, _) = today.prepare(_u8(rgb), _u8(lab), table)
    (d_in, d_org), (d_t, _) = prep(_u8(rgb), _u8(lab))
    assert torch.equal(c_in, d_in) and torch.equal(c_org, d_org) and torch.equal(c_t, d_t)


def test_jitter_rows_that_do_nothing_change_nothing():
    """The jittered kernels with every slot disabled compute what the kernels without jitter compute."""
    rgb, lab = _rand_batch(2, 48, 96, 5)
    ps = [A.identity_params()._replace(blur=True, sigma=1.1), A.identity_params()._replace(flip=True, gray=True)]
    (a_in, a_org), (a_t, _) = _aug(color_jitter=None)(_u8(rgb), _u8(lab), ps)
    (b_in, b_org), (b_t, _) = _aug()(_u8(rgb), _u8(lab), ps)                    # a jittering transform, samples without a jitter
    assert torch.equal(a_in, b_in) and torch.equal(a_org, b_org) and torch.equal(a_t, b_t)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_bad_arguments_are_refused_and_write_nothing():
    lib = _lib.load()
    N, H, W = 2, 8, 16
    aug = _aug((4, 8))
    rgb, lab = _rand_batch(N, H, W, 1)
    r, l_ = _u8(rgb), _u8(lab)
    ps = aug.draw(0, range(N), (H, W))
    table = aug.table(ps, W, H, torch.device('cuda'))
    rows = table.data_ptr() + A.jitter_offset(N, W, H)
    s = torch.cuda.current_stream().cuda_stream
    need = lib.dsrl_colour_jitter_workspace_bytes(N, H, W)
    assert need == lib.dsrl_colour_jitter_workspace_bytes(N, H, W) > 0 and lib.dsrl_colour_jitter_workspace_bytes(0, H, W) == 0
    ws = torch.full((need // 8 + 1,), -3.0, dtype=torch.float64, device='cuda')
    means = torch.full((N,), -7.0, dtype=torch.float32, device='cuda')
    BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3

    def mean_call(rgb=r.data_ptr(), jitter=rows, means_=means.data_ptr(), ws_=ws.data_ptr(), ws_bytes=need, n=N, h=H, w=W):
        return lib.dsrl_colour_jitter_means(rgb, jitter, means_, ws_, ws_bytes, n, h, w, s)

    assert mean_call(rgb=None) == BADARG
    assert mean_call(jitter=None) == BADARG
    assert mean_call(means_=None) == BADARG
    assert mean_call(ws_=None) == BADARG
    assert mean_call(jitter=rows + 2) == BADARG                                 # misaligned rows
    assert mean_call(means_=means.data_ptr() + 2) == BADARG
    assert mean_call(ws_=ws.data_ptr() + 4) == BADARG
    assert mean_call(ws_bytes=need - 1) == WORKSPACE
    assert mean_call(ws_bytes=0) == WORKSPACE
    assert mean_call(h=32768, w=32768) == UNSUPPORTED                           # 3 * 2^30 bytes in a sample
    assert mean_call(n=0) == BADARG
    assert b'colour_jitter_means' in lib.dsrl_last_error()
    torch.cuda.synchronize()
    assert bool((means == -7.0).all()) and bool((ws == -3.0).all())

    prep = aug.prep
    lut = prep.lut_host.cuda()
    img_in = torch.full((N, 4, 8, 4), -5.0, device='cuda')
    img_org = torch.full((N, 8, 16, 3), -5.0, device='cuda')
    tgt = torch.full((N, 8, 16), 77, dtype=torch.uint8, device='cuda')
    good = torch.zeros((N,), dtype=torch.float32, device='cuda')

    def prep_call(params=table.data_ptr(), jitter=rows, means_=good.data_ptr(), h=H, w=W, target=tgt.data_ptr()):
        return lib.dsrl_prepare_batch_jittered(r.data_ptr(), l_.data_ptr(), lut.data_ptr(), prep.mean, prep.std, img_in.data_ptr(), img_org.data_ptr(),
                                               target, N, h, w, 4, 8, params, jitter, means_, s)

    assert prep_call(jitter=None) == BADARG
    assert prep_call(means_=None) == BADARG                                     # a jitter table without means
    assert prep_call(jitter=rows + 1) == BADARG
    assert prep_call(means_=good.data_ptr() + 2) == BADARG
    assert prep_call(params=None) == BADARG
    assert prep_call(params=table.data_ptr() + 4) == BADARG
    assert prep_call(target=None) == BADARG                                     # labels without a target
    assert prep_call(h=1) == BADARG
    assert prep_call(h=32768, w=32768) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((img_in == -5.0).all()) and bool((img_org == -5.0).all()) and bool((tgt == 77).all())
    # the transform refuses parameters with a jitter when it was built without one, and a table of the wrong size
    with pytest.raises(ValueError):
        _aug((4, 8), None)(r, l_, ps)
    with pytest.raises(ValueError):
        aug(r, l_, table[:A.table_bytes(N, W, H)])
    # and the good call goes through
    assert mean_call() == 0 and prep_call(means_=means.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((img_org != -5.0).all())


# ---------------------------------------------------------------------------------------------- 7. loader
def _write_cache(tmp_path):
    """6 train + 2 val samples of 64x128, written as the pre-decoded cache."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L
    data = str(tmp_path / 'data')
    cache = os.path.join(data, 'dsrl_u8_cache')
    os.makedirs(cache)
    index = {'version': L.CACHE_VERSION, 'splits': {}}
    for split, n, seed in (('train', 6, 1), ('val', 2, 2)):
        rgb, lab = _rand_batch(n, 64, 128, seed)
        np.save(os.path.join(cache, f'{split}_rgb.npy'), rgb)
        np.save(os.path.join(cache, f'{split}_labels.npy'), lab)
        index['splits'][split] = {'count': n, 'height': 64, 'width': 128, 'images': [f'{split}{i}' for i in range(n)],
                                  'labels': [f'{split}{i}' for i in range(n)]}
    with open(os.path.join(cache, L.INDEX), 'w') as f:
        json.dump(index, f)
    return data


def test_loader_jitters_train_batches_only(tmp_path):
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L
    data = _write_cache(tmp_path)
    plain = {'path': data, 'settings': cs}
    jit = dict(plain, color_jitter=REFERENCE_VALUES)
    dev = torch.device('cuda')
    tr = L.loader_factory(jit, (16, 32), 54321)('train', 2, dev, 0, 1)
    assert tr.transform.jitter and tr.transform.color_jitter == A.jitter_ranges(REFERENCE_VALUES)
    assert not L.loader_factory(plain, (16, 32), 54321)('train', 2, dev, 0, 1).transform.jitter
    c = L.CityscapesCache(L.cache_dir_of(jit), 'train')
    direct = _aug((16, 32), REFERENCE_VALUES, seed=54321)
    epochs = []
    for epoch in (3, 4):
        tr.set_epoch(epoch)
        got = list(tr)
        assert len(got) == 3
        for ids, ((img, org), (tgt, _)) in zip(tr._batches(epoch), got):
            ps = direct.draw(epoch, ids, (64, 128))
            assert all(p.jitter is not None for p in ps)
            (d_img, d_org), (d_tgt, _) = direct(_u8(np.stack([c.rgb[i] for i in ids])), _u8(np.stack([c.labels[i] for i in ids])), ps)
            assert torch.equal(img, d_img) and torch.equal(org, d_org) and torch.equal(tgt, d_tgt)
        epochs.append(torch.cat([b[0][1] for b in got]))
    assert not torch.equal(epochs[0], epochs[1])
    # the jitter shows: the same loader without the key yields other images and the same targets
    tp = L.loader_factory(plain, (16, 32), 54321)('train', 2, dev, 0, 1)
    tp.set_epoch(4)
    other = list(tp)
    assert not torch.equal(torch.cat([b[0][1] for b in other]), epochs[1])
    tr.set_epoch(4)
    assert all(torch.equal(a[1][0], b[1][0]) for a, b in zip(other, list(tr)))
    # validation never jitters
    va, vb = (list(L.loader_factory(d, (16, 32), 54321)('val', 2, dev, 0, 1)) for d in (plain, jit))
    assert len(va) == len(vb) == 1
    assert torch.equal(va[0][0][0], vb[0][0][0]) and torch.equal(va[0][0][1], vb[0][0][1]) and torch.equal(va[0][1][0], vb[0][1][0])

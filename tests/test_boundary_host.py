"""CPU checks of Boundary IoU: the reference itself (tests/boundary_ref.py: the window rule against the paper's per-class erosion, and against
scipy where it is installed), the input generator of the GPU tests, the host arithmetic of functional.boundary_distance and
metrices.boundary_figures, the pure host halves of the library's entry points, and every argument check that has to come before any device work."""
import math

import numpy as np
import pytest
import torch

import boundary_ref as R

NC, IGNORE = 19, 255


def _noisy(seed, shape, C=NC, void=0.08):
    """blobs with label noise: a coarse random grid, some pixels redrawn, a share of void and of labels >= C in the target"""
    rs = np.random.RandomState(seed)
    N, H, W = shape
    coarse = rs.randint(0, C, (N, -(-H // 5), -(-W // 7))).astype(np.uint8)
    tg = np.repeat(np.repeat(coarse, 5, axis=1), 7, axis=2)[:, :H, :W].copy()
    pr = np.roll(tg, (1, 2), axis=(1, 2)).copy()
    noise = rs.uniform(size=shape) < 0.03
    pr[noise] = rs.randint(0, C, int(noise.sum()))
    u = rs.uniform(size=shape)
    tg[u < void] = IGNORE
    tg[(u >= void) & (u < void + 0.02)] = 200
    return pr, tg


@pytest.mark.parametrize('shape,d', [((1, 1, 1), 1), ((1, 3, 5), 1), ((1, 3, 5), 7), ((2, 13, 29), 1), ((2, 13, 29), 2), ((1, 37, 53), 3),
                                     ((2, 40, 61), 7), ((1, 70, 131), 16), ((1, 70, 200), 64)], ids=str)
def test_the_two_band_formulations_agree(shape, d):
    pr, tg = _noisy(sum(shape) + d, shape)
    a = R.counts(pr, tg, NC, d, IGNORE, band_of=R.band_window)
    b = R.counts(pr, tg, NC, d, IGNORE, band_of=R.band_erosion)
    assert np.array_equal(a['band'], b['band'])
    for k in ('I', 'G', 'P'):
        assert np.array_equal(a[k], b[k]), k
    assert a['counts'].shape == (3 * NC,) and a['counts'].dtype == np.int64
    assert (a['I'] <= a['G']).all() and (a['I'] <= a['P']).all()


@pytest.mark.parametrize('d', [1, 2, 3, 7, 16])
def test_band_against_scipy_binary_erosion(d):
    ndi = pytest.importorskip('scipy.ndimage')
    pr, tg = _noisy(40 + d, (2, 45, 77))
    g, p = R.normalise(pr, tg, NC, IGNORE)
    for m in (g, p):
        want = np.zeros(m.shape, bool)
        for n in range(m.shape[0]):
            for v in np.unique(m[n]):
                mask = m[n] == v
                want[n] |= mask & ~ndi.binary_erosion(mask, structure=np.ones((3, 3), bool), iterations=d, border_value=0)
        assert np.array_equal(R.band_window(m, d), want)


def test_reference_on_hand_made_maps():
    """a uniform image: the band is the frame of width d; one other pixel adds its clipped (2d+1)^2 square; void pixels leave every count"""
    H, W, d = 9, 12, 2
    m = np.full((1, H, W), 3, np.uint8)
    frame = np.ones((H, W), bool)
    frame[d:H - d, d:W - d] = False
    assert np.array_equal(R.band_window(m, d)[0], frame)
    m[0, 4, 6] = 5
    want = frame.copy()
    want[2:7, 4:9] = True
    assert np.array_equal(R.band_window(m, d)[0], want) and np.array_equal(R.band_erosion(m, d)[0], want)
    r = R.counts(m, m, NC, d)
    assert np.array_equal(r['I'], r['G']) and np.array_equal(r['G'], r['P']) and r['G'][3] == want.sum() - 1 and r['G'][5] == 1 and not r['bad']
    tg = m.copy()
    tg[0, :, :3] = IGNORE
    pr = m.copy()
    pr[0, :, :3] = 77                       # garbage under void: masked
    pr[0, 8, 11] = 40                       # on a counted pixel: bad, in no class's P, but it breaks the uniformity around it
    r = R.counts(pr, tg, NC, d)
    assert r['bad'] and r['valid'] == H * (W - 3) and (r['band'][0, :, :3] == 0).all()
    # the bad pixel leaves P and I; (6, 9), the one pixel off the frame whose window reaches it, enters the prediction's band alone
    assert r['P'].sum() == r['G'].sum() - 1 + 1 and r['I'].sum() == r['G'].sum() - 1
    assert r['band'][0, 6, 9] == 2 and r['band'][0, 8, 11] == 3 and r['band'][0, 4, 9] == 0
    b, mean = R.figures([1, 0, 2], [2, 0, 2], [1, 0, 4])
    assert b[0] == 50.0 and np.isnan(b[1]) and b[2] == 50.0 and mean == 50.0


@pytest.mark.parametrize('case', R.STRUCTURED, ids=lambda c: 'x'.join(map(str, c)))
def test_the_structured_generator_satisfies_its_conditions(case):
    """band and interior, hit and miss all occur: the band share and the share of the target band that the prediction's band hits"""
    N, H, W, d = case
    pr, tg = R.structured(N, H, W, d)
    assert pr.shape == tg.shape == (N, H, W) and pr.dtype == tg.dtype == np.uint8 and (tg == R.VOID).any() and (pr < NC).all()
    r = R.counts(pr, tg, NC, d)
    share, hit = r['G'].sum() / r['valid'], r['I'].sum() / r['G'].sum()
    print(case, 'band share %.3f' % share, 'I/G %.3f' % hit)
    assert 0.3 <= share <= 0.9 and 0.05 <= hit <= 0.95
    assert (r['band'] == 0).any() and (r['band'] == 3).any()


def test_boundary_distance_values():
    from dualsuperreslearningforsemseg_amd import functional as HF
    assert [HF.boundary_distance(*s) for s in ((1024, 2048), (512, 1024), (256, 512), (8, 8))] == [46, 23, 11, 1]
    assert HF.boundary_distance(1, 1) == 1 and HF.boundary_distance(1024, 2048, 0.01) == 23 and HF.boundary_distance(2048, 2048) == 58
    assert all(HF.boundary_distance(h, w, r) == R.distance(h, w, r) for h, w, r in ((1024, 2048, 0.02), (100, 37, 0.05), (3, 5, 0.02)))
    for bad in (0.0, -0.02, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='ratio'):
            HF.boundary_distance(64, 64, bad)
    with pytest.raises(ValueError):
        HF.boundary_distance(0, 64)


def test_boundary_figures_arithmetic():
    from dualsuperreslearningforsemseg_amd.metrices import BoundaryIoU, boundary_figures
    I, G, P = [1, 0, 2, 0], [2, 0, 2, 5], [1, 0, 4, 0]
    for counts in (np.array(I + G + P), torch.tensor(I + G + P).numpy(), I + G + P):
        f = boundary_figures(counts)
        assert f['BIoU'].dtype == np.float64 and f['BIoU'][0] == 50.0 and np.isnan(f['BIoU'][1]) and f['BIoU'][2] == 50.0 and f['BIoU'][3] == 0.0
        assert abs(f['mBIoU'] - 100.0 / 3.0) < 1e-12
        assert all(f[k].dtype == np.int64 and f[k].tolist() == v for k, v in (('I', I), ('G', G), ('P', P)))
    want, mean = R.figures(I, G, P)
    assert np.allclose(f['BIoU'], want, rtol=1e-12, atol=0, equal_nan=True) and abs(f['mBIoU'] - mean) < 1e-10
    empty = boundary_figures(np.zeros(6, np.int64))
    assert np.isnan(empty['BIoU']).all() and math.isnan(empty['mBIoU'])
    # the class before anything is fed, and merge of host tensors
    b = BoundaryIoU(4)
    assert math.isnan(b.result()['mBIoU'])
    with pytest.raises(ValueError, match='before first use'):
        b.counts
    b.merge(torch.tensor(I + G + P))
    b.merge(torch.tensor(I + G + P))
    r = b.result()
    assert r['I'].tolist() == [2 * v for v in I] and r['BIoU'][0] == 50.0
    other = BoundaryIoU(4)
    other.merge(b)
    assert other.result()['G'].tolist() == [2 * v for v in G]
    b.reset()
    assert b.result()['G'].sum() == 0
    with pytest.raises(ValueError):
        b.merge(torch.zeros(11, dtype=torch.int64))
    with pytest.raises(ValueError):
        b.merge(torch.zeros(12, dtype=torch.int32))
    for kw in (dict(ratio=0.0), dict(ratio=float('nan')), dict(distance=0)):
        with pytest.raises(ValueError):
            BoundaryIoU(4, **kw)


def test_library_queries():
    """pure host code: the maxima, and a workspace size that depends on the shape only, is monotone, and is 0 for what the launch refuses"""
    from dualsuperreslearningforsemseg_amd import functional as HF
    maxc, maxd = HF.query('dsrl_boundary_counts_max_classes'), HF.query('dsrl_boundary_counts_max_distance')
    assert 19 <= maxc <= 253 and maxd >= 64
    q = lambda *a: HF.query('dsrl_boundary_counts_workspace_bytes', *a)
    sizes = [q(8, 1024, 2048, d) for d in (1, 23, 46, maxd)]
    assert len(set(sizes)) == 1 and sizes[0] == q(8, 1024, 2048, 46)            # the same call twice, and every distance
    assert sizes[0] <= 4 * 8 * 1024 * 2048
    last = 0
    for shape in ((1, 1, 1), (1, 3, 5), (2, 3, 5), (2, 13, 29), (2, 64, 64), (2, 64, 65), (3, 64, 65), (8, 512, 1024), (8, 1024, 2048)):
        cur = q(*shape, 2)
        assert cur >= last, shape
        last = cur
    assert q(0, 8, 8, 1) == 0 and q(1, 0, 8, 1) == 0 and q(1, 8, 0, 1) == 0 and q(1, 8, 8, 0) == 0 and q(1, 8, 8, maxd + 1) == 0
    assert q(4, 32768, 16384, 1) == 0                                            # 2^31 pixels


def _args(**kw):
    a = dict(counts=torch.zeros(3 * NC, dtype=torch.int64), pred=torch.zeros((2, 8, 8), dtype=torch.uint8), target=torch.zeros((2, 8, 8), dtype=torch.uint8),
             num_classes=NC)
    a.update(kw)
    return a


BAD_ARGS = [
    (dict(target=torch.zeros((2, 8, 9), dtype=torch.uint8)), 'differ in shape'),
    (dict(pred=torch.zeros((1, 2, 8, 8), dtype=torch.uint8), target=torch.zeros((1, 2, 8, 8), dtype=torch.uint8)), r'\(N, H, W\) or \(H, W\)'),
    (dict(pred=torch.zeros((0, 8, 8), dtype=torch.uint8), target=torch.zeros((0, 8, 8), dtype=torch.uint8)), 'empty'),
    (dict(distance=0), 'distance 0'),
    (dict(distance=-3), 'distance -3'),
    (dict(distance=100000), 'distance 100000'),
    (dict(ratio=0.0), 'ratio'),
    (dict(ratio=-1.0), 'ratio'),
    (dict(ratio=float('nan')), 'ratio'),
    (dict(ratio=float('inf')), 'ratio'),
    (dict(ratio=50.0), 'distance'),                                 # a finite ratio that asks for more than the maximum
    (dict(num_classes=254), 'classes'),
    (dict(num_classes=0), 'classes'),
    (dict(counts=torch.zeros(3 * NC, dtype=torch.int32)), 'counts must be'),
    (dict(counts=torch.zeros(3 * NC + 1, dtype=torch.int64)), 'counts must be'),
    (dict(counts=torch.zeros(6 * NC, dtype=torch.int64)[::2]), 'counts must be'),
    (dict(band=torch.zeros((2, 8, 8), dtype=torch.int8)), 'band must be'),
    (dict(band=torch.zeros((2, 8, 9), dtype=torch.uint8)), 'band must be'),
    (dict(nan_flag=torch.zeros((), dtype=torch.int64)), 'nan_flag must be'),
    (dict(nan_flag=torch.zeros(2, dtype=torch.int32)), 'nan_flag must be'),
]


@pytest.mark.parametrize('kw,match', BAD_ARGS, ids=['{:02d}_{}'.format(i, '_'.join(kw)) for i, (kw, _) in enumerate(BAD_ARGS)])
def test_boundary_counts_refuses_bad_arguments_on_cpu_tensors(kw, match):
    """every one of these comes before the device check: CPU tensors get this far and no further"""
    from dualsuperreslearningforsemseg_amd import functional as HF
    with pytest.raises((ValueError, HF.DsrlHipError), match=match):
        HF.boundary_counts_(**_args(**kw))


def test_boundary_counts_on_cpu_tensors_fails_loudly_after_the_checks():
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.metrices import BoundaryIoU
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HF.boundary_counts_(**_args())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        BoundaryIoU(NC).update(torch.zeros((2, 8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8))


@pytest.mark.parametrize('value', [0, 0.0, -0.02, float('nan'), float('inf'), 'yes', (0.02,)], ids=str)
def test_benchmark_refuses_a_bad_boundary_value_before_device_work(value, tmp_path):
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    asked = []
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda *a: asked.append(a) or []}
    with pytest.raises(ValueError, match='boundary|ratio'):
        benchmark(str(tmp_path / 'no.weights'), dataset, 'gpu', 0, 2, boundary=value, output_dir=str(tmp_path / 'out'))
    assert not asked and not (tmp_path / 'out').exists()


def test_benchmark_boundary_value():
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import boundary_ratio_value
    assert boundary_ratio_value(None) is None and boundary_ratio_value(False) is None
    assert boundary_ratio_value(True) == 0.02 and boundary_ratio_value(0.01) == 0.01 and boundary_ratio_value(np.float32(0.5)) == 0.5


def test_benchmark_without_boundary_does_not_mention_it():
    """An absent or false key is off, and in the command's source nothing that names the new keys, text or launches stands at the function's own
    level: each is inside a branch on `boundary` (the run itself is compared on the device: test_boundary_gpu.py)."""
    import inspect
    from dualsuperreslearningforsemseg_amd.command_handlers import benchmark as B
    assert B.boundary_ratio_value({}.get('boundary')) is None
    lines = inspect.getsource(B.benchmark).splitlines()
    for needle in ('mBIoU_dataset', 'BIoU_per_class', 'boundary IoU', 'boundary mIoU', 'boundary_counts_(', 'band_counts.double()', 'BoundaryIoU('):
        hits = [ln for ln in lines if needle in ln]
        assert hits, needle
        assert all(len(ln) - len(ln.lstrip()) >= 8 for ln in hits), needle
    assert sum('boundary is not None' in ln or 'boundary is None' in ln for ln in lines) >= 4

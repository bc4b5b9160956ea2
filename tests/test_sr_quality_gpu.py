"""The super-resolution quality kernel on the device (`-m gpu`; csrc/sr_quality.hip behind functional.sr_quality, metrices.SRQuality,
DSRL.super_resolve, the validation pass of train_or_resume and benchmark(sisr=True)) against tests/sr_quality_ref.py.

Bounds, all measured against the float64 reference and none against the code under test:
  map       |kernel - ref64| <= max(4 E32, 2^-20) per pixel, E32 = the worst per-pixel distance of the fp32 restatement (rows then columns, taps
            ascending, every operation rounded) from the float64 map FOR THAT CASE, computed here.  The factor 4 covers a legitimately different
            order of the same operations (the kernel forms the column sums in fused multiply-adds as the rows arrive); 2^-20 is 16 ulp at 1.0.
  ssim_sum  equals the float64 sum of the kernel's OWN map to 1e-10 relative: this checks the reduction, the map is checked above.
  SSIM      per image within the map bound of the reference's (a mean cannot be further off than its worst term).
  sse       within 1e-6 relative of float64: one rounding in the difference and one in the square, about 1.8e-7 per term, double accumulation.
Each test prints its figures before it asserts (pytest -s shows them)."""
import functools
import os

import numpy as np
import pytest
import torch

import sr_quality_ref as R
from hip_helpers import DEV, HF

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TILE_H, TILE_W = 32, 64                 # the kernel's tile of the SSIM map (csrc/sr_quality.hip)
SHAPES = [(1, 3, 11, 11),                                   # one valid pixel
          (2, 3, 27, 45), (1, 3, 12, 301), (1, 1, 141, 13), (3, 3, 75, 139),
          (1, 3, TILE_H + 10, TILE_W + 10),                 # the valid region is exactly one tile
          (1, 3, TILE_H + 11, TILE_W + 11),                 # one row and one column more: four tiles, three of them slivers
          # rows of W * 3 floats that are multiples of 16 bytes take the float4 loader (none of the above does); C = 2 and C = 4 are builds of their own
          (2, 3, 40, 100), (1, 3, 100, 200), (2, 2, 33, 80), (1, 4, 20, 70), (1, 1, 30, 128)]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV).contiguous(memory_format=torch.channels_last)       # a copy: the cached cases are read-only


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64 if t.dtype == torch.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """inputs and both references of one case, computed once and shared (never written to)"""
    pred, ref, mean, std = R.make_case(kind, shape)
    r64 = R.reference64(pred, ref, mean, std)
    e32 = float(np.max(np.abs(R.restatement32(pred, ref, mean, std).astype(F64) - r64['ssim_map'])))
    for a in (pred, ref, r64['sse'], r64['ssim_map'], r64['ssim_sum']):
        a.setflags(write=False)
    return pred, ref, mean, std, r64, e32


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_records_and_map_against_the_float64_reference(shape, kind):
    pred, ref, mean, std, r64, e32 = case(kind, shape)
    N, C, H, W = shape
    if kind == 'normalised':
        for t in (pred, ref):
            raw = t * np.asarray(std, F32).reshape(1, C, 1, 1) + np.asarray(mean, F32).reshape(1, C, 1, 1)
            assert ((raw < 0) | (raw > 1)).mean() >= 0.1
    records, smap = HF.sr_quality(dev(pred), dev(ref), mean, std, ssim_map=True)
    plain = HF.sr_quality(dev(pred), dev(ref), mean, std)
    assert records.shape == (N, 2) and records.dtype == torch.float64 and smap.shape == (N, C, H - 10, W - 10) and smap.dtype == torch.float32
    rec, m = records.cpu().numpy(), smap.cpu().numpy().astype(F64)
    bound = max(4 * e32, 2.0 ** -20)
    err = float(np.max(np.abs(m - r64['ssim_map'])))
    own = m.sum(axis=(1, 2, 3))
    sum_err = float(np.max(np.abs(rec[:, 1] - own) / np.abs(own)))
    psnr, ssim = HF.sr_quality_figures(records, C, H, W)
    _, ssim64 = R.figures(r64['sse'], r64['ssim_sum'], C, H, W)
    ssim_err = float(np.max(np.abs(ssim - ssim64)))
    sse_err = float(np.max(np.abs(rec[:, 0] - r64['sse']) / r64['sse']))
    print(f'sr_quality {shape} {kind}: E32 {e32:.3e}, map error {err:.3e} = {err / e32 if e32 else 0:.2f} x E32 (bound {bound:.3e}); '
          f'ssim_sum vs own map {sum_err:.1e}; SSIM error {ssim_err:.3e}; sse relative error {sse_err:.2e}; PSNR {psnr.tolist()}')
    assert err <= bound, (err, bound, e32)
    assert sum_err <= 1e-10, sum_err
    assert ssim_err <= bound, (ssim_err, bound)
    assert sse_err <= 1e-6, sse_err
    assert np.array_equal(bits(plain), bits(records))               # the record does not depend on whether the map is asked for


# ---------------------------------------------------------------------------------------------- exact properties
BIG = (3, 3, 75, 139)


@pytest.mark.parametrize('shape', [(1, 3, 11, 11), BIG, (1, 3, 100, 200), (2, 2, 33, 80), (1, 4, 20, 70), (1, 1, 141, 13)], ids=lambda s: 'x'.join(map(str, s)))
def test_bit_equal_images_give_exactly_one(shape):
    N, C, H, W = shape
    a = np.random.RandomState(11).normal(0, 2.5, shape).astype(F32)
    records, smap = HF.sr_quality(dev(a), dev(a.copy()), R.MEAN[:C], R.STD[:C], ssim_map=True)
    assert np.array_equal(smap.cpu().numpy(), np.ones((N, C, H - 10, W - 10), F32))
    assert np.array_equal(records.cpu().numpy(), np.tile(np.array([0.0, C * (H - 10) * (W - 10)], F64), (N, 1)))
    psnr, ssim = HF.sr_quality_figures(records, C, H, W)
    assert np.all(np.isposinf(psnr)) and np.array_equal(ssim, np.ones(N))


def test_two_runs_and_a_graph_replay_are_bit_identical():
    pred, ref, mean, std, _, _ = case('normalised', BIG)
    p, r = dev(pred), dev(ref)
    first, first_map = HF.sr_quality(p, r, mean, std, ssim_map=True)
    second, second_map = HF.sr_quality(p, r, mean, std, ssim_map=True)
    assert np.array_equal(bits(first), bits(second)) and np.array_equal(bits(first_map), bits(second_map))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            HF.sr_quality(p, r, mean, std, ssim_map=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_rec, g_map = HF.sr_quality(p, r, mean, std, ssim_map=True)
    g_rec.fill_(-1.0); g_map.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(g_rec), bits(first)) and np.array_equal(bits(g_map), bits(first_map))


def test_an_image_alone_equals_the_image_in_a_batch():
    pred, ref, mean, std, _, _ = case('noisy_copy', BIG)
    batch, batch_map = HF.sr_quality(dev(pred), dev(ref), mean, std, ssim_map=True)
    for n in range(BIG[0]):
        alone, alone_map = HF.sr_quality(dev(pred[n:n + 1]), dev(ref[n:n + 1]), mean, std, ssim_map=True)
        assert np.array_equal(bits(alone), bits(batch[n:n + 1])) and np.array_equal(bits(alone_map), bits(batch_map[n:n + 1])), n


@pytest.mark.parametrize('shape', [BIG, (2, 3, 40, 100)], ids=lambda s: 'x'.join(map(str, s)))
def test_layouts_give_the_dense_result(shape):
    """an ld-4 view of a 4-channel channels-last tensor (C = 3) and an NCHW-contiguous input against dense channels-last, bit for bit"""
    pred, ref, mean, std, _, _ = case('normalised', shape)
    N, C, H, W = shape
    dense, dense_map = HF.sr_quality(dev(pred), dev(ref), mean, std, ssim_map=True)

    def wide(a):
        t = torch.full((N, 4, H, W), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)      # the fourth channel must never be read into a result
        t[:, :3].copy_(torch.from_numpy(np.array(a)))
        v = t[:, :3]
        assert HF._ld_of(v) == 4
        return v

    nchw = lambda a: torch.from_numpy(np.array(a)).to(DEV).contiguous()
    for what, p, r in (('ld 4 both', wide(pred), wide(ref)), ('ld 4 pred', wide(pred), dev(ref)), ('ld 4 ref', dev(pred), wide(ref)),
                       ('nchw', nchw(pred), nchw(ref)), ('nchw pred', nchw(pred), dev(ref))):
        rec, m = HF.sr_quality(p, r, mean, std, ssim_map=True)
        assert np.array_equal(bits(rec), bits(dense)) and np.array_equal(bits(m), bits(dense_map)), what


def test_a_nan_stays_in_its_image():
    pred, ref, mean, std, _, _ = case('normalised', BIG)
    clean = HF.sr_quality(dev(pred), dev(ref), mean, std)
    for where in ((1, 0, 0, 0), (1, 2, 74, 138), (1, 1, 40, 70)):           # corners (in the squared error only where no window reaches ... every window does) and the middle
        bad = pred.copy()
        bad[where] = np.nan
        rec = HF.sr_quality(dev(bad), dev(ref), mean, std)
        assert torch.isnan(rec[1]).all(), (where, rec)
        assert np.array_equal(bits(rec[[0, 2]]), bits(clean[[0, 2]])), where
        psnr, ssim = HF.sr_quality_figures(rec, *BIG[1:])
        assert np.isnan(psnr[1]) and np.isnan(ssim[1]) and np.isfinite(psnr[[0, 2]]).all()
    rec = HF.sr_quality(dev(pred), dev(np.where(np.arange(BIG[0]).reshape(-1, 1, 1, 1) == 2, np.nan, ref).astype(F32)), mean, std)
    assert torch.isnan(rec[2]).all() and np.array_equal(bits(rec[:2]), bits(clean[:2]))


def test_library_refuses_bad_calls():
    a = dev(np.zeros((1, 3, 16, 16), F32))
    rec = torch.zeros((1, 2), dtype=torch.float64, device=DEV)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    import ctypes
    one = (ctypes.c_float * 3)(1, 1, 1)
    zero = (ctypes.c_float * 3)(0, 0, 0)
    args = lambda **k: [k.get('pred', a.data_ptr()), k.get('ld', 3), a.data_ptr(), 3, 1, k.get('C', 3), k.get('H', 16), 16, zero, k.get('std', one),
                        rec.data_ptr(), None, ws.data_ptr(), k.get('ws_bytes', 64), HF._stream()]
    for kw, code in ((dict(ld=2), -1), (dict(C=5), -1), (dict(H=10), -1), (dict(std=zero), -1), (dict(ws_bytes=8), -3), (dict(pred=None), -1)):
        with pytest.raises(HF.DsrlHipError, match=f'code {code}'):
            HF.call('dsrl_sr_quality', *args(**kw))
    HF.call('dsrl_sr_quality', *args())
    assert rec.cpu().tolist() == [[0.0, 3.0 * 6 * 6]]


# ---------------------------------------------------------------------------------------------- the model, training and the benchmark command
@pytest.fixture(scope='module')
def model2():
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    torch.manual_seed(4321)
    return DSRL(2, CS).to(DEV).to(memory_format=torch.channels_last).eval()


def _images(seed, n, hw):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, 3) + tuple(hw), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)


def test_super_resolve_is_the_eval_forward_bit_for_bit(model2):
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    x = _images(3, 2, (32, 64))
    sr = model2.super_resolve(x)
    assert sr.shape == (2, 3, 64, 128) and not sr.requires_grad
    with torch.no_grad():
        want = model2(x)[1]
    assert np.array_equal(bits(sr), bits(want))
    assert np.array_equal(bits(model2(x)[1].detach()), bits(want))
    feats = model2.feature_extractor['backbone'](x)
    assert np.array_equal(bits(model2.super_resolve_head(*[f.detach() for f in feats])), bits(want))
    model2.train()
    try:
        with pytest.raises(HF.DsrlHipError, match='eval'):
            model2.super_resolve(x)
        with pytest.raises(HF.DsrlHipError, match='eval'):
            model2.super_resolve_head(*[f.detach() for f in feats])
    finally:
        model2.eval()
    stage1 = DSRL(1, CS).to(DEV).to(memory_format=torch.channels_last).eval()
    with pytest.raises(HF.DsrlHipError, match='stage-1'):
        stage1.super_resolve(x)


def test_training_reports_psnr_and_ssim_and_the_benchmark_reads_the_weights(tmp_path, monkeypatch):
    """one epoch at stage 2 and one at stage 1 on the synthetic loader of the end-to-end test, then benchmark(sisr=True) on what they wrote"""
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.prune_weights import prune_weights
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.metrices import SRQuality

    def factory(split, batch_size, device, rank, world):
        return TR.SyntheticCityscapes(batch_size, (32, 64), device, rank=rank, length=2)

    # what the validation pass saw: the step's outputs and originals, fed by hand to a second SRQuality
    by_hand, seen = SRQuality(cs.MEAN, cs.STD), []
    enqueue = TR.TrainStep.enqueue

    def spy(self, input_image, input_org, target, lr, momentum, weight_decay, do_train=True):
        outs = enqueue(self, input_image, input_org, target, lr, momentum, weight_decay, do_train)
        if not do_train:
            seen.append(self.stage)
            if self.stage > 1:
                by_hand.update(outs[1].clone(), input_org.clone())
        return outs

    monkeypatch.setattr(TR.TrainStep, 'enqueue', spy)
    kw = dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
              dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': factory}, val_interval=1, checkpoint_interval=1,
              checkpoint_history=0, init_weights=None, batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9,
              weights_decay=5e-4, poly_power=0.9, w1=0.1, w2=1.0, freeze_batch_norm=False, description='test', early_stopping=False,
              pretrained_backbone=False, model_input_size=(32, 64))
    hist = TR.train_or_resume(stage=2, experiment_id=str(tmp_path / 'exp2'), **kw)
    rec = hist[0]
    want = by_hand.result()
    print(f"stage 2 validation: PSNR {rec['val_PSNR']:.4f} dB, SSIM {rec['val_SSIM']:.6f} over {want['images']} images")
    assert len(rec['val']) == 7 and seen == [2, 2] and want['images'] == 4
    assert np.isfinite(rec['val_PSNR']) and -1.0 <= rec['val_SSIM'] <= 1.0
    assert rec['val_PSNR'] == want['PSNR'] and rec['val_SSIM'] == want['SSIM']
    hist1 = TR.train_or_resume(stage=1, experiment_id=str(tmp_path / 'exp1'), **kw)
    assert 'val' in hist1[0] and 'val_PSNR' not in hist1[0] and 'val_SSIM' not in hist1[0] and seen == [2, 2, 1, 1]
    monkeypatch.undo()

    weights2 = os.path.join(str(tmp_path / 'exp2'), settings.WEIGHTS_DIR.format(stage=2), settings.FINAL_WEIGHTS_FILE)
    weights1 = os.path.join(str(tmp_path / 'exp1'), settings.WEIGHTS_DIR.format(stage=1), settings.FINAL_WEIGHTS_FILE)
    batches = list(factory('val', 2, torch.device(DEV), 0, 1))
    dataset = {'settings': cs, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda *a: batches}
    plain = benchmark(weights2, dataset, 'gpu', 0, 2, model_input_size=(32, 64), output_dir=str(tmp_path / 'plain'))
    result = benchmark(weights2, dataset, 'gpu', 0, 2, model_input_size=(32, 64), output_dir=str(tmp_path / 'sisr'), sisr=True)
    assert 'PSNR' not in plain and 'SSIM' not in plain
    # the segmentation figures are those of the plain command (compared as text: a class the batches lack has IoU NaN)
    assert repr(sorted((k, v) for k, v in result.items() if k not in ('PSNR', 'SSIM'))) == repr(sorted(plain.items()))
    assert np.isfinite(result['PSNR']) and -1.0 <= result['SSIM'] <= 1.0
    text, plain_text = (open(os.path.join(str(tmp_path / d), 'benchmark.txt')).read().splitlines() for d in ('sisr', 'plain'))
    assert len(text) == len(plain_text) + 2 and text[-2].endswith('PSNR dB: {:.2f}'.format(result['PSNR'])) and text[-1].endswith('SSIM: {:.4f}'.format(result['SSIM']))
    # the figures are those of the model on the loader's batches
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import load_eval_model
    model = load_eval_model(weights2, cs, torch.device(DEV), sisr=True)
    q = SRQuality(cs.MEAN, cs.STD)
    for (img, org), _ in batches:
        q.update(model.super_resolve(img), org)
    assert q.result()['PSNR'] == result['PSNR'] and q.result()['SSIM'] == result['SSIM']
    # files without the decoder: a stage-1 run's, and a pruned stage-2 file
    pruned = prune_weights(weights2, str(tmp_path / 'pruned.weights'), {'settings': cs})
    for w in (weights1, pruned):
        with pytest.raises(RuntimeError, match='SISR_decoder.0.weight'):
            benchmark(w, dataset, 'gpu', 0, 2, model_input_size=(32, 64), output_dir=str(tmp_path / 'refused'), sisr=True)

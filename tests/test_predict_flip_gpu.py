"""GPU checks of flip-averaged inference: the two-view fused tail (dsrl_sssr_tail_predict_flip) behind functional.sssr_tail_predict(flip=True),
DSRL.predict_head / predict(flip=True), CompiledPredictor(flip=True) and the benchmark / test commands with flip=True.  The reference is the fp64
restatement in predict_flip_ref; the unfused composition (both views' logits, then torch log_softmax, flip, logaddexp) is measured beside it."""
import math
import os

import numpy as np
import pytest
import torch

import gen
import predict_fixtures as PF
import predict_flip_ref as PFR

pytestmark = pytest.mark.gpu

NC = gen.NUM_CLASSES


def _helpers():
    import hip_helpers as H
    return H


def _tail_modules(p):
    """upsample16_pred[2], [3], [6] with the parameters `p` (PFR.tail_params: the recipe of test_predict_gpu._tail_modules) on the device, in eval mode"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.nn_modules import HipBatchNorm2d, HipConvTranspose2d
    nc = p['w1'].shape[0]
    c1 = HipConvTranspose2d(nc, nc, kernel_size=2, stride=2, padding=0, bias=False)
    bn = HipBatchNorm2d(nc)
    c2 = HipConvTranspose2d(nc, nc, kernel_size=2, stride=2, padding=0, bias=p['b2'] is not None)
    with torch.no_grad():
        c1.weight.copy_(torch.from_numpy(p['w1'])); c2.weight.copy_(torch.from_numpy(p['w2']))
        bn.weight.copy_(torch.from_numpy(p['gamma'])); bn.bias.copy_(torch.from_numpy(p['beta']))
        bn.running_mean.copy_(torch.from_numpy(p['mean'])); bn.running_var.copy_(torch.from_numpy(p['var']))
        if p['b2'] is not None:
            c2.bias.copy_(torch.from_numpy(p['b2']))
    return [m.to(H.DEV).eval() for m in (c1, bn, c2)]


def _unfused_scores(logits):
    """the unfused composition on the device: (2N,C,H,W) fp32 logits -> E (N,C,H,W) with torch log_softmax, flip and logaddexp"""
    n = logits.shape[0] // 2
    la = torch.log_softmax(logits[:n], dim=1)
    lb = torch.log_softmax(logits[n:], dim=1).flip(3)
    return torch.logaddexp(la, lb) - math.log(2.0)


def _unfused_ce(scores, target, ignore=gen.IGNORE):
    return float(torch.nn.functional.nll_loss(scores, target.long(), ignore_index=ignore))


def _tail_logits_gpu(x, mods):
    from dualsuperreslearningforsemseg_amd import functional as HF
    with torch.no_grad():
        return mods[2](HF.batch_norm_act(mods[0](x), mods[1], relu=True))


def _counts():
    return torch.zeros(3 * NC + 2, dtype=torch.int64, device=_helpers().DEV)


def _flag():
    return torch.zeros((), dtype=torch.int32, device=_helpers().DEV)


# ---------------------------------------------------------------------------------------------- class maps
@pytest.mark.parametrize('fixture', PFR.TAIL_FIXTURES, ids=PFR.tail_fixture_id)
def test_tail_class_maps_against_the_fp64_ensemble(fixture):
    """(3,9,13): odd W, 351 pixels (no multiple of 16), tiles that cross rows and images; W = 1: a patch mirrored onto itself; 1x1x1: a single pixel;
    W = 16: a tile that is exactly one row; (4,32,64): 8192 pixels = 512 tiles."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    p, x, L, E = PFR.tail_fixture(fixture)
    n, h, w = fixture[2:]
    pred, ce = HF.sssr_tail_predict(H.dev(x), *_tail_modules(p), flip=True)
    assert ce is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (n, 4 * h, 4 * w)
    share = PFR.check_class_map(pred.cpu().numpy(), E, L, 'fused flip tail vs fp64 ensemble')
    print(f'{PFR.tail_fixture_id(fixture)}: band {100 * share:.3f} %')


@pytest.mark.parametrize('fixture', PF.HEAD_FIXTURES, ids=PF.fixture_id)
def test_head_class_maps_and_loss(fixture):
    """DSRL.predict_head(flip=True) against the fp64 ensemble of the oracle head and against the unfused composition on the GPU (the head's eval
    forward on both halves, torch log_softmax / flip / logaddexp): class maps may differ only inside the band; the loss budget is the one of
    test_predict_gpu.test_cross_entropy_of_the_unwritten_logits: |fused - ref| <= max(4 |unfused - ref|, 1e-6 |ref|).
    Measured on the MI355X when this test first passed (losses 3.04 - 3.18): the error of the unfused composition was 3.4e-8 ... 3.2e-7 over the six
    fixtures, the fused one 2.8e-9 ... 1.4e-7 (equal to the unfused error on two fixtures, at most 1.5 x it on the others), inside the 3.0e-6 floor of
    the budget; fused and unfused class maps were equal at every pixel, band included."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    head, _ = H.make_head(gen.SMALL, 3, fixture[0], False)
    _, x16, x4, target, L, E = PFR.head_fixture(fixture)
    x16d, x4d, td = H.dev(x16), H.dev(x4), H.dev(target)
    pred, counts, ce = DSRL.predict_head(head, x16d, x4d, flip=True)
    assert counts is None and ce is None and pred.dtype == torch.uint8 and tuple(pred.shape) == E.shape[:1] + E.shape[2:]
    pred_h = pred.cpu().numpy()
    share = PFR.check_class_map(pred_h, E, L, 'fused flip head vs fp64 ensemble')
    with torch.no_grad():
        scores = _unfused_scores(head(x16d, x4d)[0])
    unfused = torch.argmax(scores, dim=1).cpu().numpy()
    PFR.check_class_map(unfused, E, L, 'unfused composition vs fp64 ensemble')
    _, _, band = PFR.band_of(E, L)
    differ = pred_h != unfused
    assert not (differ & ~band).any(), f'{int((differ & ~band).sum())} pixels outside the band differ between the fused and the unfused path'
    # the loss
    pred2, counts, ce = DSRL.predict_head(head, x16d, x4d, td, flip=True)
    assert torch.equal(pred, pred2)
    assert np.array_equal(counts.cpu().numpy(), PF.counts_table(pred_h, target))
    ref = PFR.ce(E, target)
    e_unfused, e_fused = abs(_unfused_ce(scores, td) - ref), abs(float(ce) - ref)
    budget = max(4 * e_unfused, 1e-6 * abs(ref))
    print(f'{PF.fixture_id(fixture)}: band {100 * share:.3f} %, fused != unfused at {int(differ.sum())} band pixels; ref {ref:.9f}, unfused error '
          f'{e_unfused:.3e}, fused error {e_fused:.3e}, budget {budget:.3e}')
    assert e_fused <= budget, (e_fused, budget)


# ---------------------------------------------------------------------------------------------- counters
def test_counts_equal_the_table_of_the_kernels_own_class_map():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = PFR.TAIL_FIXTURES[0]
    p, xs, _, _ = PFR.tail_fixture(f)
    mods, x = _tail_modules(p), H.dev(xs)
    shape = (f[2], 4 * f[3], 4 * f[4])
    target = PFR.make_target(13, shape)
    counts, flag = _counts(), _flag()
    pred, ce = HF.sssr_tail_predict(x, *mods, target=H.dev(target), counts=counts, nan_flag=flag, flip=True)
    pred_h = pred.cpu().numpy()
    table = PF.counts_table(pred_h, target)
    assert np.array_equal(counts.cpu().numpy(), table)
    assert int(flag.item()) == 0 and np.isfinite(float(ce))
    # the class map is the same with and without a target
    assert np.array_equal(pred_h, HF.sssr_tail_predict(x, *mods, flip=True)[0].cpu().numpy())
    # a second call accumulates
    HF.sssr_tail_predict(x, *mods, target=H.dev(target), counts=counts, flip=True)
    assert np.array_equal(counts.cpu().numpy(), 2 * table)
    # ignore_index = 0
    t0 = np.random.RandomState(14).randint(0, NC, shape).astype(np.uint8)
    c0, f0 = _counts(), _flag()
    p0, ce0 = HF.sssr_tail_predict(x, *mods, target=H.dev(t0), ignore_index=0, counts=c0, nan_flag=f0, flip=True)
    assert np.array_equal(c0.cpu().numpy(), PF.counts_table(p0.cpu().numpy(), t0, NC, 0)) and int(f0.item()) == 0
    assert c0.cpu().numpy()[2 * NC] == 0 and np.isfinite(float(ce0))
    # a label 200: out of the counts, bit 1 of the flag, and the loss is NaN
    tb = target.copy()
    tb[1, 7, 9] = 200
    cb, fb = _counts(), _flag()
    pb, ceb = HF.sssr_tail_predict(x, *mods, target=H.dev(tb), counts=cb, nan_flag=fb, flip=True)
    assert np.array_equal(cb.cpu().numpy(), PF.counts_table(pb.cpu().numpy(), tb)) and int(fb.item()) == 2
    assert np.isnan(float(ceb))
    # every pixel ignored: NaN, as torch
    _, cen = HF.sssr_tail_predict(x, *mods, target=H.dev(np.full(shape, 255, np.uint8)), flip=True)
    assert np.isnan(float(cen))


# ---------------------------------------------------------------------------------------------- loss
def test_loss_in_log_space():
    """One tail fixture with w2 x 1e3: logit gaps of several hundred, where -log(0.5 (pa + pb)) is inf in fp32.  The fused loss is finite and within
    max(4 |unfused - ref|, 1e-6 |ref|) of the fp64 value.  No class-map assertion: ties at -ln 2 are legitimate here.
    Measured on the MI355X when this test first passed (max |L| 2793, 81 % of the target probabilities underflow in fp32): ref 464.123828, fused and
    unfused both 464.123840 - the same fp32 value, 1.2e-5 off, against a budget of 4.6e-4."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = PFR.TAIL_FIXTURES[0]
    p, xs, L, E = PFR.tail_fixture(f, 1e3)
    assert np.abs(L).max() > 300
    mods, x = _tail_modules(p), H.dev(xs)
    target = PFR.make_target(15, (f[2], 4 * f[3], 4 * f[4]))
    td = H.dev(target)
    ref = PFR.ce(E, target)
    # a probability-space evaluation of the same fp64 ensemble is inf in fp32
    picked = np.take_along_axis(np.exp(E).astype(np.float32), np.where(target == 255, 0, target).astype(np.int64)[:, None], axis=1)
    assert (picked == 0).any()
    flag = _flag()
    _, ce = HF.sssr_tail_predict(x, *mods, target=td, nan_flag=flag, flip=True)
    unfused = _unfused_ce(_unfused_scores(_tail_logits_gpu(x, mods)), td)
    e_unfused, e_fused = abs(unfused - ref), abs(float(ce) - ref)
    budget = max(4 * e_unfused, 1e-6 * abs(ref))
    print(f'w2 x 1e3: ref {ref:.9f}, fused {float(ce):.9f}, unfused {unfused:.9f}, unfused error {e_unfused:.3e}, fused error {e_fused:.3e}, budget {budget:.3e}')
    assert int(flag.item()) == 0 and np.isfinite(float(ce))
    assert e_fused <= budget, (e_fused, budget)


# ---------------------------------------------------------------------------------------------- NaN, validation, fallback
def test_nan_in_either_view_raises_bit_0():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods = _tail_modules(PFR.tail_params(21))
    xs = PFR.tail_input(22, (4, NC, 6, 10))
    flag = _flag()
    HF.sssr_tail_predict(H.dev(xs), *mods, nan_flag=flag, flip=True)
    assert int(flag.item()) == 0
    for image in (1, 3):                                  # view a only, view b only
        bad = xs.copy()
        bad[image, 4, 3, 7] = np.nan
        for kw in ({}, {'target': H.dev(PFR.make_target(23, (2, 24, 40)))}):
            flag.zero_()
            HF.sssr_tail_predict(H.dev(bad), *mods, nan_flag=flag, flip=True, **kw)
            assert int(flag.item()) == 1, (image, bool(kw))


def test_an_odd_batch_raises():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods = _tail_modules(PFR.tail_params(21))
    with pytest.raises(HF.DsrlHipError, match='odd'):
        HF.sssr_tail_predict(H.dev(PFR.tail_input(22, (3, NC, 4, 4))), *mods, flip=True)


def test_heads_the_kernel_does_not_implement_form_the_ensemble_from_logits():
    """8 channels: dsrl_sssr_tail_predict_supported says 0; the ensemble is formed from the module-by-module logits"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    p = PFR.tail_params(51, nc=8)
    xs = PFR.tail_input(52, (4, 8, 6, 8))
    L = PFR.tail_logits(xs, p)
    E = PFR.ensemble_of_views(L)
    target = np.random.RandomState(53).randint(0, 8, (2, 24, 32)).astype(np.uint8)
    target[0, :3] = 255
    counts, flag = torch.zeros(3 * 8 + 2, dtype=torch.int64, device=H.DEV), _flag()
    pred, ce = HF.sssr_tail_predict(H.dev(xs), *_tail_modules(p), target=H.dev(target), counts=counts, nan_flag=flag, flip=True)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (2, 24, 32) and int(flag.item()) == 0
    PFR.check_class_map(pred.cpu().numpy(), E, L, '8-class flip tail')
    assert np.array_equal(counts.cpu().numpy(), PF.counts_table(pred.cpu().numpy(), target, 8))
    ref = PFR.ce(E, target, num_classes=8)
    assert abs(float(ce) - ref) <= 1e-5 * abs(ref)        # fp32 logits, torch ops and the existing loss kernel against fp64
    target[1, 5, 5] = 100
    flag.zero_()
    HF.sssr_tail_predict(H.dev(xs), *_tail_modules(p), target=H.dev(target), nan_flag=flag, flip=True)
    assert int(flag.item()) == 2


# ---------------------------------------------------------------------------------------------- memory, determinism
def test_no_logits_sized_allocation():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    mods = _tail_modules(PFR.tail_params(31))
    x = H.dev(PFR.tail_input(32, (4, NC, 64, 128)))
    target = H.dev(PFR.make_target(33, (2, 256, 512)))
    counts = _counts()
    HF.sssr_tail_predict(x, *mods, target=target, counts=counts, flip=True)                 # library load, allocator warm-up
    torch.cuda.synchronize()
    for kw in ({}, {'target': target, 'counts': counts}):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = HF.sssr_tail_predict(x, *mods, flip=True, **kw)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        assert rise < 2 * 256 * 512 * 4, rise                 # N = 2 class maps of 128 KiB each; one view's logits would be 19.9 MB
        del out


def test_run_to_run_bit_identical():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = PFR.TAIL_FIXTURES[5]
    p, xs, _, _ = PFR.tail_fixture(f)
    mods, x = _tail_modules(p), H.dev(xs)
    target = H.dev(PFR.make_target(43, (f[2], 4 * f[3], 4 * f[4])))
    runs = []
    for _ in range(2):
        counts = _counts()
        pred, ce = HF.sssr_tail_predict(x, *mods, target=target, counts=counts, flip=True)
        runs.append((pred.cpu().numpy(), counts.cpu().numpy(), ce.cpu().numpy().tobytes()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


# ---------------------------------------------------------------------------------------------- the model, the compiled path and the commands
@pytest.fixture(scope='module')
def model():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    torch.manual_seed(1234)
    m = DSRL(3, CS)
    return m.to(H.DEV).to(memory_format=torch.channels_last).eval()


def _image_batch(seed, n, hw=(64, 128)):
    H = _helpers()
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, 3) + tuple(hw), generator=g).to(H.DEV).contiguous(memory_format=torch.channels_last)


def _host(out):
    pred, counts, ce = out
    return (pred.cpu().numpy().copy(), None if counts is None else counts.cpu().numpy().copy(), None if ce is None else ce.cpu().numpy().tobytes())


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])) and a[2] == b[2])


def test_model_predict_flip_and_state(model):
    from dualsuperreslearningforsemseg_amd import functional as HF
    x = _image_batch(1, 2)
    both = torch.cat([x, x.flip(3)]).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        before = model(x)
        scores = _unfused_scores(model(both)[0])
    pred, counts, ce = model.predict(x, flip=True)
    assert counts is None and ce is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (2, 128, 256) and not pred.requires_grad
    with torch.no_grad():
        after = model(x)
    for a, b in zip(before, after):
        assert torch.equal(a, b)                                # no state leaks from predict into forward
    agree = (torch.argmax(scores, dim=1) == pred).float().mean().item()
    vs_plain = (model.predict(x)[0] == pred).float().mean().item()
    print(f'predict(flip=True) agrees with the unfused composition at {100 * agree:.3f} % of the pixels, with the single view at {100 * vs_plain:.3f} %')
    assert agree > 0.99, agree
    target = torch.from_numpy(PFR.make_target(2, (2, 128, 256))).to(x.device)
    pred2, counts, ce = model.predict(x, target, flip=True)
    assert torch.equal(pred, pred2) and counts.dtype == torch.int64 and not ce.requires_grad
    assert np.array_equal(counts.cpu().numpy(), PF.counts_table(pred.cpu().numpy(), target.cpu().numpy()))
    print(f'loss {float(ce):.9f}, unfused composition {_unfused_ce(scores, target):.9f}')       # held to the fp64 model in the benchmark test below
    xn = x.clone()
    xn[1, 2, 10, 20] = float('nan')
    with pytest.raises(HF.DsrlHipError, match='NaN'):
        model.predict(xn, flip=True)


def test_compiled_flip_is_bit_identical_and_has_its_own_graph_key(model):
    x = _image_batch(1, 2)
    target = torch.from_numpy(PFR.make_target(2, (2, 128, 256))).to(x.device)
    want_flip, want_plain = _host(model.predict(x, target, flip=True)), _host(model.predict(x, target))
    assert not np.array_equal(want_flip[0], want_plain[0]) or want_flip[2] != want_plain[2]
    cp = model.compile_predict()
    try:
        assert cp.MAX_GRAPHS == 4
        for call in range(cp.GRAPH_WARMUP + 2):             # the frozen eager calls, the capture, a further replay; plain calls in between
            assert _same(_host(cp(x, target, flip=True)), want_flip), f'flip call {call}'
            assert _same(_host(cp(x, target)), want_plain), f'plain call {call}'
        assert cp.num_graphs == 2 and cp.replays == 4
        assert cp._key(x, target, True) in cp._graphs and cp._key(x, target) in cp._graphs and cp._key(x, target, True) != cp._key(x, target)
        assert _same(_host(cp(x, target, flip=True)), want_flip) and _same(_host(cp(x, target)), want_plain)
    finally:
        cp.release()


def test_benchmark_and_test_commands_with_flip(model, tmp_path):
    H = _helpers()
    from PIL import Image
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.metrices import Accuracy, AverageMeter, mIoU
    from oracle.torch_cpu_model import TorchCpuDSRL
    weights = str(tmp_path / 'final.weights')
    torch.save({'model_state_dict': model.state_dict()}, weights)
    batches = [((_image_batch(10 + i, n), None), (torch.from_numpy(PFR.make_target(20 + i, (n, 128, 256))).to(H.DEV), None)) for i, n in enumerate((2, 2, 1))]
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'), 'loader_factory': lambda *a: batches}
    out_dir = str(tmp_path / 'out')
    result = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=out_dir, flip=True)
    m, a = mIoU(NC, CS.IGNORE_CLASS_LABEL), Accuracy(NC, CS.IGNORE_CLASS_LABEL)
    ce_ref, ce_unfused = AverageMeter(), AverageMeter()
    cpu = TorchCpuDSRL(stage=1).double().eval()
    cpu.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu() for k, v in model.state_dict().items()}, strict=False)
    for (img, _), (target, _) in batches:
        pred, _, _ = model.predict(img, flip=True)
        m.update(pred, target, target != CS.IGNORE_CLASS_LABEL); a.update(pred, target, target != CS.IGNORE_CLASS_LABEL)
        both = torch.cat([img, img.flip(3)]).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ce_unfused.update(_unfused_ce(_unfused_scores(model(both)[0]), target, CS.IGNORE_CLASS_LABEL), 2)
            L = cpu(both.detach().cpu().double().contiguous())[0].numpy()
        ce_ref.update(PFR.ce(PFR.ensemble_of_views(L), target.cpu().numpy(), CS.IGNORE_CLASS_LABEL), 2)
    assert abs(result['mIoU'] - m()) < 1e-9 and abs(result['accuracy'] - a()) < 1e-9, (result, m(), a())
    e_unfused, e_fused = abs(ce_unfused() - ce_ref()), abs(result['CE'] - ce_ref())
    budget = max(4 * e_unfused, 1e-6 * abs(ce_ref()))
    # measured on the MI355X when this test first passed: CE ref 3.042781800, unfused and fused error both 4.95e-8 (budget 3.0e-6)
    print(f'benchmark(flip=True): {result}; CE ref {ce_ref():.9f}, unfused error {e_unfused:.3e}, fused error {e_fused:.3e}, budget {budget:.3e}')
    assert e_fused <= budget, (e_fused, budget)
    text = open(os.path.join(out_dir, 'benchmark.txt')).read()
    assert 'flip' in text and 'mIoU %: {:.2f}\n'.format(result['mIoU']) in text
    # without the option the file does not mention it, and the figures are the single view's
    plain = benchmark(weights, dataset, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=out_dir)
    assert 'flip' not in open(os.path.join(out_dir, 'benchmark.txt')).read() and plain != result
    # the test command writes its PNGs
    img_dir = tmp_path / 'images'
    img_dir.mkdir()
    rs = np.random.RandomState(5)
    for name, (h, w) in (('b_second.png', (90, 160)), ('a_first.png', (120, 200))):
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), mode='RGB').save(str(img_dir / name))
    vis_dir = str(tmp_path / 'vis')
    files = test_command(None, str(img_dir), None, vis_dir, weights, 'gpu', False, model_input_size=(64, 128), flip=True)
    assert files == [os.path.join(vis_dir, 'a_first.png'), os.path.join(vis_dir, 'b_second.png')]
    palette = {tuple(v) for v in CS.CLASS_RGB_COLOR.values()}
    for f in files:
        with Image.open(f) as im:
            assert im.size == (3 * 256, 128) and im.mode == 'RGB'
            middle = np.array(im)[:, 256:512].reshape(-1, 3)
        assert {tuple(c) for c in np.unique(middle, axis=0).tolist()} <= palette

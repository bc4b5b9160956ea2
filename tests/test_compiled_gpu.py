"""GPU checks of compiled inference (inference.FrozenOperands, inference.CompiledPredictor, DSRL.compile_predict), the device visualisation panel
(dsrl_class_map_visualize) and the test / benchmark commands on a compiled model file.  The reference for the predictor is eager `DSRL.predict` on the
unfrozen model, held to EXACTLY: class maps and counters equal, the loss equal byte for byte (eager predict is pinned to the fp64 oracle by
test_predict_gpu.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NC = 19
IGNORE = 255
# (generator seed, shape): two batches of one shape, a smaller batch, another image size - three shapes, i.e. three graph keys per (with target, arithmetic)
INPUTS = ((1, (2, 3, 64, 128)), (10, (2, 3, 64, 128)), (11, (1, 3, 64, 128)), (3, (1, 3, 96, 160)))
FIFTH = (4, (3, 3, 64, 128))


def _image(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)


def _target(seed, shape, share=0.1):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, NC, shape).astype(np.uint8)
    t[rs.uniform(size=shape) < share] = IGNORE
    return torch.from_numpy(t).to(DEV)


def _batch(seed, shape, with_target):
    n, _, h, w = shape
    return _image(seed, shape), (_target(100 + seed, (n, 2 * h, 2 * w)) if with_target else None)


def _host(out):
    pred, counts, ce = out
    return (pred.cpu().numpy().copy(), None if counts is None else counts.cpu().numpy().copy(), None if ce is None else ce.cpu().numpy().tobytes())


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])) and a[2] == b[2])


def _describe(a, b):
    return (f'class map differs at {int((a[0] != b[0]).sum())} of {a[0].size} pixels, counts equal: {a[1] is None or np.array_equal(a[1], b[1])}, '
            f'ce bytes {None if a[2] is None else np.frombuffer(a[2], np.float32)} vs {None if b[2] is None else np.frombuffer(b[2], np.float32)}')


@pytest.fixture(scope='module')
def model():
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    torch.manual_seed(1234)
    return DSRL(3, CS).to(DEV).to(memory_format=torch.channels_last).eval()


@pytest.fixture(autouse=True)
def _restore_precision():
    from dualsuperreslearningforsemseg_amd import functional as HF
    yield
    HF.set_conv_precision(None)


# ---------------------------------------------------------------------------------------------- 1. bit identity with the parent's path
@pytest.mark.parametrize('precision', ['f16x3', 'f16x1'])
def test_bit_identity_with_eager_predict(model, precision):
    """Eager predict on the unfrozen model first, twice (the baseline: it must be bit-identical run to run, or nothing here can be judged); then for
    every input, with and without target: (a) the frozen eager path (the predictor's two warm-up calls per key) and (b) the graph replay, from the
    first replay on, give the same class map, the same counters and the same loss bytes."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    HF.set_conv_precision(precision)
    eager = {}
    for with_target in (False, True):
        for seed, shape in INPUTS:
            x, tgt = _batch(seed, shape, with_target)
            first, second = _host(model.predict(x, tgt)), _host(model.predict(x, tgt))
            if not _same(first, second):
                pytest.fail(f'FINDING ABOUT THE PARENT: eager DSRL.predict is not bit-identical run to run ({precision}, seed {seed}, target {with_target}): '
                            + _describe(first, second))
            eager[(seed, with_target)] = first
    for with_target in (False, True):
        cp = model.compile_predict()
        try:
            for seed, shape in INPUTS:
                x, tgt = _batch(seed, shape, with_target)
                want = eager[(seed, with_target)]
                graphs_before = cp.num_graphs
                known = cp._key(x, tgt) in cp._graphs
                for call in range(4):
                    replays = cp.replays
                    got = _host(cp(x, tgt))
                    replayed = cp.replays == replays + 1
                    assert replayed == (known or call >= cp.GRAPH_WARMUP), (seed, call, replayed)      # two frozen eager calls, then the capture and replays
                    assert _same(got, want), f'{precision}, seed {seed}, target {with_target}, call {call} ({"replay" if replayed else "frozen eager"}): ' + _describe(got, want)
                assert cp.num_graphs == graphs_before + (0 if known else 1)
            assert cp.num_graphs == 3 and cp.use_graph
        finally:
            cp.release()


# ---------------------------------------------------------------------------------------------- 2. no state between replays
def test_no_state_between_replays(model):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    (x1, t1), (x10, t10) = _batch(1, INPUTS[0][1], True), _batch(10, INPUTS[1][1], True)
    want1, want10 = _host(model.predict(x1, t1)), _host(model.predict(x10, t10))
    cp = model.compile_predict()
    try:
        for _ in range(cp.GRAPH_WARMUP):
            cp(x1, t1)
        first = _host(cp(x1, t1))
        assert cp.num_graphs == 1 and cp.replays == 1 and _same(first, want1), _describe(first, want1)
        assert _same(_host(cp(x10, t10)), want10)
        assert _same(_host(cp(x1, t1)), first)
        # an eager forward of another, unfrozen model and one training step in between: neither draws from nor zeroes the graph's records
        torch.manual_seed(99)
        other = DSRL(3, CS).to(DEV).to(memory_format=torch.channels_last).eval()
        with torch.no_grad():
            other(x10)
        other.predict(x10)
        torch.manual_seed(98)
        trained = DSRL(1, CS).to(DEV).to(memory_format=torch.channels_last).train()
        flat = FlatParams(trained)
        (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
        step = TrainStep(trained, flat, 1, 0.1, 1.0, IGNORE, graph=False)
        losses, _ = step(img, org, tgt, 0.006, 0.9, 5e-4, True)
        assert np.isfinite(losses[0])
        assert _same(_host(cp(x1, t1)), first)
        # a call whose activations are 1000 x larger leaves 1000 x larger amax records: the next replay must not take its operand scales from them
        big = _host(cp(x10 * 1000.0, t10))
        assert not np.array_equal(big[0], want10[0]) or big[2] != want10[2]
        after = _host(cp(x1, t1))
        assert _same(after, first), 'the replay after a x1000 input differs: ' + _describe(after, first)
        assert _same(_host(model.predict(x10, t10)), want10)          # the eager path beside it is not disturbed either (frozen operands attached)
    finally:
        cp.release()


# ---------------------------------------------------------------------------------------------- 3. no host pacing
def test_replays_do_not_synchronise_or_allocate(model):
    """20 replays with a caller-owned flag inside torch.cuda.set_sync_debug_mode('error') (this torch raises on every synchronising call there), and the
    allocation is the same before and after.  Which check ran is printed."""
    x, tgt = _batch(1, INPUTS[0][1], True)
    flag = torch.zeros((), dtype=torch.int32, device=DEV)
    cp = model.compile_predict()
    try:
        for _ in range(cp.GRAPH_WARMUP + 2):
            out = cp(x, tgt, nan_flag=flag)
        del out
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        sync_checked = hasattr(torch.cuda, 'set_sync_debug_mode')
        if sync_checked:
            torch.cuda.set_sync_debug_mode('error')
        try:
            for _ in range(20):
                out = cp(x, tgt, nan_flag=flag)
                del out
        finally:
            if sync_checked:
                torch.cuda.set_sync_debug_mode('default')
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert cp.replays >= 22 and int(flag.item()) == 0
        print('no host pacing: ' + ("sync_debug_mode('error') and the allocation check" if sync_checked else 'the allocation check alone'))
        # copy=False hands out the static tensors themselves
        a = cp(x, tgt, nan_flag=flag, copy=False)
        b = cp(x, tgt, nan_flag=flag, copy=False)
        assert a[0].data_ptr() == b[0].data_ptr() and a[1].data_ptr() == b[1].data_ptr()
    finally:
        cp.release()


# ---------------------------------------------------------------------------------------------- 4. staleness
def test_stale_operands_raise_and_release_restores(model):
    from dualsuperreslearningforsemseg_amd import functional as HF
    x, tgt = _batch(1, INPUTS[0][1], True)
    want = _host(model.predict(x, tgt))
    with torch.no_grad():
        forward_before = [o.clone() for o in model(x)]
    cp = model.compile_predict(batch_size=2, input_size=(64, 128))
    assert cp.num_graphs == 1 and cp.compile_seconds > 0 and cp.frozen.nbytes() > 0
    bias = model.SSSR_decoder['cls_conv'].bias
    saved = bias.detach().clone()
    try:
        assert _same(_host(cp(x)), _host(model.predict(x)))
        bias.data.add_(1)                       # moves neither the address nor the version counter: the device-side fingerprint finds it
        with pytest.raises(HF.DsrlHipError, match='compile_predict'):
            cp(x)
        bias.data.copy_(saved)
        assert _same(_host(cp(x, tgt)), want)
        model.train()
        with pytest.raises(HF.DsrlHipError, match='compile_predict'):
            cp(x)
        model.eval()
        assert _same(_host(cp(x, tgt)), want)
        # a backward pass through a frozen filter fails loudly
        with pytest.raises(HF.DsrlHipError, match='inference-only'):
            cp.frozen.claim(model.SSSR_decoder['cls_conv'].weight)
        with torch.no_grad():
            bias.add_(1)                        # an in-place write torch knows about: refused on the host, before anything is launched, for good
        with pytest.raises(HF.DsrlHipError, match='compile_predict'):
            cp(x, nan_flag=torch.zeros((), dtype=torch.int32, device=DEV))
        with torch.no_grad():
            bias.copy_(saved)
        with pytest.raises(HF.DsrlHipError, match='compile_predict'):
            cp(x)
    finally:
        model.eval()
        with torch.no_grad():
            bias.copy_(saved)
        cp.release()
    assert not hasattr(model.SSSR_decoder['cls_conv'].weight, '_dsrl_arena') and not hasattr(model.SSSR_decoder['cat_conv'][1].running_var, '_dsrl_invstd')
    assert not any(hasattr(p, '_dsrl_operands') for p in model.parameters())
    assert _same(_host(model.predict(x, tgt)), want)
    with torch.no_grad():
        for a, b in zip(forward_before, model(x)):
            assert torch.equal(a, b)
    with pytest.raises(HF.DsrlHipError, match='released'):
        cp(x)


# ---------------------------------------------------------------------------------------------- 5. the fifth key
def test_fifth_key_runs_eagerly(model):
    cp = model.compile_predict()
    try:
        keys = [_batch(seed, shape, wt) for seed, shape in INPUTS[1:] for wt in (False, True)][:4]
        for x, tgt in keys:
            for _ in range(cp.GRAPH_WARMUP + 1):
                cp(x, tgt)
        assert cp.num_graphs == 4
        x5, t5 = _batch(*FIFTH, True)
        want = _host(model.predict(x5, t5))
        replays = cp.replays
        for _ in range(cp.GRAPH_WARMUP + 2):
            assert _same(_host(cp(x5, t5)), want)
        assert cp.num_graphs == 4 and cp.replays == replays
    finally:
        cp.release()


# ---------------------------------------------------------------------------------------------- 6. the visualisation panel
def _exactness_case(N, H, W, seed):
    """image bytes 0..255 along x, classes 0..255 along y (both shifted per image and channel so that every (input byte, colour byte) pair occurs when
    H, W >= 256), palette[i] = (i, 255 - i, 7 i mod 256): every channel value 0..255 somewhere"""
    rs = np.random.RandomState(seed)
    xs, ys = np.arange(W)[None, None, :, None], np.arange(H)[None, :, None, None]
    rgb = ((xs + 85 * np.arange(3)[None, None, None, :] + 31 * np.arange(N)[:, None, None, None] + 0 * ys) % 256).astype(np.uint8)
    classes = ((np.arange(H)[None, :, None] + 57 * np.arange(N)[:, None, None] + 0 * np.arange(W)[None, None, :]) % 256).astype(np.uint8)
    mask = np.where(rs.uniform(size=classes.shape) < 0.3, IGNORE, rs.randint(0, 200, classes.shape)).astype(np.uint8)
    palette = {i: (i, 255 - i, (7 * i) % 256) for i in range(256)}
    return rgb, classes, mask, palette


@pytest.mark.parametrize('N,H,W', [(1, 256, 256), (3, 256, 272), (3, 37, 251), (2, 1, 260), (1, 1, 5), (2, 19, 64)])
def test_visualization_panel_is_byte_exact(N, H, W):
    """The device panel against utils.make_input_output_visualization transposed to HWC, exactly: all 65536 (input byte, colour byte) pairs in the
    256-wide cases, N = 3, odd W (the byte path) and W % 4 == 0 but not % 16 (the 32-bit path), H = 1; then with a mask, against the host sequence the test
    command used (pred_map[target == IGNORE] = IGNORE)."""
    from dualsuperreslearningforsemseg_amd.utils import make_input_output_visualization, make_input_output_visualization_device
    rgb, classes, mask, palette = _exactness_case(N, H, W, 5)
    if H >= 256 and W >= 256:
        for c in range(3):
            col = np.array([palette[i][c] for i in range(256)], dtype=np.int64)[classes[0]]
            assert len(set((rgb[0, :, :, c].astype(np.int64) * 256 + col).reshape(-1).tolist())) == 65536, c
    d = lambda a: torch.from_numpy(a).to(DEV)         # noqa: E731
    for b in (0.4, 0.73):
        got = make_input_output_visualization_device(d(rgb), d(classes), palette, blend_factor=b)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, 3 * W, 3) and got.is_cuda
        got = got.cpu().numpy()
        for n in range(N):
            want = make_input_output_visualization(rgb[n].transpose(2, 0, 1), classes[n], palette, blend_factor=b).transpose(1, 2, 0)
            assert np.array_equal(got[n], want), (n, b, int((got[n] != want).sum()))
    got = make_input_output_visualization_device(d(rgb), d(classes), palette, mask=d(mask), ignore_index=IGNORE).cpu().numpy()
    for n in range(N):
        masked = classes[n].copy()
        masked[mask[n] == IGNORE] = IGNORE
        want = make_input_output_visualization(rgb[n].transpose(2, 0, 1), masked, palette).transpose(1, 2, 0)
        assert np.array_equal(got[n], want), n
    # a palette that names few labels: the others are black; an unaligned view takes the byte path and gives the same bytes
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    got = make_input_output_visualization_device(d(rgb), d(classes), CS.CLASS_RGB_COLOR).cpu().numpy()
    want = make_input_output_visualization(rgb[0].transpose(2, 0, 1), classes[0], CS.CLASS_RGB_COLOR).transpose(1, 2, 0)
    assert np.array_equal(got[0], want)
    shifted = torch.zeros(classes.size + 1, dtype=torch.uint8, device=DEV)[1:].view(classes.shape)
    shifted.copy_(d(classes))
    assert np.array_equal(make_input_output_visualization_device(d(rgb), shifted, CS.CLASS_RGB_COLOR).cpu().numpy(), got)


# ---------------------------------------------------------------------------------------------- 7. the commands
def test_commands_on_a_compiled_file(model, tmp_path):
    from PIL import Image
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.compile_model import compile_model
    from dualsuperreslearningforsemseg_amd.command_handlers.prune_weights import prune_weights
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.utils import make_input_output_visualization
    weights, pruned, compiled = str(tmp_path / 'final.weights'), str(tmp_path / 'pruned.weights'), str(tmp_path / 'final.compiled')
    torch.save({'model_state_dict': model.state_dict()}, weights)
    prune_weights(weights, pruned, {'settings': CS})
    compile_model(pruned, compiled, {'settings': CS}, batch_size=1, model_input_size=(64, 128))
    precision = HF.get_conv_precision()
    # the two generated images of the existing end-to-end test
    img_dir = tmp_path / 'images'
    img_dir.mkdir()
    rs = np.random.RandomState(5)
    for name, (h, w) in (('b_second.png', (90, 160)), ('a_first.png', (120, 200))):
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8), mode='RGB').save(str(img_dir / name))
    plain = test_command(None, str(img_dir), None, str(tmp_path / 'vis_plain'), weights, 'gpu', False, model_input_size=(64, 128))
    comp = test_command(None, str(img_dir), None, str(tmp_path / 'vis_compiled'), compiled, 'gpu', True, model_input_size=(64, 128))
    assert [os.path.basename(f) for f in comp] == [os.path.basename(f) for f in plain] == ['a_first.png', 'b_second.png']
    assert HF.get_conv_precision() == precision          # the arithmetic the file selected is gone with the predictor
    for a, b in zip(plain, comp):
        with Image.open(a) as ia, Image.open(b) as ib:
            pa, pb = np.array(ia), np.array(ib)
        assert pa.shape == (128, 3 * 256, 3) and np.array_equal(pa, pb), (a, int((pa != pb).sum()))
    # ... and the pixels are what the host function gives for the class map of DSRL.predict (the parent's panel)
    from dualsuperreslearningforsemseg_amd.models.transforms import DeviceBatchPreparation
    from PIL import ImageOps
    prepare = DeviceBatchPreparation(CS.LABEL_MAPPING_DICT, CS.MEAN, CS.STD, (64, 128), CS.IGNORE_CLASS_LABEL)
    with Image.open(str(img_dir / 'a_first.png')) as opened:
        rgb = np.array(ImageOps.exif_transpose(opened).convert('RGB').resize((256, 128), resample=Image.BILINEAR), dtype=np.uint8)
    (inp, _), _ = prepare(torch.from_numpy(rgb).unsqueeze(0).to(DEV))
    pred, _, _ = model.predict(inp)
    want = make_input_output_visualization(rgb.transpose(2, 0, 1), pred[0].cpu().numpy(), CS.CLASS_RGB_COLOR).transpose(1, 2, 0)
    with Image.open(plain[0]) as im:
        assert np.array_equal(np.array(im), want)
    # dataset mode: target above prediction, against the host sequence of the parent
    batches = [((_image(10 + i, (n, 3, 64, 128)), None), (_target(20 + i, (n, 128, 256)), None)) for i, n in enumerate((2, 2, 1))]
    ds_loader = lambda *a: [((b[0][0][:1], HF.upsample_bilinear_ac(b[0][0][:1], (128, 256))), (b[1][0][:1], None)) for b in batches]      # noqa: E731
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing')}
    outs = []
    for tag, wfile, flag in (('plain', weights, False), ('compiled', compiled, True)):
        files = test_command(None, None, dict(dataset, starting_index=1, max_images=1, loader_factory=ds_loader), str(tmp_path / ('ds_' + tag)), wfile, 'gpu', flag,
                             model_input_size=(64, 128))
        assert [os.path.basename(f) for f in files] == ['1.png']
        with Image.open(files[0]) as im:
            outs.append(np.array(im))
    assert outs[0].shape == (2 * 128, 3 * 256, 3) and np.array_equal(outs[0], outs[1])
    (inp, org), (tgt, _) = ds_loader()[1]
    mean, std = np.array(CS.MEAN).reshape(3, 1, 1), np.array(CS.STD).reshape(3, 1, 1)
    shown = np.clip((std * org[0].float().cpu().numpy() + mean) * 255., 0., 255.).astype(np.uint8)
    target_map, pred_map = tgt[0].cpu().numpy(), model.predict(inp)[0][0].cpu().numpy()
    pred_map[target_map == CS.IGNORE_CLASS_LABEL] = CS.IGNORE_CLASS_LABEL
    want = np.concatenate((make_input_output_visualization(shown, target_map, CS.CLASS_RGB_COLOR),
                           make_input_output_visualization(shown, pred_map, CS.CLASS_RGB_COLOR)), axis=1).transpose(1, 2, 0)
    assert np.array_equal(outs[0], want), int((outs[0] != want).sum())
    # benchmark: exactly the same dict (the full batch and the last short one are two graph keys)
    bench_ds = dict(dataset, loader_factory=lambda split, batch_size, device, rank, world: batches)
    r_plain = benchmark(weights, bench_ds, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=str(tmp_path / 'b_plain'))
    r_comp = benchmark(compiled, bench_ds, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=str(tmp_path / 'b_comp'), compiled_model=True)
    assert r_comp == r_plain, (r_comp, r_plain)
    assert HF.get_conv_precision() == precision
    # mixing up the two kinds of file raises, naming the other way
    with pytest.raises(RuntimeError, match='compile_model'):
        test_command(None, str(img_dir), None, str(tmp_path / 'x'), weights, 'gpu', True, model_input_size=(64, 128))
    with pytest.raises(RuntimeError, match='compiled_model=True'):
        test_command(None, str(img_dir), None, str(tmp_path / 'x'), compiled, 'gpu', False, model_input_size=(64, 128))
    with pytest.raises(RuntimeError, match='compile_model'):
        benchmark(weights, bench_ds, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=str(tmp_path / 'x'), compiled_model=True)
    with pytest.raises(RuntimeError, match='compiled_model=True'):
        benchmark(compiled, bench_ds, 'gpu', 0, 2, model_input_size=(64, 128), output_dir=str(tmp_path / 'x'))


# ---------------------------------------------------------------------------------------------- 8. one preparer for training and inference
@pytest.mark.parametrize('precision', ['f16x3', 'f16x1'])
def test_frozen_operands_equal_the_training_steps(precision):
    """What inference.FrozenOperands prepares for an eval head and what ddp.FlatParams leaves after zero_grad() + refresh_transposed_filters() on a
    train-mode twin with the same weights come from the same kernels on the same values through tables built by the same code: the magnitude of every
    amax record (the maximum over its 16 shards; also max |w| itself), the forward split form and the forward planes are byte-equal, filter by filter.
    planes_mode 'all' so that both sides hold planes for the same filters (the training side otherwise waits for its convs to ask)."""
    import gen
    from hip_helpers import host, make_head
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    from dualsuperreslearningforsemseg_amd.filter_operands import PLANES
    from dualsuperreslearningforsemseg_amd.inference import FrozenOperands
    HF.set_conv_precision(precision)
    mode_was, HF.planes_mode = HF.planes_mode, 'all'
    frozen = None
    try:
        head, _ = make_head(gen.SMALL, 1, 77, False)
        twin, _ = make_head(gen.SMALL, 1, 77, True)
        frozen = FrozenOperands(head)
        flat = FlatParams(twin)
        flat.zero_grad()
        flat.refresh_transposed_filters()
        torch.cuda.synchronize()
        a, b = frozen._sets[precision], flat.filters
        assert a.state == b.state == PLANES and not a.transposed and b.transposed
        names_a = {id(p): k for k, p in head.named_parameters()}
        names_b = {id(p): k for k, p in twin.named_parameters()}
        ia = {names_a[id(w)]: i for i, w in enumerate(a.filters)}
        ib = {names_b[id(w)]: i for i, w in enumerate(b.filters)}
        assert set(ia) == set(ib) and len(ia) >= 8
        mag = lambda ops: ops.amax.view(-1, 16, 16)[:, :, 0].max(dim=1).values.cpu().numpy()       # noqa: E731
        ma, mb = mag(a), mag(b)
        with_planes = 0
        for k in sorted(ia):
            i, j = ia[k], ib[k]
            want = np.abs(host(a.filters[i])).max().astype(np.float32).view(np.int32)
            assert ma[i] == mb[j] == want, (k, int(ma[i]), int(mb[j]), int(want))
            assert torch.equal(a.split(i).view(torch.int32), b.split(j).view(torch.int32)), k
            assert a.split(i, True) is None and b.split(j, True) is not None, k
            pa, pb = a.planes(i), b.planes(j)
            assert (pa is None) == (pb is None), k
            if pa is not None:
                with_planes += 1
                assert torch.equal(pa, pb), k
                assert a.planes(i, True) is None and b.planes(j, True) is not None, k
        assert 1 <= with_planes < len(ia)           # the 19-class cls_conv (K = 19) has no planes on either side
    finally:
        if frozen is not None:
            frozen.release()
        HF.amax_end_step(torch.device(DEV))
        HF.wgrad_queue = None
        HF.planes_mode = mode_was

"""Times the training augmentations and the Cityscapes loader (profiles/augment_pipeline.txt).

1. The two kernels for a batch of 8 at 1024x2048 -> 256x512 / 512x1024 with drawn parameters: HIP events, median of --reps runs after warm-up;
   dsrl_prepare_batch on the same batch for comparison.
2. TrainStep images/s fed by CityscapesLoader (synthetic full-size uint8 cache written to --cache, augmentation on the side stream) against
   SyntheticCityscapes device batches, in the same process, alternating A/B/A/B.

With --color-jitter B C S H (JointColorJitter's arguments; the reference's commented-out values are 0.4 0.4 0.4 0.4) the colour-jitter kernels are
timed too and the loader runs once without and once with jitter in every round (profiles/augment_colour_jitter.txt).

Usage: python tools/augment_bench.py [--reps 100] [--steps 30] [--images 48] [--cache DIR] [--color-jitter 0.4 0.4 0.4 0.4]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_median(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def write_cache(path, n, H, W):
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    if L.has_cache(path):
        return
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(0)
    ids = np.array(sorted(k for k in cs.LABEL_MAPPING_DICT if 0 <= k < 256), dtype=np.uint8)
    index = {'version': L.CACHE_VERSION, 'splits': {}}
    rgb = np.lib.format.open_memmap(os.path.join(path, 'train_rgb.npy'), mode='w+', dtype=np.uint8, shape=(n, H, W, 3))
    lab = np.lib.format.open_memmap(os.path.join(path, 'train_labels.npy'), mode='w+', dtype=np.uint8, shape=(n, H, W))
    for i in range(n):
        # smooth image content (a real photo compresses the blur / resample paths no differently, but keeps the values plausible)
        base = rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8)
        rgb[i] = np.repeat(np.repeat(base, 16, 0), 16, 1)
        lab[i] = np.repeat(np.repeat(ids[rng.integers(0, len(ids), (H // 32, W // 32))], 32, 0), 32, 1)
    rgb.flush(); lab.flush()
    del rgb, lab
    index['splits']['train'] = {'count': n, 'height': H, 'width': W, 'images': [str(i) for i in range(n)], 'labels': [str(i) for i in range(n)]}
    with open(os.path.join(path, L.INDEX), 'w') as f:
        json.dump(index, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--images', type=int, default=48)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--cache', default=None)
    ap.add_argument('--color-jitter', type=float, nargs=4, default=None, metavar=('B', 'C', 'S', 'H'))
    args = ap.parse_args()
    import dualsuperreslearningforsemseg_amd as D
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import loader as L
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    from dualsuperreslearningforsemseg_amd.models.transforms import DeviceBatchPreparation, DeviceJointAugmentation
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    B, Hs, Ws, size = args.batch, 1024, 2048, (256, 512)

    # ---------------------------------------------------------------- 1. the kernels
    rng = np.random.default_rng(1)
    rgb = torch.from_numpy(rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)).to(dev)
    lab = torch.from_numpy(rng.integers(0, 34, (B, Hs, Ws), dtype=np.uint8)).to(dev)
    aug = DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL, seed=settings.RANDOM_SEED)
    prep = DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL)
    ps = aug.draw(0, range(B), (Hs, Ws))
    table = aug.table(ps, Ws, Hs, dev)
    g_rgb, g_lab = aug.geometry(rgb, lab, table)
    res = {}
    res['geometry_ms'] = event_median(lambda: aug.geometry(rgb, lab, table), args.reps)
    res['prepare_augmented_ms'] = event_median(lambda: aug.prepare(g_rgb, g_lab, table), args.reps)
    res['prepare_batch_ms'] = event_median(lambda: prep(g_rgb, g_lab), args.reps)
    res['augment_call_ms (table upload + both kernels)'] = event_median(lambda: aug(rgb, lab, table), args.reps)
    augj = None
    if args.color_jitter is not None:
        from dualsuperreslearningforsemseg_amd.models.transforms.augment import jitter_offset
        augj = DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, size, cs.IGNORE_CLASS_LABEL, seed=settings.RANDOM_SEED,
                                       color_jitter=tuple(args.color_jitter))
        psj = augj.draw(0, range(B), (Hs, Ws))
        assert [p[:7] for p in psj] == [p[:7] for p in ps]
        tablej = augj.table(psj, Ws, Hs, dev)
        rows = tablej.data_ptr() + jitter_offset(B, Ws, Hs)
        means = augj.jitter_means(g_rgb, rows)
        res['colour_jitter_means_ms'] = event_median(lambda: augj.jitter_means(g_rgb, rows), args.reps)
        res['prepare_jittered_ms (means given)'] = event_median(lambda: augj._prepare(g_rgb, g_lab, tablej, means), args.reps)
        res['augment_call_ms, jitter (geometry + means + jittered)'] = event_median(lambda: augj(rgb, lab, tablej), args.reps)
    t0 = time.perf_counter()
    for e in range(20):
        aug.draw(e, range(B), (Hs, Ws))
    res['host_draw_ms_per_batch'] = (time.perf_counter() - t0) / 20 * 1e3
    from dualsuperreslearningforsemseg_amd.models.transforms.augment import pack_table
    t0 = time.perf_counter()
    for _ in range(20):
        pack_table(ps, Ws, Hs)
    res['host_pack_ms_per_batch'] = (time.perf_counter() - t0) / 20 * 1e3
    flags = {k: sum(getattr(p, k) for p in ps) for k in ('flip', 'blur', 'gray')}
    if augj is not None:
        print(f'colour jitter {augj.color_jitter}; contrast enabled in {sum(p.jitter.contrast is not None for p in psj)} of {B} samples')
    print(f'kernels, B={B}, {Hs}x{Ws} -> {size[0]}x{size[1]} / {2 * size[0]}x{2 * size[1]} (median, min of {args.reps} runs, HIP events; drawn flags {flags}):')
    for k, v in res.items():
        print(f'  {k:48s} ' + (f'{v[0]:.4f} ms (min {v[1]:.4f})' if isinstance(v, tuple) else f'{v:.4f} ms'))
    del rgb, lab, g_rgb, g_lab
    torch.cuda.synchronize()

    # ---------------------------------------------------------------- 2. TrainStep fed by the loader vs synthetic batches
    tmp = None
    cache = args.cache
    if cache is None:
        tmp = tempfile.TemporaryDirectory()
        cache = os.path.join(tmp.name, 'cache')
    t0 = time.perf_counter()
    write_cache(cache, args.images, Hs, Ws)
    print(f'synthetic cache of {args.images} x {Hs}x{Ws} written in {time.perf_counter() - t0:.1f} s')
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    step = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL)
    synth = SyntheticCityscapes(B, size, dev, length=args.steps)
    loader = L.CityscapesLoader(L.CityscapesCache(cache, 'train'), B, dev, aug, train=True, seed=settings.RANDOM_SEED)
    loaders = {'loader': loader}
    if augj is not None:
        loaders['loader+jitter'] = L.CityscapesLoader(L.CityscapesCache(cache, 'train'), B, dev, augj, train=True, seed=settings.RANDOM_SEED)
    hp = (0.006, 0.9, 5e-4)

    def run(it, n):
        k = 0
        t0 = time.perf_counter()
        for (img, org), (tgt, _) in it:
            step.enqueue(img, org, tgt, *hp, True)
            while step.pending() > 1:
                step.collect()
            k += 1
            if k == n:
                break
        while step.pending():
            step.collect()
        torch.cuda.synchronize()
        return k, time.perf_counter() - t0

    def loader_batches(ld):
        while True:
            for b in ld:
                yield b

    run(synth, 6)
    for ld in loaders.values():
        warm = loader_batches(ld)
        run(warm, 6)
        warm.close()
    rates = {name: [] for name in ('synthetic', *loaders)}
    for r in range(args.rounds):
        for name in rates:
            it = iter(synth) if name == 'synthetic' else loader_batches(loaders[name])
            k, el = run(it, args.steps)
            if name != 'synthetic':
                it.close()               # stops the loader's reader thread before the next run starts one
            rates[name].append(k * B / el)
    s, l_ = statistics.median(rates['synthetic']), statistics.median(rates['loader'])
    print(f'TrainStep stage 3, batch {B}, {size[0]}x{size[1]} input, {args.steps} steps per run, {args.rounds} alternating rounds:')
    print(f'  SyntheticCityscapes   {s:8.1f} img/s   runs {[round(v, 1) for v in rates["synthetic"]]}')
    print(f'  CityscapesLoader      {l_:8.1f} img/s   runs {[round(v, 1) for v in rates["loader"]]}')
    print(f'  loader / synthetic    {100 * l_ / s:8.1f} %')
    if augj is not None:
        j_ = statistics.median(rates['loader+jitter'])
        print(f'  CityscapesLoader, colour jitter {j_:8.1f} img/s   runs {[round(v, 1) for v in rates["loader+jitter"]]}')
        print(f'  loader+jitter / synthetic {100 * j_ / s:8.1f} %')
    step.release()
    if tmp is not None:
        tmp.cleanup()


if __name__ == '__main__':
    main()

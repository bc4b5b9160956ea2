#!/usr/bin/env python3
"""Compiled inference, A/B/C in one process: A = the parent's path (DSRL.predict on an unfrozen model), B = the same call on frozen operands
(inference.FrozenOperands attached: eager launches), C = inference.CompiledPredictor (hipGraph replay).  Caller-owned nan_flag on every side: nothing
reads the device back inside a window.  Alternating windows of >= --window seconds per side, --rounds alternations A B C A B C .., device events around
every window, after a warm-up of all sides at that shape (which also captures C's graph).  Stage-1 model, random weights, eval.

Below the table: library launches per call of A and B (every call through the ctypes binding counted; torch's own fills and copies are not) and what C
enqueues instead, the time compile_predict() took, the bytes the frozen operands hold, and the `test` command over 16 generated PNGs, plain weights
against a compiled model file (whole command, model load and capture included, per image).

    python tools/compiled_predict_bench.py [--out profiles/compiled_predict.txt] [--window 0.5] [--rounds 3]
"""
import argparse
import math
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dualsuperreslearningforsemseg_amd import functional as HF                        # noqa: E402
from dualsuperreslearningforsemseg_amd import inference                                # noqa: E402
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS       # noqa: E402
from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL                         # noqa: E402


def window(fn, seconds):
    """-> ms per call over one window of at least `seconds` of device work"""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(5):
        fn()
    e[1].record()
    torch.cuda.synchronize()
    n = max(5, int(math.ceil(seconds * 1e3 / max(e[0].elapsed_time(e[1]) / 5, 1e-3))))
    e[0].record()
    for _ in range(n):
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / n


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def count_launches(fn):
    """library calls that take a stream (launches) during one fn(), through the binding functional.py and inference.py use"""
    n = [0]
    real_f, real_i = HF.call, inference.call

    def counting(name, *args):
        n[0] += 1
        return real_f(name, *args)
    HF.call = inference.call = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        HF.call, inference.call = real_f, real_i
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--images', type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'compiled_predict_bench.py measures on the GPU only'
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(7)
    model_a = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
    model_b = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
    model_b.load_state_dict(model_a.state_dict())
    flag = torch.zeros((), dtype=torch.int32, device=dev)
    base = torch.cuda.memory_allocated()
    say(f'compiled inference, {torch.cuda.get_device_name(0)}, conv arithmetic {HF.get_conv_precision()}: A = DSRL.predict (unfrozen model), B = DSRL.predict on frozen '
        f'operands (eager), C = CompiledPredictor (hipGraph replay); caller-owned nan_flag')
    say(f'windows of >= {args.window} s per side, {args.rounds} alternations A B C ..; ms per call: mean [each window]; peak memory = rise of the allocation during one call')
    say()
    losses = []
    held = rose = 0
    for (N, H, W) in ((1, 256, 512), (8, 256, 512), (1, 512, 1024)):
        cp = model_b.compile_predict()          # one predictor per shape: its two keys (with and without target) stay under the cap of 4 graphs
        for with_target in (False, True):
            img = torch.randn(N, 3, H, W, device=dev).contiguous(memory_format=torch.channels_last)
            target = None
            if with_target:
                target = torch.randint(0, 19, (N, 2 * H, 2 * W), device=dev, dtype=torch.uint8)
                target[torch.rand(target.shape, device=dev) < 0.1] = 255
            a = lambda: model_a.predict(img, target, nan_flag=flag)            # noqa: E731
            b = lambda: model_b.predict(img, target, nan_flag=flag)            # noqa: E731
            c = lambda: cp(img, target, nan_flag=flag)                         # noqa: E731
            for _ in range(4):
                a(); b(); c()
            torch.cuda.synchronize()
            ra, rb, rc = a(), b(), c()
            same = all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(ra, rb, rc) if x is not None)
            del ra, rb, rc
            t = {'A': [], 'B': [], 'C': []}
            for _ in range(args.rounds):
                for k, fn in (('A', a), ('B', b), ('C', c)):
                    t[k].append(window(fn, args.window))
            m = {k: sum(v) / len(v) for k, v in t.items()}
            for k in ('B', 'C'):
                if m[k] > m['A']:
                    losses.append((k, N, H, W, with_target))
            say(f'input {H}x{W} batch {N} target={"yes" if with_target else "no "}:  ' + '   '.join(
                f'{k} {m[k]:7.3f} ms [{", ".join(f"{v:.3f}" for v in t[k])}] {N / m[k] * 1e3:8.1f} img/s' for k in ('A', 'B', 'C')) +
                f'   A/B {m["A"] / m["B"]:5.2f}  A/C {m["A"] / m["C"]:5.2f}   bit-identical: {"yes" if same else "NO"}')
            say(f'      peak memory A {peak_bytes(a) / 1e6:8.1f} MB  B {peak_bytes(b) / 1e6:8.1f} MB  C {peak_bytes(c) / 1e6:8.1f} MB (C: the copies of its static outputs)   '
                f'library launches per call A {count_launches(a)}  B {count_launches(b)}  C {count_launches(c)} + 1 hipGraphLaunch of B\'s launches')
        assert cp.num_graphs == 2, cp.num_graphs
        torch.cuda.synchronize()
        held, rose = cp.frozen.nbytes(), max(rose, torch.cuda.memory_allocated() - base)
        cp.release()
        del cp
    say()
    say(f'frozen operands hold {held / 1e6:.1f} MB (amax records, w_split, w_planes, BatchNorm 1/std, fingerprints); with the two graphs of a shape captured the allocation '
        f'stood at most {rose / 1e6:.1f} MB above the two models')
    t0 = time.perf_counter()
    cp2_model = model_a
    cp2 = cp2_model.compile_predict(batch_size=1, input_size=(256, 512))
    say(f'compile_predict(batch_size=1, input_size=(256, 512)): {time.perf_counter() - t0:.3f} s (freeze {cp2.frozen.nbytes() / 1e6:.1f} MB of operands, two eager calls, one capture)')
    own = torch.randn(1, 3, 256, 512, device=dev).contiguous(memory_format=torch.channels_last)
    for _ in range(3):
        cp2(own)
    t0 = time.perf_counter()
    for _ in range(20):
        cp2(own)
    say(f'the synchronous form (own flag: fingerprint check of the whole model + one readback): {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms per call at 256x512 batch 1')
    t0 = time.perf_counter()
    for _ in range(200):
        cp2.frozen.check()
    say(f'FrozenOperands.check() (host loop over {len(cp2.frozen._watch)} tensors): {(time.perf_counter() - t0) / 200 * 1e6:.1f} us per call')
    cp2.release()
    say('rows where B or C is slower than A: ' + (', '.join(str(r) for r in losses) if losses else 'none'))
    # the test command over generated PNGs, whole command
    import numpy as np
    from PIL import Image
    from dualsuperreslearningforsemseg_amd.command_handlers.compile_model import compile_model
    from dualsuperreslearningforsemseg_amd.command_handlers.test import test as test_command
    with tempfile.TemporaryDirectory() as d:
        rs = np.random.RandomState(5)
        os.makedirs(os.path.join(d, 'images'))
        for i in range(args.images):
            Image.fromarray(rs.randint(0, 256, (512, 1024, 3)).astype(np.uint8), mode='RGB').save(os.path.join(d, 'images', f'{i:02d}.png'))
        weights, compiled = os.path.join(d, 'final.weights'), os.path.join(d, 'final.compiled')
        torch.save({'model_state_dict': model_a.state_dict()}, weights)
        compile_model(weights, compiled, {'settings': CS})
        res = {}
        for tag, f, flag_ in (('plain weights', weights, False), ('compiled file', compiled, True), ('plain weights again', weights, False), ('compiled file again', compiled, True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            test_command(None, os.path.join(d, 'images'), None, os.path.join(d, 'out_' + tag.replace(' ', '_')), f, 'gpu', flag_)
            res[tag] = (time.perf_counter() - t0) / args.images
    say()
    say(f'test command over {args.images} generated 512x1024 PNGs, whole command (model load, and for the compiled file freeze + capture, included), seconds per image: ' +
        ', '.join(f'{k} {v:.4f}' for k, v in res.items()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Cost of the super-resolution quality metric, written to profiles/sr_quality.txt.  Every figure is measured on the device this
runs on, at 8 x 3 x 512 x 1024 (the stage-2 output of the default 256 x 512 step) and 8 x 3 x 1024 x 2048 (config 5):
  (a) the DEFAULT replayed step (bench.py --gpus 1) of this tree against the parent commit on the same box: the parent's tree with its own library
      under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again.  The step launches nothing of the metric, so the difference
      should lie inside the parent's own run-to-run spread.  Skipped (and said so) when ab/prev_tree is not there;
  (b) the two launches of dsrl_sr_quality, HIP events around back-to-back calls, alternating with
  (c) the torch composition on the same tensors: de-normalise and clamp, grouped F.conv2d with the same 11 x 11 window over the five planes
      x, y, xx, xy, yy, the formula, the mean and the PSNR.  The kernel is expected to be faster at both sizes; the ratio is recorded;
  (d) dsrl_copy2d moving as many bytes as the kernel reads (both images once: the copy reads one image and writes one), and the fraction of the
      copy's byte rate the kernel reaches.  None is prescribed;
  (e) peak device memory of both legs above the two input tensors;
  (f) the validation pass of a stage-2 run (batch 8, 256 x 512, eager as validation runs) with and without the metric, alternating.
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/sr_quality_bench.py [--steps K] [--rounds R] [--no-parent] [--no-val] [VAR=value ...]"""
import json
import os
import subprocess
import sys
import time

args = [a for a in sys.argv[1:] if '=' not in a]
for kv in sys.argv[1:]:
    if '=' in kv:
        k, v = kv.split('=', 1); os.environ[k] = v
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = int(args[args.index('--steps') + 1]) if '--steps' in args else 30
ROUNDS = int(args[args.index('--rounds') + 1]) if '--rounds' in args else 2
PREV = os.path.join(ROOT, 'ab', 'prev_tree')
dev = 'cuda:0'
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def bench_line(tree):
    """one `bench.py --gpus 1` in a fresh process in `tree` -> (ms per step, losses of the last step)"""
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(STEPS), '--warmup', '8'], cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f'bench.py in {tree} ended with {r.returncode}: {r.stderr[-400:]}')
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    return float(d['ms_per_step']), d['config']['losses_last_step']


def against_parent():
    say(f'(a) default replayed step, bench.py --gpus 1 --steps {STEPS} --warmup 8, ms per step: the parent commit in its own tree with its own library,')
    say('    this tree; each round parent, this, parent again:')
    if '--no-parent' in args or not os.path.isfile(os.path.join(PREV, 'bench.py')):
        say('    NOT MEASURED: no parent tree under ab/prev_tree')
        return
    parent, this, losses = [], [], set()
    for r in range(ROUNDS):
        a, la = bench_line(PREV)
        b, lb = bench_line(ROOT)
        c, lc = bench_line(PREV)
        parent += [a, c]; this.append(b)
        losses |= {json.dumps(x) for x in (la, lb, lc)}
        say(f'    round {r + 1}: parent {a:.3f}  this {b:.3f}  parent-again {c:.3f}')
    spread = max(parent) - min(parent)
    pm, tm = sum(parent) / len(parent), sum(this) / len(this)
    say(f'    parent: {len(parent)} runs {min(parent):.3f} .. {max(parent):.3f} (spread {spread:.3f}, mean {pm:.3f})')
    say(f'    this:   {len(this)} runs {min(this):.3f} .. {max(this):.3f} (mean {tm:.3f}); this - parent mean {tm - pm:+.3f} ms: '
        + ('inside' if abs(tm - pm) <= spread else 'OUTSIDE') + " the parent's own spread")
    say(f'    losses of the last step, all {len(parent) + len(this)} runs: ' + ('identical ' + next(iter(losses)) if len(losses) == 1 else 'DIFFERENT ' + ' '.join(sorted(losses))))


against_parent()                # before this process opens the device: one bench at a time has it to itself

import numpy as np                                                                                    # noqa: E402
import torch                                                                                          # noqa: E402
import torch.nn.functional as F                                                                       # noqa: E402
import dualsuperreslearningforsemseg_amd as D                                                         # noqa: E402
from dualsuperreslearningforsemseg_amd import functional as HF, settings                              # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import call                                               # noqa: E402
from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep, _do_train_val      # noqa: E402
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs                      # noqa: E402
from dualsuperreslearningforsemseg_amd.ddp import FlatParams                                          # noqa: E402
from dualsuperreslearningforsemseg_amd.metrices import SRQuality                                      # noqa: E402


def ab(fa, fb, reps=10, rounds=5):
    """us per call of two launch sequences, alternating windows of `reps` back-to-back calls; -> (min a, min b, all a, all b)"""
    ta, tb = [], []
    for f in (fa, fb):
        for _ in range(3):
            f()
    for _ in range(rounds):
        for f, acc in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record(); torch.cuda.synchronize()
            acc.append(a.elapsed_time(b) / reps * 1e3)
    return min(ta), min(tb), ta, tb


def window2d():
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / 4.5)
    g = (g / g.sum()).astype(np.float32)
    return torch.from_numpy(np.outer(g, g).astype(np.float32))


def torch_composition(pred, ref, mean, std, win):
    """-> (psnr (N,), ssim (N,)) with torch ops only"""
    C = pred.shape[1]
    m, s = torch.tensor(mean, device=pred.device).reshape(1, C, 1, 1), torch.tensor(std, device=pred.device).reshape(1, C, 1, 1)
    x, y = (pred * s + m).clamp(0, 1), (ref * s + m).clamp(0, 1)
    planes = torch.cat([x, y, x * x, x * y, y * y], dim=1)
    f = F.conv2d(planes, win.to(pred.device).reshape(1, 1, 11, 11).repeat(5 * C, 1, 1, 1), groups=5 * C)
    mx, my, exx, exy, eyy = f.split(C, dim=1)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    ssim = ((2 * mxy + 1e-4) * (2 * (exy - mxy) + 9e-4)) / ((mxx + myy + 1e-4) * ((exx - mxx) + (eyy - myy) + 9e-4))
    mse = ((x - y) ** 2).double().mean(dim=(1, 2, 3))
    return -10.0 * torch.log10(mse), ssim.double().mean(dim=(1, 2, 3))


def kernel_legs():
    win = window2d()
    st = HF._stream()
    for shape in ((8, 3, 512, 1024), (8, 3, 1024, 2048)):
        N, C, H, W = shape
        g = torch.Generator().manual_seed(7)
        ref = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        pred = (ref + 0.3 * torch.randn(shape, generator=g).to(dev)).contiguous(memory_format=torch.channels_last)
        nbytes = 2 * pred.numel() * 4
        kern = lambda: HF.sr_quality(pred, ref, cs.MEAN, cs.STD)
        comp = lambda: torch_composition(pred, ref, cs.MEAN, cs.STD, win)
        psnr_k, ssim_k = HF.sr_quality_figures(kern(), C, H, W)
        psnr_t, ssim_t = (v.cpu().numpy() for v in comp())
        peaks = {}
        for name, f in (('kernel', kern), ('torch', comp)):
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            f()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        tk, tt, ak, at = ab(kern, comp)
        src, dst = pred.reshape(-1), torch.empty_like(pred).reshape(-1)
        rows = src.numel() // 64
        tk2, tc, _, _ = ab(kern, lambda: call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, rows, 64, st))
        say(f'{N} x {C} x {H} x {W} (two tensors of {nbytes / 2e6:.1f} MB), us per call, min of 5 alternating windows of 10 calls:')
        say(f'  (b) dsrl_sr_quality, both launches      {tk:9.1f}   (' + ' '.join(f'{v:.1f}' for v in ak) + ')')
        say(f'  (c) torch composition                   {tt:9.1f}   (' + ' '.join(f'{v:.1f}' for v in at) + f')   torch / kernel = {tt / tk:.1f} x: the kernel is '
            + ('faster' if tk < tt else 'NOT FASTER'))
        say(f'      figures of image 0: kernel PSNR {psnr_k[0]:.4f} dB SSIM {ssim_k[0]:.6f}; torch PSNR {psnr_t[0]:.4f} dB SSIM {ssim_t[0]:.6f}')
        say(f'  (d) the kernel reads {nbytes / 1e6:.1f} MB in {tk2:.1f} us = {nbytes / tk2 / 1e6:.2f} TB/s; dsrl_copy2d moves {nbytes / 1e6:.1f} MB (half read, half written) in '
            f'{tc:.1f} us = {nbytes / tc / 1e6:.2f} TB/s: the kernel reaches {100 * tc / tk2:.0f} % of the copy\'s byte rate')
        say(f'  (e) peak device memory above the inputs: kernel {peaks["kernel"] / 2 ** 20:.2f} MiB (records + block partials), torch {peaks["torch"] / 2 ** 20:.1f} MiB')
        del pred, ref, src, dst
        torch.cuda.empty_cache()


def validation_pass():
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(2, cs).to(dev).to(memory_format=torch.channels_last)
    flat = FlatParams(model)
    step = TrainStep(model, flat, 2, 0.1, 1.0, cs.IGNORE_CLASS_LABEL)
    loader = SyntheticCityscapes(8, (256, 512), torch.device(dev), length=8)
    res = {'without': [], 'with': []}
    figures = None

    def run(metric):
        details = {'sr_quality': SRQuality(cs.MEAN, cs.STD)} if metric else {}
        _do_train_val(False, 1, model, step, loader, 0.0, 0.9, 0.0, False, True, details)
        torch.cuda.synchronize()
        return details

    try:
        for metric in (False, True):
            run(metric)
        for _ in range(max(ROUNDS, 3)):
            for k, metric in (('without', False), ('with', True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = run(metric)
                res[k].append((time.perf_counter() - t0) * 1e3)
                if metric:
                    figures = (d['PSNR'], d['SSIM'])
    finally:
        step.release()
    say('(f) validation pass of a stage-2 run (batch 8, 256 x 512 in, 512 x 1024 out, 8 batches, eager), ms per pass, alternating:')
    for k in res:
        say(f'    {k:<8} the metric  ' + '  '.join(f'{v:.2f}' for v in res[k]) + f'   min {min(res[k]):.2f}')
    dlt = min(res['with']) - min(res['without'])
    say(f"    with - without (min): {dlt:+.2f} ms per pass = {dlt / 8 * 1e3:+.0f} us per batch ({100 * dlt / min(res['without']):+.2f} %); "
        f'figures of the random-init model: PSNR {figures[0]:.3f} dB, SSIM {figures[1]:.5f}')


kernel_legs()
if '--no-val' not in args:
    validation_pass()
out = os.path.join(ROOT, 'profiles', 'sr_quality.txt')
KEEP = '## recorded beside the tool'
tail = ''
if os.path.isfile(out):
    old = open(out).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

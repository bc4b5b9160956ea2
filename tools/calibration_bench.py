#!/usr/bin/env python3
"""Cost of the calibration record and the confidence map, written to profiles/calibration.txt.  Every figure is measured on the
device this runs on, at tail inputs 8 x 19 x 128 x 256 and 8 x 19 x 256 x 512 (class maps 512 x 1024 and 1024 x 2048):
  (a) the DEFAULT replayed step (bench.py --gpus 1) of this tree against the parent commit on the same box: the parent's tree with its own library
      under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again.  The step launches nothing of the feature.  Skipped (and said
      so) when ab/prev_tree is not there;
  (b) the single-view and the flip tail (target, counters, loss and confusion matrix as the benchmark command asks for them) with the record only,
      with the map only and with both, each against the same launch without them, alternating windows; the spread of every series is printed;
  (c) dsrl_calibration_from_logits (record only, record and map) against dsrl_seg_metrics on the same logits and against dsrl_copy2d moving as many
      bytes;
  (d) the torch composition on written logits (softmax -> max -> bucketise -> three bincounts; checked against the kernel's n and hit rows), in
      time and peak memory;
  (e) DSRL.predict with its confusion matrix at batch 8, 256 x 512 in, as the benchmark command runs it, with and without `calibration`,
      alternating: the added cost per benchmark batch; and the default predict launch of this tree against the parent's (ab/prev_tree), each in a
      process of its own, alternating;
  (f) the confidence map against fp64 on the two test shapes: the kernel's and the fp32 restatement's maximum absolute error
      (tests/calibration_ref.py), and the smallest power-of-two margin the kernel stays within.
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/calibration_bench.py [--steps K] [--rounds R] [--no-parent] [--no-predict] [VAR=value ...]"""
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
NC, IGNORE, BINS = 19, 255, 15
lines = []

PREDICT_PROBE = r'''
import sys, time, torch
sys.path.insert(0, sys.argv[1])
import dualsuperreslearningforsemseg_amd as D
from dualsuperreslearningforsemseg_amd import settings
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
torch.manual_seed(settings.RANDOM_SEED)
model = D.DSRL(1, cs).to('cuda:0').to(memory_format=torch.channels_last).eval()
g = torch.Generator().manual_seed(3)
img = torch.randn((8, 3, 256, 512), generator=g).to('cuda:0').contiguous(memory_format=torch.channels_last)
target = torch.randint(0, 19, (8, 512, 1024), generator=g).to(torch.uint8).to('cuda:0')
flag = torch.zeros((), dtype=torch.int32, device='cuda:0')
cm = torch.zeros(361, dtype=torch.int64, device='cuda:0')
for _ in range(3):
    model.predict(img, target, nan_flag=flag, confusion=cm)
best = 1e9
for _ in range(5):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10):
        model.predict(img, target, nan_flag=flag, confusion=cm)
    torch.cuda.synchronize(); best = min(best, (time.perf_counter() - t0) / 10 * 1e3)
print('PREDICT_MS', best)
'''


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


def predict_line(tree):
    r = subprocess.run([sys.executable, '-c', PREDICT_PROBE, tree], cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f'the predict probe in {tree} ended with {r.returncode}: {r.stderr[-400:]}')
    return float([ln for ln in r.stdout.splitlines() if ln.startswith('PREDICT_MS')][-1].split()[1])


def against_parent():
    have = '--no-parent' not in args and os.path.isfile(os.path.join(PREV, 'bench.py'))
    for what, line, unit in ((f'(a) default replayed step, bench.py --gpus 1 --steps {STEPS} --warmup 8, ms per step', bench_line, 'step'),
                             ('(e2) default DSRL.predict (target, confusion matrix; batch 8, 256 x 512 in, eager), ms per batch, min of 5 windows of 10', predict_line,
                              'batch')):
        say(what + ': the parent commit in its own tree with its own library,')
        say('    this tree; each round parent, this, parent again:')
        if not have:
            say('    NOT MEASURED: no parent tree under ab/prev_tree')
            continue
        parent, this, losses = [], [], set()
        for r in range(ROUNDS):
            res = [line(PREV), line(ROOT), line(PREV)]
            if unit == 'step':
                losses |= {json.dumps(x[1]) for x in res}
                res = [x[0] for x in res]
            parent += [res[0], res[2]]; this.append(res[1])
            say(f'    round {r + 1}: parent {res[0]:.3f}  this {res[1]:.3f}  parent-again {res[2]:.3f}')
        spread = max(parent) - min(parent)
        pm, tm = sum(parent) / len(parent), sum(this) / len(this)
        say(f'    parent: {len(parent)} runs {min(parent):.3f} .. {max(parent):.3f} (spread {spread:.3f}, mean {pm:.3f})')
        say(f'    this:   {len(this)} runs {min(this):.3f} .. {max(this):.3f} (mean {tm:.3f}); this - parent mean {tm - pm:+.3f} ms: '
            + ('inside' if abs(tm - pm) <= spread else 'OUTSIDE') + " the parent's own spread")
        if unit == 'step':
            say(f'    losses of the last step, all {len(parent) + len(this)} runs: ' + ('identical ' + next(iter(losses)) if len(losses) == 1 else 'DIFFERENT ' + ' '.join(sorted(losses))))


if '--no-predict' not in args:
    against_parent()            # before this process opens the device: one bench at a time has it to itself

import numpy as np                                                                                    # noqa: E402
import torch                                                                                          # noqa: E402
import dualsuperreslearningforsemseg_amd as D                                                         # noqa: E402
from dualsuperreslearningforsemseg_amd import functional as HF, settings                              # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import call                                               # noqa: E402
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs                      # noqa: E402
from dualsuperreslearningforsemseg_amd.nn_modules import HipBatchNorm2d, HipConvTranspose2d           # noqa: E402


def window(f, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def ab(fa, fb, reps=(10, 10), rounds=5, warm=(3, 3)):
    """us per call of two launch sequences, alternating windows of back-to-back calls; -> (min a, min b, all a, all b)"""
    ta, tb = [], []
    for f, n in ((fa, warm[0]), (fb, warm[1])):
        for _ in range(n):
            f()
    for _ in range(rounds):
        ta.append(window(fa, reps[0]))
        tb.append(window(fb, reps[1]))
    return min(ta), min(tb), ta, tb


def series(v):
    return f'min {min(v):8.1f}  (' + ' '.join(f'{x:.1f}' for x in v) + f'; spread {max(v) - min(v):.1f})'


def tail_modules(seed):
    rs = np.random.RandomState(seed)
    c1 = HipConvTranspose2d(NC, NC, kernel_size=2, stride=2, padding=0, bias=False)
    bn = HipBatchNorm2d(NC)
    c2 = HipConvTranspose2d(NC, NC, kernel_size=2, stride=2, padding=0, bias=True)
    with torch.no_grad():
        for m in (c1, c2):
            m.weight.copy_(torch.from_numpy((rs.standard_normal((NC, NC, 2, 2)) * np.sqrt(2.0 / (NC * 4))).astype(np.float32)))
        bn.running_var.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, NC).astype(np.float32)))
        bn.running_mean.copy_(torch.from_numpy((rs.standard_normal(NC) * 0.1).astype(np.float32)))
    return [m.to(dev).eval() for m in (c1, bn, c2)]


def torch_composition(logits, target):
    """-> int64 [n | hit | sum of conf (float64 per bin, returned apart)] with torch ops only"""
    p, pred = torch.softmax(logits, dim=1).max(dim=1)
    live = (target != IGNORE) & (target < NC)
    c = p[live]
    b = torch.clamp((c * float(BINS)).long(), max=BINS - 1)
    hit = (pred[live] == target[live].long())
    return torch.bincount(b, minlength=BINS), torch.bincount(b, weights=hit.double(), minlength=BINS), torch.bincount(b, weights=c.double(), minlength=BINS)


def kernel_legs():
    st = HF._stream()
    mods = tail_modules(5)
    for shape in ((8, NC, 128, 256), (8, NC, 256, 512)):
        N, _, h, w = shape
        g = torch.Generator().manual_seed(9)
        tshape = (N, 4 * h, 4 * w)
        target = torch.randint(0, NC, tshape, generator=g).to(torch.uint8)
        target[torch.rand(tshape, generator=g) < 0.1] = IGNORE
        target = target.to(dev)
        P = target.numel()
        say(f'tail input {N} x {NC} x {h} x {w} -> class maps {4 * h} x {4 * w} ({P / 1e6:.1f} M pixels), us per call, alternating windows of 10 back-to-back calls:')
        for flip in (False, True):
            x = torch.randn(((2 * N) if flip else N, NC, h, w), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            counts, cm, rec = (torch.zeros(n, dtype=torch.int64, device=dev) for n in (3 * NC + 2, NC * NC, 3 * BINS))
            base = lambda: HF.sssr_tail_predict(x, *mods, target=target, counts=counts, confusion=cm, flip=flip)
            name = 'flip tail  ' if flip else 'single view'
            for what, kw in (('record only', {'calibration': rec}), ('map only   ', {'confidence': True}), ('both       ', {'calibration': rec, 'confidence': True})):
                with_ = lambda: HF.sssr_tail_predict(x, *mods, target=target, counts=counts, confusion=cm, flip=flip, **kw)
                t0, t1, a0, a1 = ab(base, with_)
                say(f'  (b) {name} without {series(a0)}')
                say(f'      {name} {what} {series(a1)}   added {t1 - t0:+.1f} us' + (f' for {4 * P / 1e6:.0f} MB of map: {4 * P / max(t1 - t0, 1e-3) / 1e6:.2f} TB/s' if 'confidence' in kw else ''))
            del x
        logits = torch.randn((N, NC, 4 * h, 4 * w), generator=g).mul_(3.0).to(dev).contiguous(memory_format=torch.channels_last)
        lg, ld = HF.pm(logits)
        counts, rec = torch.zeros(3 * NC + 2, dtype=torch.int64, device=dev), torch.zeros(3 * BINS, dtype=torch.int64, device=dev)
        cmap = torch.empty(tshape, device=dev)
        seg = lambda: call('dsrl_seg_metrics', lg.data_ptr(), ld, target.data_ptr(), P, NC, IGNORE, counts.data_ptr(), st)
        k3 = lambda: HF.calibration_counts_(rec, logits, target, IGNORE, BINS)
        k3m = lambda: HF.calibration_counts_(rec, logits, target, IGNORE, BINS, cmap)
        t0, t1, a0, a1 = ab(seg, k3)
        say(f'  (c) dsrl_seg_metrics on {4 * NC * P / 1e6:.0f} MB of logits   {series(a0)}')
        say(f'      dsrl_calibration_from_logits, record  {series(a1)}   = {t1 / t0:.2f} x seg_metrics, {4 * NC * P / t1 / 1e6:.2f} TB/s')
        floats = (NC * P + P) // 64 * 64 // 2
        src, dst = torch.empty(floats, device=dev), torch.empty(floats, device=dev)
        t2, tc, a2, ac = ab(k3m, lambda: call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, floats // 64, 64, st))
        say(f'      dsrl_calibration_from_logits, + map   {series(a2)}   {4 * (NC + 1) * P / t2 / 1e6:.2f} TB/s')
        say(f'      dsrl_copy2d moving as many bytes      {series(ac)}   {4 * (NC + 1) * P / tc / 1e6:.2f} TB/s: the kernel reaches {100 * tc / t2:.0f} % of the copy\'s byte rate')
        del src, dst
        rec.zero_(); k3()
        n_t, hit_t, _ = torch_composition(logits, target)
        got = rec.cpu().numpy().reshape(3, BINS)
        same = np.array_equal(got[0], n_t.cpu().numpy()) and np.array_equal(got[1], hit_t.cpu().numpy().astype(np.int64))
        peaks = {}
        for nm, f in (('kernel', k3), ('torch', lambda: torch_composition(logits, target))):
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            b0 = torch.cuda.memory_allocated()
            f()
            torch.cuda.synchronize()
            peaks[nm] = torch.cuda.max_memory_allocated() - b0
        tk, tt, ak, at = ab(k3, lambda: torch_composition(logits, target), reps=(10, 3), rounds=4, warm=(3, 1))
        say(f'  (d) torch composition on the written logits {series(at)}   torch / kernel = {tt / tk:.1f} x; n and hit rows '
            + ('equal the kernel\'s' if same else 'differ from the kernel\'s in pixels at a bin edge (torch.softmax rounds differently)'))
        say(f'      peak device memory above the logits: kernel {peaks["kernel"] / 2 ** 20:.1f} MiB, torch {peaks["torch"] / 2 ** 20:.1f} MiB')
        del logits, lg, cmap
        torch.cuda.empty_cache()


def predict_leg():
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(1, cs).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(3)
    img = torch.randn((8, 3, 256, 512), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    target = torch.randint(0, NC, (8, 512, 1024), generator=g).to(torch.uint8).to(dev)
    cm, rec = torch.zeros(NC * NC, dtype=torch.int64, device=dev), torch.zeros(3 * BINS, dtype=torch.int64, device=dev)
    flag = torch.zeros((), dtype=torch.int32, device=dev)

    def batch(cal):
        model.predict(img, target, ignore_index=IGNORE, nan_flag=flag, confusion=cm, **({'calibration': rec} if cal else {}))

    res = {False: [], True: []}
    for b in (False, True):
        for _ in range(3):
            batch(b)
    for _ in range(5):
        for b in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                batch(b)
            torch.cuda.synchronize()
            res[b].append((time.perf_counter() - t0) / 10 * 1e3)
    say('(e) one batch of the benchmark command (DSRL.predict with its confusion matrix, batch 8, 256 x 512 in, class maps 512 x 1024, eager), ms per batch,')
    say('    windows of 10 batches, alternating:')
    for b, name in ((False, 'without'), (True, 'with')):
        say(f'    {name:<8} calibration  ' + '  '.join(f'{v:.3f}' for v in res[b]) + f'   min {min(res[b]):.3f}')
    dlt = min(res[True]) - min(res[False])
    say(f'    with - without (min): {dlt * 1e3:+.0f} us per batch ({100 * dlt / min(res[False]):+.2f} %)')


def accuracy_leg():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import calibration_ref as R
    say('(f) the confidence map of the single-view tail against fp64 (tests/calibration_ref.py), maximum absolute error:')
    for shape in ((2, NC, 5, 7), (1, NC, 96, 352)):
        rs = np.random.RandomState(101 + shape[2])
        p = {'w1': rs.standard_normal((NC, NC, 2, 2)) * np.sqrt(2.0 / (NC * 4)), 'w2': rs.standard_normal((NC, NC, 2, 2)) * np.sqrt(2.0 / (NC * 4)),
             'gamma': rs.uniform(0.5, 1.5, NC), 'beta': rs.standard_normal(NC) * 0.1, 'mean': rs.standard_normal(NC) * 0.1, 'var': rs.uniform(0.5, 1.5, NC),
             'b2': rs.standard_normal(NC) * 0.05}
        p = {k: np.asarray(v, np.float32) for k, v in p.items()}
        mods = tail_modules(0)
        with torch.no_grad():
            mods[0].weight.copy_(torch.from_numpy(p['w1'])); mods[2].weight.copy_(torch.from_numpy(p['w2'])); mods[2].bias.copy_(torch.from_numpy(p['b2']))
            mods[1].weight.copy_(torch.from_numpy(p['gamma'])); mods[1].bias.copy_(torch.from_numpy(p['beta']))
            mods[1].running_mean.copy_(torch.from_numpy(p['mean'])); mods[1].running_var.copy_(torch.from_numpy(p['var']))
        x = np.random.RandomState(102 + shape[2]).standard_normal(shape).astype(np.float32)
        c64, _ = R.confidence64(R.tail_logits(x, p, mods[1].eps, np.float64))
        e32 = np.abs(R.confidence32(R.tail_logits(x, p, mods[1].eps, np.float32)).astype(np.float64) - c64).max()
        _, _, conf = HF.sssr_tail_predict(torch.from_numpy(x).to(dev).contiguous(memory_format=torch.channels_last), *mods, confidence=True)
        ek = np.abs(conf.cpu().numpy().astype(np.float64) - c64).max()
        margin = 1.0
        while ek > margin * e32:
            margin *= 2.0
        say(f'    tail input {shape}: kernel {ek:.3e}, fp32 restatement {e32:.3e}; smallest power-of-two margin the kernel stays within: {margin:g}')


kernel_legs()
if '--no-predict' not in args:
    predict_leg()
accuracy_leg()
out = os.path.join(ROOT, 'profiles', 'calibration.txt')
KEEP = '## recorded beside the tool'
tail = ''
if os.path.isfile(out):
    old = open(out).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

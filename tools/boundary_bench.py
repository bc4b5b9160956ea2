#!/usr/bin/env python3
"""Cost of the Boundary IoU counters, written to profiles/boundary_iou.txt.  Every figure is measured on the device this runs on,
at 8 x 512 x 1024 with d = 23 (the class maps of the default 256 x 512 input) and 8 x 1024 x 2048 with d = 46, on blob-structured maps:
  (a) the DEFAULT replayed step (bench.py --gpus 1) of this tree against the parent commit on the same box: the parent's tree with its own library
      under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again.  The step launches nothing of the metric.  Skipped (and said
      so) when ab/prev_tree is not there;
  (b) the two launches of dsrl_boundary_counts, HIP events around back-to-back calls, alternating with each of
  (c) a torch composition that produces the same counters (checked): max_pool2d of +label and of -label with the (2d+1)^2 window, the image frame,
      bincount; its peak memory beside the kernel's;
  (d) dsrl_confusion_matrix on the same two maps: the cost of merely reading them;
  (e) dsrl_copy2d moving as many bytes as the two launches move, workspace included, and the share of the copy's byte rate they reach;
  (f) DSRL.predict with its confusion matrix at batch 8, 256 x 512 in, as the benchmark command runs it, with and without boundary_counts_ on the
      class map it returns, alternating.
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/boundary_bench.py [--steps K] [--rounds R] [--no-parent] [--no-predict] [VAR=value ...]"""
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
NC, IGNORE = 19, 255
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
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs                      # noqa: E402


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


def blob_maps(N, H, W, seed):
    """a target of rectangular blobs of a quarter of the height and a sixth of the width with random classes and a few void regions; a prediction whose outlines are
    displaced by a few pixels and which disagrees on some blobs: what a segmentation network's output looks like to this metric"""
    rs = np.random.RandomState(seed)
    ch, cw = max(8, H // 4), max(8, W // 6)
    cells = rs.randint(0, NC, (N, -(-H // ch) + 1, -(-W // cw) + 1)).astype(np.uint8)
    full = np.repeat(np.repeat(cells, ch, axis=1), cw, axis=2)
    target = full[:, ch // 3:ch // 3 + H, cw // 2:cw // 2 + W].copy()
    wrong = cells.copy()
    flip = rs.uniform(size=cells.shape) < 0.15
    wrong[flip] = rs.randint(0, NC, int(flip.sum()))
    fullp = np.repeat(np.repeat(wrong, ch, axis=1), cw, axis=2)
    pred = fullp[:, ch // 3 - 3:ch // 3 - 3 + H, cw // 2 + 5:cw // 2 + 5 + W].copy()
    for n in range(N):
        y, x = rs.randint(0, H - ch), rs.randint(0, W - cw)
        target[n, y:y + ch, x:x + cw] = IGNORE
    return np.ascontiguousarray(pred), np.ascontiguousarray(target)


def torch_composition(pred, target, d):
    """-> int64 [I | G | P] with torch ops only: the window is uniform iff the maximum and the minimum over it equal the pixel; max_pool2d pads with
    -inf, which no pixel sees, so the frame of width d is added by hand"""
    N, H, W = pred.shape
    live = (target < NC) & (target != IGNORE)
    g = torch.where(live, target, torch.full_like(target, 255)).float().unsqueeze(1)
    p = torch.where(live, torch.where(pred < NC, pred, torch.full_like(pred, 254)), torch.full_like(pred, 255)).float().unsqueeze(1)
    frame = torch.ones((H, W), dtype=torch.bool, device=pred.device)
    if H > 2 * d and W > 2 * d:
        frame[d:H - d, d:W - d] = False
    k = 2 * d + 1

    def band(m):
        return (F.max_pool2d(m, k, 1, d) != m) | (-F.max_pool2d(-m, k, 1, d) != m) | frame

    gb, pb = band(g).squeeze(1), band(p).squeeze(1)
    gl, pl = g.squeeze(1).long(), p.squeeze(1).long()
    G = torch.bincount(gl[live & gb], minlength=256)[:NC]
    P = torch.bincount(pl[live & pb & (pl < NC)], minlength=256)[:NC]
    I = torch.bincount(gl[live & gb & pb & (gl == pl)], minlength=256)[:NC]
    return torch.cat([I, G, P])


def kernel_legs():
    st = HF._stream()
    for (N, H, W), d in (((8, 512, 1024), 23), ((8, 1024, 2048), 46)):
        assert HF.boundary_distance(H, W) == d
        prn, tgn = blob_maps(N, H, W, 7)
        pred, target = torch.from_numpy(prn).to(dev), torch.from_numpy(tgn).to(dev)
        P = N * H * W
        counts = torch.zeros(3 * NC, dtype=torch.int64, device=dev)
        cm = torch.zeros(NC * NC, dtype=torch.int64, device=dev)
        kern = lambda: HF.boundary_counts_(counts, pred, target, NC, IGNORE, distance=d)
        comp = lambda: torch_composition(pred, target, d)
        conf = lambda: HF.confusion_matrix_(cm, pred, target, NC, IGNORE)
        kern()
        got, want = counts.cpu().numpy().copy(), comp().cpu().numpy()
        assert np.array_equal(got, want), 'the torch composition and the kernel disagree'
        I, G, Pp = got.reshape(3, NC)
        valid = int(((tgn < NC) & (tgn != IGNORE)).sum())
        peaks = {}
        for name, f in (('kernel', kern), ('torch', comp)):
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            f()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        tk, tt, ak, at = ab(kern, comp, reps=(10, 2), rounds=4, warm=(3, 1))
        tk2, tf, _, af = ab(kern, conf)
        # bytes the two launches move: the row pass reads both maps and writes 2 bytes per pixel; a wave of the column pass reads 64 + 2d rows of
        # that result for 64 output rows, and both maps again
        moved = P * (2 + 2 + 2 * (64 + 2 * d) / 64 + 2)
        floats = int(moved / 2 / 4) // 64 * 64
        src, dst = torch.empty(floats, device=dev), torch.empty(floats, device=dev)
        tk3, tc, _, ac = ab(kern, lambda: call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, floats // 64, 64, st))
        say(f'{N} x {H} x {W}, d = {d} (two maps of {P / 1e6:.1f} MB; band share {G.sum() / valid:.2f} of the counted pixels, I / G = {I.sum() / G.sum():.2f}),')
        say('us per call, min of alternating windows of back-to-back calls:')
        say(f'  (b) dsrl_boundary_counts, both launches {tk:9.1f}   (' + ' '.join(f'{v:.1f}' for v in ak) + ')')
        say(f'  (c) torch composition, same counters    {tt:9.1f}   (' + ' '.join(f'{v:.1f}' for v in at) + f')   torch / kernel = {tt / tk:.0f} x: the kernel is '
            + ('faster' if tk < tt else 'NOT FASTER'))
        say(f'      peak device memory above the maps: kernel {peaks["kernel"] / 2 ** 20:.1f} MiB (the 2-byte-per-pixel workspace), torch {peaks["torch"] / 2 ** 20:.1f} MiB')
        say(f'  (d) dsrl_confusion_matrix, same maps    {tf:9.1f}   (' + ' '.join(f'{v:.1f}' for v in af) + f')   kernel / confusion matrix = {tk2 / tf:.1f} x')
        say(f'  (e) the two launches move {moved / 1e6:.0f} MB (maps twice, workspace written once and read {(64 + 2 * d) / 64:.2f} x) in {tk3:.1f} us = '
            f'{moved / tk3 / 1e6:.2f} TB/s; dsrl_copy2d moves as many bytes in {tc:.1f} us = {moved / tc / 1e6:.2f} TB/s: '
            f'the kernels reach {100 * tc / tk3:.0f} % of the copy\'s byte rate')
        del pred, target, src, dst
        torch.cuda.empty_cache()


def predict_leg():
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(1, cs).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(3)
    img = torch.randn((8, 3, 256, 512), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    _, tgn = blob_maps(8, 512, 1024, 11)
    target = torch.from_numpy(tgn).to(dev)
    cm = torch.zeros(NC * NC, dtype=torch.int64, device=dev)
    counts = torch.zeros(3 * NC, dtype=torch.int64, device=dev)
    flag = torch.zeros((), dtype=torch.int32, device=dev)

    def batch(boundary):
        pred, _, _ = model.predict(img, target, ignore_index=IGNORE, nan_flag=flag, confusion=cm)
        if boundary:
            HF.boundary_counts_(counts, pred, target, NC, IGNORE, ratio=0.02, nan_flag=flag)

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
    say('(f) one batch of the benchmark command (DSRL.predict with its confusion matrix, batch 8, 256 x 512 in, class maps 512 x 1024, eager), ms per batch,')
    say('    windows of 10 batches, alternating:')
    for b, name in ((False, 'without'), (True, 'with')):
        say(f'    {name:<8} boundary_counts_  ' + '  '.join(f'{v:.3f}' for v in res[b]) + f'   min {min(res[b]):.3f}')
    dlt = min(res[True]) - min(res[False])
    say(f'    with - without (min): {dlt * 1e3:+.0f} us per batch ({100 * dlt / min(res[False]):+.2f} %)')


kernel_legs()
if '--no-predict' not in args:
    predict_leg()
out = os.path.join(ROOT, 'profiles', 'boundary_iou.txt')
KEEP = '## recorded beside the tool'
tail = ''
if os.path.isfile(out):
    old = open(out).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

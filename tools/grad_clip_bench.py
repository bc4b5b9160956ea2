#!/usr/bin/env python3
"""Cost of gradient-norm clipping at the real arena size, written to profiles/grad_clip.txt.  Five measurements, each measured:
  (a) the DEFAULT replayed stage-3 step (batch 8, 256 x 512; bench.py --gpus 1) of this tree against the parent commit on the same box: the parent's
      tree with its own library under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again, so that the parent's run-to-run
      spread stands beside the difference.  Condition: the difference lies inside that spread - the default step launches what it launched.
      Skipped (and said so) when ab/prev_tree is not there;
  (b) the same step with clipping on (max_norm 1.0) against off, alternating in one process.  No preset bound: the figure is recorded;
  (c) dsrl_grad_sumsq over the whole gradient arena, HIP events around back-to-back launches, and its byte rate (4 bytes read per gradient) as a
      share of dsrl_copy2d's on as many bytes READ (the copy writes as many again);
  (d) dsrl_grad_clip_finish alone (its two launches) on the arena's tile count;
  (e) the comparison leg: torch.nn.utils.clip_grad_norm_ over the per-parameter gradient views of the same arena (several hundred small launches
      and a host read), wall time per call with a synchronise, beside sumsq + finish measured the same way.
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/grad_clip_bench.py [--steps K] [--rounds R] [--no-parent] [--no-step] [VAR=value ...]"""
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
ROUNDS = int(args[args.index('--rounds') + 1]) if '--rounds' in args else 3
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
    say(f'(a) default replayed step (no clipping), bench.py --gpus 1 --steps {STEPS} --warmup 8, ms per step: the parent commit in its own tree with its own')
    say('    library, this tree; each round parent, this, parent again:')
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

import torch                                                                                          # noqa: E402
import dualsuperreslearningforsemseg_amd as D                                                         # noqa: E402
from dualsuperreslearningforsemseg_amd import functional as HF, settings                              # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import call                                               # noqa: E402
from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep      # noqa: E402
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs                      # noqa: E402
from dualsuperreslearningforsemseg_amd.ddp import FlatParams                                          # noqa: E402


def make(clip):
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    if clip:
        flat.enable_grad_clip(1.0)
    return model, flat


def replayed_step():
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(8, (256, 512), torch.device(dev), length=1)))

    def run(step, n):
        for _ in range(n):
            step.enqueue(img, org, tgt, 0.0, 0.9, 0.0, True)      # lr 0: every step trains the same parameters
            while step.pending() > 1:
                step.collect()
        while step.pending():
            step.collect()
    res, replays = {'off': [], 'on': []}, {}
    models = {k: make(k == 'on') for k in res}
    for _ in range(ROUNDS):                     # one captured step at a time (the device-resident dropout key has one binding): build, warm, time, release
        for k, (model, flat) in models.items():
            s = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL)
            run(s, s.GRAPH_WARMUP + 6)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(s, STEPS)
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / STEPS * 1e3)
            replays[k] = s.graph_replays
            s.release()
    say(f'(b) replayed step (stage 3, batch 8, 256 x 512, {STEPS} steps per figure, {ROUNDS} alternating rounds in one process), ms per step:')
    for k in res:
        say(f'    clipping {k:<4} ' + '  '.join(f'{v:.3f}' for v in res[k]) + f'   min {min(res[k]):.3f}  (replays {replays[k]})')
    d = min(res['on']) - min(res['off'])
    st = models['on'][1].grad_clip_stats()
    say(f"    on - off (min): {d * 1e3:+.0f} us ({100 * d / min(res['off']):+.2f} %); the device record: {st['steps']} steps, {st['clipped']} clipped, "
        f"{st['nonfinite']} non-finite, last norm {st['norm']:.4g}, last coefficient {st['coef']:.4g}")
    return models['on'][1]


def ab(fa, fb, reps=20, rounds=5):
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


def wall(f, reps=10, rounds=3):
    """us per call, wall clock with a synchronise after every call (what a caller who reads the norm pays)"""
    f(); torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            f(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return min(out), out


def kernels(flat):
    n = flat.numel
    st = HF._stream()
    g, tiles, rec, eff = flat.g_flat, flat.clip_tiles, flat.clip_rec, flat.hyper_eff
    g.copy_(torch.randn(n, device=dev) * 1e-3)
    hyper = torch.tensor([0.0, 0.9, 0.0, 1.0], device=dev)
    nt = tiles.numel()
    rows = n // 64
    src, dst = torch.randn(rows * 64, device=dev), torch.empty(rows * 64, device=dev)

    def sumsq():
        call('dsrl_grad_sumsq', g.data_ptr(), 0, n, tiles.data_ptr(), st)

    def copy():
        call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, rows, 64, st)

    def fin():
        call('dsrl_grad_clip_finish', tiles.data_ptr(), nt, hyper.data_ptr(), 0.0, 0.0, 0.0, 0.0, rec.data_ptr(), eff.data_ptr(), st)

    def both():
        sumsq(); fin()

    ts, tc, as_, ac = ab(sumsq, copy)
    say(f'(c) dsrl_grad_sumsq over the whole gradient arena ({n} floats = {n * 4 / 1e6:.1f} MB, {nt} tiles), us per call, min of 5 alternating windows of 20 calls:')
    say(f'    dsrl_grad_sumsq                      {ts:7.1f}   (' + ' '.join(f'{v:.1f}' for v in as_) + f')   {n * 4 / ts / 1e6:.2f} TB/s read')
    say(f'    dsrl_copy2d, as many bytes read      {tc:7.1f}   (' + ' '.join(f'{v:.1f}' for v in ac) + f')   {rows * 64 * 4 / tc / 1e6:.2f} TB/s read (and as many written)')
    say(f'    the sum of squares reads at {100 * (n * 4 / ts) / (rows * 64 * 4 / tc):.0f} % of the byte rate at which the copy reads')
    tf, tb, af, ab_ = ab(fin, both)
    say(f'(d) dsrl_grad_clip_finish alone ({nt} tiles: two launches), us per call:   {tf:7.1f}   (' + ' '.join(f'{v:.1f}' for v in af) + ')')
    say(f'    sum of squares + finish back to back                                  {tb:7.1f}   (' + ' '.join(f'{v:.1f}' for v in ab_) + ')')
    params = [p for p in flat.params]

    for foreach in (None, False):
        def torch_clip(foreach=foreach):
            torch.nn.utils.clip_grad_norm_(params, 1e30, foreach=foreach)           # a threshold that never clips: the gradients keep their values
        tw, aw = wall(torch_clip)
        say(f'(e) torch.nn.utils.clip_grad_norm_ over the {len(params)} per-parameter views (foreach={foreach}), wall us per call with a synchronise: '
            f'{tw:9.1f}   (' + ' '.join(f'{v:.1f}' for v in aw) + ')')
    to, ao = wall(both)
    say(f'    dsrl_grad_sumsq + dsrl_grad_clip_finish measured the same way:                                                      {to:9.1f}   (' + ' '.join(f'{v:.1f}' for v in ao) + ')')
    r = flat.grad_clip_stats()
    ref = float(g.double().pow(2).sum().sqrt())
    say(f'    norm of the arena: device record {r["norm"]!r}, float64 torch {ref!r}')
    torch.cuda.synchronize()


if '--no-step' in args:
    _, flat_ = make(True)
else:
    flat_ = replayed_step()
kernels(flat_)
out = os.path.join(ROOT, 'profiles', 'grad_clip.txt')
KEEP = '## recorded beside the tool'
tail = ''
if os.path.isfile(out):
    old = open(out).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

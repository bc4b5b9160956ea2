#!/usr/bin/env python3
"""Cost of AdamW at the real arena size, written to profiles/adamw.txt (or --out).  Each figure is measured:
  (a) the DEFAULT replayed stage-3 step (batch 8, 256 x 512; bench.py --gpus 1) of this tree against the parent commit on the same box: the parent's
      tree with its own library under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again, so that the parent's run-to-run
      spread stands beside the difference.  Condition: the difference lies inside that spread - the default step launches what it launched.
      Skipped (and said so) when ab/prev_tree is not there;
  (b) the same step with AdamW against SGD, alternating in one process.  No preset bound: the figure is recorded;
  (c) the optimiser launches over the whole arena, HIP events around back-to-back launches, alternating: dsrl_adamw_step_dev_segments with and
      without _ema against dsrl_sgd_step_dev_segments, and a dsrl_copy2d of as many bytes as the AdamW launch moves (28 per parameter: p, g, m, v
      read, p, m, v written; SGD 20).  7 arenas against 5 make 1.4 x the SGD launch an expectation from byte counts, not a condition;
  (d) torch.optim.AdamW over the per-parameter views of the same arenas, foreach and fused, host clock around a step that ends in a synchronise.
And the memory of the extra arena.
Everything in the output file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/adamw_bench.py [--steps K] [--rounds R] [--no-parent] [--no-step] [--out FILE] [VAR=value ...]"""
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
OUT = args[args.index('--out') + 1] if '--out' in args else os.path.join(ROOT, 'profiles', 'adamw.txt')
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
    say(f'(a) default replayed step (SGD), bench.py --gpus 1 --steps {STEPS} --warmup 8, ms per step: the parent commit in its own tree with its own')
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


def make(adamw):
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    if adamw:
        flat.enable_adamw()
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
    res, replays, peak = {'sgd': [], 'adamw': []}, {}, {}
    models = {}
    torch.cuda.synchronize()
    for k in res:
        base = torch.cuda.memory_allocated()
        models[k] = make(k == 'adamw')
        peak[k] = torch.cuda.memory_allocated() - base
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
        say(f'    {k:<6} ' + '  '.join(f'{v:.3f}' for v in res[k]) + f'   min {min(res[k]):.3f}  (replays {replays[k]})')
    d = min(res['adamw']) - min(res['sgd'])
    flat = models['adamw'][1]
    say(f"    adamw - sgd (min): {d * 1e3:+.0f} us ({100 * d / min(res['sgd']):+.2f} %); steps counted on the device: {flat.adamw_step_count()}")
    say(f"memory: model + arenas {peak['sgd'] / 2 ** 20:.1f} MiB with SGD, {peak['adamw'] / 2 ** 20:.1f} MiB with AdamW: "
        f"+{(peak['adamw'] - peak['sgd']) / 2 ** 20:.1f} MiB (v_flat {flat.v_flat.numel() * 4 / 1e6:.1f} MB, the 64-byte record)")
    return flat


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


def kernels(flat):
    n = flat.numel
    tab, nseg = flat._segments(0, n)
    hyper = torch.tensor([0.0, 0.9, 0.0, 1.0], device=dev)      # lr 0: the parameters keep their values over the repetitions
    st = HF._stream()
    p, g, m, v, rec = flat.p_flat, flat.g_flat, flat.m_flat, flat.v_flat, flat.adamw_rec
    g.normal_(0.0, 1e-3)
    HF.adamw_set_step_(rec, 10)
    e = p.clone()
    erec = HF.ema_record(0.999, True, 0, dev)
    amax = flat.filters.amax

    def adamw():
        call('dsrl_adamw_step_dev_segments', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), tab.data_ptr(), nseg, hyper.data_ptr(), rec.data_ptr(), st)

    def adamw_ema():
        call('dsrl_adamw_step_dev_segments_ema', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), tab.data_ptr(), nseg, hyper.data_ptr(), rec.data_ptr(),
             e.data_ptr(), erec.data_ptr(), st)

    def adamw_flat():
        call('dsrl_adamw_step_dev', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(), rec.data_ptr(), st)

    def sgd():
        call('dsrl_sgd_step_dev_segments', p.data_ptr(), g.data_ptr(), m.data_ptr(), tab.data_ptr(), nseg, hyper.data_ptr(), st)

    amax.zero_()
    ta, ts, aa, as_ = ab(adamw, sgd)
    te, _, ae, _ = ab(adamw_ema, sgd)
    tf, _, af, _ = ab(adamw_flat, sgd)
    say(f'(c) optimiser pass over the whole arena ({n} floats = {n * 4 / 1e6:.1f} MB, {nseg} segments), us per call, min of 5 alternating windows of 20 calls:')
    say(f'    dsrl_adamw_step_dev_segments        {ta:7.1f}   (' + ' '.join(f'{x:.1f}' for x in aa) + ')')
    say(f'    dsrl_adamw_step_dev_segments_ema    {te:7.1f}   (' + ' '.join(f'{x:.1f}' for x in ae) + ')')
    say(f'    dsrl_adamw_step_dev (grid-stride)   {tf:7.1f}   (' + ' '.join(f'{x:.1f}' for x in af) + ')')
    say(f'    dsrl_sgd_step_dev_segments          {ts:7.1f}   (' + ' '.join(f'{x:.1f}' for x in as_) + ')')
    say(f'    AdamW / SGD = {ta / ts:.2f} (7 arenas against 5: 1.40 by bytes); the average adds {te - ta:+.1f} us')
    nbytes = 28 * n
    rows = nbytes // (2 * 4 * 64)
    src, dst = torch.randn(rows * 64, device=dev), torch.empty(rows * 64, device=dev)
    ta2, tc, _, _ = ab(adamw, lambda: call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, rows, 64, st))
    say(f'    bytes per second: the AdamW launch moves 28 bytes per parameter = {nbytes / 1e6:.1f} MB in {ta2:.1f} us = {nbytes / ta2 / 1e6:.2f} TB/s; dsrl_copy2d moves')
    say(f'    {rows * 64 * 8 / 1e6:.1f} MB (half read, half written) in {tc:.1f} us = {rows * 64 * 8 / tc / 1e6:.2f} TB/s: the AdamW launch reaches '
        f'{100 * (nbytes / ta2) / (rows * 64 * 8 / tc):.0f} % of the copy\'s rate; the SGD launch moves {20 * n / 1e6:.1f} MB at {20 * n / ts / 1e6:.2f} TB/s')
    torch.cuda.synchronize()
    # (d) torch's own optimiser over the per-parameter views of the arenas
    say(f'(d) torch.optim.AdamW over the {len(flat.params)} per-parameter views (lr 0), ms per step(), host clock to a synchronise, min of 5 windows of 5 steps:')
    for kind in ('foreach', 'fused'):
        try:
            opt = torch.optim.AdamW(flat.params, lr=0.0, weight_decay=0.0, **{kind: True})
            for _ in range(3):
                opt.step()
            best = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    opt.step()
                torch.cuda.synchronize()
                best.append((time.perf_counter() - t0) / 5 * 1e3)
            say(f'    {kind:<8} {min(best):7.3f}   (' + ' '.join(f'{x:.3f}' for x in best) + f')   = {min(best) * 1e3 / ta:.1f} x the segment launch')
            del opt
        except Exception as ex:          # a torch build without that implementation: said, not hidden
            say(f'    {kind:<8} NOT MEASURED: {type(ex).__name__}: {ex}')


if '--no-step' in args:
    _, flat_ = make(True)
else:
    flat_ = replayed_step()
kernels(flat_)
KEEP = '## recorded beside the tool'
tail = ''
if os.path.isfile(OUT):
    old = open(OUT).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

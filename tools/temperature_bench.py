#!/usr/bin/env python3
"""Cost of temperature scaling, written to profiles/temperature.txt.  Every figure is measured on the device this runs on, on
(8, 19, 512, 1024) and (8, 19, 1024, 2048) logits (the SSSR output of the default 256 x 512 input and of full-size Cityscapes) with ~10 % ignored labels:
  (a) the DEFAULT replayed step (bench.py --gpus 1) of this tree against the parent commit on the same box: the parent's tree with its own library
      under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again.  The step launches nothing of the feature.  Skipped (and said
      so) when ab/prev_tree is not there;
  (b) dsrl_temperature_stats (both launches) at K = 1 and K = 16, HIP events around back-to-back calls, alternating with each of
  (c) dsrl_copy2d on as many bytes as the logits (read + write: twice the traffic of a read), and the share of its byte rate the K = 1 launch reaches;
  (d) dsrl_calibration_from_logits on the same logits: another one-pass softmax consumer;
  (e) a torch composition giving the same 3 K sums (checked to 1e-6 relative), one softmax pass per beta; its peak memory beside the kernel's;
  (f) the fused tail with a temperature (dsrl_sssr_tail_predict_t) against the one without (dsrl_sssr_tail_predict_ex), record and confidence map on,
      at the tail input of the two sizes ((8, 19, 128, 256) and (8, 19, 256, 512));
  (g) the two passes of fit_temperature on 4 synthetic loader batches of 8 x 3 x 256 x 512, wall time per pass.
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/temperature_bench.py [--steps K] [--rounds R] [--no-parent] [--no-fit] [VAR=value ...]"""
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
        + ('inside' if min(parent) <= tm <= max(parent) else 'BELOW (faster than)' if tm < min(parent) else 'ABOVE (slower than)') + " the parent's own spread")
    say(f'    losses of the last step, all {len(parent) + len(this)} runs: ' + ('identical ' + next(iter(losses)) if len(losses) == 1 else 'DIFFERENT ' + ' '.join(sorted(losses))))


against_parent()                # before this process opens the device: one bench at a time has it to itself

import numpy as np                                                                                    # noqa: E402
import torch                                                                                          # noqa: E402
from dualsuperreslearningforsemseg_amd import functional as HF                                         # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import call                                               # noqa: E402


def window(f, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def ab(fa, fb, reps=(10, 10), rounds=5, warm=(3, 3)):
    """us per call of two launch sequences, alternating windows of back-to-back calls; -> (min a, min b)"""
    ta, tb = [], []
    for f, n in ((fa, warm[0]), (fb, warm[1])):
        for _ in range(n):
            f()
    for _ in range(rounds):
        ta.append(window(fa, reps[0]))
        tb.append(window(fb, reps[1]))
    return min(ta), min(tb)


def torch_composition(logits, target, betas):
    """the same 1 + 3 K sums from torch ops: one log-softmax pass per beta (float32 terms, float64 sums)"""
    live = (target != IGNORE) & (target < NC)
    t = torch.where(live, target, torch.zeros_like(target)).long().unsqueeze(1)
    m = logits.amax(dim=1, keepdim=True)
    d = logits - m
    dt = d.gather(1, t)[:, 0]
    out = [live.sum().double()]
    for b in betas:
        e = torch.exp(d * b)
        s = e.sum(1)
        mu = (e * d).sum(1) / s
        L = torch.log(s) - b * dt
        G = mu - dt
        Hh = (e * d * d).sum(1) / s - mu * mu
        out += [x[live].double().sum() for x in (L, G, Hh)]
    return torch.stack(out)


def kernel_legs():
    for N, H, W in ((8, 512, 1024), (8, 1024, 2048)):
        g = torch.Generator(device=dev).manual_seed(N * H)
        logits = (3.0 * torch.randn((N, NC, H, W), device=dev, generator=g)).contiguous(memory_format=torch.channels_last)
        target = torch.randint(0, NC, (N, H, W), device=dev, generator=g).to(torch.uint8)
        target[torch.rand((N, H, W), device=dev, generator=g) < 0.1] = IGNORE
        P = N * H * W
        nbytes = logits.numel() * 4
        say(f'--- logits ({N}, {NC}, {H}, {W}): {P} pixels, {nbytes / 2 ** 20:.0f} MiB')
        grid = HF.temperature_grid(0.25, 4.0, 16)
        recs, runs = {}, {}
        for K in (1, 16):
            betas = torch.tensor(grid[:K] if K > 1 else grid[9:10], dtype=torch.float32).to(dev)
            rec = torch.zeros(1 + 3 * K, dtype=torch.float64, device=dev)
            runs[K] = (lambda rec=rec, betas=betas: HF.temperature_stats_(rec, logits, target, betas, IGNORE))
            recs[K] = (rec, betas)
        copy_out = torch.empty_like(logits)
        copy = lambda: call('dsrl_copy2d', logits.data_ptr(), NC, copy_out.data_ptr(), NC, P, NC, HF._stream())
        cal = torch.zeros(45, dtype=torch.int64, device=dev)
        calib = lambda: HF.calibration_counts_(cal, logits, target, IGNORE, 15)
        t1, tc = ab(runs[1], copy)
        t16, tcal = ab(runs[16], calib)
        say(f'(b) dsrl_temperature_stats: K = 1 {t1:.1f} us, K = 16 {t16:.1f} us ({(t16 - t1) / 15:.1f} us per further beta; '
            f'{P * NC * 16 / t16 * 1e-3:.0f} G exponentials / s at K = 16)')
        say(f'(c) dsrl_copy2d on the same {nbytes / 2 ** 20:.0f} MiB (read + write): {tc:.1f} us = {2 * nbytes / tc * 1e-3:.0f} GB/s; '
            f'the K = 1 launch reads at {nbytes / t1 * 1e-3:.0f} GB/s, {100 * (nbytes / t1) / (2 * nbytes / tc):.0f} % of that rate')
        say(f'(d) dsrl_calibration_from_logits on the same logits: {tcal:.1f} us')
        del copy_out
        # (e) the torch composition: checked, timed, peak memory
        rec, betas = recs[16]
        rec.zero_(); runs[16](); torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
        want = torch_composition(logits, target, [float(b) for b in betas.cpu()])
        torch.cuda.synchronize()
        peak_t = torch.cuda.max_memory_allocated() - base
        err = ((rec - want).abs() / want.abs().clamp(min=1e-30)).max().item()
        torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
        runs[16](); torch.cuda.synchronize()
        peak_k = torch.cuda.max_memory_allocated() - base
        t0 = time.perf_counter()
        for _ in range(2):
            torch_composition(logits, target, [float(b) for b in betas.cpu()])
        torch.cuda.synchronize()
        tt = (time.perf_counter() - t0) / 2 * 1e6
        say(f'(e) torch composition of the same 49 sums (max relative difference {err:.1e}): {tt / 1e3:.1f} ms = {tt / t16:.0f} x the K = 16 launch; '
            f'peak memory {peak_t / 2 ** 20:.0f} MiB against {peak_k / 2 ** 20:.2f} MiB')
        assert err < 1e-5, err
        del logits, target, want
        torch.cuda.empty_cache()


def tail_leg():
    from dualsuperreslearningforsemseg_amd.nn_modules import HipBatchNorm2d, HipConvTranspose2d
    torch.manual_seed(5)
    c1 = HipConvTranspose2d(NC, NC, kernel_size=2, stride=2, padding=0, bias=False)
    bn = HipBatchNorm2d(NC)
    c2 = HipConvTranspose2d(NC, NC, kernel_size=2, stride=2, padding=0, bias=True)
    mods = [m.to(dev).eval() for m in (c1, bn, c2)]
    for N, H, W in ((8, 128, 256), (8, 256, 512)):
        x = torch.randn((N, NC, H, W), device=dev).contiguous(memory_format=torch.channels_last)
        target = torch.randint(0, NC, (N, 4 * H, 4 * W), device=dev).to(torch.uint8)
        rec = torch.zeros(45, dtype=torch.int64, device=dev)
        plain = lambda: HF.sssr_tail_predict(x, *mods, target=target, calibration=rec, confidence=True)
        temp = lambda: HF.sssr_tail_predict(x, *mods, target=target, calibration=rec, confidence=True, temperature=1.5)
        tp, tt = ab(plain, temp)
        say(f'(f) fused tail, input ({N}, {NC}, {H}, {W}), loss + record + confidence map: dsrl_sssr_tail_predict_ex {tp:.1f} us, _t {tt:.1f} us ({tt - tp:+.1f} us)')


def fit_leg():
    from dualsuperreslearningforsemseg_amd.command_handlers import fit_temperature as FT
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.models import DSRL
    torch.manual_seed(7)
    model = DSRL(stage=1, dataset_settings=cs).to(dev).to(memory_format=torch.channels_last).eval()
    batches = []
    for i in range(4):
        x = torch.randn((8, 3, 256, 512), device=dev).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            t = torch.distributions.Categorical(logits=1.5 * model._eval_sssr_logits(x).permute(0, 2, 3, 1)).sample().to(torch.uint8)
        batches.append(((x, None), (t, None)))
    marks = []

    def loader():
        torch.cuda.synchronize(); marks.append(time.perf_counter())
        return batches
    FT.fit_passes(model, loader, IGNORE, torch.device(dev))             # warm-up: allocator, library
    marks.clear()
    r = FT.fit_passes(model, loader, IGNORE, torch.device(dev))
    torch.cuda.synchronize(); marks.append(time.perf_counter())
    per = [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]
    with torch.no_grad():
        t0 = time.perf_counter()
        for (x, _), _ in batches:
            model._eval_sssr_logits(x)
        torch.cuda.synchronize()
        fwd = (time.perf_counter() - t0) * 1e3
    say(f"(g) fit_temperature on 4 batches of 8 x 3 x 256 x 512 ({r['pixels']} labelled pixels): {', '.join(f'pass {i + 1} {p:.1f} ms' for i, p in enumerate(per))} "
        f"(the 4 eval forwards alone: {fwd:.1f} ms); T = {r['temperature']:.4f}, NLL {r['nll_before']:.4f} -> {r['nll_after']:.4f}")


kernel_legs()
tail_leg()
if '--no-fit' not in args:
    fit_leg()
out = os.path.join(ROOT, 'profiles', 'temperature.txt')
keep = []
if os.path.isfile(out):
    old = open(out).read().splitlines()
    if '## recorded beside the tool' in old:
        keep = old[old.index('## recorded beside the tool'):]
with open(out, 'w') as f:
    f.write('\n'.join([f'# tools/temperature_bench.py on {torch.cuda.get_device_name(0)}'] + lines + keep) + '\n')
print('written', out)

#!/usr/bin/env python3
"""Cost of the label-smoothed cross entropy at the step's shape (N = 8, tail input 256 x 512, 19 -> 19), written to profiles/label_smoothing_ce.txt:
  * kernel-only times through the C ABI, HIP events around back-to-back launches: the four smoothing paths (dsrl_ce_fwd_s + dsrl_ce_bwd_s,
    dsrl_ce_fused_s, dsrl_convt2x2_fwd_ce_s, dsrl_convt2x2_bwd_ce_s) against their _w siblings, eps = 0.1;
  * the replayed training step (stage 3, batch 8, 256 x 512 input, hipGraph): default, class weights, class weights + eps = 0.1, alternating in
    one process.
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/label_smoothing_ce_bench.py [--steps K] [--no-step] [VAR=value ...]"""
import os
import sys
import time

args = [a for a in sys.argv[1:] if '=' not in a]
for kv in sys.argv[1:]:
    if '=' in kv:
        k, v = kv.split('=', 1); os.environ[k] = v
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                                                    # noqa: E402
import torch                                                                                          # noqa: E402
from dualsuperreslearningforsemseg_amd import functional as HF                                        # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import call, query                                        # noqa: E402

dev = 'cuda:0'
STEPS = int(args[args.index('--steps') + 1]) if '--steps' in args else 30
EPS = 0.1
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeit(f, reps=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def kernels():
    N, H, W, C = 8, 256, 512, 19
    P = N * 4 * H * W
    rs = np.random.RandomState(1)
    x = torch.randn(N, H, W, C, device=dev); w = torch.randn(C, C, 2, 2, device=dev) * 0.2; b = torch.randn(C, device=dev)
    y = torch.empty(N, 2 * H, 2 * W, C, device=dev)
    tg = torch.randint(0, C, (N, 2 * H, 2 * W), device=dev, dtype=torch.uint8)
    tg[torch.rand(tg.shape, device=dev) < 0.1] = 255
    wt = HF.class_weight_table(rs.uniform(0.25, 8.0, C), dev)
    dx = torch.empty_like(x); dw = torch.empty_like(w); db = torch.empty(C, device=dev); dl = torch.empty_like(y)
    scal = torch.zeros(8, device=dev); flag = torch.zeros(1, dtype=torch.int32, device=dev); one = torch.ones(1, device=dev)
    ftg = torch.randn(N, H // 4, W // 4, device=dev); ftw = torch.randn(C, device=dev)
    st = HF._stream()

    def ws(name, *a):
        return torch.empty(query(name, *a), dtype=torch.uint8, device=dev)
    wfw = ws('dsrl_convt2x2_fwd_ce_s_workspace_bytes', N, H, W)
    wb = ws('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C)
    wcw = ws('dsrl_ce_fused_s_workspace_bytes', P)
    wa = ws('dsrl_ce_s_workspace_bytes', P)
    t = {}
    t['fwd_ce_w'] = timeit(lambda: call('dsrl_convt2x2_fwd_ce_w', x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), N, H, W, C, C, tg.data_ptr(), 255,
                                        wt.data_ptr(), scal.data_ptr(), flag.data_ptr(), wfw.data_ptr(), wfw.numel(), st))
    t['fwd_ce_s'] = timeit(lambda: call('dsrl_convt2x2_fwd_ce_s', x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), N, H, W, C, C, tg.data_ptr(), 255,
                                        wt.data_ptr(), EPS, scal.data_ptr(), flag.data_ptr(), wfw.data_ptr(), wfw.numel(), st))
    for waves in ('12', '8'):                   # the smoothing backward is the 8-wave build under either setting
        os.environ['DSRL_CONVT_CE_WAVES'] = waves
        t[f'bwd_ce_w/{waves}'] = timeit(lambda: call('dsrl_convt2x2_bwd_ce_w', x.data_ptr(), w.data_ptr(), y.data_ptr(), tg.data_ptr(), 255, wt.data_ptr(),
                                                     scal.data_ptr() + 4, ftg.data_ptr(), ftw.data_ptr(), 8, dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                     N, H, W, C, C, wb.data_ptr(), wb.numel(), st))
        t[f'bwd_ce_s/{waves}'] = timeit(lambda: call('dsrl_convt2x2_bwd_ce_s', x.data_ptr(), w.data_ptr(), y.data_ptr(), tg.data_ptr(), 255, wt.data_ptr(), EPS,
                                                     scal.data_ptr() + 4, ftg.data_ptr(), ftw.data_ptr(), 8, dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                     N, H, W, C, C, wb.data_ptr(), wb.numel(), st))
    os.environ.pop('DSRL_CONVT_CE_WAVES')
    t['ce_fused_w'] = timeit(lambda: call('dsrl_ce_fused_w', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), dl.data_ptr(), C, scal.data_ptr(),
                                          flag.data_ptr(), wcw.data_ptr(), wcw.numel(), st))
    t['ce_fused_s'] = timeit(lambda: call('dsrl_ce_fused_s', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), EPS, dl.data_ptr(), C, scal.data_ptr(),
                                          flag.data_ptr(), wcw.data_ptr(), wcw.numel(), st))
    t['ce_fwd_w'] = timeit(lambda: call('dsrl_ce_fwd_w', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), scal.data_ptr(), wa.data_ptr(), wa.numel(), st))
    t['ce_fwd_s'] = timeit(lambda: call('dsrl_ce_fwd_s', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), EPS, scal.data_ptr(), wa.data_ptr(), wa.numel(), st))
    t['ce_bwd_w'] = timeit(lambda: call('dsrl_ce_bwd_w', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), scal.data_ptr(), one.data_ptr(), dl.data_ptr(), C, st))
    t['ce_bwd_s'] = timeit(lambda: call('dsrl_ce_bwd_s', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), EPS, scal.data_ptr(), one.data_ptr(), dl.data_ptr(),
                                        C, st))
    say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} pixels; eps = {EPS}; mean of 20 back-to-back calls; every call but ce_bwd and')
    say('convt2x2_bwd_ce holds the D pre-pass):')
    say(f"  A  dsrl_ce_fwd            weighted {t['ce_fwd_w']:7.1f}   smoothed {t['ce_fwd_s']:7.1f}   ({t['ce_fwd_s'] - t['ce_fwd_w']:+.1f})")
    say(f"  A  dsrl_ce_bwd            weighted {t['ce_bwd_w']:7.1f}   smoothed {t['ce_bwd_s']:7.1f}   ({t['ce_bwd_s'] - t['ce_bwd_w']:+.1f})")
    say(f"  B  dsrl_ce_fused          weighted {t['ce_fused_w']:7.1f}   smoothed {t['ce_fused_s']:7.1f}   ({t['ce_fused_s'] - t['ce_fused_w']:+.1f})")
    say(f"  C  dsrl_convt2x2_fwd_ce   weighted {t['fwd_ce_w']:7.1f}   smoothed {t['fwd_ce_s']:7.1f}   ({t['fwd_ce_s'] - t['fwd_ce_w']:+.1f})")
    for waves in ('12', '8'):
        a, bb = t[f'bwd_ce_w/{waves}'], t[f'bwd_ce_s/{waves}']
        say(f'  D  dsrl_convt2x2_bwd_ce   weighted {a:7.1f} ({waves:>2} waves)   smoothed {bb:7.1f} (8 waves, DSRL_CONVT_CE_WAVES={waves})   ({bb - a:+.1f})')


def replayed_step():
    import dualsuperreslearningforsemseg_amd as D
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(settings.RANDOM_SEED)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(8, (256, 512), torch.device(dev), length=1)))
    w = np.random.RandomState(2).uniform(0.25, 8.0, cs.NUM_CLASSES)

    def run(step, n):
        for _ in range(n):
            step.enqueue(img, org, tgt, 0.0, 0.9, 0.0, True)      # lr 0: every step trains the same parameters
            while step.pending() > 1:
                step.collect()
        while step.pending():
            step.collect()
    kinds = {'default': (None, 0.0), 'weighted': (w, 0.0), 'smoothed': (w, EPS)}
    res, replays = {k: [] for k in kinds}, {}
    for _ in range(2):                          # one captured step at a time (the device-resident dropout key has one binding): build, warm, time, release
        for k, (cw, e) in kinds.items():
            s = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, class_weights=cw, label_smoothing=e)
            run(s, s.GRAPH_WARMUP + 6)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(s, STEPS)
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / STEPS * 1e3)
            replays[k] = s.graph_replays
            s.release()
    say(f'replayed step (stage 3, batch 8, 256 x 512, {STEPS} steps per figure, two alternating rounds in one process), ms per step:')
    for k in res:
        say(f'  {k:<9} ' + '  '.join(f'{v:.3f}' for v in res[k]) + f'   min {min(res[k]):.3f}  (replays {replays[k]})')
    say(f"  smoothed - weighted (min): {(min(res['smoothed']) - min(res['weighted'])) * 1e3:+.0f} us;  smoothed - default (min): "
        f"{(min(res['smoothed']) - min(res['default'])) * 1e3:+.0f} us")


kernels()
if '--no-step' not in args:
    replayed_step()
out = os.path.join(ROOT, 'profiles', 'label_smoothing_ce.txt')
os.makedirs(os.path.dirname(out), exist_ok=True)
KEEP = '## recorded beside the tool'            # the same-box A/B against the parent commit and the kernel resource tables: kept across runs
tail = ''
if os.path.isfile(out):
    old = open(out).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

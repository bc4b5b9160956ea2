#!/usr/bin/env python3
"""Inference tail, A/B in one process: A = the unfused way to a class map (upsample16_pred[2:] modules in eval mode + torch.argmax; with a target also
dsrl_seg_metrics + HF.cross_entropy), B = functional.sssr_tail_predict (one launch).  Alternating windows of >= --window seconds of device work each,
device events around every window, after a warm-up of both sides at that shape.  Bytes and FLOPs are counted from the shapes here; the floor of B is
the larger of FLOPs / fp32 matrix rate and bytes / HBM rate.  One more table: DSRL.predict against DSRL.forward + arg-max for the whole stage-1 model.

    python tools/predict_bench.py [--out FILE] [--window 0.5] [--rounds 3]

--flip measures the horizontal-flip ensemble instead (profiles/predict_flip.txt), at tail input 256x512, batch 1 and 8:
  (a) the two-view tail (dsrl_sssr_tail_predict_flip) against the unfused composition on the same 2N tail input (modules, two sets of logits, torch
      log_softmax / flip / logaddexp / argmax, with a target also dsrl_seg_metrics and the loss),
  (b) the two-view tail on N class maps against the single-view tail on 2N images: the same input bytes and MFMAs, so the ratio is the price of the two
      softmaxes per output pixel,
  (c) DSRL.predict(flip=True) on N images against DSRL.predict on 2N: eager, on frozen operands, and replayed from the hipGraph,
and lists the registers of the tail kernels (tools/kernel_resources.py on the built library).

    python tools/predict_bench.py --flip [--out profiles/predict_flip.txt]

--confusion measures the device confusion matrix (profiles/predict_confusion.txt), at tail input 256x512, batch 1 and 8, plain and flip, with a target,
on uniform labels and on labels / predictions that are class 0 on ~90 % of the pixels:
  (a) the tail with counters and loss and no `confusion` (with --baseline only this: the form that also runs on a tree without the feature),
  (b) the same call with `confusion`, (c) the two-launch composition: (a), then dsrl_confusion_matrix on its class map,
  (d) dsrl_confusion_matrix alone on 8x1024x2048 pixels against the time 2 bytes per pixel take at the HBM rate,
  (e) dsrl_seg_metrics_cm against dsrl_seg_metrics on 8x19x512x1024 logits.

    python tools/predict_bench.py --confusion [--baseline] [--out profiles/predict_confusion.txt]

--multiscale measures the multi-scale ensemble (profiles/predict_multiscale.txt) on 256x512 images, batch 1 and 8, scales 0.5 ... 1.75, plain and flip:
  (a) the merge launches alone (functional.multiscale_merge, all views) against torch interpolate / softmax / add / argmax on the same logits, with
      the peak memory of each,
  (b) one dsrl_prob_merge launch against the bytes it must move (accumulator read + write + logits once), beside a dsrl_copy2d of as many bytes,
  (c) DSRL.predict(scales=...) against the sum of DSRL.predict calls on the same view sizes,
and lists the registers of the merge kernels.

    python tools/predict_bench.py --multiscale [--out profiles/predict_multiscale.txt]

--window WITHOUT a value measures sliding-window inference (profiles/predict_window.txt) on 512x1024 images, batch 1 and 8, window 256x512 at the default
stride (3 x 3 positions), plain and flip (timing windows of --seconds, default 0.5):
  (a) the merge and finish launches (functional.window_merge, all views) against the torch composition on the same logits (softmax, add into a canvas,
      divide by a count map, argmax), alternating in one call, with the peak memory of each,
  (b) one dsrl_window_merge launch and the dsrl_window_merge_finish launch against the bytes they must move, beside a dsrl_copy2d of as many bytes,
  (c) DSRL.predict(window=...) against the nine DSRL.predict calls on the crops,
  (d) the default DSRL.predict (256x512, batch 8) and the default train step (bench.py --gpus 1) of this tree against the parent commit in its own
      tree with its own library under ab/prev_tree (as tools/ab_tree.sh), each round parent, this, parent again; skipped, and said so, without it,
and lists the registers of the window kernels.

    python tools/predict_bench.py --window [--out profiles/predict_window.txt]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dualsuperreslearningforsemseg_amd import functional as HF                        # noqa: E402
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS       # noqa: E402
from dualsuperreslearningforsemseg_amd.metrices import _Counts                         # noqa: E402
from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL                         # noqa: E402
from dualsuperreslearningforsemseg_amd.nn_modules import HipSequential                 # noqa: E402

NC = 19
HBM_BPS, F32_MATRIX_FLOPS = 6.29e12, 155e12            # measured rates of the MI355X (MFMA f32 16x16x4 / 32x32x2)
MACS_PER_PIXEL = NC * 4 * NC + 4 * NC * 4 * NC           # 2x2 mid pixels, then 2x2 logits of each: 7220


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


def ab(a, b, seconds, rounds):
    for _ in range(3):
        a(); b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(a, seconds)); tb.append(window(b, seconds))
    return ta, tb


def _row(say, label, ta, tb, unit_scale=1e3, unit='us', extra=''):
    ma, mb = sum(ta) / len(ta), sum(tb) / len(tb)
    d = 1 if unit == 'us' else 3
    say(f'{label}:  A {ma * unit_scale:9.{d}f} {unit} [{", ".join(f"{t * unit_scale:.{d}f}" for t in ta)}]   B {mb * unit_scale:9.{d}f} {unit} '
        f'[{", ".join(f"{t * unit_scale:.{d}f}" for t in tb)}]   A/B {ma / mb:5.3f}{extra}')
    return ma, mb


def flip_main(args):
    import kernel_resources as KR
    from dualsuperreslearningforsemseg_amd import _lib
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(7)
    up = DSRL._define_SSSR_decoder(256, 48, 256, NC)['upsample16_pred'].to(dev).eval()
    with torch.no_grad():
        up[3].running_mean.normal_(0, 0.1); up[3].running_var.uniform_(0.5, 1.5)
    tail = HipSequential(*list(up)[2:]).eval()
    H, W = 256, 512
    say(f'Horizontal-flip ensemble, {torch.cuda.get_device_name(0)}, tail input {H}x{W}; windows of >= {args.window} s per side, {args.rounds} alternations '
        f'A B A B ..; mean [each window]')
    say()
    say('(a) A = unfused composition on the 2N tail input (modules -> two sets of logits -> torch log_softmax, flip, logaddexp, argmax; with a target also '
        'dsrl_seg_metrics + HF.cross_entropy of the scores), B = dsrl_sssr_tail_predict_flip')
    slower = []
    for with_target in (False, True):
        for N in (1, 8):
            x = torch.randn(2 * N, NC, H, W, device=dev).contiguous(memory_format=torch.channels_last)
            target = torch.randint(0, NC, (N, 4 * H, 4 * W), device=dev, dtype=torch.uint8) if with_target else None
            if with_target:
                target[torch.rand(target.shape, device=dev) < 0.1] = 255
            counter = _Counts(NC)

            def a():
                with torch.no_grad():
                    scores = HF._flip_ensemble(tail(x))
                    pred = torch.argmax(scores, dim=1)
                    if not with_target:
                        return pred
                    counter.batches = []
                    counter.add_logits(scores, target)
                    return pred, counter.batches[0], HF.cross_entropy(scores, target, 255)

            def b():
                if not with_target:
                    return HF.sssr_tail_predict(x, up[2], up[3], up[6], flip=True)
                counts = torch.zeros(3 * NC + 2, dtype=torch.int64, device=dev)
                return HF.sssr_tail_predict(x, up[2], up[3], up[6], target=target, counts=counts, flip=True), counts

            ta, tb = ab(a, b, args.window, args.rounds)
            mem_a, mem_b = peak_bytes(a), peak_bytes(b)
            ma, mb = _row(say, f'N={N} target={"yes" if with_target else "no "}', ta, tb,
                          extra=f'   peak memory A {mem_a / 1e6:8.1f} MB  B {mem_b / 1e6:6.2f} MB')
            if mb > ma:
                slower.append(('a', N, with_target))
    say()
    say('(b) A = dsrl_sssr_tail_predict on 2N images (2N class maps), B = dsrl_sssr_tail_predict_flip on the same 2N images (N class maps): '
        'the same input bytes and MFMAs; B/A is the price of the two softmaxes per output pixel')
    for with_target in (False, True):
        for N in (1, 8):
            x = torch.randn(2 * N, NC, H, W, device=dev).contiguous(memory_format=torch.channels_last)
            t2 = torch.randint(0, NC, (2 * N, 4 * H, 4 * W), device=dev, dtype=torch.uint8) if with_target else None
            t1 = t2[:N].contiguous() if with_target else None

            def a():
                return HF.sssr_tail_predict(x, up[2], up[3], up[6], target=t2)

            def b():
                return HF.sssr_tail_predict(x, up[2], up[3], up[6], target=t1, flip=True)

            ta, tb = ab(a, b, args.window, args.rounds)
            ma, mb = _row(say, f'N={N} target={"yes" if with_target else "no "}', ta, tb)
            px = 2 * N * H * W
            say(f'      B/A {mb / ma:5.2f};  B: {2.0 * MACS_PER_PIXEL * px / (mb * 1e-3) / 1e12:6.2f} TFLOP/s of MFMA work, {38 * 8 * px / (mb * 1e-3) / 1e9:7.1f} G exp/s '
                f'(floor of the MFMAs at {F32_MATRIX_FLOPS / 1e12:.0f} TF: {2.0 * MACS_PER_PIXEL * px / F32_MATRIX_FLOPS * 1e6:6.1f} us)')
    say()
    say('(c) whole model (stage 1, random weights, eval, 256x512 input, caller-owned nan_flag: no readback): A = predict on 2N images, B = predict(flip=True) on N')
    model = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
    flag = torch.zeros((), dtype=torch.int32, device=dev)
    for N in (1, 8):
        img = torch.randn(N, 3, 256, 512, device=dev).contiguous(memory_format=torch.channels_last)
        img2 = torch.cat([img, img.flip(3)]).contiguous(memory_format=torch.channels_last)
        ta, tb = ab(lambda: model.predict(img2, nan_flag=flag)[0], lambda: model.predict(img, nan_flag=flag, flip=True)[0], args.window, args.rounds)
        _row(say, f'batch {N} eager ', ta, tb, 1.0, 'ms', f'   peak memory A {peak_bytes(lambda: model.predict(img2, nan_flag=flag)[0]) / 1e6:8.1f} MB  '
             f'B {peak_bytes(lambda: model.predict(img, nan_flag=flag, flip=True)[0]) / 1e6:8.1f} MB')
        for graph, name in ((False, 'frozen'), (True, 'replay')):
            cp = model.compile_predict(graph=graph)
            try:
                ta, tb = ab(lambda: cp(img2, nan_flag=flag, copy=False)[0], lambda: cp(img, nan_flag=flag, copy=False, flip=True)[0], args.window, args.rounds)
                _row(say, f'batch {N} {name} ', ta, tb, 1.0, 'ms', f'   graphs {cp.num_graphs}')
            finally:
                cp.release()
    say()
    say('rows of (a) where B is slower than A: ' + (', '.join(str(r) for r in slower) if slower else 'none'))
    say()
    say('kernel resources (tools/kernel_resources.py on libdsrl_hip.so):')
    ks = KR.kernels(_lib.LIB_PATH)
    for k, n in zip(ks, KR.demangle([k['name'] for k in ks])):
        if 'sssr_tail_predict' in n:
            say(f"vgpr {k.get('vgpr', 0):3d} agpr {k.get('agpr', 0):3d} sgpr {k.get('sgpr', 0):3d} scratch {k.get('scratch', 0):5d} B  spills v{k.get('vgpr_spill', 0)} "
                f"s{k.get('sgpr_spill', 0)}  lds {k.get('lds', 0):6d}  {n[:110]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def _spread(ts):
    return (max(ts) - min(ts)) / (sum(ts) / len(ts))


def confusion_main(args):
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def windows(fns):
        """alternating windows over `fns` -> one list of ms per call for each"""
        for f in fns:
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(args.rounds):
            for i, f in enumerate(fns):
                ts[i].append(window(f, args.window))
        return ts

    def fmt(ts):
        return f'{sum(ts) / len(ts) * 1e3:8.1f} us [{", ".join(f"{t * 1e3:.1f}" for t in ts)}] spread {100 * _spread(ts):4.1f} %'

    torch.manual_seed(7)
    up = DSRL._define_SSSR_decoder(256, 48, 256, NC)['upsample16_pred'].to(dev).eval()
    with torch.no_grad():
        up[3].running_mean.normal_(0, 0.1); up[3].running_var.uniform_(0.5, 1.5)
    torch.manual_seed(7)
    skew = DSRL._define_SSSR_decoder(256, 48, 256, NC)['upsample16_pred'].to(dev).eval()         # the same tail, class 0 pushed up: ~all predictions 0
    with torch.no_grad():
        skew[3].running_mean.copy_(up[3].running_mean); skew[3].running_var.copy_(up[3].running_var)
        skew[6].bias[0] += 20.0
    H, W = 256, 512
    say(f'Device confusion matrix, {torch.cuda.get_device_name(0)}, tail input {H}x{W} with a target; windows of >= {args.window} s per side, {args.rounds} '
        f'alternations; us per call: mean [each window], spread = (max - min) / mean of the windows')
    say()
    say('(a) tail with counters and loss, no confusion' + ('' if args.baseline else
        ';  (b) the same launch with confusion;  (c) (a) followed by dsrl_confusion_matrix on its class map'))
    for labels, head in (('uniform', up), ('90 % class 0', skew)):
        for flip in (False, True):
            for N in (1, 8):
                x = torch.randn((2 if flip else 1) * N, NC, H, W, device=dev).contiguous(memory_format=torch.channels_last)
                target = torch.randint(0, NC, (N, 4 * H, 4 * W), device=dev, dtype=torch.uint8)
                if labels != 'uniform':
                    target[torch.rand(target.shape, device=dev) < 0.9] = 0
                target[torch.rand(target.shape, device=dev) < 0.1] = 255
                counts = torch.zeros(3 * NC + 2, dtype=torch.int64, device=dev)
                cm = torch.zeros(NC * NC, dtype=torch.int64, device=dev)
                mods = (head[2], head[3], head[6])

                def a():
                    return HF.sssr_tail_predict(x, *mods, target=target, counts=counts, flip=flip)

                def b():
                    return HF.sssr_tail_predict(x, *mods, target=target, counts=counts, flip=flip, confusion=cm)

                def c():
                    out = HF.sssr_tail_predict(x, *mods, target=target, counts=counts, flip=flip)
                    HF.confusion_matrix_(cm, out[0], target, NC)
                    return out

                label = f'{labels:13s} {"flip " if flip else "plain"} N={N}'
                if args.baseline:
                    say(f'{label}:  (a) {fmt(windows([a])[0])}')
                    continue
                ta, tb, tc = windows([a, b, c])
                ma, mb, mc = (sum(t) / len(t) for t in (ta, tb, tc))
                say(f'{label}:  (a) {fmt(ta)}')
                say(f'{"":25s}  (b) {fmt(tb)}   (b) - (a) {(mb - ma) * 1e3:+7.1f} us ({100 * (mb - ma) / ma:+5.1f} %)')
                say(f'{"":25s}  (c) {fmt(tc)}   (c) - (b) {(mc - mb) * 1e3:+7.1f} us: the fusion {"pays" if mb <= mc else "DOES NOT PAY"}')
    if not args.baseline:
        say()
        P = 8 * 1024 * 2048
        floor = 2.0 * P / HBM_BPS
        say(f'(d) dsrl_confusion_matrix alone, {P} pixels; 2 bytes per pixel at {HBM_BPS / 1e12:.2f} TB/s: {floor * 1e6:.1f} us')
        cm = torch.zeros(NC * NC, dtype=torch.int64, device=dev)
        for labels in ('uniform', '90 % class 0'):
            tg = torch.randint(0, NC, (P,), device=dev, dtype=torch.uint8)
            pr = torch.where(torch.rand(P, device=dev) < 0.7, tg, torch.randint(0, NC, (P,), device=dev, dtype=torch.uint8))
            if labels != 'uniform':
                m = torch.rand(P, device=dev) < 0.9
                tg[m] = 0; pr[m] = 0
            tg[torch.rand(P, device=dev) < 0.1] = 255
            (td,) = windows([lambda: HF.confusion_matrix_(cm, pr, tg, NC)])
            md = sum(td) / len(td)
            say(f'{labels:13s}:  {fmt(td)}   {2.0 * P / (md * 1e-3) / 1e12:5.2f} TB/s, {100 * floor / (md * 1e-3):.0f} % of the HBM rate')
        say()
        say('(e) A = dsrl_seg_metrics, B = dsrl_seg_metrics_cm (counts and matrix) on 8x19x512x1024 logits')
        from dualsuperreslearningforsemseg_amd._lib import call
        logits = torch.randn(8, NC, 512, 1024, device=dev).contiguous(memory_format=torch.channels_last)
        tg = torch.randint(0, NC, (8, 512, 1024), device=dev, dtype=torch.uint8)
        tg[torch.rand(tg.shape, device=dev) < 0.1] = 255
        counts = torch.zeros(3 * NC + 2, dtype=torch.int64, device=dev)
        Pl = 8 * 512 * 1024
        ta, tb = windows([lambda: call('dsrl_seg_metrics', logits.data_ptr(), NC, tg.data_ptr(), Pl, NC, 255, counts.data_ptr(), HF._stream()),
                          lambda: call('dsrl_seg_metrics_cm', logits.data_ptr(), NC, tg.data_ptr(), Pl, NC, 255, counts.data_ptr(), cm.data_ptr(), HF._stream())])
        ma, mb = sum(ta) / len(ta), sum(tb) / len(tb)
        say(f'A {fmt(ta)}')
        say(f'B {fmt(tb)}   B - A {(mb - ma) * 1e3:+7.1f} us ({100 * (mb - ma) / ma:+5.1f} %)')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


MS_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def multiscale_main(args):
    import kernel_resources as KR
    from dualsuperreslearningforsemseg_amd import _lib
    from dualsuperreslearningforsemseg_amd._lib import call
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def fmt(ts, scale=1e3, unit='us'):
        return f'{sum(ts) / len(ts) * scale:9.1f} {unit} [{", ".join(f"{t * scale:.1f}" for t in ts)}]'

    H, W = 256, 512
    Ho, Wo = 2 * H, 2 * W
    sizes = HF.multiscale_sizes(H, W, MS_SCALES)
    say(f'Multi-scale ensemble, {torch.cuda.get_device_name(0)}, images {H}x{W} (class maps {Ho}x{Wo}), scales {MS_SCALES} -> views of '
        f'{", ".join(f"{h}x{w}" for h, w in sizes)}; windows of >= {args.window} s per side, {args.rounds} alternations A B A B ..; mean [each window]')
    say()
    say('(a) the merge alone, on the same logits (random normal, one (N,19,2h,2w) tensor per view; with flip two per scale, the second mirrored): '
        'A = torch interpolate(align_corners=True) -> softmax -> add per view, then argmax; B = functional.multiscale_merge (dsrl_prob_merge for all but '
        'the last view, dsrl_prob_merge_finish)')
    slower = []
    for flip in (False, True):
        for N in (1, 8):
            views = [(torch.randn(N, NC, 2 * h, 2 * w, device=dev).contiguous(memory_format=torch.channels_last), bool(v))
                     for h, w in sizes for v in range(2 if flip else 1)]

            def a():
                with torch.no_grad():
                    total = None
                    for L, m in views:
                        p = torch.softmax(torch.nn.functional.interpolate(L.flip(3) if m else L, size=(Ho, Wo), mode='bilinear', align_corners=True), dim=1)
                        total = p if total is None else total.add_(p)
                    return torch.argmax(total, dim=1)

            def b():
                return HF.multiscale_merge(views, (Ho, Wo))[0]

            ta, tb = ab(a, b, args.window, args.rounds)
            mem_a, mem_b = peak_bytes(a), peak_bytes(b)
            agree = (a() == b()).float().mean().item()
            ma, mb = _row(say, f'N={N} {"flip " if flip else "plain"} {len(views):2d} views', ta, tb,
                          extra=f'   peak memory A {mem_a / 1e6:8.1f} MB  B {mem_b / 1e6:7.1f} MB   class maps agree at {100 * agree:.3f} %')
            if mb > ma:
                slower.append((N, flip))
            del views
    say('rows where B is slower than A: ' + (', '.join(str(r) for r in slower) if slower else 'none'))
    say()
    say('(b) dsrl_prob_merge, one launch that adds a view (first = 0): bytes it must move = accumulator read + write + the view\'s logits once; beside it '
        'dsrl_copy2d moving the same number of bytes (half read, half written)')
    for N in (1, 8):
        acc = torch.zeros(_lib.query('dsrl_prob_merge_acc_bytes', N, Ho, Wo, NC) // 4, device=dev)
        for h, w in (sizes[0], sizes[2], sizes[5]):
            L = torch.randn(N, NC, 2 * h, 2 * w, device=dev).contiguous(memory_format=torch.channels_last)
            nbytes = 2 * acc.numel() * 4 + L.numel() * 4
            rows = nbytes // (2 * 4 * 64)
            src, dst = torch.randn(rows * 64, device=dev), torch.empty(rows * 64, device=dev)
            st = HF._stream()
            tm, tc = ab(lambda: call('dsrl_prob_merge', L.data_ptr(), NC, N, 2 * h, 2 * w, NC, 0, acc.data_ptr(), Ho, Wo, 0, st),
                        lambda: call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, rows, 64, st), args.window, args.rounds)
            mm, mc = sum(tm) / len(tm), sum(tc) / len(tc)
            say(f'N={N} view {2 * h}x{2 * w}: {nbytes / 1e6:7.1f} MB   merge {fmt(tm)} = {nbytes / (mm * 1e-3) / 1e12:5.2f} TB/s   copy2d {fmt(tc)} = '
                f'{nbytes / (mc * 1e-3) / 1e12:5.2f} TB/s   ({100 * mc / mm:.0f} % of the copy\'s rate; HBM {HBM_BPS / 1e12:.2f} TB/s)')
            acc.zero_()
            del L, src, dst
        del acc
    say()
    say('(c) whole model (stage 1, random weights, eval, caller-owned nan_flag: no readback): A = the sum of DSRL.predict calls on the same view sizes '
        '(class maps only; what the trunk and the fused tail cost), B = DSRL.predict(scales=...) (logits written, merged, released per scale)')
    model = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
    flag = torch.zeros((), dtype=torch.int32, device=dev)
    for flip in (False, True):
        for N in (1, 8):
            img = torch.randn(N, 3, H, W, device=dev).contiguous(memory_format=torch.channels_last)
            resized = [HF.resize_image_ac(img, s) for s in sizes]

            def a():
                return [model.predict(r, nan_flag=flag, flip=flip)[0] for r in resized]

            def b():
                return model.predict(img, nan_flag=flag, flip=flip, scales=MS_SCALES)[0]

            ta, tb = ab(a, b, args.window, args.rounds)
            _row(say, f'batch {N} {"flip " if flip else "plain"}', ta, tb, 1.0, 'ms',
                 f'   peak memory A {peak_bytes(a) / 1e6:8.1f} MB  B {peak_bytes(b) / 1e6:8.1f} MB   single-scale predict '
                 f'{window(lambda: model.predict(img, nan_flag=flag, flip=flip)[0], args.window):7.3f} ms')
    say()
    say('kernel resources (tools/kernel_resources.py on libdsrl_hip.so):')
    ks = KR.kernels(_lib.LIB_PATH)
    for k, n in zip(ks, KR.demangle([k['name'] for k in ks])):
        if 'prob_merge' in n:
            say(f"vgpr {k.get('vgpr', 0):3d} agpr {k.get('agpr', 0):3d} sgpr {k.get('sgpr', 0):3d} scratch {k.get('scratch', 0):5d} B  spills v{k.get('vgpr_spill', 0)} "
                f"s{k.get('sgpr_spill', 0)}  lds {k.get('lds', 0):6d}  {n[:110]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


WIN_IMAGE, WIN_SIZE = (512, 1024), (256, 512)
# (d): what a fresh process runs in each tree: the default predict on a 256x512 batch of 8, ms per call over three windows
_PREDICT_PROBE = '''
import sys, torch
sys.path.insert(0, "tools"); sys.path.insert(0, ".")
import predict_bench as PB
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
torch.manual_seed(7)
dev = torch.device("cuda:0")
model = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
flag = torch.zeros((), dtype=torch.int32, device=dev)
img = torch.randn(8, 3, 256, 512, device=dev).contiguous(memory_format=torch.channels_last)
fn = lambda: model.predict(img, nan_flag=flag)[0]
for _ in range(5):
    fn()
print("PREDICT_MS", min(PB.window(fn, 0.5) for _ in range(3)), int(fn().sum().item()))
'''


def window_against_parent(say, steps=30, rounds=2):
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prev = os.path.join(root, 'ab', 'prev_tree')
    say(f'(d) this tree against the parent commit (its own tree and library under ab/prev_tree), fresh processes, each round parent, this, parent again: '
        f'the default DSRL.predict (stage 1, 256x512, batch 8, best of three windows, ms per call) and the default replayed train step '
        f'(bench.py --gpus 1 --steps {steps} --warmup 8, ms per step)')
    if not os.path.isfile(os.path.join(prev, 'bench.py')):
        say('    NOT MEASURED: no parent tree under ab/prev_tree')
        return

    def predict_ms(tree):
        r = subprocess.run([sys.executable, '-c', _PREDICT_PROBE], cwd=tree, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f'the predict probe in {tree} ended with {r.returncode}: {r.stderr[-400:]}')
        w = [ln for ln in r.stdout.splitlines() if ln.startswith('PREDICT_MS')][-1].split()
        return float(w[1]), w[2]

    def step_ms(tree):
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '8'], cwd=tree, capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f'bench.py in {tree} ended with {r.returncode}: {r.stderr[-400:]}')
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
        return float(d['ms_per_step']), json.dumps(d['config']['losses_last_step'])

    for name, probe in (('default predict', predict_ms), ('default train step', step_ms)):
        parent, this, marks = [], [], set()
        for r in range(rounds):
            (a, ma), (b, mb), (c, mc) = probe(prev), probe(root), probe(prev)
            parent += [a, c]; this.append(b)
            marks |= {ma, mb, mc}
            say(f'    {name}, round {r + 1}: parent {a:.3f}  this {b:.3f}  parent-again {c:.3f}')
        pm, tm = sum(parent) / len(parent), sum(this) / len(this)
        say(f'    {name}: parent {min(parent):.3f} .. {max(parent):.3f} (spread {max(parent) - min(parent):.3f}, mean {pm:.3f}); this {min(this):.3f} .. '
            f'{max(this):.3f} (mean {tm:.3f}); this - parent mean {tm - pm:+.3f} ms: '
            + ('inside' if min(parent) <= tm <= max(parent) else 'BELOW (faster than)' if tm < min(parent) else 'ABOVE (slower than)')
            + " the parent's own spread; results (class-map checksum / losses of the last step) "
            + ('identical in all runs' if len(marks) == 1 else 'DIFFERENT: ' + ' '.join(sorted(marks))))


def window_main(args):
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    seconds = args.seconds
    say(f'Sliding-window inference: images {WIN_IMAGE[0]}x{WIN_IMAGE[1]}, window {WIN_SIZE[0]}x{WIN_SIZE[1]}, default stride; timing windows of >= '
        f'{seconds} s per side, {args.rounds} alternations A B A B ..; mean [each window]')
    say()
    window_against_parent(say)              # before this process opens the device: one bench at a time has it to itself
    say()
    import kernel_resources as KR
    from dualsuperreslearningforsemseg_amd import _lib
    from dualsuperreslearningforsemseg_amd._lib import call
    import ctypes
    dev = torch.device('cuda:0')

    def fmt(ts, scale=1e3, unit='us'):
        return f'{sum(ts) / len(ts) * scale:9.1f} {unit} [{", ".join(f"{t * scale:.1f}" for t in ts)}]'

    H, W = WIN_IMAGE
    (h, w), stride = HF.window_value(WIN_SIZE)
    ys, xs = HF.window_plan(H, W, WIN_SIZE)
    Ho, Wo, hw, ww = 2 * H, 2 * W, 2 * h, 2 * w
    oys, oxs = tuple(2 * y for y in ys), tuple(2 * x for x in xs)
    say(f'{torch.cuda.get_device_name(0)}; stride {stride[0]}x{stride[1]} -> positions y {ys} x {xs}: {len(ys)} x {len(xs)}; class maps {Ho}x{Wo}, a window\'s logits '
        f'{hw}x{ww}')
    say()
    say('(a) the merge alone, on the same logits (random normal, one (N,19,2h,2w) tensor per view; with flip two per position, the second mirrored): '
        'A = torch softmax -> add into a zeroed canvas per view, divide by the count map, argmax; B = functional.window_merge (dsrl_window_merge per '
        'view, dsrl_window_merge_finish)')
    slower = []
    for flip in (False, True):
        vpp = 2 if flip else 1
        for N in (1, 8):
            views = [torch.randn(N, NC, hw, ww, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(len(ys) * len(xs) * vpp)]
            cnt = torch.zeros(Ho, Wo, device=dev)
            for y in oys:
                for x in oxs:
                    cnt[y:y + hw, x:x + ww] += vpp

            def a():
                with torch.no_grad():
                    canvas = torch.zeros(N, NC, Ho, Wo, device=dev)
                    for k, L in enumerate(views):
                        pos, v = divmod(k, vpp)
                        i, j = divmod(pos, len(oxs))
                        canvas[:, :, oys[i]:oys[i] + hw, oxs[j]:oxs[j] + ww] += torch.softmax(L.flip(3) if v else L, dim=1)
                    return torch.argmax(canvas / cnt, dim=1)

            def b():
                return HF.window_merge(views, oys, oxs, (Ho, Wo), flip=flip)[0]

            ta, tb = ab(a, b, seconds, args.rounds)
            mem_a, mem_b = peak_bytes(a), peak_bytes(b)
            agree = (a() == b()).float().mean().item()
            ma, mb = _row(say, f'N={N} {"flip " if flip else "plain"} {len(views):2d} views', ta, tb,
                          extra=f'   peak memory A {mem_a / 1e6:8.1f} MB  B {mem_b / 1e6:7.1f} MB   class maps agree at {100 * agree:.3f} %')
            if mb > ma:
                slower.append((N, flip))
            del views
    say('rows where B is slower than A: ' + (', '.join(str(r) for r in slower) if slower else 'none'))
    say()
    say('(b) bytes per launch.  dsrl_window_merge that ADDS a whole window (fresh_y = window rows): window area of the accumulator read + written + the '
        'logits once; one that STORES it (fresh 0, 0): written + logits; dsrl_window_merge_finish: the accumulator read + one byte of class map per pixel.  '
        'Beside each a dsrl_copy2d moving the same number of bytes (half read, half written)')
    cy, cx = (ctypes.c_int * len(oys))(*oys), (ctypes.c_int * len(oxs))(*oxs)
    for N in (1, 8):
        acc = torch.zeros(_lib.query('dsrl_prob_merge_acc_bytes', N, Ho, Wo, NC) // 4, device=dev)
        pred = torch.empty((N, Ho, Wo), device=dev, dtype=torch.uint8)
        L = torch.randn(N, NC, hw, ww, device=dev).contiguous(memory_format=torch.channels_last)
        st = HF._stream()
        for label, nbytes, fn in (
                ('merge, add  ', 3 * L.numel() * 4, lambda: call('dsrl_window_merge', L.data_ptr(), NC, N, hw, ww, NC, 0, acc.data_ptr(), Ho, Wo, oys[1], oxs[1], hw, 0, st)),
                ('merge, store', 2 * L.numel() * 4, lambda: call('dsrl_window_merge', L.data_ptr(), NC, N, hw, ww, NC, 0, acc.data_ptr(), Ho, Wo, oys[1], oxs[1], 0, 0, st)),
                ('finish      ', acc.numel() * 4 + pred.numel(), lambda: call('dsrl_window_merge_finish', acc.data_ptr(), N, NC, Ho, Wo, cy, len(oys), cx, len(oxs),
                                                                              hw, ww, 1, pred.data_ptr(), None, 255, None, None, None, None, 0, None, st))):
            rows = nbytes // (2 * 4 * 64)
            src, dst = torch.randn(rows * 64, device=dev), torch.empty(rows * 64, device=dev)
            tm, tc = ab(fn, lambda: call('dsrl_copy2d', src.data_ptr(), 64, dst.data_ptr(), 64, rows, 64, st), seconds, args.rounds)
            mm, mc = sum(tm) / len(tm), sum(tc) / len(tc)
            say(f'N={N} {label}: {nbytes / 1e6:7.1f} MB   launch {fmt(tm)} = {nbytes / (mm * 1e-3) / 1e12:5.2f} TB/s   copy2d {fmt(tc)} = '
                f'{nbytes / (mc * 1e-3) / 1e12:5.2f} TB/s   ({100 * mc / mm:.0f} % of the copy\'s rate; HBM {HBM_BPS / 1e12:.2f} TB/s)')
            del src, dst
        del acc, L, pred
    say()
    say('(c) whole model (stage 1, random weights, eval, caller-owned nan_flag: no readback): A = the nine DSRL.predict calls on the crops (class maps '
        'only: what the trunk and the fused tail cost), B = DSRL.predict(window=...) (logits written, merged, released per position)')
    model = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
    flag = torch.zeros((), dtype=torch.int32, device=dev)
    for flip in (False, True):
        for N in (1, 8):
            img = torch.randn(N, 3, H, W, device=dev).contiguous(memory_format=torch.channels_last)
            crops = [img[:, :, y:y + h, x:x + w].contiguous(memory_format=torch.channels_last) for y in ys for x in xs]

            def a():
                return [model.predict(c, nan_flag=flag, flip=flip)[0] for c in crops]

            def b():
                return model.predict(img, nan_flag=flag, flip=flip, window=WIN_SIZE)[0]

            ta, tb = ab(a, b, seconds, args.rounds)
            _row(say, f'batch {N} {"flip " if flip else "plain"}', ta, tb, 1.0, 'ms',
                 f'   peak memory A {peak_bytes(a) / 1e6:8.1f} MB  B {peak_bytes(b) / 1e6:8.1f} MB   whole-image predict '
                 f'{window(lambda: model.predict(img, nan_flag=flag, flip=flip)[0], seconds):7.3f} ms')
    say()
    say('kernel resources (tools/kernel_resources.py on libdsrl_hip.so):')
    ks = KR.kernels(_lib.LIB_PATH)
    for k, n in zip(ks, KR.demangle([k['name'] for k in ks])):
        if 'window_merge' in n or 'window_finish' in n:
            say(f"vgpr {k.get('vgpr', 0):3d} agpr {k.get('agpr', 0):3d} sgpr {k.get('sgpr', 0):3d} scratch {k.get('scratch', 0):5d} B  spills v{k.get('vgpr_spill', 0)} "
                f"s{k.get('sgpr_spill', 0)}  lds {k.get('lds', 0):6d}  {n[:110]}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--window', type=float, nargs='?', default=0.5, const=None,
                    help='seconds of device work per timing window; WITHOUT a value: measure sliding-window inference (profiles/predict_window.txt)')
    ap.add_argument('--seconds', type=float, default=0.5, help='with a bare --window: seconds of device work per timing window')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--flip', action='store_true', help='measure the horizontal-flip ensemble (profiles/predict_flip.txt)')
    ap.add_argument('--confusion', action='store_true', help='measure the device confusion matrix (profiles/predict_confusion.txt)')
    ap.add_argument('--baseline', action='store_true', help='with --confusion: only (a), the calls a tree without the feature also has')
    ap.add_argument('--multiscale', action='store_true', help='measure the multi-scale ensemble (profiles/predict_multiscale.txt)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'predict_bench.py measures on the GPU only'
    if args.window is None:
        return window_main(args)
    if args.multiscale:
        return multiscale_main(args)
    if args.confusion:
        return confusion_main(args)
    if args.flip:
        return flip_main(args)
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(7)
    up = DSRL._define_SSSR_decoder(256, 48, 256, NC)['upsample16_pred'].to(dev).eval()
    with torch.no_grad():
        up[3].running_mean.normal_(0, 0.1); up[3].running_var.uniform_(0.5, 1.5)
    tail = HipSequential(*list(up)[2:]).eval()
    say(f'SSSR inference tail, {torch.cuda.get_device_name(0)}: A = ConvT -> BN/ReLU -> ConvT modules + torch.argmax (+ dsrl_seg_metrics + HF.cross_entropy with a target), '
        f'B = dsrl_sssr_tail_predict')
    say(f'windows of >= {args.window} s per side, {args.rounds} alternations A B A B ..; times in us per call: mean [each window]; rates of B from the bytes / FLOPs '
        f'the algorithm needs; floor = max(FLOPs / {F32_MATRIX_FLOPS / 1e12:.0f} TF, bytes / {HBM_BPS / 1e12:.2f} TB/s)')
    say()
    losses = []
    for with_target in (False, True):
        for (N, H, W) in ((1, 128, 256), (8, 128, 256), (1, 256, 512), (8, 256, 512)):
            px = N * H * W
            x = torch.randn(N, NC, H, W, device=dev).contiguous(memory_format=torch.channels_last)
            target = torch.randint(0, NC, (N, 4 * H, 4 * W), device=dev, dtype=torch.uint8) if with_target else None
            if with_target:
                target[torch.rand(target.shape, device=dev) < 0.1] = 255
            counter = _Counts(NC)

            def a():
                with torch.no_grad():
                    logits = tail(x)
                    pred = torch.argmax(logits, dim=1)
                    if not with_target:
                        return pred
                    counter.batches = []
                    counter.add_logits(logits, target)
                    return pred, counter.batches[0], HF.cross_entropy(logits, target, 255)

            def b():
                if not with_target:
                    return HF.sssr_tail_predict(x, up[2], up[3], up[6])
                counts = torch.zeros(3 * NC + 2, dtype=torch.int64, device=dev)
                return HF.sssr_tail_predict(x, up[2], up[3], up[6], target=target, counts=counts), counts

            ta, tb = ab(a, b, args.window, args.rounds)
            ma, mb = sum(ta) / len(ta), sum(tb) / len(tb)
            mem_a, mem_b = peak_bytes(a), peak_bytes(b)
            logit_b = 16 * px * NC * 4
            bytes_a = px * NC * 4 + 4 * px * NC * 4 + 2 * 4 * px * NC * 4 + 4 * px * NC * 4 + logit_b + logit_b + 16 * px * 8
            bytes_b = px * NC * 4 + 16 * px
            if with_target:
                bytes_a += 2 * (logit_b + 16 * px)
                bytes_b += 16 * px
            flops = 2.0 * MACS_PER_PIXEL * px
            t_f, t_m = flops / F32_MATRIX_FLOPS, bytes_b / HBM_BPS
            floor, bound = max(t_f, t_m), 'fp32 matrix rate' if t_f >= t_m else 'HBM'
            verdict = 'B faster' if mb <= ma else 'B SLOWER'
            if mb > ma:
                losses.append((with_target, N, H, W))
            say(f'(N,H,W)=({N},{H},{W}) target={"yes" if with_target else "no "}:  A {ma * 1e3:8.1f} us [{", ".join(f"{t * 1e3:.1f}" for t in ta)}]   '
                f'B {mb * 1e3:8.1f} us [{", ".join(f"{t * 1e3:.1f}" for t in tb)}]   A/B {ma / mb:5.2f}  {verdict}')
            say(f'      bytes A {bytes_a / 1e6:8.1f} MB  B {bytes_b / 1e6:6.1f} MB   FLOPs {flops / 1e9:6.2f} G   B achieves {bytes_b / (mb * 1e-3) / 1e9:7.1f} GB/s, '
                f'{flops / (mb * 1e-3) / 1e12:6.2f} TFLOP/s   floor {floor * 1e6:6.1f} us ({bound}; {100 * floor / (mb * 1e-3):.0f} % of it reached)   '
                f'peak memory A {mem_a / 1e6:8.1f} MB  B {mem_b / 1e6:6.2f} MB')
    say()
    say('whole model (stage 1, random weights, eval, 256x512 input): A = DSRL.forward + torch.argmax, B = DSRL.predict (caller-owned nan_flag: no readback)')
    model = DSRL(1, CS).to(dev).to(memory_format=torch.channels_last).eval()
    flag = torch.zeros((), dtype=torch.int32, device=dev)
    for N in (1, 8):
        img = torch.randn(N, 3, 256, 512, device=dev).contiguous(memory_format=torch.channels_last)

        def a():
            with torch.no_grad():
                return torch.argmax(model(img)[0], dim=1)

        def b():
            return model.predict(img, nan_flag=flag)[0]

        ta, tb = ab(a, b, args.window, args.rounds)
        ma, mb = sum(ta) / len(ta), sum(tb) / len(tb)
        if mb > ma:
            losses.append(('model', N, 256, 512))
        say(f'batch {N}:  A {ma:8.3f} ms [{", ".join(f"{t:.3f}" for t in ta)}]   B {mb:8.3f} ms [{", ".join(f"{t:.3f}" for t in tb)}]   A/B {ma / mb:5.3f}   '
            f'peak memory A {peak_bytes(a) / 1e6:8.1f} MB  B {peak_bytes(b) / 1e6:8.1f} MB')
    say()
    say('rows where B is slower than A: ' + (', '.join(str(r) for r in losses) if losses else 'none'))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

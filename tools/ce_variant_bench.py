#!/usr/bin/env python3
"""Cost of one cross-entropy variant at the step's shape (N = 8, tail input 256 x 512, 19 -> 19), written to profiles/<variant>_ce.txt
(class_weighted_ce.txt, focal_ce.txt, label_smoothing_ce.txt, ohem_ce.txt, dice_ce.txt, lovasz_ce.txt, label_relax_ce.txt):
  * kernel-only times through the C ABI, HIP events around back-to-back launches, the variant's entry points against their base:
      weighted   dsrl_convt2x2_fwd_ce_w, dsrl_convt2x2_bwd_ce_w and dsrl_ce_fused_w against the unweighted calls, and the D pre-pass alone
                 (dsrl_ce_weight_sum: label histogram + weight sum);
      focal      dsrl_ce_fwd_f + dsrl_ce_bwd_f, dsrl_ce_fused_f, dsrl_convt2x2_fwd_ce_f, dsrl_convt2x2_bwd_ce_f against their _w siblings, gamma = 2;
      smoothed   the same four _s paths against their _w siblings, eps = 0.1;
      ohem       dsrl_ohem_prob beside dsrl_ce_fused on the same logits (time and bytes per second), dsrl_ohem_select, dsrl_ohem_apply and the whole
                 dsrl_ohem_target, thresh = 0.7, min_kept = 100000;
      dice       dsrl_dice_fwd beside dsrl_copy2d on as many bytes, dsrl_ohem_prob on the same logits and the torch composition (softmax, one-hot,
                 sums); dsrl_dice_bwd; dsrl_convt2x2_bwd_ce_d against dsrl_convt2x2_bwd_ce_w on the same inputs; five windows each, lambda = smooth = 1;
      lovasz     dsrl_lovasz_fwd at K = 1024 and K = 4096, on random logits and on near-one-hot logits (almost every background error in level 0: the
                 contended case), each with the per-wave aggregation of levels 0 and K - 1 and without it (DSRL_LOVASZ_AGG=0), beside dsrl_dice_fwd
                 and dsrl_copy2d on as many bytes; dsrl_lovasz_bwd; dsrl_convt2x2_bwd_ce_l against _d and _w; the torch composition (softmax, 19 x
                 torch.sort, cumsum); five windows each, lambda = 1;
      relaxed    dsrl_relax_mask (radius 1, 2 and 4) beside dsrl_copy2d of as many bytes; dsrl_convt2x2_fwd_ce_r, dsrl_convt2x2_bwd_ce_r and
                 dsrl_ce_fused_r against their _w siblings on the same logits, with the masks of labels on an 8 x 8 block grid and with all-singleton
                 masks (zeros); five windows each;
  * the replayed training step (stage 3, batch 8, 256 x 512 input, hipGraph): default, class weights and (focal, smoothed) class weights + gamma
    or eps, alternating in one process (ohem: default against ohem = (0.7, 100000); dice / lovasz: default, class weights, class weights + the term;
    relaxed: default, class weights, class weights + label_relax = 1, on labels of an 8 x 8 block grid, three rounds).
Everything in that file from the line '## recorded beside the tool' on is kept as it is.
Usage: python tools/ce_variant_bench.py weighted|focal|smoothed|ohem|dice|lovasz|relaxed [--steps K] [--no-step] [VAR=value ...]"""
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

# variant -> (entry-point suffix, suffix of the base it is measured against, gamma or eps, its name in the output, what it is called there,
#             the TrainStep keyword of the parameter, output file)
VARIANTS = {'weighted': ('_w', '', None, None, 'weighted', None, 'class_weighted_ce.txt'),
            'focal': ('_f', '_w', 2.0, 'gamma', 'focal', 'focal_gamma', 'focal_ce.txt'),
            'smoothed': ('_s', '_w', 0.1, 'eps', 'smoothed', 'label_smoothing', 'label_smoothing_ce.txt'),
            'ohem': ('', '', (0.7, 100000), 'ohem', 'ohem', 'ohem', 'ohem_ce.txt'),
            'dice': ('_d', '_w', (1.0, 1.0), 'dice', 'dice', 'dice', 'dice_ce.txt'),
            'lovasz': ('_l', '_w', (1.0, 1024), 'lovasz', 'lovasz', 'lovasz', 'lovasz_ce.txt'),
            'relaxed': ('_r', '_w', 1, 'radius', 'relaxed', 'label_relax', 'label_relax_ce.txt')}
if not args or args[0] not in VARIANTS:
    sys.exit(__doc__)
VARIANT = args[0]
SFX, BASE, PARAM, PNAME, WORD, STEP_KW, OUT = VARIANTS[VARIANT]
dev = 'cuda:0'
STEPS = int(args[args.index('--steps') + 1]) if '--steps' in args else 30
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
    wb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=dev)
    extra = {'': (), '_w': (wt.data_ptr(),), SFX: (wt.data_ptr(),) + (() if PARAM is None else (PARAM,))}      # what follows ignore_index
    wsp = {}

    def ws(name, *a):
        if (name, a) not in wsp:
            wsp[name, a] = torch.empty(query(name, *a), dtype=torch.uint8, device=dev)
        return wsp[name, a].data_ptr(), wsp[name, a].numel()

    def ce_fwd(s):
        call('dsrl_ce_fwd' + s, y.data_ptr(), C, tg.data_ptr(), P, C, 255, *extra[s], scal.data_ptr(), *ws(f'dsrl_ce{s}_workspace_bytes', P), st)

    def ce_bwd(s):
        call('dsrl_ce_bwd' + s, y.data_ptr(), C, tg.data_ptr(), P, C, 255, *extra[s], scal.data_ptr(), one.data_ptr(), dl.data_ptr(), C, st)

    def ce_fused(s):
        call('dsrl_ce_fused' + s, y.data_ptr(), C, tg.data_ptr(), P, C, 255, *extra[s], dl.data_ptr(), C, scal.data_ptr(), flag.data_ptr(),
             *ws(f'dsrl_ce_fused{s}_workspace_bytes', P), st)

    def fwd_ce(s):
        call('dsrl_convt2x2_fwd_ce' + s, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), N, H, W, C, C, tg.data_ptr(), 255, *extra[s],
             scal.data_ptr(), flag.data_ptr(), *ws(f'dsrl_convt2x2_fwd_ce{s}_workspace_bytes', N, H, W), st)

    def bwd_ce(s):
        call('dsrl_convt2x2_bwd_ce' + s, x.data_ptr(), w.data_ptr(), y.data_ptr(), tg.data_ptr(), 255, *extra[s], scal.data_ptr() + 4,
             ftg.data_ptr(), ftw.data_ptr(), 8, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wb.data_ptr(), wb.numel(), st)

    t = {}
    for s in (BASE, SFX):
        t['fwd_ce' + s] = timeit(lambda: fwd_ce(s))
    for waves in ('12', '8'):                   # the focal and the smoothed backward are the 8-wave build under either setting
        os.environ['DSRL_CONVT_CE_WAVES'] = waves
        for s in (BASE, SFX):
            fwd_ce(s)                           # its pixel count or D in scal[1]
            t[f'bwd_ce{s}/{waves}'] = timeit(lambda: bwd_ce(s))
    os.environ.pop('DSRL_CONVT_CE_WAVES')
    for s in (BASE, SFX):
        t['ce_fused' + s] = timeit(lambda: ce_fused(s))
    if VARIANT == 'weighted':
        wd = ws('dsrl_ce_weight_sum_workspace_bytes')
        t['D pre-pass'] = timeit(lambda: call('dsrl_ce_weight_sum', tg.data_ptr(), P, C, 255, wt.data_ptr(), scal.data_ptr() + 4, *wd, st))
        say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} labels = {P / 1e6:.1f} MB; mean of 20 back-to-back calls):')
        say(f"  dsrl_convt2x2_fwd_ce      {t['fwd_ce']:7.1f}   weighted {t['fwd_ce_w']:7.1f}   (+{t['fwd_ce_w'] - t['fwd_ce']:.1f}; the weighted call holds the D pre-pass)")
        for waves in ('12', '8'):
            a, bb = t[f'bwd_ce/{waves}'], t[f'bwd_ce_w/{waves}']
            say(f'  dsrl_convt2x2_bwd_ce ({waves:>2} waves) {a:7.1f}   weighted {bb:7.1f}   ({bb - a:+.1f})')
        say(f"  dsrl_ce_fused             {t['ce_fused']:7.1f}   weighted {t['ce_fused_w']:7.1f}   ({t['ce_fused_w'] - t['ce_fused']:+.1f}; count pre-pass -> D pre-pass)")
        say(f"  D pre-pass alone (class_hist_kernel + ce_weight_sum_kernel) {t['D pre-pass']:.1f}")
        return
    for key, f in (('ce_fwd', ce_fwd), ('ce_bwd', ce_bwd)):
        for s in (BASE, SFX):
            t[key + s] = timeit(lambda: f(s))
    say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} pixels; {PNAME} = {PARAM}; mean of 20 back-to-back calls; every call but ce_bwd and')
    say('convt2x2_bwd_ce holds the D pre-pass):')
    for path, label, key in (('A', 'dsrl_ce_fwd', 'ce_fwd'), ('A', 'dsrl_ce_bwd', 'ce_bwd'), ('B', 'dsrl_ce_fused', 'ce_fused'), ('C', 'dsrl_convt2x2_fwd_ce', 'fwd_ce')):
        a, bb = t[key + BASE], t[key + SFX]
        say(f'  {path}  {label:<22} weighted {a:7.1f}   {WORD} {bb:7.1f}   ({bb - a:+.1f})')
    for waves in ('12', '8'):
        a, bb = t[f'bwd_ce{BASE}/{waves}'], t[f'bwd_ce{SFX}/{waves}']
        say(f'  D  dsrl_convt2x2_bwd_ce   weighted {a:7.1f} ({waves:>2} waves)   {WORD} {bb:7.1f} (8 waves, DSRL_CONVT_CE_WAVES={waves})   ({bb - a:+.1f})')


def ohem_kernels():
    N, H, W, C = 8, 256, 512, 19
    P = N * 4 * H * W
    thresh, min_kept = PARAM
    # logits of a few units whose labels follow their own ranking in part: p from about 0 to about 1, as in training after the first epochs
    y = torch.randn(N, 2 * H, 2 * W, C, device=dev) * 3
    top = y.argmax(dim=-1).to(torch.uint8)
    tg = torch.randint(0, C, (N, 2 * H, 2 * W), device=dev, dtype=torch.uint8)
    tg = torch.where(torch.rand(tg.shape, device=dev) < 0.6, top, tg)
    tg[torch.rand(tg.shape, device=dev) < 0.1] = 255
    dl = torch.empty_like(y); out = torch.empty_like(tg)
    scal = torch.zeros(8, device=dev); flag = torch.zeros(1, dtype=torch.int32, device=dev); stats = torch.zeros(4, dtype=torch.int32, device=dev)
    st = HF._stream()
    wsf = torch.empty(query('dsrl_ce_fused_workspace_bytes', P), dtype=torch.uint8, device=dev)
    wso = torch.empty(query('dsrl_ohem_workspace_bytes', P), dtype=torch.uint8, device=dev)
    p = torch.empty(P, device=dev)
    t = {}
    t['fused'] = timeit(lambda: call('dsrl_ce_fused', y.data_ptr(), C, tg.data_ptr(), P, C, 255, dl.data_ptr(), C, scal.data_ptr(), flag.data_ptr(),
                                     wsf.data_ptr(), wsf.numel(), st))
    t['value'] = timeit(lambda: call('dsrl_ce_fused', y.data_ptr(), C, tg.data_ptr(), P, C, 255, None, C, scal.data_ptr(), flag.data_ptr(),
                                     wsf.data_ptr(), wsf.numel(), st))
    t['prob'] = timeit(lambda: call('dsrl_ohem_prob', y.data_ptr(), C, tg.data_ptr(), P, C, 255, p.data_ptr(), flag.data_ptr(), st))
    t['select'] = timeit(lambda: call('dsrl_ohem_select', p.data_ptr(), P, thresh, min_kept, stats.data_ptr(), wso.data_ptr(), wso.numel(), st))
    t['apply'] = timeit(lambda: call('dsrl_ohem_apply', p.data_ptr(), tg.data_ptr(), P, 255, stats.data_ptr(), out.data_ptr(), st))
    t['target'] = timeit(lambda: call('dsrl_ohem_target', y.data_ptr(), C, tg.data_ptr(), P, C, 255, thresh, min_kept, out.data_ptr(), stats.data_ptr(),
                                      flag.data_ptr(), wso.data_ptr(), wso.numel(), st))
    torch.cuda.synchronize()
    s4 = stats.cpu().numpy().view(np.uint32)
    lb = P * C * 4
    say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} pixels, {lb / 1e6:.0f} MB of logits; thresh = {thresh}, min_kept = {min_kept}; mean of 20')
    say(f'back-to-back calls; this batch: {int(s4[1])} candidates, {int(s4[2])} kept, thr = {float(s4[:1].view(np.float32)[0]):.6f}):')
    rows = (('dsrl_ce_fused, value + gradient (count pre-pass + ce_fused_kernel + finalize)', 'fused', 2 * lb + 2 * P),
            ('dsrl_ce_fused, value only, as in the hand-over step', 'value', lb + 2 * P),
            ('dsrl_ohem_prob (ohem_prob_kernel)', 'prob', lb + P + 4 * P),
            ('dsrl_ohem_select (4 x histogram + pick)', 'select', 4 * 4 * P),
            ('dsrl_ohem_apply', 'apply', 4 * P + 2 * P),
            ('dsrl_ohem_target (the three above)', 'target', lb + P + 4 * P + 4 * 4 * P + 4 * P + 2 * P))
    for label, key, nbytes in rows:
        say(f'  {label:<78} {t[key]:7.1f}   {nbytes / 1e6:6.1f} MB   {nbytes / t[key] / 1e6:5.2f} TB/s')


def dice_kernels():
    N, H, W, C = 8, 256, 512, 19
    P = N * 4 * H * W
    lam, smooth = PARAM
    rs = np.random.RandomState(1)
    y = torch.randn(N, 2 * H, 2 * W, C, device=dev) * 3
    top = y.argmax(dim=-1).to(torch.uint8)
    tg = torch.randint(0, C, (N, 2 * H, 2 * W), device=dev, dtype=torch.uint8)
    tg = torch.where(torch.rand(tg.shape, device=dev) < 0.5, top, tg)
    tg[torch.rand(tg.shape, device=dev) < 0.1] = 255
    x = torch.randn(N, H, W, C, device=dev); w = torch.randn(C, C, 2, 2, device=dev) * 0.2
    wt = HF.class_weight_table(rs.uniform(0.25, 8.0, C), dev)
    dx = torch.empty_like(x); dw = torch.empty_like(w); db = torch.empty(C, device=dev); dl = torch.zeros_like(y)
    scal = torch.zeros(8, device=dev); flag = torch.zeros(1, dtype=torch.int32, device=dev); rec = torch.zeros(128, device=dev)
    ftg = torch.randn(N, H // 4, W // 4, device=dev); ftw = torch.randn(C, device=dev)
    p = torch.empty(P, device=dev)
    st = HF._stream()
    wb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=dev)
    wsd = torch.empty(query('dsrl_dice_workspace_bytes', P), dtype=torch.uint8, device=dev)
    wsf = torch.empty(query('dsrl_ce_fused_w_workspace_bytes', P), dtype=torch.uint8, device=dev)
    call('dsrl_ce_fused_w', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), None, C, scal.data_ptr(), flag.data_ptr(), wsf.data_ptr(), wsf.numel(), st)

    def torch_dice():
        live = tg != 255
        pr = torch.softmax(y, dim=-1)[live]
        oh = torch.nn.functional.one_hot(tg[live].long(), C).float()
        I, Pc, G = (pr * oh).sum(0), pr.sum(0), oh.sum(0)
        present = G > 0
        return lam * (1 - ((2 * I + smooth) / (Pc + G + smooth))[present].sum() / present.sum())

    def bwd(s, extra):
        call('dsrl_convt2x2_bwd_ce' + s, x.data_ptr(), w.data_ptr(), y.data_ptr(), tg.data_ptr(), 255, *extra, scal.data_ptr() + 4, ftg.data_ptr(),
             ftw.data_ptr(), 8, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wb.data_ptr(), wb.numel(), st)

    lb = P * C * 4
    rows = [('dsrl_dice_fwd (dice_sums_kernel + dice_finish_kernel)', lb + P,
             lambda: call('dsrl_dice_fwd', y.data_ptr(), C, tg.data_ptr(), P, C, 255, lam, smooth, rec.data_ptr(), flag.data_ptr(), wsd.data_ptr(), wsd.numel(), st)),
            ('dsrl_copy2d, half the logits: as many bytes read + written', lb,
             lambda: call('dsrl_copy2d', y.data_ptr(), C, dl.data_ptr(), C, P // 2, C, st)),
            ('dsrl_ohem_prob on the same logits', lb + P + 4 * P,
             lambda: call('dsrl_ohem_prob', y.data_ptr(), C, tg.data_ptr(), P, C, 255, p.data_ptr(), flag.data_ptr(), st)),
            ('torch: softmax, one-hot, sums', 0, torch_dice),
            ('dsrl_dice_bwd, accumulate = 1', 3 * lb + P,
             lambda: call('dsrl_dice_bwd', y.data_ptr(), C, tg.data_ptr(), P, C, 255, rec.data_ptr(), 1, dl.data_ptr(), C, st))]
    for waves in ('12', '8'):
        rows.append((f'dsrl_convt2x2_bwd_ce_w (DSRL_CONVT_CE_WAVES={waves})', 0, lambda waves=waves: (os.environ.__setitem__('DSRL_CONVT_CE_WAVES', waves), bwd('_w', (wt.data_ptr(),)))))
    rows.append(('dsrl_convt2x2_bwd_ce_d (8 waves)', 0, lambda: bwd('_d', (wt.data_ptr(), rec.data_ptr()))))
    say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} pixels, {lb / 1e6:.0f} MB of logits; lambda = {lam}, smooth = {smooth}; five windows of 20')
    say('back-to-back calls each: min / median / max of the windows; bytes and rate at the median):')
    for label, nbytes, f in rows:
        wins = sorted(timeit(f) for _ in range(5))
        rate = f'   {nbytes / 1e6:6.1f} MB   {nbytes / wins[2] / 1e6:5.2f} TB/s' if nbytes else ''
        say(f'  {label:<62} {wins[0]:7.1f} / {wins[2]:7.1f} / {wins[4]:7.1f}{rate}')
    os.environ.pop('DSRL_CONVT_CE_WAVES', None)
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    say(f'  this batch: lambda L_dice = {r[0]:.6f}, |K| = {int(r[1])}, torch composition {float(torch_dice()):.6f}')


def lovasz_kernels():
    N, H, W, C = 8, 256, 512, 19
    P = N * 4 * H * W
    lam = PARAM[0]
    rs = np.random.RandomState(1)
    y = torch.randn(N, 2 * H, 2 * W, C, device=dev) * 3
    top = y.argmax(dim=-1).to(torch.uint8)
    tg = torch.randint(0, C, (N, 2 * H, 2 * W), device=dev, dtype=torch.uint8)
    tg = torch.where(torch.rand(tg.shape, device=dev) < 0.5, top, tg)
    tg[torch.rand(tg.shape, device=dev) < 0.1] = 255
    # a confident model: the label's logit 12 above noise of 0.5 on 97 % of the pixels - p of the others about 6e-6, level 0 at either K
    hot = torch.randn(N, 2 * H, 2 * W, C, device=dev) * 0.5
    lab = torch.where(tg == 255, torch.zeros_like(tg), tg).long()
    right = torch.rand(tg.shape, device=dev) < 0.97
    hot.scatter_add_(3, torch.where(right, lab, (lab + 1) % C).unsqueeze(-1), torch.full((N, 2 * H, 2 * W, 1), 12.0, device=dev))
    x = torch.randn(N, H, W, C, device=dev); w = torch.randn(C, C, 2, 2, device=dev) * 0.2
    wt = HF.class_weight_table(rs.uniform(0.25, 8.0, C), dev)
    dx = torch.empty_like(x); dw = torch.empty_like(w); db = torch.empty(C, device=dev); dl = torch.zeros_like(y)
    scal = torch.zeros(8, device=dev); flag = torch.zeros(1, dtype=torch.int32, device=dev); drec = torch.zeros(128, device=dev)
    ftg = torch.randn(N, H // 4, W // 4, device=dev); ftw = torch.randn(C, device=dev)
    st = HF._stream()
    wb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=dev)
    wsd = torch.empty(query('dsrl_dice_workspace_bytes', P), dtype=torch.uint8, device=dev)
    wsf = torch.empty(query('dsrl_ce_fused_w_workspace_bytes', P), dtype=torch.uint8, device=dev)
    recs = {K: torch.zeros(query('dsrl_lovasz_record_floats', C, K), device=dev) for K in (1024, 4096)}
    wsl = {K: torch.empty(query('dsrl_lovasz_workspace_bytes', P, C, K), dtype=torch.uint8, device=dev) for K in (1024, 4096)}
    call('dsrl_ce_fused_w', y.data_ptr(), C, tg.data_ptr(), P, C, 255, wt.data_ptr(), None, C, scal.data_ptr(), flag.data_ptr(), wsf.data_ptr(), wsf.numel(), st)
    call('dsrl_dice_fwd', y.data_ptr(), C, tg.data_ptr(), P, C, 255, 1.0, 1.0, drec.data_ptr(), flag.data_ptr(), wsd.data_ptr(), wsd.numel(), st)

    def fwd(lg, K, agg):
        os.environ['DSRL_LOVASZ_AGG'] = agg
        call('dsrl_lovasz_fwd', lg.data_ptr(), C, tg.data_ptr(), P, C, 255, lam, K, recs[K].data_ptr(), flag.data_ptr(), wsl[K].data_ptr(), wsl[K].numel(), st)

    def torch_lovasz(lg):
        live = tg != 255
        pr = torch.softmax(lg, dim=-1)[live]
        lab = tg[live].long()
        losses = []
        for c in range(C):
            fg = (lab == c).float()
            if fg.sum() == 0:
                continue
            es, perm = torch.sort((fg - pr[:, c]).abs(), descending=True)
            fs = fg[perm]
            gts = fs.sum()
            jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1.0 - fs).cumsum(0))
            jac[1:] = jac[1:] - jac[:-1]
            losses.append(torch.dot(es, jac))
        return lam * torch.stack(losses).mean()

    def bwd(s, extra):
        call('dsrl_convt2x2_bwd_ce' + s, x.data_ptr(), w.data_ptr(), y.data_ptr(), tg.data_ptr(), 255, *extra, scal.data_ptr() + 4, ftg.data_ptr(),
             ftw.data_ptr(), 8, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wb.data_ptr(), wb.numel(), st)

    lb = P * C * 4
    rows = []
    for K in (1024, 4096):
        npass = 1 if K == 1024 else 3
        for name, lg in (('random logits', y), ('near-one-hot logits', hot)):
            for agg in ('1', '0'):
                rows.append((f'dsrl_lovasz_fwd K = {K}, {name}, {"aggregated" if agg == "1" else "plain LDS atomics"}', npass * (lb + P),
                             lambda lg=lg, K=K, agg=agg: fwd(lg, K, agg)))
    rows += [('dsrl_dice_fwd on the random logits', lb + P,
              lambda: call('dsrl_dice_fwd', y.data_ptr(), C, tg.data_ptr(), P, C, 255, 1.0, 1.0, drec.data_ptr(), flag.data_ptr(), wsd.data_ptr(), wsd.numel(), st)),
             ('dsrl_copy2d, half the logits: as many bytes read + written', lb,
              lambda: call('dsrl_copy2d', y.data_ptr(), C, dl.data_ptr(), C, P // 2, C, st)),
             ('torch: softmax, 19 x torch.sort, cumsum (random logits)', 0, lambda: torch_lovasz(y))]
    say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} pixels, {lb / 1e6:.0f} MB of logits; lambda = {lam}; five windows of 20 back-to-back')
    say('calls each: min / median / max of the windows; bytes (the logits once per class group: 1 pass at K = 1024, 3 at K = 4096) and rate at the median):')

    def table(rows):
        for label, nbytes, f in rows:
            wins = sorted(timeit(f, 5 if label.startswith('torch') else 20) for _ in range(5))
            rate = f'   {nbytes / 1e6:6.1f} MB   {nbytes / wins[2] / 1e6:5.2f} TB/s' if nbytes else ''
            say(f'  {label:<72} {wins[0]:8.1f} / {wins[2]:8.1f} / {wins[4]:8.1f}{rate}')
    table(rows)
    os.environ.pop('DSRL_LOVASZ_AGG', None)
    fwd(y, 1024, '1'); os.environ.pop('DSRL_LOVASZ_AGG', None)
    rows = [('dsrl_lovasz_bwd K = 1024, accumulate = 1', 3 * lb + P,
             lambda: call('dsrl_lovasz_bwd', y.data_ptr(), C, tg.data_ptr(), P, C, 255, recs[1024].data_ptr(), 1024, 1, dl.data_ptr(), C, st))]
    for waves in ('12', '8'):
        rows.append((f'dsrl_convt2x2_bwd_ce_w (DSRL_CONVT_CE_WAVES={waves})', 0, lambda waves=waves: (os.environ.__setitem__('DSRL_CONVT_CE_WAVES', waves), bwd('_w', (wt.data_ptr(),)))))
    rows.append(('dsrl_convt2x2_bwd_ce_d (8 waves)', 0, lambda: bwd('_d', (wt.data_ptr(), drec.data_ptr()))))
    rows.append(('dsrl_convt2x2_bwd_ce_l (8 waves), K = 1024', 0, lambda: bwd('_l', (wt.data_ptr(), recs[1024].data_ptr(), 1024))))
    table(rows)
    os.environ.pop('DSRL_CONVT_CE_WAVES', None)
    torch.cuda.synchronize()
    r = recs[1024].cpu().numpy()
    say(f'  random logits: lambda L = {r[0]:.6f} at K = 1024, |Present| = {int(r[1])}, torch (sorted, unquantised) {float(torch_lovasz(y)):.6f}')
    fwd(hot, 1024, '1'); os.environ.pop('DSRL_LOVASZ_AGG', None)
    torch.cuda.synchronize()
    r = recs[1024].cpu().numpy()
    h = wsl[1024][:2 * C * 1024 * 4].cpu().numpy().view(np.uint32).reshape(2, C, 1024)
    say(f'  near-one-hot logits: lambda L = {r[0]:.6f}, torch {float(torch_lovasz(hot)):.6f}; {h[1][:, 0].sum() / h[1].sum():.4f} of the background and '
        f'{h[0][:, 0].sum() / h[0].sum():.4f} of the foreground errors in level 0')


def block_labels(N, H, W, C, b, ignore=0.08):
    """(N, H, W) uint8 labels on the device: one class per b x b block, some blocks ignored"""
    g = torch.randint(0, C, (N, H // b, W // b), device=dev, dtype=torch.uint8)
    g[torch.rand(g.shape, device=dev) < ignore] = 255
    return g.repeat_interleave(b, 1).repeat_interleave(b, 2).contiguous()


def relaxed_kernels():
    N, H, W, C = 8, 256, 512, 19
    P = N * 4 * H * W
    rs = np.random.RandomState(1)
    x = torch.randn(N, H, W, C, device=dev); w = torch.randn(C, C, 2, 2, device=dev) * 0.2; b = torch.randn(C, device=dev)
    y = torch.empty(N, 2 * H, 2 * W, C, device=dev)
    tg = block_labels(N, 2 * H, 2 * W, C, 8)
    wt = HF.class_weight_table(rs.uniform(0.25, 8.0, C), dev)
    dx = torch.empty_like(x); dw = torch.empty_like(w); db = torch.empty(C, device=dev); dl = torch.empty_like(y)
    scal = torch.zeros(8, device=dev); flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ftg = torch.randn(N, H // 4, W // 4, device=dev); ftw = torch.randn(C, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    st = HF._stream()
    wb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=dev)
    masks = {'block-8 masks': HF.relax_mask(tg, C, 255, 1, stats), 'singleton masks': torch.zeros(N, 2 * H, 2 * W, dtype=torch.int32, device=dev)}
    live, multi = stats.cpu().tolist()
    wsp = {}

    def ws(name, *a):
        if (name, a) not in wsp:
            wsp[name, a] = torch.empty(query(name, *a), dtype=torch.uint8, device=dev)
        return wsp[name, a].data_ptr(), wsp[name, a].numel()

    def extra(s, m):
        return (wt.data_ptr(),) if s == '_w' else (wt.data_ptr(), m.data_ptr())

    def fwd_ce(s, m):
        call('dsrl_convt2x2_fwd_ce' + s, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), N, H, W, C, C, tg.data_ptr(), 255, *extra(s, m),
             scal.data_ptr(), flag.data_ptr(), *ws(f'dsrl_convt2x2_fwd_ce{s}_workspace_bytes', N, H, W), st)

    def bwd_ce(s, m):
        call('dsrl_convt2x2_bwd_ce' + s, x.data_ptr(), w.data_ptr(), y.data_ptr(), tg.data_ptr(), 255, *extra(s, m), scal.data_ptr() + 4,
             ftg.data_ptr(), ftw.data_ptr(), 8, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wb.data_ptr(), wb.numel(), st)

    def ce_fused(s, m):
        call('dsrl_ce_fused' + s, y.data_ptr(), C, tg.data_ptr(), P, C, 255, *extra(s, m), dl.data_ptr(), C, scal.data_ptr(), flag.data_ptr(),
             *ws(f'dsrl_ce_fused{s}_workspace_bytes', P), st)

    mk = torch.empty(N, 2 * H, 2 * W, dtype=torch.int32, device=dev)
    rows = [(f'dsrl_relax_mask, radius {r}, with the counters', 5 * P,
             lambda r=r: call('dsrl_relax_mask', tg.data_ptr(), N, 2 * H, 2 * W, C, 255, r, mk.data_ptr(), stats.data_ptr(), st)) for r in (1, 2, 4)]
    rows.append(('dsrl_relax_mask, radius 1, no counters', 5 * P,
                 lambda: call('dsrl_relax_mask', tg.data_ptr(), N, 2 * H, 2 * W, C, 255, 1, mk.data_ptr(), None, st)))
    nf = 5 * P // 8                                 # floats whose read + write is as many bytes as P labels read + P words written
    rows.append(('dsrl_copy2d of as many bytes', 5 * P, lambda: call('dsrl_copy2d', y.data_ptr(), C, dl.data_ptr(), C, nf // C, C, st)))
    fwd_ce('_w', None)                              # the logits, and D in scal[1]
    for name, f in (('dsrl_convt2x2_fwd_ce', fwd_ce), ('dsrl_convt2x2_bwd_ce', bwd_ce), ('dsrl_ce_fused', ce_fused)):
        for waves in (('12', '8') if f is bwd_ce else (None,)):
            tag = f' (DSRL_CONVT_CE_WAVES={waves})' if waves else ''
            rows.append((f'{name}_w{tag}', 0, lambda f=f, waves=waves: (waves and os.environ.__setitem__('DSRL_CONVT_CE_WAVES', waves), f('_w', None))))
        for label, m in masks.items():
            rows.append((f'{name}_r, {label}' + (' (8 waves)' if f is bwd_ce else ''), 0, lambda f=f, m=m: f('_r', m)))
    say(f'kernel-only, us per call (N = {N}, tail input {H} x {W}, {P} pixels; labels on an 8 x 8 block grid: {multi / live:.3f} of the live pixels have')
    say('more than one class in their set at radius 1; five windows of 20 back-to-back calls each: min / median / max of the windows; bytes and rate at')
    say('the median):')
    for label, nbytes, f in rows:
        wins = sorted(timeit(f) for _ in range(5))
        rate = f'   {nbytes / 1e6:6.1f} MB   {nbytes / wins[2] / 1e6:5.2f} TB/s' if nbytes else ''
        say(f'  {label:<58} {wins[0]:7.1f} / {wins[2]:7.1f} / {wins[4]:7.1f}{rate}')
    os.environ.pop('DSRL_CONVT_CE_WAVES', None)


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
    if VARIANT == 'relaxed':
        tgt = block_labels(*tgt.shape, cs.NUM_CLASSES, 8)          # labels with borders: the synthetic ones are noise, every set would be full
    w = np.random.RandomState(2).uniform(0.25, 8.0, cs.NUM_CLASSES)

    def run(step, n):
        for _ in range(n):
            step.enqueue(img, org, tgt, 0.0, 0.9, 0.0, True)      # lr 0: every step trains the same parameters
            while step.pending() > 1:
                step.collect()
        while step.pending():
            step.collect()
    if VARIANT == 'weighted':
        kinds = {'unweighted': {}, 'weighted': {'class_weights': w}}
    elif VARIANT == 'ohem':
        kinds = {'default': {}, 'ohem': {'ohem': PARAM}}
    elif VARIANT in ('dice', 'lovasz'):
        kinds = {'default': {}, 'weighted': {'class_weights': w}, VARIANT: {'class_weights': w, VARIANT: PARAM}}
    else:
        kinds = {'default': {}, 'weighted': {'class_weights': w}, WORD: {'class_weights': w, STEP_KW: PARAM}}
    res, replays = {k: [] for k in kinds}, {}
    for _ in range(3 if VARIANT in ('dice', 'lovasz', 'relaxed') else 2):      # one captured step at a time (the device-resident dropout key has one binding): build, warm, time, release
        for k, kw in kinds.items():
            s = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, **kw)
            run(s, s.GRAPH_WARMUP + 6)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(s, STEPS)
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / STEPS * 1e3)
            replays[k] = s.graph_replays
            s.release()
    say(f'replayed step (stage 3, batch 8, 256 x 512, {STEPS} steps per figure, {len(next(iter(res.values())))} alternating rounds in one process), ms per step:')
    width = 11 if VARIANT == 'weighted' else 9
    for k in res:
        say(f'  {k:<{width}} ' + '  '.join(f'{v:.3f}' for v in res[k]) + f'   min {min(res[k]):.3f}  (replays {replays[k]})')
    if VARIANT == 'weighted':
        say(f"  weighted - unweighted (min): {(min(res['weighted']) - min(res['unweighted'])) * 1e3:+.0f} us")
    elif VARIANT == 'ohem':
        say(f"  ohem - default (min): {(min(res['ohem']) - min(res['default'])) * 1e3:+.0f} us")
    else:
        say(f"  {WORD} - weighted (min): {(min(res[WORD]) - min(res['weighted'])) * 1e3:+.0f} us;  {WORD} - default (min): "
            f"{(min(res[WORD]) - min(res['default'])) * 1e3:+.0f} us")
        if VARIANT == 'relaxed':
            say('  spread (max - min) per kind, us: ' + '  '.join(f'{k} {(max(v) - min(v)) * 1e3:.0f}' for k, v in res.items()))


(ohem_kernels() if VARIANT == 'ohem' else dice_kernels() if VARIANT == 'dice' else lovasz_kernels() if VARIANT == 'lovasz' else
 relaxed_kernels() if VARIANT == 'relaxed' else kernels())
if '--no-step' not in args:
    replayed_step()
out = os.path.join(ROOT, 'profiles', OUT)
os.makedirs(os.path.dirname(out), exist_ok=True)
KEEP = '## recorded beside the tool'            # the same-box A/B against the parent commit and the kernel resource tables: kept across runs
tail = ''
if os.path.isfile(out):
    old = open(out).read()
    if KEEP in old:
        tail = old[old.index(KEEP):]
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n' + tail)

"""The soft Dice loss term, loss = CE + lambda L_dice, through every layer that carries it, each against the float64 restatement
of tests/dice_ref.py (fp32 logits taken to float64; closed-form gradient):

    dsrl_dice_fwd / dsrl_dice_bwd    the class sums, the record {lambda L, |K|, a, b} and the unfused gradient row     (HF.dice_loss)
    dsrl_convt2x2_bwd_ce_d           the weighted CE row + the Dice row formed inside the ConvTranspose backward         (HF.LogitsGrad.dice)
    HF.fused_losses(dice=)           on the head: the hand-over, values and parameter gradients against cross_entropy + dice_loss through autograd
    TrainStep(dice=)                 captured == eager, validation keeps the plain CE, off is the step built without the argument

Cases: randn, spread, offset_1e4, onehot and bad_label of test_cross_entropy_edges.make_case, and `overlap` (dice_ref.make_overlap): half the live
labels are the arg-max, about 10 % are ignored, class C - 1 is absent; asserted on the reference: 0.2 < L_dice < 0.9 and a largest gradient element
beyond 100 x the gradient bound, so that a kernel that ignores Dice, or that counts the absent class, fails.

Tolerances (fixed):
    G_c, |K|      exact
    value         |record[0] - ref| <= 1e-6 lambda
    a_c, b_c      within 4 ulp of the float64 coefficients rounded to fp32
    gradient      (2^-20 + 2^-22) max_c (|a_c| + |b_c|) per element against float64: the weighted CE bound with Dice's own scale where w / D stands;
                  pixels that are not live exactly 0; accumulate = 1 equals the fp32 sum bitwise; the record's bits repeat
    fused         dx, dw, db bit-identical to dsrl_ce_fused_w -> dsrl_dice_bwd(accumulate) -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd, and
                  1e-5 of the range against the float64 gradient pushed through oracle.conv_transpose2d_k2s2_bwd; one wave build: DSRL_CONVT_CE_WAVES
                  unset and '8' give the same bytes.  The kernel takes W % 128 == 0 only (W = 128, N x H = 1 x 3 and 2 x 5)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dice_ref as DR          # noqa: E402
import gen                     # noqa: E402
import oracle as O             # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402
from ce_variant_runners import _place, table   # noqa: E402
from test_class_weighted_ce_gpu import _bits, _bits_equal, _five, make_weights, reference   # noqa: E402
from test_cross_entropy_edges import LOSS_REL, M_ULPS, make_case, ulp32     # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import DsrlHipError   # noqa: E402

CASES = ['randn', 'spread', 'offset_1e4', 'onehot', 'bad_label', 'overlap']
GRAD_TOL = DR.GRAD_TOL


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def dice_case(case, P, C, rs, ii=255):
    if case == 'overlap':
        lg, tg = DR.make_overlap(P, C, rs, ii)
        DR.assert_overlap(lg, tg, ii)
        return lg, tg
    return make_case(case, P, C, rs, ii)


_refs = {}


def dice_reference(lg, tg, ii, lam, smooth):
    """(lambda L, gradient, |K|, a, b, G) in float64, computed once per input"""
    key = (lg.tobytes(), tg.tobytes(), ii, lam, smooth)
    if key not in _refs:
        if len(_refs) > 64:
            _refs.clear()
        _refs[key] = DR.dice_loss_and_grad(lg, tg, ii, lam, smooth)
    return _refs[key]


def run_fwd(lg, tg, ii, lam, smooth, layout='dense', expect_error=False):
    """dsrl_dice_fwd -> (record (128,), G (64,) from the totals at the head of the workspace, flag); everything pre-filled with 7"""
    call, query = _lib()
    P, C = lg.shape
    buf, ptr, ld = _place(lg, layout)
    target = torch.tensor(tg, device=DEV)
    rec = torch.full((128,), 7.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.full((query('dsrl_dice_workspace_bytes', P),), 7, dtype=torch.uint8, device=DEV)
    args = (ptr, ld, target.data_ptr(), P, C, ii, lam, smooth, rec.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), HF._stream())
    if expect_error:
        with pytest.raises(DsrlHipError):
            call('dsrl_dice_fwd', *args)
    else:
        call('dsrl_dice_fwd', *args)
    torch.cuda.synchronize()
    if expect_error:
        assert bool((ws == 7).all())
    G = ws[64 * 16:64 * 20].cpu().numpy().view(np.uint32)
    return rec, G, int(flag)


def run_bwd(lg, tg, ii, rec, accumulate=0, layout='dense', into=None):
    """dsrl_dice_bwd -> gradient (P, C); accumulate: into a copy of `into`"""
    call, _ = _lib()
    P, C = lg.shape
    buf, ptr, ld = _place(lg, layout)
    target = torch.tensor(tg, device=DEV)
    if layout == 'slice':
        big = torch.full((P, C + 3), 7.0, device=DEV)
        if into is not None:
            big[:, 1:1 + C] = torch.tensor(into, device=DEV)
        call('dsrl_dice_bwd', ptr, ld, target.data_ptr(), P, C, ii, rec.data_ptr(), accumulate, big.data_ptr() + 4, C + 3, HF._stream())
        torch.cuda.synchronize()
        assert bool((big[:, 0] == 7).all()) and bool((big[:, 1 + C:] == 7).all()), 'wrote outside the rows'
        return host(big[:, 1:1 + C])
    dl = torch.full((P, C), 7.0, device=DEV) if into is None else torch.tensor(into, device=DEV)
    call('dsrl_dice_bwd', ptr, ld, target.data_ptr(), P, C, ii, rec.data_ptr(), accumulate, dl.data_ptr(), C, HF._stream())
    torch.cuda.synchronize()
    return host(dl)


def ulps_apart(got, want64):
    """|got - fp32(want)| in ulps of fp32(want), elementwise"""
    w32 = np.asarray(want64).astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(w32), np.float32(1e-37)))
    return np.abs(got.astype(np.float64) - w32.astype(np.float64)) / sp.astype(np.float64)


def check_record(rec, G, lg, tg, ii, lam, smooth, name):
    val, _, K, a, b, Gref = dice_reference(lg, tg, ii, lam, smooth)
    C = lg.shape[1]
    r = host(rec)
    assert np.array_equal(G[:C].astype(np.int64), Gref) and not G[C:].any(), f'{name}: G_c {G[:C]} vs {Gref}'
    assert r[1] == K, f'{name}: |K| = {r[1]} vs {K}'
    print(f'{name}: value {r[0]!r} ref {val!r} error / bound = {abs(r[0] - val) / (1e-6 * lam):.3f}')
    assert abs(r[0] - val) <= 1e-6 * lam, f'{name}: value {r[0]!r} vs {val!r}'
    ua, ub = ulps_apart(r[2:2 + C], a), ulps_apart(r[2 + C:2 + 2 * C], b)
    print(f'{name}: coefficients within {max(ua.max(), ub.max()):.2f} ulp')
    assert ua.max() <= 4 and ub.max() <= 4, f'{name}: a within {ua.max()} ulp, b within {ub.max()} ulp'
    assert np.all(r[2:2 + C][Gref == 0] == 0) and np.all(r[2 + C:2 + 2 * C][Gref == 0] == 0), f'{name}: an absent class has a coefficient'
    assert not r[2 + 2 * C:].any(), f'{name}: the tail of the record is not zero'


def check_dice_grad(g, lg, tg, ii, lam, smooth, name):
    _, gref, _, a, b, _ = dice_reference(lg, tg, ii, lam, smooth)
    C = lg.shape[1]
    t = tg.astype(np.int64)
    live = (t != ii) & (t < C)
    assert np.all(g[~live] == 0), f'{name}: nonzero gradient on a pixel that is not live'
    bound = GRAD_TOL * float((np.abs(a) + np.abs(b)).max())
    err = np.abs(g[live].astype(np.float64) - gref[live])
    print(f'{name}: max gradient error / bound = {float(err.max(initial=0.0)) / max(bound, 1e-300):.3f}')
    assert not np.isnan(err).any(), f'{name}: NaN in the gradient of a live pixel'
    assert err.max(initial=0.0) <= bound, f'{name}: gradient error {err.max():.3e} beyond (2^-20 + 2^-22) max(|a| + |b|) = {bound:.3e}'


# ------------------------------------------------------------------------------------------------------------------------------ dsrl_dice_fwd / _bwd
@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('case', CASES)
def test_dice_fwd_and_bwd(case, C):
    for P in (1536, 1000):
        for layout in ('dense', 'slice'):
            for lam, smooth in ((1.0, 1.0), (0.4, 0.0)) if layout == 'dense' else ((1.0, 1.0),):
                rs = np.random.RandomState(1000 * C + 100 * CASES.index(case) + P % 7 + (layout == 'slice'))
                lg, tg = dice_case(case, P, C, rs)
                name = f'{case} C={C} P={P} {layout} lambda={lam} smooth={smooth}'
                rec, G, fl = run_fwd(lg, tg, 255, lam, smooth, layout)
                assert fl == 0, (name, fl)
                check_record(rec, G, lg, tg, 255, lam, smooth, name)
                g = run_bwd(lg, tg, 255, rec, 0, layout)
                check_dice_grad(g, lg, tg, 255, lam, smooth, name)
                # the plain fp32 restatement of the same arithmetic stays well inside the bound: the bound is not what the kernel happens to give
                _, ge, _, _ = DR.emulate_fp32(lg, tg, 255, lam, smooth)
                check_dice_grad(ge, lg, tg, 255, lam, smooth, 'fp32 numpy ' + name)
                # accumulate = 1: the fp32 sum, bitwise (a pixel that is not live adds +0)
                base = rs.standard_normal(lg.shape).astype(np.float32)
                base[tg == 255] = 0
                acc = run_bwd(lg, tg, 255, rec, 1, layout, into=base)
                assert _bits(acc) == _bits(base + g), f'{name}: accumulate differs from the fp32 sum'
                # twice: the same bits, record and gradient
                rec2, G2, _ = run_fwd(lg, tg, 255, lam, smooth, layout)
                assert _bits(host(rec)) == _bits(host(rec2)) and np.array_equal(G, G2), f'{name}: the record does not repeat'
                assert _bits(g) == _bits(run_bwd(lg, tg, 255, rec2, 0, layout)), f'{name}: the gradient does not repeat'
                if layout == 'slice':           # the layout changes the loads, not the arithmetic
                    recd, _, _ = run_fwd(lg, tg, 255, lam, smooth, 'dense')
                    assert _bits(host(rec)) == _bits(host(recd)), f'{name}: dense and strided logits give different records'


def test_ignore_indices_all_ignored_and_one_pixel():
    C = 19
    for ii in (0, 18, -1):
        rs = np.random.RandomState(40 + (ii & 0xff))
        lg, tg = make_case('randn', 1000, C, rs, ii)
        rec, G, fl = run_fwd(lg, tg, ii, 1.0, 1.0)
        assert fl == 0
        check_record(rec, G, lg, tg, ii, 1.0, 1.0, f'ii={ii}')
        check_dice_grad(run_bwd(lg, tg, ii, rec), lg, tg, ii, 1.0, 1.0, f'ii={ii}')
    lg, tg = make_case('randn', 300, C, np.random.RandomState(1))
    tg[:] = 255
    rec, G, fl = run_fwd(lg, tg, 255, 1.0, 1.0)
    assert not host(rec).any() and not G.any() and fl == 0              # K empty: value 0, every coefficient 0
    assert not run_bwd(lg, tg, 255, rec).any()
    lg, tg = make_case('randn', 1, C, np.random.RandomState(2))
    rec, G, fl = run_fwd(lg, tg, 255, 2.0, 1.0)
    check_record(rec, G, lg, tg, 255, 2.0, 1.0, 'one pixel')
    check_dice_grad(run_bwd(lg, tg, 255, rec), lg, tg, 255, 2.0, 1.0, 'one pixel')


def test_a_nan_logit_raises_the_flag_in_a_live_pixel_only():
    C = 19
    lg, tg = make_case('randn', 1000, C, np.random.RandomState(5))
    live = np.where(tg != 255)[0]
    dead = np.where(tg == 255)[0]
    lg2 = lg.copy(); lg2[dead[0], 3] = np.nan
    rec, G, fl = run_fwd(lg2, tg, 255, 1.0, 1.0)
    assert fl == 0
    check_record(rec, G, lg, tg, 255, 1.0, 1.0, 'NaN in an ignored pixel')
    lg2 = lg.copy(); lg2[live[0], 3] = np.nan
    rec, G, fl = run_fwd(lg2, tg, 255, 1.0, 1.0)
    assert fl == 1 and np.isnan(host(rec)[0])


def test_the_bad_label_case_takes_no_part_and_raises_nothing():
    lg, tg = make_case('bad_label', 1000, 19, np.random.RandomState(6))
    assert (tg[tg != 255] >= 19).sum() >= 1
    rec, G, fl = run_fwd(lg, tg, 255, 1.0, 1.0)
    assert fl == 0                                                      # CE reports such a label through its own flag bit
    tg2 = tg.copy(); tg2[(tg != 255) & (tg >= 19)] = 255
    rec2, G2, _ = run_fwd(lg, tg2, 255, 1.0, 1.0)
    assert _bits(host(rec)) == _bits(host(rec2)) and np.array_equal(G, G2)


@pytest.mark.parametrize('lam,smooth', [(0.0, 1.0), (-1.0, 1.0), (float('nan'), 1.0), (float('inf'), 1.0), (1.0, -1.0), (1.0, float('nan')), (1.0, float('inf'))])
def test_a_bad_lambda_or_smooth_is_an_error_and_writes_nothing(lam, smooth):
    lg, tg = make_case('randn', 300, 19, np.random.RandomState(4))
    rec, G, fl = run_fwd(lg, tg, 255, lam, smooth, expect_error=True)
    assert bool((rec == 7.0).all()) and fl == 0


def test_a_larger_input_spans_many_chunks():
    # 300 007 pixels: 1172 tiles in 1024 chunks of two tiles, the trailing chunks empty, the last tile ragged
    C, P = 19, 300007
    rs = np.random.RandomState(8)
    lg, tg = DR.make_overlap(P, C, rs)
    rec, G, fl = run_fwd(lg, tg, 255, 1.0, 1.0)
    check_record(rec, G, lg, tg, 255, 1.0, 1.0, 'P=300007')
    check_dice_grad(run_bwd(lg, tg, 255, rec), lg, tg, 255, 1.0, 1.0, 'P=300007')


# ------------------------------------------------------------------------------------------------------------------------------ fused backward
def run_D(x, wgt, logits, target, ii, w, rec, ftg, ftw, ft):
    """-> (four-call results (dx, dw, db, dl of CE + Dice, flag), one-call results (dx, dw, db)): dsrl_ce_fused_w -> dsrl_dice_bwd(accumulate = 1) ->
    dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd against dsrl_convt2x2_bwd_ce_d"""
    call, query = _lib()
    N, H, W, C = x.shape
    P = N * 4 * H * W
    st = HF._stream()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    wsb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=DEV)
    assert query('dsrl_convt2x2_bwd_ce_supported', x.data_ptr(), logits.data_ptr(), target.data_ptr(), N, H, W, C, C) == 1
    scal = torch.zeros(8, device=DEV); dl = torch.empty_like(logits)
    ws = torch.empty(query('dsrl_ce_fused_w_workspace_bytes', P), dtype=torch.uint8, device=DEV)
    wt = table(w)
    call('dsrl_ce_fused_w', logits.data_ptr(), C, target.data_ptr(), P, C, ii, wt.data_ptr(), dl.data_ptr(), C, scal.data_ptr(), flag.data_ptr(),
         ws.data_ptr(), ws.numel(), st)
    call('dsrl_dice_bwd', logits.data_ptr(), C, target.data_ptr(), P, C, ii, rec.data_ptr(), 1, dl.data_ptr(), C, st)
    dl_loss = dl.clone()
    if ft:
        dwf = torch.empty(C, device=DEV)
        wsf = torch.empty(query('dsrl_pointwise_strided_bwd_workspace_bytes', N, 2 * H, 2 * W, C, ft), dtype=torch.uint8, device=DEV)
        call('dsrl_pointwise_strided_bwd', logits.data_ptr(), ftw.data_ptr(), ftg.data_ptr(), dl.data_ptr(), dwf.data_ptr(), 1, N, 2 * H, 2 * W, C, ft,
             wsf.data_ptr(), wsf.numel(), st)
    dx = torch.empty_like(x); dw = torch.empty_like(wgt); db = torch.empty(C, device=DEV)
    call('dsrl_convt2x2_bwd', x.data_ptr(), wgt.data_ptr(), dl.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    dx2 = torch.full_like(x, 7.0); dw2 = torch.full_like(wgt, 7.0); db2 = torch.full((C,), 7.0, device=DEV)
    ftp = (None, None) if not ft else (ftg.data_ptr(), ftw.data_ptr())
    call('dsrl_convt2x2_bwd_ce_d', x.data_ptr(), wgt.data_ptr(), logits.data_ptr(), target.data_ptr(), ii, wt.data_ptr(), rec.data_ptr(), scal.data_ptr() + 4,
         ftp[0], ftp[1], ft, dx2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    torch.cuda.synchronize()
    return (dx, dw, db, dl_loss, int(flag)), (dx2, dw2, db2)


@pytest.mark.parametrize('weights', ['weights', 'ones'])
@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('N,H', [(1, 3), (2, 5)])
@pytest.mark.parametrize('case', ['overlap', 'bad_label'])
def test_fused_backward_is_the_unfused_sequence(case, N, H, ft, weights, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    W, C, ii, lam, smooth = 128, 19, 255, 1.0, 1.0
    P = N * 4 * H * W
    rs = np.random.RandomState(CASES.index(case) + ft + 1000 * (N - 1) + (weights == 'ones'))
    lg, tg = dice_case(case, P, C, rs)
    w = make_weights(C, rs) if weights == 'weights' else np.ones(C, np.float32)
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wgt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor(lg.reshape(N, 2 * H, 2 * W, C), device=DEV)
    target = torch.tensor(tg.reshape(N, 2 * H, 2 * W), device=DEV)
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    rec, _, _ = run_fwd(lg, tg, ii, lam, smooth)
    res = {}
    for waves in (None, '8'):                   # one wave build: both settings, the same bytes
        if waves is None:
            monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
        else:
            monkeypatch.setenv('DSRL_CONVT_CE_WAVES', waves)
        (dx, dw, db, dl_loss, fl), (dx2, dw2, db2) = run_D(x, wgt, logits, target, ii, w, rec, ftg, ftw, ft)
        assert fl == (2 if case == 'bad_label' else 0)
        assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2), f'waves={waves}: the one call differs from the four'
        res[waves] = (dx2, dw2, db2)
    assert all(_bits_equal(a, b) for a, b in zip(res[None], res['8']))
    if case == 'bad_label':                     # the launch completed; a label >= C has weight 0 and no Dice row: a finite gradient
        assert bool(torch.isfinite(dx2).all())
        return
    _, gce, _ = reference(lg, tg, ii, w)
    _, gd, _, a, b, _ = dice_reference(lg, tg, ii, lam, smooth)
    assert np.abs(gd).max() > 100 * GRAD_TOL * float((np.abs(a) + np.abs(b)).max())     # the Dice row is there to be missed
    g64 = (gce + gd).reshape(N, 2 * H, 2 * W, C).copy()
    check(host(dl_loss), g64, 1e-5, 'CE + Dice row')
    if ft:
        g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
    dxo_, dwo_, dbo_ = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(wgt).astype(np.float64), g64.transpose(0, 3, 1, 2),
                                                  has_bias=True)
    check(host(dx2).transpose(0, 3, 1, 2), dxo_, 1e-5, 'dx'); check(host(dw2), dwo_, 1e-5, 'dw'); check(host(db2), dbo_, 1e-5, 'db')
    # and without the Dice row the result is another one: the weighted entry point on the same inputs
    from ce_variant_runners import run_D_one
    scal = torch.zeros(8, device=DEV)
    call, query = _lib()
    ws = torch.empty(query('dsrl_ce_fused_w_workspace_bytes', P), dtype=torch.uint8, device=DEV)
    call('dsrl_ce_fused_w', logits.data_ptr(), C, target.data_ptr(), P, C, ii, table(w).data_ptr(), None, C, scal.data_ptr(), None, ws.data_ptr(), ws.numel(),
         HF._stream())
    dxw, _, _ = run_D_one('_w', x, wgt, logits, target, ii, w, None, scal, ftg, ftw, ft)
    assert not _bits_equal(dxw, dx2)


# ------------------------------------------------------------------------------------------------------------------------------ head: hand-over, gradients
@pytest.mark.parametrize('weights', ['weights', 'none'])
def test_dice_fused_losses_on_the_head_hands_over_and_matches_autograd(weights, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    w = make_weights(19, np.random.RandomState(17)) if weights == 'weights' else None
    dice = (0.7, 1.0)

    def step(mode):
        """'plain': no hand-over, no gradient slots, HF.cross_entropy + HF.dice_loss + mse + FA through autograd; 'fused': fused_losses(dice=);
        'second': fused_losses(dice=) while another consumer sends the logits a gradient of its own (zeros): the unfused branch of the backward"""
        monkeypatch.setattr(HF, 'convt_ce_enabled', mode != 'plain')
        monkeypatch.setattr(HF, 'grad_slots_enabled', mode != 'plain')
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        tgt = dev(target); o = dev(org)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        calls = []
        if mode == 'plain':
            outs = head(a, b)
            ce = HF.cross_entropy(outs[0], tgt, gen.IGNORE, weight=w) + HF.dice_loss(outs[0], tgt, gen.IGNORE, *dice)
            total = ce + 0.1 * HF.mse_loss(outs[1], o) + 1.0 * D.FALoss()(outs[2], outs[3])
            total.backward()
            ce, tot = float(ce.detach()), float(total.detach())
        else:
            with HF.logits_target(tgt, gen.IGNORE, flag, w, dice=dice):
                outs = head(a, b)
            h = getattr(outs[0], '_dsrl_logits_grad', None)
            assert h is not None and h.value is not None, 'the forward did not evaluate the CE value'
            orig = HF.call
            monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
            vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=w, dice=dice)
            assert h.armed and h.dice is not None and h.weight is not None, 'the hand-over did not engage'
            assert 'dsrl_dice_fwd' in calls and 'dsrl_dice_bwd' not in calls and not any(c.startswith('dsrl_ce_fused') for c in calls), calls
            assert vals.grad_fn.grads[0] is None, 'fused_losses allocated the logits gradient'
            if mode == 'second':
                torch.autograd.backward([vals, outs[0]], [torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=DEV), torch.zeros_like(outs[0])])
            else:
                vals[3].backward()
            monkeypatch.setattr(HF, 'call', orig)
            assert not h.armed and h.dice is None and h.weight is None, 'holder left armed'
            if mode == 'fused':
                assert 'dsrl_convt2x2_bwd_ce_d' in calls and 'dsrl_dice_bwd' not in calls, calls
            else:
                assert 'dsrl_convt2x2_bwd_ce_d' not in calls and calls.count('dsrl_dice_bwd') == 1 and 'dsrl_ce_fused_w' in calls, calls
            ce, tot = float(vals[0]), float(vals[3])
        torch.cuda.synchronize()
        assert int(flag) == 0
        return {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad), ce, tot, host(outs[0])

    ref = step('plain')
    for mode in ('fused', 'second'):
        got = step(mode)
        for k in ref[0]:
            check(got[0][k], ref[0][k], 1e-6, f'{mode}: grad {k}')
        check(got[1], ref[1], 1e-6, 'dx16'); check(got[2], ref[2], 1e-6, 'dx4')
        assert abs(got[3] - ref[3]) <= 2e-6 * abs(ref[3]) and abs(got[4] - ref[4]) <= 2e-6 * abs(ref[4]), (mode, got[3:5], ref[3:5])
    # the value against float64 on the head's own logits: CE + lambda L_dice, and the Dice part is not small
    lg = got[5].transpose(0, 2, 3, 1).reshape(-1, 19)
    tgh = target.reshape(-1).astype(np.uint8)
    wref = w if w is not None else np.ones(19, np.float32)
    ce_ref = reference(lg, tgh, gen.IGNORE, wref)[0]
    d_ref = dice_reference(lg, tgh, gen.IGNORE, *dice)[0]
    live = tgh != gen.IGNORE
    tol = LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max())) + 1e-6 * dice[0]
    print(f'head: CE + Dice {got[3]!r} ref {ce_ref + d_ref!r} error / bound = {abs(got[3] - ce_ref - d_ref) / tol:.3f}')
    assert abs(got[3] - (ce_ref + d_ref)) <= tol
    assert d_ref > 0.1 * dice[0]


# ------------------------------------------------------------------------------------------------------------------------------ TrainStep
def _model_and_step(graph, **kw):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(77)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    HF.set_dropout_seed(1234)
    return model, TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph, **kw)


def _batch():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    return next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))


def test_train_step_with_dice_captured_equals_eager_and_validation_keeps_the_ce():
    (img, org), (tgt, _) = _batch()
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, dice=True)
        assert step.dice == (1.0, 1.0)
        n = step.GRAPH_WARMUP + 2                                       # graph: the eager iterations, the capture, then a replay
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        if graph:
            assert step.graph_replays >= 1, 'the step with the Dice term was not captured and replayed'
        else:
            five, outs = _five(step, img, org, tgt, do_train=False)    # validation: the configured CE, no Dice term
            lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            tgh = tgt.cpu().numpy().reshape(-1)
            ce_ref = reference(lg, tgh, 255, np.ones(19, np.float32))[0]
            d_ref = dice_reference(lg, tgh, 255, 1.0, 1.0)[0]
            live = tgh != 255
            tol = LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max()))
            assert abs(float(five[0]) - ce_ref) <= tol, (five[0], ce_ref)
            assert d_ref > 100 * tol
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


def test_the_training_ce_figure_includes_the_dice_term():
    (img, org), (tgt, _) = _batch()
    tgh = tgt.cpu().numpy().reshape(-1)
    for fused in (True, False):
        model, step = _model_and_step(False, dice=(0.5, 1.0))
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
        ce_ref = reference(lg, tgh, 255, np.ones(19, np.float32))[0]
        d_ref = dice_reference(lg, tgh, 255, 0.5, 1.0)[0]
        live = tgh != 255
        tol = LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max())) + 1e-6 * 0.5
        print(f'fused_losses={fused}: CE + Dice {float(five[0])!r} ref {ce_ref + d_ref!r} error / bound = {abs(float(five[0]) - ce_ref - d_ref) / tol:.3f}')
        assert abs(float(five[0]) - (ce_ref + d_ref)) <= tol
        assert d_ref > 100 * tol
        step.release()


def test_off_is_the_step_built_without_the_argument():
    (img, org), (tgt, _) = _batch()
    res = []
    for kw in ({}, {'dice': None}, {'dice': False}, {'dice': 0}):
        model, step = _model_and_step(False, **kw)
        assert step.dice is None
        calls = []
        orig = HF.call
        HF.call = lambda name, *args: (calls.append(name), orig(name, *args))[1]
        try:
            fives = [_five(step, img, org, tgt)[0].tobytes() for _ in range(2)]
        finally:
            HF.call = orig
        torch.cuda.synchronize()
        res.append((fives, calls, [p.detach().clone() for p in model.parameters()]))
        step.release()
    for fives, calls, params in res[1:]:
        assert fives == res[0][0] and calls == res[0][1]
        assert all(_bits_equal(p, q) for p, q in zip(params, res[0][2]))
    assert not any('dice' in c or c.endswith('_d') for c in res[0][1])


def test_check_dice_reads_the_dataset():
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    assert TR.check_dice({'settings': cs}) is None
    assert TR.check_dice({'settings': cs, 'dice': {'weight': 0.5}}) == (0.5, 1.0)

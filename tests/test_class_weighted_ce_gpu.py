"""Class-weighted cross entropy (nn.CrossEntropyLoss(weight=, ignore_index=)) through the four paths of the training step, each against an
INDEPENDENT reference: torch.nn.functional.cross_entropy(x64, t, weight=w64, ignore_index) on CPU in float64, fed the same fp32 logits and
fp32 weights, gradient from CPU autograd.

    A  dsrl_ce_fwd_w / dsrl_ce_bwd_w     HF.cross_entropy(weight=)
    B  dsrl_ce_fused_w                   the loss pass of HF.fused_losses(weight=)
    C  dsrl_convt2x2_fwd_ce_w            the value inside the last ConvTranspose forward (HF.logits_target(weight=))
    D  dsrl_convt2x2_bwd_ce_w            the gradient formed inside the ConvTranspose backward (HF.LogitsGrad.weight), both wave builds

Shapes and cases are those of test_cross_entropy_edges.py (its make_case).  Weights: uniform(0.25, 8) with one class at 0.

Tolerances (fixed):
    loss       1e-6 |ref| + 2 ulp(max |m|): the bound of the unweighted tests - a weighted mean of per-pixel errors cannot exceed the largest one
    gradient   (2^-20 + 2^-22) * w[t_i] / D per element: the unweighted 2^-20 x scale, plus four fp32 roundings (D, its reciprocal, the product
               with w and one to spare); ignored pixels exactly 0
    D          loss_out[1] == np.float32(sum over c ascending of n_c * float64(w_c)), exactly
    D path     dx, dw, db bit-identical to dsrl_ce_fused_w -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd; 1e-5 of the range against the fp64
               gradient pushed through oracle.conv_transpose2d_k2s2_bwd
All-ones weights must give the bits of the unweighted entry points (w * scale == scale, (double)1 * nll == nll), and every weighted entry point
the same bytes when it runs twice."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gen                     # noqa: E402
import oracle as O             # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402
from ce_variant_runners import _place, table, run_A_w as run_A, run_B_w as run_B, run_C_w as run_C, run_D_w as run_D   # noqa: E402,F401
from test_cross_entropy_edges import check_loss, make_case     # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402

GRAD_TOL = 2.0 ** -20 + 2.0 ** -22          # x w[t_i] / D, per gradient element
CASES = ['randn', 'spread', 'offset_1e4', 'onehot', 'bad_label']
IGNORES = [255, 0, 18, -1]


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def make_weights(C, rs, zero=None):
    w = rs.uniform(0.25, 8.0, C).astype(np.float32)
    w[rs.randint(C) if zero is None else zero] = 0.0
    return w


def case_for(case, P, C, rs, ii):
    if case == 'bad_label' and P == 1:          # make_case needs a live pixel to relabel; one pixel: relabel it directly (C is never an ignore index here)
        lg, tg = make_case('randn', P, C, rs, ii)
        tg[0] = C
        return lg, tg
    return make_case(case, P, C, rs, ii)


def expected_D(tg, ii, w):
    """np.float32(sum over c ascending of n_c * float64(w_c)), n_c from integer counts of the live pixels"""
    t = tg.astype(np.int64)
    n = np.bincount(t[t != ii], minlength=256)
    d = 0.0
    for c in range(len(w)):
        d += float(n[c]) * float(np.float64(w[c]))
    return np.float32(d)


def reference(lg, tg, ii, w):
    """-> (loss, gradient (P, C), D as float64): torch CPU float64 on the same fp32 logits and fp32 weights"""
    x = torch.tensor(lg.astype(np.float64), requires_grad=True)
    t = torch.tensor(tg.astype(np.int64))
    loss = F.cross_entropy(x, t, weight=torch.tensor(w.astype(np.float64)), ignore_index=ii, reduction='mean')
    loss.backward()
    live = tg.astype(np.int64) != ii
    return float(loss), x.grad.numpy(), float(w.astype(np.float64)[tg[live]].sum())


def check_grad(g, gref, tg, ii, w, Dref, name):
    live = tg.astype(np.int64) != ii
    assert np.all(g[~live] == 0), f'{name}: nonzero gradient on an ignored pixel'
    err = np.abs(g[live].astype(np.float64) - gref[live])
    bound = GRAD_TOL * w.astype(np.float64)[tg[live]] / Dref
    print(f'{name}: max gradient error / bound = {float((err / np.maximum(bound, 1e-300)[:, None]).max(initial=0.0)):.3f}')
    assert not np.isnan(err).any(), f'{name}: NaN in the gradient of a live pixel'
    assert np.all(err <= bound[:, None]), f'{name}: gradient error {err.max():.3e} beyond (2^-20 + 2^-22) w / D'


def check_against_reference(L, Dgot, g, lg, tg, ii, w, case, name):
    assert np.float32(Dgot) == expected_D(tg, ii, w), (name, Dgot, expected_D(tg, ii, w))
    if case == 'bad_label':
        assert np.isnan(L), (name, L)
        return
    ref, gref, Dref = reference(lg, tg, ii, w)
    if Dref == 0.0:                             # no live pixel, or all of them in the zero-weight class: 0 / 0 = NaN, as torch
        assert np.isnan(L) and np.isnan(ref) and Dgot == 0.0, (name, L, ref, Dgot)
        return
    print(f'{name}: loss {L!r} ref {ref!r}')
    check_loss(L, ref, lg, tg, ii, name)
    if g is not None:
        check_grad(g, gref, tg, ii, w, Dref, name)


# ------------------------------------------------------------------------------------------------------------------------------ paths A and B
@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('case', CASES)
def test_paths_A_and_B_weighted(case, C):
    for P in (300, 1):
        for ii in IGNORES:
            for layout in ('dense', 'slice'):
                rs = np.random.RandomState(1000 * C + 100 * CASES.index(case) + 10 * IGNORES.index(ii) + P % 7 + (layout == 'slice'))
                lg, tg = case_for(case, P, C, rs, ii)
                w = make_weights(C, rs)
                name = f'{case} C={C} P={P} ii={ii} {layout}'
                La, Da, ga = run_A(lg, tg, ii, w, layout)
                check_against_reference(La, Da, None if case == 'bad_label' else ga, lg, tg, ii, w, case, 'A ' + name)
                Lb, Db, fl, gb = run_B(lg, tg, ii, w, layout)
                assert fl == (2 if case == 'bad_label' else 0), (name, fl)
                check_against_reference(Lb, Db, gb, lg, tg, ii, w, case, 'B ' + name)
                assert np.float32(Da).tobytes() == np.float32(Db).tobytes(), 'A and B disagree on D'
                if case == 'bad_label':         # the backward launches completed; a label >= C has weight 0 in B (zeros), a NaN row in A (as unweighted)
                    bad = (tg.astype(np.int64) != ii) & (tg >= C)
                    assert np.isnan(ga[bad]).all() and not np.isnan(ga[~bad]).any()
                    assert Db == 0.0 or not np.isnan(gb).any()          # (D = 0, the one pixel of P = 1: 0 * (1 / 0), as torch's 0 / 0)


def test_every_live_pixel_in_the_zero_weight_class_is_nan():
    C, P = 19, 300
    rs = np.random.RandomState(5)
    lg, tg = make_case('randn', P, C, rs, 255)
    live = tg != 255
    tg[live] = 4
    w = make_weights(C, rs, zero=4)
    for run in (run_A, run_B):
        r = run(lg, tg, 255, w)
        assert np.isnan(r[0]) and r[1] == 0.0, r[:2]
    ref, _, _ = reference(lg, tg, 255, w)
    assert np.isnan(ref)


def test_weight_sum_prepass_and_large_counts():
    # the pre-pass alone: 300007 labels over several blocks, the buffer 7 bytes past a 16-byte boundary (head and tail bytes), labels outside the
    # classes (weight 0), an ignore index that is a class and one no label matches
    call, query = _lib()
    C, P, off = 19, 300007, 7
    rs = np.random.RandomState(11)
    tgn = rs.randint(0, C + 2, P).astype(np.uint8)          # C and C + 1: outside the classes, weight 0
    tgn[rs.uniform(size=P) < 0.1] = 255
    w = make_weights(C, rs)
    big = torch.zeros(P + 64, dtype=torch.uint8, device=DEV)
    tgt = big[off:off + P]; tgt.copy_(torch.tensor(tgn, device=DEV))
    ws = torch.empty(query('dsrl_ce_weight_sum_workspace_bytes'), dtype=torch.uint8, device=DEV)
    for ii in (255, 3, -1):
        d = torch.full((2,), 7.0, device=DEV)
        call('dsrl_ce_weight_sum', tgt.data_ptr(), P, C, ii, table(w).data_ptr(), d.data_ptr(), ws.data_ptr(), ws.numel(), HF._stream())
        torch.cuda.synchronize()
        got = host(d)
        assert got[1] == 7.0 and np.float32(got[0]) == expected_D(tgn, ii, w), (ii, got, expected_D(tgn, ii, w))


# ------------------------------------------------------------------------------------------------------------------------------ identity: all-ones weights, twice
def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()


@pytest.mark.parametrize('C,layout', [(19, 'dense'), (3, 'slice')])
@pytest.mark.parametrize('case', ['randn', 'spread', 'offset_1e4', 'onehot'])
def test_all_ones_weights_are_the_unweighted_bits_and_runs_repeat(case, C, layout):
    for P, ii in ((300, 255), (1, 255), (300, 0), (300, -1)):
        rs = np.random.RandomState(31 * C + CASES.index(case) + P + (ii & 0xff))
        lg, tg = make_case(case, P, C, rs, ii)
        ones = np.ones(C, np.float32)
        for run in (run_A, run_B):
            u = run(lg, tg, ii, None, layout)
            o = run(lg, tg, ii, ones, layout)
            assert _bits(u[0]) == _bits(o[0]) and _bits(u[1]) == _bits(o[1]) and _bits(u[-1]) == _bits(o[-1]), (run.__name__, case, P, ii)
            w = make_weights(C, rs)
            r1 = run(lg, tg, ii, w, layout); r2 = run(lg, tg, ii, w, layout)
            assert _bits(r1[0]) == _bits(r2[0]) and _bits(r1[1]) == _bits(r2[1]) and _bits(r1[-1]) == _bits(r2[-1])


# ------------------------------------------------------------------------------------------------------------------------------ path C
@pytest.mark.parametrize('case,ii', [(c, 255) for c in ('randn', 'spread', 'offset_1e4', 'onehot', 'bad_label')] + [('randn', ii) for ii in (0, 18, -1)])
def test_path_C_weighted_value_inside_the_convT_forward(case, ii, monkeypatch):
    call, query = _lib()
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    N, H, W, C = 1, 3, 200, 19
    P = N * 4 * H * W
    rs = np.random.RandomState(CASES.index(case) + 7 * (ii & 0xff))
    x = (rs.standard_normal((N, H, W, C)) * 0.5).astype(np.float32)
    wgt = (rs.standard_normal((C, C, 2, 2)) * 0.5).astype(np.float32)
    b = rs.standard_normal(C).astype(np.float32)
    tg = rs.randint(0, C, (N, 2 * H, 2 * W)).astype(np.int64)
    if 0 <= ii <= 255:
        tg[rs.uniform(size=tg.shape) < 0.1] = ii
    live = tg != ii
    if case == 'spread':
        b[3] = 3e38; b[4] = -3e38; tg[live & (tg == 4)] = 3
    elif case == 'offset_1e4':
        b += np.float32(1e4)
    elif case == 'onehot':
        wgt[:] = 0; b[:] = -100; b[4] = 100
    elif case == 'bad_label':
        tg[0, 0, 1] = 200
    tg = tg.astype(np.uint8)
    w = make_weights(C, rs)
    xt = torch.tensor(x, device=DEV); wt = torch.tensor(wgt, device=DEV); bt = torch.tensor(b, device=DEV)
    assert query('dsrl_convt2x2_fwd_ce_supported', xt.data_ptr(), xt.data_ptr(), N, H, W, C, C) == 1
    y0 = torch.empty((N, 2 * H, 2 * W, C), device=DEV)
    call('dsrl_convt2x2_fwd', xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y0.data_ptr(), N, H, W, C, C, HF._stream())
    y1, L, Dg, fl = run_C(x, wgt, b, tg, ii, w)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))          # the logits themselves, bit for bit
    lg = host(y1).reshape(P, C)
    LB, DB, flB, _ = run_B(lg, tg.reshape(P), ii, w, want_grad=False)      # path B on the same logits: the same D, as floats, and the same flag
    assert _bits(Dg) == _bits(DB) and fl == flB == (2 if case == 'bad_label' else 0)
    check_against_reference(L, Dg, None, lg, tg.reshape(P), ii, w, case, f'C {case} ii={ii}')
    check_against_reference(LB, DB, None, lg, tg.reshape(P), ii, w, case, f'B on C {case} ii={ii}')
    # all-ones weights: the unweighted call's bits (not with a label outside the classes: the table gives it weight 0, so D is the count less
    # that pixel - both losses are NaN and flagged all the same); and the weighted call twice
    yu, Lu, nu, flu = run_C(x, wgt, b, tg, ii, None)
    yo, Lo, no, flo = run_C(x, wgt, b, tg, ii, np.ones(C, np.float32))
    assert _bits(Lu) == _bits(Lo) and flu == flo and torch.equal(yu.view(torch.int32), yo.view(torch.int32))
    assert _bits(nu) == _bits(no) if case != 'bad_label' else no == nu - 1
    y2, L2, D2, fl2 = run_C(x, wgt, b, tg, ii, w)
    assert _bits(L) == _bits(L2) and _bits(Dg) == _bits(D2) and fl == fl2


# ------------------------------------------------------------------------------------------------------------------------------ path D
def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('waves', [None, '8'])
@pytest.mark.parametrize('case,ii', [(c, 255) for c in ('randn', 'spread', 'onehot', 'bad_label')] + [('randn', ii) for ii in (0, 18, -1)])
def test_path_D_weighted_gradient_inside_the_convT_backward(case, ii, waves, ft, monkeypatch):
    _check_path_D(case, ii, waves, ft, 1, 3, monkeypatch)


@pytest.mark.parametrize('waves', [None, '8'])
def test_path_D_weighted_transformer_rows_and_images(waves, monkeypatch):
    # N = 2, H = 5: output rows 0 and 8 are on the stride-8 grid (row 1 of the transformer's gradient) and the second image's rows follow the first's
    _check_path_D('randn', 255, waves, 8, 2, 5, monkeypatch)


def _check_path_D(case, ii, waves, ft, N, H, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    if waves is None:
        monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
    else:
        monkeypatch.setenv('DSRL_CONVT_CE_WAVES', waves)
    W, C = 128, 19
    P = N * 4 * H * W
    rs = np.random.RandomState(CASES.index(case) + 11 * (ii & 0xff) + ft + 1000 * (N - 1))
    lg, tg = make_case(case, P, C, rs, ii)
    w = make_weights(C, rs)
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wgt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor(lg.reshape(N, 2 * H, 2 * W, C), device=DEV)
    target = torch.tensor(tg.reshape(N, 2 * H, 2 * W), device=DEV)
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    (dx, dw, db, dl_ce, fl), (dx2, dw2, db2) = run_D(x, wgt, logits, target, ii, w, ftg, ftw, ft)
    assert fl == (2 if case == 'bad_label' else 0)
    assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2)
    (_, _, _, _, _), (dx3, dw3, db3) = run_D(x, wgt, logits, target, ii, w, ftg, ftw, ft)           # twice: the same bytes
    assert _bits_equal(dx2, dx3) and _bits_equal(dw2, dw3) and _bits_equal(db2, db3)
    if case == 'bad_label':                     # the launch completed; a label >= C has weight 0: a finite gradient (and D is not the pixel count,
        assert bool(torch.isfinite(dx2).all())  # so all-ones weights are not the unweighted bits here)
        return
    # all-ones weights: the unweighted one-call's bits
    (_, _, _, _, _), (dxu, dwu, dbu) = run_D(x, wgt, logits, target, ii, None, ftg, ftw, ft)
    (_, _, _, _, _), (dxo, dwo, dbo) = run_D(x, wgt, logits, target, ii, np.ones(C, np.float32), ftg, ftw, ft)
    assert _bits_equal(dxu, dxo) and _bits_equal(dwu, dwo) and _bits_equal(dbu, dbo)
    ref, g64, Dref = reference(lg, tg, ii, w)
    check_grad(host(dl_ce).reshape(P, C), g64, tg, ii, w, Dref, f'D {case} ii={ii}')
    g64 = g64.reshape(N, 2 * H, 2 * W, C)
    if ft:
        g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
    dxo_, dwo_, dbo_ = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(wgt).astype(np.float64), g64.transpose(0, 3, 1, 2),
                                                  has_bias=True)
    check(host(dx2).transpose(0, 3, 1, 2), dxo_, 1e-5, 'dx'); check(host(dw2), dwo_, 1e-5, 'dw'); check(host(db2), dbo_, 1e-5, 'db')


# ------------------------------------------------------------------------------------------------------------------------------ dsrl_class_histogram
def test_class_histogram_with_a_lut_off_alignment_accumulates():
    call, _ = _lib()
    rs = np.random.RandomState(9)
    lab = rs.randint(0, 256, (3, 37, 53)).astype(np.uint8)
    lab[rs.uniform(size=lab.shape) < 0.5] = 7                   # one heavy bin (a wave's lanes meet in it)
    lut = rs.randint(0, 256, 256).astype(np.uint8)
    big = torch.zeros(lab.size + 64, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    lut_d = torch.tensor(lut, device=DEV)
    for off in (5, 0):
        view = big[off:off + lab.size]
        view.copy_(torch.tensor(lab.reshape(-1), device=DEV))
        counts = torch.zeros(256, dtype=torch.int64, device=DEV)
        call('dsrl_class_histogram', view.data_ptr(), lab.size, lut_d.data_ptr(), counts.data_ptr(), HF._stream())
        torch.cuda.synchronize()
        want = np.bincount(lut[lab.reshape(-1)], minlength=256)
        assert np.array_equal(counts.cpu().numpy(), want)
        call('dsrl_class_histogram', view.data_ptr(), lab.size, None, counts.data_ptr(), HF._stream())          # accumulates; no LUT: the raw bytes
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want + np.bincount(lab.reshape(-1), minlength=256))
        assert int(counts.sum()) == 2 * lab.size


# ------------------------------------------------------------------------------------------------------------------------------ head: hand-over, gradients, memory
def test_weighted_fused_losses_on_the_head_hands_over_and_matches_autograd(monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    w = make_weights(19, np.random.RandomState(17))
    logits_bytes = 2 * 19 * 64 * 256 * 4

    def step(mode):
        """'plain': no hand-over, no gradient slots, HF.cross_entropy(weight=) + mse + FA through autograd; 'fused' / 'unweighted': fused_losses"""
        monkeypatch.setattr(HF, 'convt_ce_enabled', mode != 'plain')
        monkeypatch.setattr(HF, 'grad_slots_enabled', mode != 'plain')
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        tgt = dev(target); o = dev(org)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        wt = None if mode == 'unweighted' else w
        if mode == 'plain':
            outs = head(a, b)
            total = HF.cross_entropy(outs[0], tgt, gen.IGNORE, weight=w) + 0.1 * HF.mse_loss(outs[1], o) + 1.0 * D.FALoss()(outs[2], outs[3])
            total.backward()
            ce = None
        else:
            with HF.logits_target(tgt, gen.IGNORE, flag, wt):
                outs = head(a, b)
            vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=wt)
            h = getattr(outs[0], '_dsrl_logits_grad', None)
            assert h is not None and h.armed, 'the hand-over did not engage'
            assert (h.weight is None) == (wt is None)
            assert h.value is not None and vals is not None            # the producing layer evaluated the (weighted) value in its forward
            vals[3].backward()
            assert not h.armed, 'holder left armed'
            ce = float(vals[0])
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert int(flag) == 0
        return {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad), ce, peak, host(outs[0])

    ref = step('plain')
    step('fused'); step('unweighted')           # the allocator and the workspaces are warm before the peaks are compared
    got = step('fused')
    unw = step('unweighted')
    for k in ref[0]:
        check(got[0][k], ref[0][k], 1e-6, f'grad {k}')
    check(got[1], ref[1], 1e-6, 'dx16'); check(got[2], ref[2], 1e-6, 'dx4')
    lg = got[5].transpose(0, 2, 3, 1).reshape(-1, 19)
    ce_ref, _, _ = reference(lg, target.reshape(-1), gen.IGNORE, w)
    check_loss(got[3], ce_ref, lg, target.reshape(-1), gen.IGNORE, 'head CE')
    assert abs(got[3] - unw[3]) > 1e-3                                  # ... and it is not the unweighted value
    print(f'peak above the start of the step: weighted {got[4]}, unweighted {unw[4]}, logits {logits_bytes}')
    assert got[4] - unw[4] < logits_bytes, 'the weighted step allocated a logits-sized tensor the unweighted step does not'


# ------------------------------------------------------------------------------------------------------------------------------ TrainStep, train_or_resume
def _model_and_step(graph, w):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(77)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    HF.set_dropout_seed(1234)
    return model, TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph, class_weights=w)


def _five(step, img, org, tgt, do_train=True):
    """the five scalars of one iteration as they reach the host: CE, w1 MSE, w2 FA, total, NaN flag"""
    while step._pending:
        step.collect()
    outs = step.enqueue(img, org, tgt, 0.006, 0.9, 5e-4, do_train)
    hostbuf, ev = step._pending[-1]
    ev.synchronize()
    five = hostbuf.clone().numpy()
    step.collect()
    return five, outs


def test_train_step_with_class_weights_captured_equals_eager():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    w = make_weights(19, np.random.RandomState(23))
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, w)
        n = step.GRAPH_WARMUP + 3                                       # graph: two eager iterations, the capture, then replays
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        if graph:
            assert step.graph_replays >= 2, 'the weighted step was not captured and replayed'
        else:
            five, outs = _five(step, img, org, tgt, do_train=False)    # validation: the weighted CE too
            lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            tgh = tgt.cpu().numpy().reshape(-1)
            ce_ref, _, _ = reference(lg, tgh, 255, w)
            check_loss(float(five[0]), ce_ref, lg, tgh, 255, 'do_train=False')
            ce_unw = float(F.cross_entropy(torch.tensor(lg.astype(np.float64)), torch.tensor(tgh.astype(np.int64)), ignore_index=255))
            assert abs(ce_ref - ce_unw) > 1e-3
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


def test_unfused_losses_of_the_train_step_use_the_weights():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    w = make_weights(19, np.random.RandomState(23))
    tgh = tgt.cpu().numpy().reshape(-1)
    for fused in (True, False):
        model, step = _model_and_step(False, w)
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
        ce_ref, _, _ = reference(lg, tgh, 255, w)
        check_loss(float(five[0]), ce_ref, lg, tgh, 255, f'fused_losses={fused}')
        step.release()


def test_train_or_resume_with_enet_weights_counts_once(tmp_path, monkeypatch):
    from test_augment_gpu import _cache_tree
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import train_or_resume
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import class_weights as CW, loader as L, settings as cs
    from dualsuperreslearningforsemseg_amd.models.transforms import DeviceBatchPreparation
    data, _ = _cache_tree(tmp_path)
    calls = []
    orig = CW.call
    monkeypatch.setattr(CW, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])

    def run(tag):
        torch.manual_seed(1234)
        HF.set_dropout_seed(77)
        kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                  dataset={'path': data, 'settings': cs, 'class_weights': 'enet'}, val_interval=1, checkpoint_interval=1, checkpoint_history=2,
                  init_weights=None, batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9, weights_decay=5e-4,
                  poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / tag), description='test',
                  early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))
        return train_or_resume(is_resuming_training=False, **kw)

    h1 = run('a')
    path = os.path.join(data, 'dsrl_u8_cache', 'class_counts_train.json')
    assert os.path.isfile(path) and calls.count('dsrl_class_histogram') == 1        # four images: one chunk
    with open(path) as f:
        rec = json.load(f)
    cache = L.CityscapesCache(os.path.join(data, 'dsrl_u8_cache'), 'train')
    lut = DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, (32, 64), cs.IGNORE_CLASS_LABEL).lut_host.numpy()
    assert rec['counts'] == np.bincount(lut[np.asarray(cache.labels).reshape(-1)], minlength=256).tolist()
    assert all(np.isfinite(v) for v in h1[0]['train'][:4]) and h1[0]['train'][0] > 0 and np.isfinite(h1[0]['val'][3])
    stamp = os.stat(path).st_mtime_ns
    h2 = run('b')
    assert calls.count('dsrl_class_histogram') == 1 and os.stat(path).st_mtime_ns == stamp, 'the counts file was not reused'
    assert h2[0]['train'][:4] == h1[0]['train'][:4]
    # the weights change the loss: the same run without them
    monkeypatch.setattr(CW, 'enet_weights', lambda counts: np.ones(len(counts)))
    h3 = run('c')
    assert h3[0]['train'][0] != h1[0]['train'][0]

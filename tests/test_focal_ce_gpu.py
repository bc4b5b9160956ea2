"""Focal cross entropy, term_i = w[t] (1 - p_t)^gamma (-log p_t) over D = sum w[t], through the four paths of the training step, each against the
float64 restatement of tests/focal_ref.py (fp32 logits and fp32 weights taken to float64; closed-form gradient).

    A  dsrl_ce_fwd_f / dsrl_ce_bwd_f     HF.cross_entropy(focal_gamma=)
    B  dsrl_ce_fused_f                   the loss pass of HF.fused_losses(focal_gamma=)
    C  dsrl_convt2x2_fwd_ce_f            the value inside the last ConvTranspose forward (HF.logits_target(focal_gamma=))
    D  dsrl_convt2x2_bwd_ce_f            the gradient formed inside the ConvTranspose backward (HF.LogitsGrad.gamma)

Cases: randn, spread, offset_1e4, onehot and bad_label of test_cross_entropy_edges.make_case, and `graded` (focal_ref.make_graded): p_t from about
1e-3 to about 1, at least a quarter of the live pixels with 0.1 < p_t < 0.9 (asserted), and a focal loss more than 5 % away from the weighted CE of
the same inputs (asserted: a kernel that ignores gamma fails).

Tolerances (fixed):
    loss       |L - ref| <= (1 + gamma) (1e-6 |CE_ref| + 2 ulp(max |m|)), CE_ref the float64 WEIGHTED CE of the same inputs: check_loss's bound times
               the largest sensitivity of q^gamma nll to an error in nll, q^gamma + gamma q^(gamma-1) p nll <= 1 + gamma / e
    gradient   (1 + gamma) (2^-20 + 2^-22) w[t] / D per element: the weighted bound times the same factor (mod <= 1 + gamma / e); ignored pixels 0
    D          as the weighted tests: np.float32(sum over c ascending of n_c * float64(w_c)), exactly, and the same bits from every path
    D path     dx, dw, db bit-identical to dsrl_ce_fused_f -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd; 1e-5 of the range against the float64
               gradient pushed through oracle.conv_transpose2d_k2s2_bwd.  The focal backward has one wave build (8 waves): DSRL_CONVT_CE_WAVES unset
               and '8' must give the same bytes.  The kernel takes W % 128 == 0 only (as the weighted test: W = 128, N x H = 1 x 3 and 2 x 5).
gamma == 0 must be today's bytes, a bad gamma must return an error and write nothing, and every entry point must repeat its bytes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import focal_ref as FR         # noqa: E402
import gen                     # noqa: E402
import oracle as O             # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402
from ce_variant_runners import (_convt_inputs, run_A_f as run_A, run_B_f as run_B, run_C_f as run_C, run_D_f as run_D,   # noqa: E402,F401
                                run_D_one_f as run_D_one)
from test_class_weighted_ce_gpu import (GRAD_TOL, _bits, _bits_equal, _five, _place, case_for, expected_D, make_weights,   # noqa: E402
                                        reference, table)
from test_cross_entropy_edges import LOSS_REL, M_ULPS, make_case, ulp32     # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import DsrlHipError   # noqa: E402

CASES = ['randn', 'spread', 'offset_1e4', 'onehot', 'bad_label', 'graded']
IGNORES = [255, 0, 18, -1]


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def focal_case(case, P, C, rs, ii):
    if case == 'graded':
        return FR.make_graded(P, C, rs, ii)
    return case_for(case, P, C, rs, ii)


def assert_graded(lg, tg, ii, w, gamma, name):
    """the two conditions of the graded case, on the float64 reference"""
    p = FR.target_probability(lg, tg, ii)
    frac = float(((p > 0.1) & (p < 0.9)).mean())
    assert frac >= 0.25, f'{name}: only {frac:.2f} of the live pixels have 0.1 < p_t < 0.9'
    ce = reference(lg, tg, ii, w)[0]
    fl = FR.focal_loss_and_grad(lg, tg, ii, w, gamma)[0]
    assert abs(fl - ce) > 0.05 * abs(ce), f'{name}: focal {fl} within 5 % of the weighted CE {ce}'


def check_focal_loss(L, ref, ce_ref, lg, tg, ii, gamma, name):
    if np.isinf(ref):
        assert L == ref, (name, L, ref)
        return
    live = tg.astype(np.int64) != ii
    tol = (1.0 + gamma) * (LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max())))
    print(f'{name}: loss {L!r} ref {ref!r} error / bound = {abs(L - ref) / tol:.3f}')
    assert abs(L - ref) <= tol, f'{name}: loss {L!r} vs {ref!r} (|d| = {abs(L - ref):.3e} > {tol:.3e})'


def check_focal_grad(g, gref, tg, ii, w, Dref, gamma, name):
    live = tg.astype(np.int64) != ii
    assert np.all(g[~live] == 0), f'{name}: nonzero gradient on an ignored pixel'
    err = np.abs(g[live].astype(np.float64) - gref[live])
    bound = (1.0 + gamma) * GRAD_TOL * w.astype(np.float64)[tg[live]] / Dref
    print(f'{name}: max gradient error / bound = {float((err / np.maximum(bound, 1e-300)[:, None]).max(initial=0.0)):.3f}')
    assert not np.isnan(err).any(), f'{name}: NaN in the gradient of a live pixel'
    assert np.all(err <= bound[:, None]), f'{name}: gradient error {err.max():.3e} beyond (1 + gamma) (2^-20 + 2^-22) w / D'


_refs = {}


def focal_reference(lg, tg, ii, w, gamma):
    """(focal loss, gradient, D, weighted CE) in float64, computed once per input"""
    key = (lg.tobytes(), tg.tobytes(), ii, w.tobytes(), gamma)
    if key not in _refs:
        if len(_refs) > 64:
            _refs.clear()
        _refs[key] = FR.focal_loss_and_grad(lg, tg, ii, w, gamma) + (reference(lg, tg, ii, w)[0],)
    return _refs[key]


def check_against_reference(L, Dgot, g, lg, tg, ii, w, gamma, case, name):
    assert np.float32(Dgot) == expected_D(tg, ii, w), (name, Dgot, expected_D(tg, ii, w))
    if case == 'bad_label':
        assert np.isnan(L), (name, L)
        return
    ref, gref, Dref, ce_ref = focal_reference(lg, tg, ii, w, gamma)
    if Dref == 0.0:                             # no live pixel, or all of them in the zero-weight class: 0 / 0 = NaN
        assert np.isnan(L) and np.isnan(ref) and Dgot == 0.0, (name, L, ref, Dgot)
        return
    check_focal_loss(L, ref, ce_ref, lg, tg, ii, gamma, name)
    if g is not None:
        check_focal_grad(g, gref, tg, ii, w, Dref, gamma, name)


# ------------------------------------------------------------------------------------------------------------------------------ paths A and B
PARAMS_AB = [(case, 2.0) for case in CASES] + [(case, g) for case in ('randn', 'graded') for g in (0.5, 1.0, 5.0)]


@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('case,gamma', PARAMS_AB)
def test_paths_A_and_B_focal(case, gamma, C):
    for P in (300, 1):
        for ii in IGNORES:
            for layout in ('dense', 'slice'):
                for ones in (False, True):
                    rs = np.random.RandomState(1000 * C + 100 * CASES.index(case) + 10 * IGNORES.index(ii) + P % 7 + (layout == 'slice') + 2 * ones)
                    lg, tg = focal_case(case, P, C, rs, ii)
                    w = np.ones(C, np.float32) if ones else make_weights(C, rs)
                    name = f'{case} gamma={gamma} C={C} P={P} ii={ii} {layout} {"ones" if ones else "weights"}'
                    if case == 'graded' and P > 1 and gamma == 2.0:
                        assert_graded(lg, tg, ii, w, gamma, name)
                    La, Da, ga = run_A(lg, tg, ii, w, gamma, layout)
                    check_against_reference(La, Da, None if case == 'bad_label' else ga, lg, tg, ii, w, gamma, case, 'A ' + name)
                    Lb, Db, fl, gb = run_B(lg, tg, ii, w, gamma, layout)
                    assert fl == (2 if case == 'bad_label' else 0), (name, fl)
                    check_against_reference(Lb, Db, gb, lg, tg, ii, w, gamma, case, 'B ' + name)
                    assert _bits(Da) == _bits(Db), 'A and B disagree on D'
                    if case == 'bad_label':         # the launches completed; a label >= C has weight 0 in B (no NaN), a NaN row in A (as weighted)
                        bad = (tg.astype(np.int64) != ii) & (tg >= C)
                        assert np.isnan(ga[bad]).all() and not np.isnan(ga[~bad]).any()
                        assert Db == 0.0 or not np.isnan(gb).any()
                    if layout == 'dense' and not ones:      # every entry point twice: the same bytes
                        La2, Da2, ga2 = run_A(lg, tg, ii, w, gamma, layout)
                        Lb2, Db2, fl2, gb2 = run_B(lg, tg, ii, w, gamma, layout)
                        assert _bits(La) == _bits(La2) and _bits(Da) == _bits(Da2) and _bits(ga) == _bits(ga2)
                        assert _bits(Lb) == _bits(Lb2) and _bits(Db) == _bits(Db2) and _bits(gb) == _bits(gb2) and fl == fl2


# ------------------------------------------------------------------------------------------------------------------------------ gamma = 0, bad gamma
def test_gamma_zero_is_todays_bytes():
    rs = np.random.RandomState(3)
    N, C, H, W = 2, 19, 16, 32
    lg, tg = FR.make_graded(N * H * W, C, rs, 255)
    w = make_weights(C, rs)
    target = torch.tensor(tg.reshape(N, H, W), device=DEV)
    sisr = dev(rs.standard_normal((N, 3, H, W)).astype(np.float32)); org = dev(rs.standard_normal((N, 3, H, W)).astype(np.float32))
    ft1 = dev(rs.uniform(0.1, 1, (N, 1, H, W)).astype(np.float32)); ft2 = dev(rs.uniform(0.1, 1, (N, 1, H, W)).astype(np.float32))

    def logits():
        return torch.tensor(lg.reshape(N, H, W, C), device=DEV).permute(0, 3, 1, 2).requires_grad_(True)

    for weight in (None, w):
        res = []
        for kw in ({}, {'focal_gamma': 0.0}, {'focal_gamma': 0}):
            x = logits()
            loss = HF.cross_entropy(x, target, 255, weight, **kw)
            loss.backward()
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            x2 = logits()
            vals = HF.fused_losses((x2, sisr, ft1, ft2), target, org, 255, 0.1, 1.0, 3, flag, 8, weight=weight, **kw)
            vals[3].backward()
            torch.cuda.synchronize()
            res.append((_bits(host(loss)), _bits(host(x.grad)), _bits(host(vals)), _bits(host(x2.grad)), int(flag)))
        assert res[0] == res[1] == res[2]
        # and gamma > 0 is something else, in both functions
        loss = HF.cross_entropy(logits(), target, 255, weight, focal_gamma=2.0)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        vals = HF.fused_losses((logits(), sisr, ft1, ft2), target, org, 255, 0.1, 1.0, 3, flag, 8, weight=weight, focal_gamma=2.0)
        assert abs(float(loss) - float(host(vals)[0])) <= 1e-6 * abs(float(loss))
        assert abs(float(loss) - float(np.frombuffer(res[0][0], np.float32)[0])) > 0.05 * abs(float(loss))
    # gamma == 0 through the _f entry points themselves: the _w bytes
    from test_class_weighted_ce_gpu import run_A as run_A_w, run_B as run_B_w
    a0, a1 = run_A(lg, tg, 255, w, 0.0), run_A_w(lg, tg, 255, w)
    b0, b1 = run_B(lg, tg, 255, w, 0.0), run_B_w(lg, tg, 255, w)
    assert all(_bits(p) == _bits(q) for p, q in zip(a0, a1)) and all(_bits(p) == _bits(q) for p, q in zip(b0[:2] + b0[3:], b1[:2] + b1[3:]))


@pytest.mark.parametrize('gamma', [-1.0, -1e-30, float('nan'), float('inf'), -float('inf')])
def test_a_bad_gamma_is_an_error_and_writes_nothing(gamma, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    rs = np.random.RandomState(4)
    lg, tg = make_case('randn', 300, 19, rs, 255)
    w = make_weights(19, rs)
    L, Dg, g = run_A(lg, tg, 255, w, gamma, expect_error=True)
    assert L == 7.0 and Dg == 7.0 and np.all(g == 7.0)
    L, Dg, fl, g = run_B(lg, tg, 255, w, gamma, expect_error=True)
    assert L == 7.0 and Dg == 7.0 and fl == 0 and np.all(g == 7.0)
    x, wgt, b, tgc = _convt_inputs('randn', 255, rs)
    y, L, Dg, fl = run_C(x, wgt, b, tgc, 255, w, gamma, expect_error=True)
    assert L == 7.0 and Dg == 7.0 and fl == 0 and bool((y == 7.0).all())
    N, H, W, C = 1, 3, 128, 19
    xt = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    lgd, tgd = make_case('randn', N * 4 * H * W, C, rs, 255)
    one = run_D_one(xt, wt, torch.tensor(lgd.reshape(N, 2 * H, 2 * W, C), device=DEV), torch.tensor(tgd.reshape(N, 2 * H, 2 * W), device=DEV), 255, w, gamma,
                    torch.ones(8, device=DEV), None, None, 0, expect_error=True)
    assert all(bool((t == 7.0).all()) for t in one)


# ------------------------------------------------------------------------------------------------------------------------------ path C
@pytest.mark.parametrize('case,ii', [(c, 255) for c in CASES] + [('randn', ii) for ii in (0, 18, -1)])
def test_path_C_focal_value_inside_the_convT_forward(case, ii, monkeypatch):
    call, query = _lib()
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    N, H, W, C = 1, 3, 200, 19                  # a ragged 72-pixel segment
    P = N * 4 * H * W
    gamma = 2.0
    rs = np.random.RandomState(CASES.index(case) + 7 * (ii & 0xff))
    x, wgt, b, tg = _convt_inputs(case, ii, rs)
    w = make_weights(C, rs)
    xt = torch.tensor(x, device=DEV); wt = torch.tensor(wgt, device=DEV); bt = torch.tensor(b, device=DEV)
    assert query('dsrl_convt2x2_fwd_ce_supported', xt.data_ptr(), xt.data_ptr(), N, H, W, C, C) == 1
    y0 = torch.empty((N, 2 * H, 2 * W, C), device=DEV)
    call('dsrl_convt2x2_fwd', xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y0.data_ptr(), N, H, W, C, C, HF._stream())
    y1, L, Dg, fl = run_C(x, wgt, b, tg, ii, w, gamma)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))          # the logits themselves, bit for bit
    lg = host(y1).reshape(P, C)
    if case == 'graded':
        assert_graded(lg, tg.reshape(P), ii, w, gamma, 'C graded')
    LB, DB, flB, _ = run_B(lg, tg.reshape(P), ii, w, gamma, want_grad=False)      # path B on the same logits: the same D, as floats, and the same flag
    assert _bits(Dg) == _bits(DB) and fl == flB == (2 if case == 'bad_label' else 0)
    check_against_reference(L, Dg, None, lg, tg.reshape(P), ii, w, gamma, case, f'C {case} ii={ii}')
    check_against_reference(LB, DB, None, lg, tg.reshape(P), ii, w, gamma, case, f'B on C {case} ii={ii}')
    y2, L2, D2, fl2 = run_C(x, wgt, b, tg, ii, w, gamma)
    assert _bits(L) == _bits(L2) and _bits(Dg) == _bits(D2) and fl == fl2 and torch.equal(y1.view(torch.int32), y2.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------ path D
@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('case,ii', [(c, 255) for c in ('randn', 'graded', 'spread', 'onehot', 'bad_label')] + [('randn', ii) for ii in (0, 18, -1)])
def test_path_D_focal_gradient_inside_the_convT_backward(case, ii, ft, monkeypatch):
    _check_path_D(case, ii, ft, 1, 3, monkeypatch)


def test_path_D_focal_transformer_rows_and_images(monkeypatch):
    # N = 2, H = 5: output rows 0 and 8 are on the stride-8 grid and the second image's rows follow the first's
    _check_path_D('randn', 255, 8, 2, 5, monkeypatch)


def _check_path_D(case, ii, ft, N, H, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    W, C = 128, 19
    P = N * 4 * H * W
    gamma = 2.0
    rs = np.random.RandomState(CASES.index(case) + 11 * (ii & 0xff) + ft + 1000 * (N - 1))
    lg, tg = focal_case(case, P, C, rs, ii)
    w = make_weights(C, rs)
    if case == 'graded':
        assert_graded(lg, tg, ii, w, gamma, 'D graded')
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wgt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor(lg.reshape(N, 2 * H, 2 * W, C), device=DEV)
    target = torch.tensor(tg.reshape(N, 2 * H, 2 * W), device=DEV)
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    res = {}
    for waves in (None, '8'):                   # one wave build: both settings, the same bytes
        if waves is None:
            monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
        else:
            monkeypatch.setenv('DSRL_CONVT_CE_WAVES', waves)
        (dx, dw, db, dl_ce, fl), (dx2, dw2, db2) = run_D(x, wgt, logits, target, ii, w, gamma, ftg, ftw, ft)
        assert fl == (2 if case == 'bad_label' else 0)
        assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2), f'waves={waves}: the one call differs from the three'
        res[waves] = (dx2, dw2, db2)
    assert all(_bits_equal(a, b) for a, b in zip(res[None], res['8']))
    if case == 'bad_label':                     # the launch completed; a label >= C has weight 0: a finite gradient
        assert bool(torch.isfinite(dx2).all())
        return
    ref, g64, Dref, _ = focal_reference(lg, tg, ii, w, gamma)
    check_focal_grad(host(dl_ce).reshape(P, C), g64, tg, ii, w, Dref, gamma, f'D {case} ii={ii}')
    g64 = g64.reshape(N, 2 * H, 2 * W, C).copy()
    if ft:
        g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
    dxo_, dwo_, dbo_ = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(wgt).astype(np.float64), g64.transpose(0, 3, 1, 2),
                                                  has_bias=True)
    check(host(dx2).transpose(0, 3, 1, 2), dxo_, 1e-5, 'dx'); check(host(dw2), dwo_, 1e-5, 'dw'); check(host(db2), dbo_, 1e-5, 'db')


# ------------------------------------------------------------------------------------------------------------------------------ head: hand-over, gradients
def _focal_cpu(logits_nchw, target, ii, w, gamma):
    """the definition on CPU float64 tensors, differentiable (the head's logits are nowhere near q == 0)"""
    C = logits_nchw.shape[1]
    x = logits_nchw.permute(0, 2, 3, 1).reshape(-1, C)
    t = target.reshape(-1).long()
    live = t != ii
    w64 = torch.tensor(np.asarray(w).astype(np.float64))
    return FR.focal_terms(x[live], t[live], w64, gamma)[0].sum() / w64[t[live]].sum()


def test_focal_fused_losses_on_the_head_hands_over_and_matches_autograd(monkeypatch):
    """The head itself has no float64 twin, so the parameter gradients are held in a chain: hand-over step == the step through HF.cross_entropy +
    autograd (path A, no hand-over) at the weighted head test's 1e-6; path A == the float64 closed form (test_paths_A_and_B_focal); and the closed
    form == CPU float64 autograd of the definition on this head's own logits at 1e-12 (below).  The value is checked against float64 directly."""
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    w = make_weights(19, np.random.RandomState(17))
    gamma = 2.0

    def step(mode):
        """'plain': no hand-over, no gradient slots, HF.cross_entropy(focal_gamma=) + mse + FA through autograd; 'fused': fused_losses;
        'other_gamma': the producer armed with another gamma - its value must not be reused"""
        monkeypatch.setattr(HF, 'convt_ce_enabled', mode != 'plain')
        monkeypatch.setattr(HF, 'grad_slots_enabled', mode != 'plain')
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        tgt = dev(target); o = dev(org)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        if mode == 'plain':
            outs = head(a, b)
            total = HF.cross_entropy(outs[0], tgt, gen.IGNORE, weight=w, focal_gamma=gamma) + 0.1 * HF.mse_loss(outs[1], o) + 1.0 * D.FALoss()(outs[2], outs[3])
            total.backward()
            ce = None
        else:
            with HF.logits_target(tgt, gen.IGNORE, flag, w, focal_gamma=gamma if mode == 'fused' else 3.0):
                outs = head(a, b)
            h = getattr(outs[0], '_dsrl_logits_grad', None)
            assert h is not None and h.value is not None and h.value_key[-1] == (gamma if mode == 'fused' else 3.0)
            produced = h.value
            calls = []
            orig = HF.call
            monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
            vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=w, focal_gamma=gamma)
            monkeypatch.setattr(HF, 'call', orig)
            assert h.armed and h.gamma == gamma and h.weight is not None, 'the hand-over did not engage'
            # the value comes from the producer's forward exactly when it was armed with the same gamma; else the loss pass computes it (no gradient)
            assert ('dsrl_ce_fused_f' in calls) == (mode != 'fused'), calls
            assert (h.count is produced) == (mode == 'fused')
            vals[3].backward()
            assert not h.armed and h.gamma == 0.0 and h.weight is None, 'holder left armed'
            ce = float(vals[0])
        torch.cuda.synchronize()
        assert int(flag) == 0
        return {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad), ce, host(outs[0])

    ref = step('plain')
    got = step('fused')
    oth = step('other_gamma')
    for k in ref[0]:
        check(got[0][k], ref[0][k], 1e-6, f'grad {k}')
    check(got[1], ref[1], 1e-6, 'dx16'); check(got[2], ref[2], 1e-6, 'dx4')
    for k in ref[0]:                            # armed with another gamma: the same gradients (the hand-over itself carries fused_losses' gamma)
        check(oth[0][k], ref[0][k], 1e-6, f'other gamma: grad {k}')
    assert abs(got[3] - oth[3]) <= 1e-6 * abs(got[3]), 'the value of the loss pass differs from the producer\'s'
    # the value, and the parameter gradients of the CE term alone, against CPU float64 autograd of the definition on the head's own logits
    lg = got[4].transpose(0, 2, 3, 1).reshape(-1, 19)
    tgh = target.reshape(-1)
    fl_ref, _, _, ce_ref = focal_reference(lg, tgh.astype(np.uint8), gen.IGNORE, w, gamma)
    check_focal_loss(got[3], fl_ref, ce_ref, lg, tgh, gen.IGNORE, gamma, 'head focal')
    assert abs(fl_ref - ce_ref) > 1e-3
    xl = torch.tensor(got[4].astype(np.float64), requires_grad=True)
    _focal_cpu(xl, torch.tensor(target), gen.IGNORE, w, gamma).backward()
    g_closed = FR.focal_loss_and_grad(lg, tgh.astype(np.uint8), gen.IGNORE, w, gamma)[1]
    assert np.abs(xl.grad.numpy().transpose(0, 2, 3, 1).reshape(-1, 19) - g_closed).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------ TrainStep, train_or_resume
def _model_and_step(graph, w, gamma):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(77)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    HF.set_dropout_seed(1234)
    return model, TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph, class_weights=w, focal_gamma=gamma)


def test_train_step_with_focal_gamma_captured_equals_eager():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    w = make_weights(19, np.random.RandomState(23))
    gamma = 2.0
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, w, gamma)
        n = step.GRAPH_WARMUP + 3                                       # graph: the eager iterations, the capture, then replays
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        if graph:
            assert step.graph_replays >= 2, 'the focal step was not captured and replayed'
        else:
            five, outs = _five(step, img, org, tgt, do_train=False)    # validation: the focal value too
            lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            tgh = tgt.cpu().numpy().reshape(-1)
            fl_ref, _, _, ce_ref = focal_reference(lg, tgh, 255, w, gamma)
            check_focal_loss(float(five[0]), fl_ref, ce_ref, lg, tgh, 255, gamma, 'do_train=False')
            assert abs(fl_ref - ce_ref) > 1e-3
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


@pytest.mark.parametrize('weights', ['weights', 'none'])
def test_unfused_losses_of_the_train_step_use_gamma(weights):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    w = make_weights(19, np.random.RandomState(23)) if weights == 'weights' else None
    wref = w if w is not None else np.ones(19, np.float32)             # no weights: the all-ones table
    tgh = tgt.cpu().numpy().reshape(-1)
    for fused in (True, False):
        model, step = _model_and_step(False, w, 2.0)
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
        fl_ref, _, _, ce_ref = focal_reference(lg, tgh, 255, wref, 2.0)
        check_focal_loss(float(five[0]), fl_ref, ce_ref, lg, tgh, 255, 2.0, f'fused_losses={fused} {weights}')
        assert abs(fl_ref - ce_ref) > 1e-3
        step.release()


def test_train_or_resume_passes_the_datasets_gamma_to_the_step(tmp_path, monkeypatch):
    from test_augment_gpu import _cache_tree
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    data, _ = _cache_tree(tmp_path)
    seen = []

    class Spy(TR.TrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append((self.focal_gamma, self.class_weight))

    monkeypatch.setattr(TR, 'TrainStep', Spy)

    def run(tag, **ds):
        torch.manual_seed(1234)
        HF.set_dropout_seed(77)
        kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                  dataset=dict({'path': data, 'settings': cs}, **ds), val_interval=1, checkpoint_interval=1, checkpoint_history=2,
                  init_weights=None, batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9, weights_decay=5e-4,
                  poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / tag), description='test',
                  early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))
        return TR.train_or_resume(is_resuming_training=False, **kw)

    h2 = run('a', focal_gamma=2.0)
    assert seen == [(2.0, None)]
    assert all(np.isfinite(v) for v in h2[0]['train'][:4]) and h2[0]['train'][0] > 0 and np.isfinite(h2[0]['val'][3])
    h0 = run('b')
    assert seen[1] == (0.0, None)
    assert h0[0]['train'][0] != h2[0]['train'][0]                      # gamma changes the loss
    with pytest.raises(ValueError, match='focal_gamma'):
        run('c', focal_gamma=-2.0)
    assert len(seen) == 2 and not os.path.exists(str(tmp_path / 'c'))   # refused before a step, a device buffer or an experiment directory existed

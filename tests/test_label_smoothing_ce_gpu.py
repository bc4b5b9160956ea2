"""Label-smoothed cross entropy, nn.CrossEntropyLoss(weight=, ignore_index=, label_smoothing=eps), through the four paths of the training step,
each against the float64 restatement of tests/label_smoothing_ref.py (fp32 logits and fp32 weights taken to float64; closed-form gradient), which
tests/test_label_smoothing_host.py holds equal to torch's CPU float64 call.

    A  dsrl_ce_fwd_s / dsrl_ce_bwd_s     HF.cross_entropy(label_smoothing=)
    B  dsrl_ce_fused_s                   the loss pass of HF.fused_losses(label_smoothing=)
    C  dsrl_convt2x2_fwd_ce_s            the value inside the last ConvTranspose forward (HF.logits_target(label_smoothing=))
    D  dsrl_convt2x2_bwd_ce_s            the gradient formed inside the ConvTranspose backward (HF.LogitsGrad.eps)

Cases: randn, spread, offset_1e4, onehot and bad_label of test_cross_entropy_edges.make_case, and `graded` (focal_ref.make_graded), on which the
smoothed loss is more than 5 % away from the weighted CE of the same inputs (asserted: a kernel that ignores eps fails).

Tolerances (fixed, label_smoothing_ref.loss_bound / grad_bound):
    loss       |L - ref| <= 1e-6 (|(1 - eps) CE part| + |smoothing part|) + 2 ulp32(max |v| over live pixels) ((1 - eps) + 2 eps (W / C) n_live / D)
    gradient   (2^-20 + 2^-22) ((1 - eps) w[t] + (eps / C) (W + w_c)) / D per element; ignored pixels exactly 0
    D          np.float32(sum over c ascending of n_c * float64(w_c)), exactly, and the same bits from every path
    spread     for the class at -3e38 m - v_c overflows fp32: the value is +inf when a live pixel holding that logit has a positive weight on its
               class, inside the bound otherwise (the zero weight chosen on that class, the other such pixels ignored), and never NaN
    D path     dx, dw, db bit-identical to dsrl_ce_fused_s -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd; 1e-5 of the range against the float64
               gradient pushed through oracle.conv_transpose2d_k2s2_bwd.  One wave build (8 waves): DSRL_CONVT_CE_WAVES unset and '8' must give the
               same bytes.  The kernel takes W % 128 == 0 only (W = 128, N x H = 1 x 3 and 2 x 5).
eps == 0 must be today's bytes, a bad eps must return an error and write nothing, and every entry point must repeat its bytes.
D == 0 gives what IEEE division gives: NaN without a live pixel, +inf when the live pixels' targets all have weight 0 (their smoothing terms remain)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import focal_ref as FR         # noqa: E402
import gen                     # noqa: E402
import label_smoothing_ref as SR   # noqa: E402
import oracle as O             # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402
from ce_variant_runners import run_A_s as run_A, run_B_s as run_B, run_C_s as run_C, run_D_s as run_D, run_D_one_s as run_D_one   # noqa: E402
from test_class_weighted_ce_gpu import (_bits, _bits_equal, _five, _place, case_for, expected_D, make_weights, reference, table)   # noqa: E402
from test_cross_entropy_edges import make_case     # noqa: E402
from test_focal_ce_gpu import _convt_inputs        # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import DsrlHipError   # noqa: E402

CASES = ['randn', 'spread', 'offset_1e4', 'onehot', 'bad_label', 'graded']
IGNORES = [255, 0, 18, -1]
LOW = np.float32(-3e38)


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def smooth_case(case, P, C, rs, ii):
    if case == 'graded':
        return FR.make_graded(P, C, rs, ii)
    return case_for(case, P, C, rs, ii)


def spread_zero_on_low(lg, tg, ii, C, rs):
    """the finite branch of `spread`: the zero weight on the -3e38 class that the live spread pixels hold most often; the live spread pixels that
    hold it elsewhere are ignored when a label can say so (labels only: the logits stay make_case's) -> (labels, weights)"""
    has = (lg == LOW).any(axis=1)
    low = np.where(has, (lg == LOW).argmax(axis=1), -1)
    live = tg.astype(np.int64) != ii
    sel = live & has
    z = int(np.bincount(low[sel], minlength=C).argmax()) if sel.any() else int(rs.randint(C))
    tg = tg.copy()
    if 0 <= ii <= 255:
        tg[sel & (low != z)] = ii
    return tg, make_weights(C, rs, zero=z)


def overflows(lg, tg, ii, w):
    """does a live pixel hold a -3e38 logit in a class of positive weight?  Then m - v_c = +inf in fp32 enters the smoothing sum."""
    live = tg.astype(np.int64) != ii
    return bool(((lg[live] == LOW) & (np.asarray(w)[None, :] > 0)).any())


_refs = {}


def smooth_reference(lg, tg, ii, w, eps):
    """(loss, gradient, D, CE part, smoothing part, loss bound) in float64, computed once per input"""
    key = (lg.tobytes(), tg.tobytes(), ii, w.tobytes(), eps)
    if key not in _refs:
        if len(_refs) > 64:
            _refs.clear()
        r = SR.smooth_loss_and_grad(lg, tg, ii, w, eps)
        _refs[key] = r + ((SR.loss_bound(lg, tg, ii, w, eps) if r[2] > 0 else float('nan')),)
    return _refs[key]


def check_smooth_loss(L, lg, tg, ii, w, eps, name):
    ref, _, Dref, _, _, tol = smooth_reference(lg, tg, ii, w, eps)
    assert not np.isnan(L), f'{name}: NaN loss'
    if overflows(lg, tg, ii, w):
        assert L == np.inf, f'{name}: {L!r} where m - v_c overflows fp32 under a positive weight'
        return
    if np.isinf(np.float32(ref)):               # (a finite float64 value that the fp32 result cannot hold)
        assert L == np.float32(ref), (name, L, ref)
        return
    print(f'{name}: loss {L!r} ref {ref!r} error / bound = {abs(L - ref) / tol:.3f}')
    assert abs(L - ref) <= tol, f'{name}: loss {L!r} vs {ref!r} (|d| = {abs(L - ref):.3e} > {tol:.3e})'


def check_smooth_grad(g, lg, tg, ii, w, eps, name):
    _, gref, Dref = smooth_reference(lg, tg, ii, w, eps)[:3]
    live = tg.astype(np.int64) != ii
    assert np.all(g[~live] == 0), f'{name}: nonzero gradient on an ignored pixel'
    err = np.abs(g[live].astype(np.float64) - gref[live])
    bound = SR.grad_bound(tg, ii, w, eps, Dref)
    print(f'{name}: max gradient error / bound = {float((err / bound).max(initial=0.0)):.3f}')
    assert not np.isnan(err).any(), f'{name}: NaN in the gradient of a live pixel'
    assert np.all(err <= bound), f'{name}: gradient error / bound = {float((err / bound).max()):.3f}'


def check_against_reference(L, Dgot, g, lg, tg, ii, w, eps, case, name):
    assert np.float32(Dgot) == expected_D(tg, ii, w), (name, Dgot, expected_D(tg, ii, w))
    if case == 'bad_label':
        assert np.isnan(L), (name, L)
        return
    ref, _, Dref = smooth_reference(lg, tg, ii, w, eps)[:3]
    if Dref == 0.0:                             # no live pixel: 0 / 0 = NaN; live pixels whose targets all have weight 0: their smoothing terms / 0 = +inf
        assert Dgot == 0.0 and ((np.isnan(L) and np.isnan(ref)) or (L == np.inf and ref == np.inf)), (name, L, ref, Dgot)
        return
    check_smooth_loss(L, lg, tg, ii, w, eps, name)
    if g is not None:
        check_smooth_grad(g, lg, tg, ii, w, eps, name)


# ------------------------------------------------------------------------------------------------------------------------------ paths A and B
def assert_eps_matters(lg, tg, ii, w, eps, name):
    """near-uniform predictions (an untrained net) move little under smoothing: the weighted CE must still lie far outside the bound around the
    smoothed reference, so that a kernel that ignores eps fails the value check"""
    sl, tol = smooth_reference(lg, tg, ii, w, eps)[0], smooth_reference(lg, tg, ii, w, eps)[5]
    ce = reference(lg, tg, ii, w)[0]
    assert abs(sl - ce) > 20 * tol, f'{name}: smoothed {sl} and weighted CE {ce} are {abs(sl - ce) / tol:.1f} bounds apart'


def assert_graded(lg, tg, ii, w, eps, name):
    ce = reference(lg, tg, ii, w)[0]
    sl = smooth_reference(lg, tg, ii, w, eps)[0]
    assert abs(sl - ce) > 0.05 * abs(ce), f'{name}: smoothed {sl} within 5 % of the weighted CE {ce}'


PARAMS_AB = [(case, 0.1) for case in CASES] + [(case, e) for case in ('randn', 'graded') for e in (0.5, 1.0)]


@pytest.mark.parametrize('C', [19, 3])
@pytest.mark.parametrize('case,eps', PARAMS_AB)
def test_paths_A_and_B_smoothed(case, eps, C):
    branches = set()
    for P in (300, 1):
        for ii in IGNORES:
            for layout in ('dense', 'slice'):
                for wkind in ('weights', 'ones') + (('zero_on_low',) if case == 'spread' else ()):
                    rs = np.random.RandomState(1000 * C + 100 * CASES.index(case) + 10 * IGNORES.index(ii) + P % 7 + (layout == 'slice')
                                               + 2 * ['weights', 'ones', 'zero_on_low'].index(wkind))
                    lg, tg = smooth_case(case, P, C, rs, ii)
                    if wkind == 'zero_on_low':
                        tg, w = spread_zero_on_low(lg, tg, ii, C, rs)
                    else:
                        w = np.ones(C, np.float32) if wkind == 'ones' else make_weights(C, rs)
                    name = f'{case} eps={eps} C={C} P={P} ii={ii} {layout} {wkind}'
                    if case == 'graded' and P > 1 and eps == 0.1:
                        assert_graded(lg, tg, ii, w, eps, name)
                    if case == 'spread' and (lg[tg.astype(np.int64) != ii] == LOW).any():
                        branches.add(overflows(lg, tg, ii, w))
                    La, Da, ga = run_A(lg, tg, ii, w, eps, layout)
                    check_against_reference(La, Da, None if case == 'bad_label' else ga, lg, tg, ii, w, eps, case, 'A ' + name)
                    Lb, Db, fl, gb = run_B(lg, tg, ii, w, eps, layout)
                    assert fl == (2 if case == 'bad_label' else 0), (name, fl)
                    check_against_reference(Lb, Db, gb, lg, tg, ii, w, eps, case, 'B ' + name)
                    assert _bits(Da) == _bits(Db), 'A and B disagree on D'
                    if case == 'bad_label':         # the launches completed; a label >= C has weight 0 in B (no NaN), a NaN row in A (as weighted)
                        bad = (tg.astype(np.int64) != ii) & (tg >= C)
                        assert np.isnan(ga[bad]).all() and not np.isnan(ga[~bad]).any()
                        assert Db == 0.0 or not np.isnan(gb).any()
                    if layout == 'dense' and wkind == 'weights':      # every entry point twice: the same bytes
                        La2, Da2, ga2 = run_A(lg, tg, ii, w, eps, layout)
                        Lb2, Db2, fl2, gb2 = run_B(lg, tg, ii, w, eps, layout)
                        assert _bits(La) == _bits(La2) and _bits(Da) == _bits(Da2) and _bits(ga) == _bits(ga2)
                        assert _bits(Lb) == _bits(Lb2) and _bits(Db) == _bits(Db2) and _bits(gb) == _bits(gb2) and fl == fl2
    if case == 'spread':
        assert branches == {True, False}, f'spread: only the branches {branches} occurred'


# ------------------------------------------------------------------------------------------------------------------------------ eps = 0, bad eps
def test_eps_zero_is_todays_bytes():
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
        for kw in ({}, {'label_smoothing': 0.0}, {'label_smoothing': 0}):
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
        # and eps > 0 is something else, in both functions
        loss = HF.cross_entropy(logits(), target, 255, weight, label_smoothing=0.1)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        vals = HF.fused_losses((logits(), sisr, ft1, ft2), target, org, 255, 0.1, 1.0, 3, flag, 8, weight=weight, label_smoothing=0.1)
        assert abs(float(loss) - float(host(vals)[0])) <= 1e-6 * abs(float(loss))
        assert abs(float(loss) - float(np.frombuffer(res[0][0], np.float32)[0])) > 0.05 * abs(float(loss))
    with pytest.raises(ValueError, match='focal_gamma'):
        HF.cross_entropy(logits(), target, 255, w, focal_gamma=2.0, label_smoothing=0.1)
    # eps == 0 through the _s entry points themselves: the _w bytes
    from test_class_weighted_ce_gpu import run_A as run_A_w, run_B as run_B_w
    a0, a1 = run_A(lg, tg, 255, w, 0.0), run_A_w(lg, tg, 255, w)
    b0, b1 = run_B(lg, tg, 255, w, 0.0), run_B_w(lg, tg, 255, w)
    assert all(_bits(p) == _bits(q) for p, q in zip(a0, a1)) and all(_bits(p) == _bits(q) for p, q in zip(b0[:2] + b0[3:], b1[:2] + b1[3:]))


@pytest.mark.parametrize('eps', [-1.0, -1e-30, 1.5, float('nan'), float('inf'), -float('inf')])
def test_a_bad_eps_is_an_error_and_writes_nothing(eps, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    rs = np.random.RandomState(4)
    lg, tg = make_case('randn', 300, 19, rs, 255)
    w = make_weights(19, rs)
    L, Dg, g = run_A(lg, tg, 255, w, eps, expect_error=True)
    assert L == 7.0 and Dg == 7.0 and np.all(g == 7.0)
    L, Dg, fl, g = run_B(lg, tg, 255, w, eps, expect_error=True)
    assert L == 7.0 and Dg == 7.0 and fl == 0 and np.all(g == 7.0)
    x, wgt, b, tgc = _convt_inputs('randn', 255, rs)
    y, L, Dg, fl = run_C(x, wgt, b, tgc, 255, w, eps, expect_error=True)
    assert L == 7.0 and Dg == 7.0 and fl == 0 and bool((y == 7.0).all())
    N, H, W, C = 1, 3, 128, 19
    xt = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    lgd, tgd = make_case('randn', N * 4 * H * W, C, rs, 255)
    one = run_D_one(xt, wt, torch.tensor(lgd.reshape(N, 2 * H, 2 * W, C), device=DEV), torch.tensor(tgd.reshape(N, 2 * H, 2 * W), device=DEV), 255, w, eps,
                    torch.ones(8, device=DEV), None, None, 0, expect_error=True)
    assert all(bool((t == 7.0).all()) for t in one)


# ------------------------------------------------------------------------------------------------------------------------------ path C
@pytest.mark.parametrize('case,ii,zero', [(c, 255, None) for c in CASES] + [('spread', 255, 4)] + [('randn', ii, None) for ii in (0, 18, -1)])
def test_path_C_smoothed_value_inside_the_convT_forward(case, ii, zero, monkeypatch):
    call, query = _lib()
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    N, H, W, C = 1, 3, 200, 19                  # a ragged 72-pixel segment
    P = N * 4 * H * W
    eps = 0.1
    rs = np.random.RandomState(CASES.index(case) + 7 * (ii & 0xff))
    x, wgt, b, tg = _convt_inputs(case, ii, rs)
    w = make_weights(C, rs, zero=7 if (case == 'spread' and zero is None) else zero)      # spread holds -3e38 in class 4: zero there, or elsewhere
    xt = torch.tensor(x, device=DEV); wt = torch.tensor(wgt, device=DEV); bt = torch.tensor(b, device=DEV)
    assert query('dsrl_convt2x2_fwd_ce_supported', xt.data_ptr(), xt.data_ptr(), N, H, W, C, C) == 1
    y0 = torch.empty((N, 2 * H, 2 * W, C), device=DEV)
    call('dsrl_convt2x2_fwd', xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y0.data_ptr(), N, H, W, C, C, HF._stream())
    y1, L, Dg, fl = run_C(x, wgt, b, tg, ii, w, eps)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))          # the logits themselves, bit for bit
    lg = host(y1).reshape(P, C)
    if case == 'graded':
        assert_graded(lg, tg.reshape(P), ii, w, eps, 'C graded')
    if case == 'spread':
        assert (lg[:, 4] == LOW).all() and overflows(lg, tg.reshape(P), ii, w) == (zero is None)
    LB, DB, flB, _ = run_B(lg, tg.reshape(P), ii, w, eps, want_grad=False)      # path B on the same logits: the same D, as floats, and the same flag
    assert _bits(Dg) == _bits(DB) and fl == flB == (2 if case == 'bad_label' else 0)
    check_against_reference(L, Dg, None, lg, tg.reshape(P), ii, w, eps, case, f'C {case} ii={ii} zero={zero}')
    check_against_reference(LB, DB, None, lg, tg.reshape(P), ii, w, eps, case, f'B on C {case} ii={ii} zero={zero}')
    y2, L2, D2, fl2 = run_C(x, wgt, b, tg, ii, w, eps)
    assert _bits(L) == _bits(L2) and _bits(Dg) == _bits(D2) and fl == fl2 and torch.equal(y1.view(torch.int32), y2.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------ path D
@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('case,ii', [(c, 255) for c in ('randn', 'graded', 'spread', 'onehot', 'bad_label')] + [('randn', ii) for ii in (0, 18, -1)])
def test_path_D_smoothed_gradient_inside_the_convT_backward(case, ii, ft, monkeypatch):
    _check_path_D(case, ii, ft, 1, 3, monkeypatch)


def test_path_D_smoothed_transformer_rows_and_images(monkeypatch):
    # N = 2, H = 5: output rows 0 and 8 are on the stride-8 grid and the second image's rows follow the first's
    _check_path_D('randn', 255, 8, 2, 5, monkeypatch)


def _check_path_D(case, ii, ft, N, H, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    W, C = 128, 19
    P = N * 4 * H * W
    eps = 0.1
    rs = np.random.RandomState(CASES.index(case) + 11 * (ii & 0xff) + ft + 1000 * (N - 1))
    lg, tg = smooth_case(case, P, C, rs, ii)
    w = make_weights(C, rs)
    if case == 'spread' and ft:                 # the gradients in both branches: ft = 8 the finite one, ft = 0 the +inf one
        tg, w = spread_zero_on_low(lg, tg, ii, C, rs)
        assert not overflows(lg, tg, ii, w)
    elif case == 'spread':
        assert overflows(lg, tg, ii, w)
    if case == 'graded':
        assert_graded(lg, tg, ii, w, eps, 'D graded')
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
        (dx, dw, db, dl_ce, fl), (dx2, dw2, db2) = run_D(x, wgt, logits, target, ii, w, eps, ftg, ftw, ft)
        assert fl == (2 if case == 'bad_label' else 0)
        assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2), f'waves={waves}: the one call differs from the three'
        res[waves] = (dx2, dw2, db2)
    assert all(_bits_equal(a, b) for a, b in zip(res[None], res['8']))
    if case == 'bad_label':                     # the launch completed; a label >= C has weight 0: a finite gradient
        assert bool(torch.isfinite(dx2).all())
        return
    g64 = smooth_reference(lg, tg, ii, w, eps)[1]
    check_smooth_grad(host(dl_ce).reshape(P, C), lg, tg, ii, w, eps, f'D {case} ii={ii}')
    g64 = g64.reshape(N, 2 * H, 2 * W, C).copy()
    if ft:
        g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
    dxo_, dwo_, dbo_ = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(wgt).astype(np.float64), g64.transpose(0, 3, 1, 2),
                                                  has_bias=True)
    check(host(dx2).transpose(0, 3, 1, 2), dxo_, 1e-5, 'dx'); check(host(dw2), dwo_, 1e-5, 'dw'); check(host(db2), dbo_, 1e-5, 'db')


# ------------------------------------------------------------------------------------------------------------------------------ head: hand-over, gradients
def test_smoothed_fused_losses_on_the_head_hands_over_and_matches_autograd(monkeypatch):
    """The head has no float64 twin, so the parameter gradients are held in a chain: hand-over step == the step through HF.cross_entropy + autograd
    (path A, no hand-over) at 1e-6; path A == the float64 closed form (test_paths_A_and_B_smoothed); the closed form == torch's CPU float64 call
    (tests/test_label_smoothing_host.py).  The value is checked against float64 directly."""
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    w = make_weights(19, np.random.RandomState(17))
    eps = 0.1

    def step(mode):
        """'plain': no hand-over, no gradient slots, HF.cross_entropy(label_smoothing=) + mse + FA through autograd; 'fused': fused_losses;
        'other_eps': the producer armed with another eps - its value must not be reused"""
        monkeypatch.setattr(HF, 'convt_ce_enabled', mode != 'plain')
        monkeypatch.setattr(HF, 'grad_slots_enabled', mode != 'plain')
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        tgt = dev(target); o = dev(org)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        if mode == 'plain':
            outs = head(a, b)
            total = HF.cross_entropy(outs[0], tgt, gen.IGNORE, weight=w, label_smoothing=eps) + 0.1 * HF.mse_loss(outs[1], o) + 1.0 * D.FALoss()(outs[2], outs[3])
            total.backward()
            ce = None
        else:
            armed_eps = eps if mode == 'fused' else 0.3
            with HF.logits_target(tgt, gen.IGNORE, flag, w, label_smoothing=armed_eps):
                outs = head(a, b)
            h = getattr(outs[0], '_dsrl_logits_grad', None)
            assert h is not None and h.value is not None and armed_eps in h.value_key and h.value_key[-1] == 0.0 and h.value_key[-2] == armed_eps
            produced = h.value
            calls = []
            orig = HF.call
            monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
            vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=w, label_smoothing=eps)
            monkeypatch.setattr(HF, 'call', orig)
            assert h.armed and h.eps == eps and h.gamma == 0.0 and h.weight is not None, 'the hand-over did not engage'
            # the value comes from the producer's forward exactly when it was armed with the same eps; else the loss pass computes it (no gradient)
            assert ('dsrl_ce_fused_s' in calls) == (mode != 'fused'), calls
            assert (h.count is produced) == (mode == 'fused')
            calls.clear()
            monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
            vals[3].backward()
            monkeypatch.setattr(HF, 'call', orig)
            assert 'dsrl_convt2x2_bwd_ce_s' in calls, calls
            assert not h.armed and h.eps == 0.0 and h.gamma == 0.0 and h.weight is None, 'holder left armed'
            ce = float(vals[0])
        torch.cuda.synchronize()
        assert int(flag) == 0
        return {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad), ce, host(outs[0])

    ref = step('plain')
    got = step('fused')
    oth = step('other_eps')
    for k in ref[0]:
        check(got[0][k], ref[0][k], 1e-6, f'grad {k}')
    check(got[1], ref[1], 1e-6, 'dx16'); check(got[2], ref[2], 1e-6, 'dx4')
    for k in ref[0]:                            # armed with another eps: the same gradients (the hand-over itself carries fused_losses' eps)
        check(oth[0][k], ref[0][k], 1e-6, f'other eps: grad {k}')
    assert abs(got[3] - oth[3]) <= 1e-6 * abs(got[3]), 'the value of the loss pass differs from the producer\'s'
    lg = got[4].transpose(0, 2, 3, 1).reshape(-1, 19)
    tgh = target.reshape(-1).astype(np.uint8)
    check_smooth_loss(got[3], lg, tgh, gen.IGNORE, w, eps, 'head smoothed')
    assert_eps_matters(lg, tgh, gen.IGNORE, w, eps, 'head smoothed')


# ------------------------------------------------------------------------------------------------------------------------------ TrainStep, train_or_resume
def _model_and_step(graph, w, eps):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(77)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    HF.set_dropout_seed(1234)
    return model, TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph, class_weights=w, label_smoothing=eps)


def test_train_step_with_label_smoothing_captured_equals_eager():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    w = make_weights(19, np.random.RandomState(23))
    eps = 0.1
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, w, eps)
        n = step.GRAPH_WARMUP + 3                                       # graph: the eager iterations, the capture, then replays
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        if graph:
            assert step.graph_replays >= 2, 'the smoothed step was not captured and replayed'
        else:
            five, outs = _five(step, img, org, tgt, do_train=False)    # validation: the smoothed value too
            lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            tgh = tgt.cpu().numpy().reshape(-1)
            check_smooth_loss(float(five[0]), lg, tgh, 255, w, eps, 'do_train=False')
            assert_eps_matters(lg, tgh, 255, w, eps, 'do_train=False')
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


@pytest.mark.parametrize('weights', ['weights', 'none'])
def test_fused_and_unfused_losses_of_the_train_step_use_eps(weights):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    w = make_weights(19, np.random.RandomState(23)) if weights == 'weights' else None
    wref = w if w is not None else np.ones(19, np.float32)             # no weights: the all-ones table
    tgh = tgt.cpu().numpy().reshape(-1)
    for fused in (True, False):
        model, step = _model_and_step(False, w, 0.1)
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
        check_smooth_loss(float(five[0]), lg, tgh, 255, wref, 0.1, f'fused_losses={fused} {weights}')
        assert_eps_matters(lg, tgh, 255, wref, 0.1, f'fused_losses={fused} {weights}')
        step.release()


def test_train_step_refuses_eps_with_gamma():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    with pytest.raises(ValueError, match='focal_gamma'):
        TrainStep(None, None, 3, 0.1, 1.0, 255, focal_gamma=2.0, label_smoothing=0.1)


def test_train_or_resume_passes_the_datasets_label_smoothing_to_the_step(tmp_path, monkeypatch):
    from test_augment_gpu import _cache_tree
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    data, _ = _cache_tree(tmp_path)
    seen = []

    class Spy(TR.TrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append((self.label_smoothing, self.focal_gamma, self.class_weight))

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

    h1 = run('a', label_smoothing=0.1)
    assert seen == [(0.1, 0.0, None)]
    assert all(np.isfinite(v) for v in h1[0]['train'][:4]) and h1[0]['train'][0] > 0 and np.isfinite(h1[0]['val'][3])
    h0 = run('b')
    assert seen[1] == (0.0, 0.0, None)
    assert h0[0]['train'][0] != h1[0]['train'][0]                      # eps changes the loss
    with pytest.raises(ValueError, match='label_smoothing'):
        run('c', label_smoothing=2)
    with pytest.raises(ValueError, match='label_smoothing'):
        run('d', label_smoothing=0.1, focal_gamma=2.0)
    # refused before a step, a device buffer or an experiment directory existed
    assert len(seen) == 2 and not os.path.exists(str(tmp_path / 'c')) and not os.path.exists(str(tmp_path / 'd'))

"""The quantised Lovasz-Softmax term, loss = CE + lambda L, through every layer that carries it, against the float64 restatement
of tests/lovasz_ref.py (fp32 logits taken to float64):

    dsrl_lovasz_fwd / dsrl_lovasz_bwd   the histograms, the record {lambda L, |Present|, 0, 0, gf, gb} and the unfused row   (HF.lovasz_softmax_loss)
    dsrl_convt2x2_bwd_ce_l              the weighted CE row + the Lovasz row formed inside the ConvTranspose backward          (HF.LogitsGrad.lovasz)
    HF.fused_losses(lovasz=)            on the head: the hand-over, values and parameter gradients against cross_entropy(lovasz=) through autograd
    TrainStep(lovasz=)                  captured == eager, validation keeps the plain CE, off is the step built without the argument

Cases: lovasz_ref.make_case with the seeds of lovasz_ref.case_seed (checked on the CPU by test_lovasz_host.test_the_cases_of_the_gpu_test).

Bounds (fixed; none of them comes from what the kernels give):
    histograms    sum_b nf_c = G_c and sum_b (nf_c + nb_c) = the live count, exactly; sum |h_device - h_ref| <= 2 x the reference's borderline elements
                  (a float32 softmax may move such an element one level: two bins change by one); the K = 16, P = 2048 seeds have none: equality
    tables        within 1 fp32 ulp of the float64 closed form recomputed from the DEVICE's histograms; record[0] within 1e-6 relative of it
    value         |record[0] / lambda - exact| <= 1 / (2 K) + 1e-6: the extension is monotone and 1-Lipschitz in the sup norm, the levels move an error
                  by at most 1 / (2 K), and 1e-6 covers the float32 softmax through the same argument
    rows          on the pixels the reference does not mark (always more than three quarters): max |device - float64| <= 4 x max |float32 numpy -
                  float64|, both from the device's tables (the convention of tests/temperature_ref.py); pixels that are not live exactly 0;
                  accumulate = 1 equals the fp32 sum bitwise; record and rows repeat bit for bit
    fused         dx, dw, db bit-identical to dsrl_ce_fused_w -> dsrl_lovasz_bwd(accumulate) -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd
                  (W = 128, N x H = 1 x 3 and 2 x 5, the weights and transformer of test_dice_gpu.test_fused_backward_is_the_unfused_sequence)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gen                     # noqa: E402
import lovasz_ref as LR        # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402
from ce_variant_runners import _place, table   # noqa: E402
from test_class_weighted_ce_gpu import _bits, _bits_equal, _five, make_weights, reference   # noqa: E402
from test_cross_entropy_edges import LOSS_REL, M_ULPS, make_case, ulp32     # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import DsrlHipError   # noqa: E402

HEAD = 4            # floats of the record before the tables


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


_refs = {}


def lovasz_reference(lg, tg, ii, lam, K):
    """lovasz_ref.binned in float64, computed once per input and left unchanged"""
    key = (lg.tobytes(), tg.tobytes(), ii, lam, K)
    if key not in _refs:
        if len(_refs) > 64:
            _refs.clear()
        _refs[key] = LR.binned(lg, tg, ii, lam, K)
    return _refs[key]


def run_fwd(lg, tg, ii, lam, K, layout='dense', expect_error=False, reuse=None, **bad):
    """dsrl_lovasz_fwd -> (record (4 + 2 C K,) on the host, nf (C, K), nb (C, K) from the head of the workspace, flag, workspace); everything
    pre-filled with 7; `bad`: arguments replaced by name"""
    call, query = _lib()
    P, C = lg.shape
    buf, ptr, ld = _place(lg, layout)
    target = torch.tensor(tg, device=DEV)
    rec = torch.full((4 + 2 * C * K,), 7.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = reuse
    if ws is None:
        ws = torch.full((query('dsrl_lovasz_workspace_bytes', P, C, K),), 7, dtype=torch.uint8, device=DEV)
    a = dict(logits=ptr, ld=ld, target=target.data_ptr(), P=P, C=C, ii=ii, bins=K, record=rec.data_ptr(), flag=flag.data_ptr(), ws=ws.data_ptr(),
             ws_bytes=ws.numel())
    a['lambda'] = lam
    a.update(bad)
    args = (a['logits'], a['ld'], a['target'], a['P'], a['C'], a['ii'], a['lambda'], a['bins'], a['record'], a['flag'], a['ws'], a['ws_bytes'], HF._stream())
    if expect_error:
        with pytest.raises(DsrlHipError):
            call('dsrl_lovasz_fwd', *args)
        torch.cuda.synchronize()
        assert bool((ws == 7).all()) and bool((rec == 7.0).all()) and int(flag) == 0, 'an argument error wrote something'
        return None
    call('dsrl_lovasz_fwd', *args)
    torch.cuda.synchronize()
    h = ws[:2 * C * K * 4].cpu().numpy().view(np.uint32).reshape(2, C, K).astype(np.int64)
    return host(rec), h[0], h[1], int(flag), ws


def run_bwd(lg, tg, ii, rec, K, accumulate=0, layout='dense', into=None):
    """dsrl_lovasz_bwd -> gradient (P, C); accumulate: into a copy of `into`"""
    call, _ = _lib()
    P, C = lg.shape
    buf, ptr, ld = _place(lg, layout)
    target = torch.tensor(tg, device=DEV)
    recd = torch.tensor(rec, device=DEV)
    if layout == 'slice':
        big = torch.full((P, C + 3), 7.0, device=DEV)
        if into is not None:
            big[:, 1:1 + C] = torch.tensor(into, device=DEV)
        call('dsrl_lovasz_bwd', ptr, ld, target.data_ptr(), P, C, ii, recd.data_ptr(), K, accumulate, big.data_ptr() + 4, C + 3, HF._stream())
        torch.cuda.synchronize()
        assert bool((big[:, 0] == 7).all()) and bool((big[:, 1 + C:] == 7).all()), 'wrote outside the rows'
        return host(big[:, 1:1 + C])
    dl = torch.full((P, C), 7.0, device=DEV) if into is None else torch.tensor(into, device=DEV)
    call('dsrl_lovasz_bwd', ptr, ld, target.data_ptr(), P, C, ii, recd.data_ptr(), K, accumulate, dl.data_ptr(), C, HF._stream())
    torch.cuda.synchronize()
    return host(dl)


def ulps_apart(got, want64):
    """|got - fp32(want)| in ulps of fp32(want), elementwise"""
    w32 = np.asarray(want64).astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(w32), np.float32(1e-37)))
    return np.abs(got.astype(np.float64) - w32.astype(np.float64)) / sp.astype(np.float64)


def tables_of(rec, C, K):
    return rec[HEAD:HEAD + C * K].reshape(C, K), rec[HEAD + C * K:].reshape(C, K)


def check_record(rec, nf, nb, lg, tg, ii, lam, K, name):
    ref = lovasz_reference(lg, tg, ii, lam, K)
    C = lg.shape[1]
    nlive = int(ref['live'].sum())
    assert np.array_equal(nf.sum(axis=1), ref['G']), f'{name}: sum_b nf_c {nf.sum(axis=1)} vs G_c {ref["G"]}'
    assert np.array_equal((nf + nb).sum(axis=1), np.full(C, nlive)), f'{name}: sum_b (nf_c + nb_c) is not the live count {nlive}'
    moved = int(np.abs(nf - ref['nf']).sum() + np.abs(nb - ref['nb']).sum())
    nbl = int(ref['borderline'].sum())
    print(f'{name}: {moved} histogram differences, {nbl} borderline elements')
    assert moved <= 2 * nbl, f'{name}: {moved} histogram differences with {nbl} borderline elements'
    T = LR.tables_from_hist(nf, nb, float(np.float32(lam)))             # float64, from the device's own histograms and the fp32 lambda it was given
    gf, gb = tables_of(rec, C, K)
    uf, ub = ulps_apart(gf, T['gf']), ulps_apart(gb, T['gb'])
    print(f'{name}: tables within {max(uf.max(), ub.max()):.2f} ulp; value {rec[0]!r} closed form {T["value"]!r} exact {lam * ref["exact"]!r}')
    assert uf.max() <= 1 and ub.max() <= 1, f'{name}: gf within {uf.max()} ulp, gb within {ub.max()} ulp'
    assert not gf[ref['G'] == 0].any() and not gb[ref['G'] == 0].any(), f'{name}: an absent class has a table'
    assert rec[1] == T['present'] == ref['present'] and rec[2] == 0 and rec[3] == 0, f'{name}: |Present| = {rec[1]} vs {ref["present"]}'
    assert abs(rec[0] - T['value']) <= 1e-6 * abs(T['value']), f'{name}: value {rec[0]!r} vs {T["value"]!r}'
    assert abs(rec[0] / lam - ref['exact']) <= 1.0 / (2 * K) + 1e-6, f'{name}: value / lambda {rec[0] / lam!r} vs the sorted loss {ref["exact"]!r}'


def check_rows(g, rec, lg, tg, ii, lam, K, name):
    """-> device error / float32 numpy error on the pixels the reference does not mark"""
    ref = lovasz_reference(lg, tg, ii, lam, K)
    C = lg.shape[1]
    live = ref['live']
    assert np.all(g[~live] == 0), f'{name}: nonzero gradient on a pixel that is not live'
    ok = live & ~ref['borderline'].any(axis=1)
    assert (live & ~ok).sum() < 0.25 * live.sum(), f'{name}: {int((live & ~ok).sum())} of {int(live.sum())} live pixels skipped'
    gf, gb = tables_of(rec, C, K)
    row64 = LR.rows_from_tables(lg, tg, ii, gf, gb, K)
    row32 = LR.rows_fp32(lg, tg, ii, gf, gb, K)
    e_dev = float(np.abs(g[ok].astype(np.float64) - row64[ok]).max(initial=0.0))
    e_32 = float(np.abs(row32[ok].astype(np.float64) - row64[ok]).max(initial=0.0))
    ratio = e_dev / e_32 if e_32 > 0 else (0.0 if e_dev == 0 else float('inf'))
    print(f'{name}: row error {e_dev:.3e}, float32 numpy {e_32:.3e}, ratio {ratio:.3f}; largest element {np.abs(row64[ok]).max(initial=0.0):.3e}')
    assert not np.isnan(g).any()
    assert e_dev <= 4 * e_32, f'{name}: row error {e_dev:.3e} beyond 4 x {e_32:.3e}'
    return ratio


# ------------------------------------------------------------------------------------------------------------------------------ dsrl_lovasz_fwd / _bwd
@pytest.mark.parametrize('C', LR.CS)
@pytest.mark.parametrize('K', LR.KS)
def test_lovasz_fwd_and_bwd(K, C):
    worst = 0.0
    for P in LR.PS:
        for layout in LR.LAYOUTS:
            lam = 1.0 if layout == 'dense' else 0.4
            lg, tg = LR.make_case(P, C, LR.case_seed(C, K, P, layout))
            name = f'C={C} K={K} P={P} {layout} lambda={lam}'
            rec, nf, nb, fl, _ = run_fwd(lg, tg, 255, lam, K, layout)
            assert fl == 0, (name, fl)
            check_record(rec, nf, nb, lg, tg, 255, lam, K, name)
            if K == 16 and P == 2048:                                   # a seed without a borderline element: the reference's histograms, exactly
                ref = lovasz_reference(lg, tg, 255, lam, K)
                assert not ref['borderline'].any() and np.array_equal(nf, ref['nf']) and np.array_equal(nb, ref['nb']), name
            g = run_bwd(lg, tg, 255, rec, K, 0, layout)
            worst = max(worst, check_rows(g, rec, lg, tg, 255, lam, K, name))
            assert np.abs(g).max() > 0
            if P in (63, 2048):
                # accumulate = 1: the fp32 sum, bitwise (a pixel that is not live adds +0)
                base = np.random.RandomState(P).standard_normal(lg.shape).astype(np.float32)
                base[tg == 255] = 0
                acc = run_bwd(lg, tg, 255, rec, K, 1, layout, into=base)
                assert _bits(acc) == _bits(base + g), f'{name}: accumulate differs from the fp32 sum'
                # twice: the same bits, record and rows
                rec2, nf2, nb2, _, _ = run_fwd(lg, tg, 255, lam, K, layout)
                assert _bits(rec) == _bits(rec2) and np.array_equal(nf, nf2) and np.array_equal(nb, nb2), f'{name}: the record does not repeat'
                assert _bits(g) == _bits(run_bwd(lg, tg, 255, rec2, K, 0, layout)), f'{name}: the rows do not repeat'
                if layout == 'slice':       # the layout changes the loads, not the arithmetic
                    recd = run_fwd(lg, tg, 255, lam, K, 'dense')[0]
                    assert _bits(rec) == _bits(recd), f'{name}: dense and strided logits give different records'
    print(f'C={C} K={K}: worst row error ratio device / float32 numpy = {worst:.3f}')


def test_the_aggregated_and_the_plain_histogram_pass_count_alike(monkeypatch):
    lg, tg = LR.make_case(70001, 19, LR.case_seed(19, 1024, 70001, 'dense'))
    res = {}
    for agg in ('1', '0'):
        monkeypatch.setenv('DSRL_LOVASZ_AGG', agg)
        rec, nf, nb, fl, _ = run_fwd(lg, tg, 255, 1.0, 1024)
        res[agg] = (_bits(rec), nf, nb)
    assert res['1'][0] == res['0'][0] and np.array_equal(res['1'][1], res['0'][1]) and np.array_equal(res['1'][2], res['0'][2])


# ------------------------------------------------------------------------------------------------------------------------------ edges
def test_all_pixels_ignored_and_other_ignore_indices():
    C, K = 19, 64
    lg, tg = LR.make_case(300, C, 1)
    tg[:] = 255
    rec, nf, nb, fl, _ = run_fwd(lg, tg, 255, 1.0, K)
    assert not rec.any() and not nf.any() and not nb.any() and fl == 0       # Present empty: value 0, zero tables
    assert not run_bwd(lg, tg, 255, rec, K).any()
    for ii in (0, 17, -1):
        lg, tg = LR.make_case(1000, C, 40 + (ii & 0xff))
        rec, nf, nb, fl, _ = run_fwd(lg, tg, ii, 1.0, K)
        assert fl == 0
        check_record(rec, nf, nb, lg, tg, ii, 1.0, K, f'ii={ii}')
        if ii >= 0:
            assert not nf[ii].any()                                      # the ignored label's class is absent
        check_rows(run_bwd(lg, tg, ii, rec, K), rec, lg, tg, ii, 1.0, K, f'ii={ii}')


def test_labels_beyond_the_classes_take_no_part():
    lg, tg = make_case('bad_label', 1000, 19, np.random.RandomState(6))
    assert (tg[tg != 255] >= 19).sum() >= 1
    rec, nf, nb, fl, _ = run_fwd(lg, tg, 255, 1.0, 256)
    assert fl == 0                                                      # CE reports such a label through its own flag bit
    tg2 = tg.copy(); tg2[(tg != 255) & (tg >= 19)] = 255
    rec2, nf2, nb2, _, _ = run_fwd(lg, tg2, 255, 1.0, 256)
    assert _bits(rec) == _bits(rec2) and np.array_equal(nf, nf2) and np.array_equal(nb, nb2)
    g = run_bwd(lg, tg, 255, rec, 256)
    assert not g[tg >= 19].any() and _bits(g) == _bits(run_bwd(lg, tg2, 255, rec2, 256))


def test_a_class_that_owns_every_live_pixel():
    C, K, P = 5, 64, 700
    lg, tg = LR.make_case(P, C, 9)
    tg[tg != 255] = 2
    rec, nf, nb, fl, _ = run_fwd(lg, tg, 255, 1.0, K)
    check_record(rec, nf, nb, lg, tg, 255, 1.0, K, 'one class')
    assert not nb[2].any() and rec[1] == 1 and not nf[[0, 1, 3, 4]].any()
    gf, gb = tables_of(rec, C, K)
    n = int((tg == 2).sum())
    # no background above any level: wf = 1 / G everywhere; wb = (G - NFincl) / G^2 is what a background element would get, and none exists
    nf_incl = np.cumsum(nf[2][::-1])[::-1]
    assert np.all(gf[2] == np.float32(-1.0 / n)) and np.array_equal(gb[2], ((n - nf_incl) / (float(n) * n)).astype(np.float32))
    check_rows(run_bwd(lg, tg, 255, rec, K), rec, lg, tg, 255, 1.0, K, 'one class')


def test_errors_of_exactly_zero_and_exactly_one():
    """One logit 200 above the others: p is exactly 1 and exactly 0 in float32 and in float64.  Labelled with the hot class the pixel's errors are all 0
    (level 0); labelled otherwise its foreground error and the hot class's background error are exactly 1 (level K - 1, not K)."""
    C, P = 19, 1300
    rs = np.random.RandomState(12)
    hot = rs.randint(0, C, P)
    lg = np.zeros((P, C), np.float32)
    lg[np.arange(P), hot] = 200.0
    tg = np.where(rs.rand(P) < 0.5, hot, (hot + 1 + rs.randint(0, C - 1, P)) % C).astype(np.uint8)
    tg[::11] = 255
    for K in (16, 4096):
        ref = lovasz_reference(lg, tg, 255, 1.0, K)
        assert ref['nf'][:, 1:K - 1].sum() == 0 and ref['nb'][:, 1:K - 1].sum() == 0 and ref['nf'][:, K - 1].sum() > 100 and ref['nf'][:, 0].sum() > 100
        rec, nf, nb, fl, _ = run_fwd(lg, tg, 255, 1.0, K)
        assert fl == 0 and np.array_equal(nf, ref['nf']) and np.array_equal(nb, ref['nb'])
        T = LR.tables_from_hist(nf, nb, 1.0)
        gf, gb = tables_of(rec, C, K)
        assert ulps_apart(gf, T['gf']).max() <= 1 and ulps_apart(gb, T['gb']).max() <= 1 and abs(rec[0] - T['value']) <= 1e-6 * T['value']
        g = run_bwd(lg, tg, 255, rec, K)
        assert not g.any()                                              # p (g - sum p g) with p in {0, 1}: every element is exactly 0
        assert np.isfinite(g).all()


def test_a_nan_logit_raises_the_flag_in_a_live_pixel_only():
    C, K = 19, 1024
    lg, tg = LR.make_case(1000, C, 5)
    live = np.where(tg != 255)[0]
    dead = np.where(tg == 255)[0]
    lg2 = lg.copy(); lg2[dead[0], 3] = np.nan
    rec, nf, nb, fl, _ = run_fwd(lg2, tg, 255, 1.0, K)
    assert fl == 0
    check_record(rec, nf, nb, lg, tg, 255, 1.0, K, 'NaN in an ignored pixel')
    lg2 = lg.copy(); lg2[live[0], 3] = np.nan; lg2[live[1], :] = np.nan; lg2[live[2], 0] = np.inf; lg2[live[3], 1] = -np.inf
    rec, nf, nb, fl, ws = run_fwd(lg2, tg, 255, 1.0, K)
    assert fl == 1 and np.isnan(rec[0])
    assert np.array_equal((nf + nb).sum(axis=1), np.full(C, len(live)))                # every element was counted in some level of its class
    assert bool((ws[2 * C * K * 4 + 64 * 12 + 4:] == 0).all())                         # nothing past the tail's NaN word but the cleared padding
    g = run_bwd(lg2, tg, 255, np.where(np.isnan(rec), 0, rec).astype(np.float32), K)   # the rows of the other pixels are numbers; nothing faulted
    ok = np.ones(len(tg), bool); ok[live[:3]] = False
    assert np.isfinite(g[ok]).all()


def test_a_reused_workspace_gives_the_new_call_its_own_record():
    C, K = 19, 1024
    lg1, tg1 = LR.make_case(2048, C, 21)
    lg2, tg2 = LR.make_case(2048, C, 22)
    rec1, nf1, nb1, _, ws = run_fwd(lg1, tg1, 255, 1.0, K)
    rec2, nf2, nb2, _, _ = run_fwd(lg2, tg2, 255, 1.0, K, reuse=ws)                      # the workspace as the first call left it
    fresh = run_fwd(lg2, tg2, 255, 1.0, K)
    assert _bits(rec2) == _bits(fresh[0]) and np.array_equal(nf2, fresh[1]) and np.array_equal(nb2, fresh[2])
    assert not np.array_equal(nf1, nf2)
    check_record(rec2, nf2, nb2, lg2, tg2, 255, 1.0, K, 'second call')


@pytest.mark.parametrize('bad', [{'lambda': 0.0}, {'lambda': -1.0}, {'lambda': float('nan')}, {'lambda': float('inf')}, dict(bins=8), dict(bins=8192),
                                 dict(bins=1000), dict(logits=None), dict(target=None), dict(record=None), dict(ws=None), dict(P=0), dict(P=2 ** 31 - 256),
                                 dict(C=0), dict(C=61), dict(ld=18), dict(ws_bytes=1000)])
def test_a_bad_argument_is_an_error_and_writes_nothing(bad):
    lg, tg = LR.make_case(300, 19, 4)
    run_fwd(lg, tg, 255, 1.0, 1024, expect_error=True, **bad)


def test_a_bad_argument_of_the_backward_writes_nothing():
    call, _ = _lib()
    lg, tg = LR.make_case(300, 19, 4)
    rec = run_fwd(lg, tg, 255, 1.0, 64)[0]
    recd = torch.tensor(rec, device=DEV); x = torch.tensor(lg, device=DEV); t = torch.tensor(tg, device=DEV)
    dl = torch.full((300, 19), 7.0, device=DEV)
    ok = dict(logits=x.data_ptr(), ld=19, target=t.data_ptr(), P=300, C=19, ii=255, record=recd.data_ptr(), bins=64, accumulate=0, dl=dl.data_ptr(), lddl=19)
    for bad in (dict(accumulate=2), dict(accumulate=-1), dict(lddl=18), dict(ld=18), dict(bins=48), dict(bins=8), dict(P=0), dict(C=61), dict(logits=None),
                dict(target=None), dict(record=None), dict(dl=None)):
        a = dict(ok, **bad)
        with pytest.raises(DsrlHipError):
            call('dsrl_lovasz_bwd', a['logits'], a['ld'], a['target'], a['P'], a['C'], a['ii'], a['record'], a['bins'], a['accumulate'], a['dl'], a['lddl'],
                 HF._stream())
    torch.cuda.synchronize()
    assert bool((dl == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------------ fused backward
def run_D(x, wgt, logits, target, ii, w, rec, K, ftg, ftw, ft):
    """-> (four-call results (dx, dw, db, dl of CE + Lovasz, flag), one-call results (dx, dw, db)): dsrl_ce_fused_w -> dsrl_lovasz_bwd(accumulate = 1)
    -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd against dsrl_convt2x2_bwd_ce_l"""
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
    call('dsrl_lovasz_bwd', logits.data_ptr(), C, target.data_ptr(), P, C, ii, rec.data_ptr(), K, 1, dl.data_ptr(), C, st)
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
    call('dsrl_convt2x2_bwd_ce_l', x.data_ptr(), wgt.data_ptr(), logits.data_ptr(), target.data_ptr(), ii, wt.data_ptr(), rec.data_ptr(), K, scal.data_ptr() + 4,
         ftp[0], ftp[1], ft, dx2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    torch.cuda.synchronize()
    return (dx, dw, db, dl_loss, int(flag)), (dx2, dw2, db2)


@pytest.mark.parametrize('weights', ['weights', 'ones'])
@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('N,H', [(1, 3), (2, 5)])
@pytest.mark.parametrize('case', ['levels', 'bad_label'])
def test_fused_backward_is_the_unfused_sequence(case, N, H, ft, weights, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    W, C, ii, lam = 128, 19, 255, 1.0
    P = N * 4 * H * W
    rs = np.random.RandomState((case == 'bad_label') + ft + 1000 * (N - 1) + (weights == 'ones'))
    lg, tg = LR.make_case(P, C, 500 + ft + N) if case == 'levels' else make_case('bad_label', P, C, rs, ii)
    w = make_weights(C, rs) if weights == 'weights' else np.ones(C, np.float32)
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wgt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor(lg.reshape(N, 2 * H, 2 * W, C), device=DEV)
    target = torch.tensor(tg.reshape(N, 2 * H, 2 * W), device=DEV)
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    for K in (1024, 16):
        rec = torch.tensor(run_fwd(lg, tg, ii, lam, K)[0], device=DEV)
        res = {}
        for waves in (None, '8'):                   # one wave build: both settings, the same bytes
            if waves is None:
                monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
            else:
                monkeypatch.setenv('DSRL_CONVT_CE_WAVES', waves)
            (dx, dw, db, dl_loss, fl), (dx2, dw2, db2) = run_D(x, wgt, logits, target, ii, w, rec, K, ftg, ftw, ft)
            assert fl == (2 if case == 'bad_label' else 0)
            assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2), f'K={K} waves={waves}: the one call differs from the four'
            res[waves] = (dx2, dw2, db2)
        assert all(_bits_equal(a, b) for a, b in zip(res[None], res['8']))
        if case == 'bad_label':                     # the launch completed; a label >= C has weight 0 and no Lovasz row: a finite gradient
            assert bool(torch.isfinite(dx2).all())
            continue
        # the loss row against float64: the CE row of torch plus the Lovasz row from the record's tables, on the pixels the reference does not mark
        _, gce, _ = reference(lg, tg, ii, w)
        recn = host(rec)
        gl = LR.rows_from_tables(lg, tg, ii, *tables_of(recn, C, K), K)
        ok = ~lovasz_reference(lg, tg, ii, lam, K)['borderline'].any(axis=1)
        assert np.abs(gl).max() > 100 * 1e-5 * np.abs(gce + gl).max()           # the Lovasz row is there to be missed
        check(host(dl_loss).reshape(P, C)[ok], (gce + gl)[ok], 1e-5, 'CE + Lovasz row')
        # and without the Lovasz row the result is another one: the weighted entry point on the same inputs
        from ce_variant_runners import run_D_one
        scal = torch.zeros(8, device=DEV)
        call, query = _lib()
        ws = torch.empty(query('dsrl_ce_fused_w_workspace_bytes', P), dtype=torch.uint8, device=DEV)
        call('dsrl_ce_fused_w', logits.data_ptr(), C, target.data_ptr(), P, C, ii, table(w).data_ptr(), None, C, scal.data_ptr(), None, ws.data_ptr(),
             ws.numel(), HF._stream())
        dxw, _, _ = run_D_one('_w', x, wgt, logits, target, ii, w, None, scal, ftg, ftw, ft)
        assert not _bits_equal(dxw, dx2)


# ------------------------------------------------------------------------------------------------------------------------------ head: hand-over, gradients
@pytest.mark.parametrize('weights', ['weights', 'none'])
def test_lovasz_fused_losses_on_the_head_hands_over_and_matches_autograd(weights, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    w = make_weights(19, np.random.RandomState(17)) if weights == 'weights' else None
    lov = (0.7, 1024)

    def step(mode):
        """'plain': no hand-over, no gradient slots, HF.cross_entropy(lovasz=) + mse + FA through autograd; 'fused': fused_losses(lovasz=); 'second':
        fused_losses(lovasz=) while another consumer sends the logits a gradient of its own (zeros): the unfused branch of the backward"""
        monkeypatch.setattr(HF, 'convt_ce_enabled', mode != 'plain')
        monkeypatch.setattr(HF, 'grad_slots_enabled', mode != 'plain')
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        tgt = dev(target); o = dev(org)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        calls = []
        if mode == 'plain':
            outs = head(a, b)
            ce = HF.cross_entropy(outs[0], tgt, gen.IGNORE, weight=w, lovasz=lov)
            total = ce + 0.1 * HF.mse_loss(outs[1], o) + 1.0 * D.FALoss()(outs[2], outs[3])
            total.backward()
            ce, tot = float(ce.detach()), float(total.detach())
        else:
            with HF.logits_target(tgt, gen.IGNORE, flag, w, lovasz=lov):
                outs = head(a, b)
            h = getattr(outs[0], '_dsrl_logits_grad', None)
            assert h is not None and h.value is not None, 'the forward did not evaluate the CE value'
            orig = HF.call
            monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
            vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=w, lovasz=lov)
            assert h.armed and h.lovasz is not None and h.lovasz[1] == 1024 and h.dice is None and h.weight is not None, 'the hand-over did not engage'
            assert 'dsrl_lovasz_fwd' in calls and 'dsrl_lovasz_bwd' not in calls and not any(c.startswith('dsrl_ce_fused') for c in calls), calls
            assert vals.grad_fn.grads[0] is None, 'fused_losses allocated the logits gradient'
            if mode == 'second':
                torch.autograd.backward([vals, outs[0]], [torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=DEV), torch.zeros_like(outs[0])])
            else:
                vals[3].backward()
            monkeypatch.setattr(HF, 'call', orig)
            assert not h.armed and h.lovasz is None and h.weight is None, 'holder left armed'
            if mode == 'fused':
                assert 'dsrl_convt2x2_bwd_ce_l' in calls and 'dsrl_lovasz_bwd' not in calls, calls
            else:
                assert 'dsrl_convt2x2_bwd_ce_l' not in calls and calls.count('dsrl_lovasz_bwd') == 1 and 'dsrl_ce_fused_w' in calls, calls
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
    # the value against float64 on the head's own logits: CE + lambda L with L within the quantisation bound of the sorted loss; the term is not small
    lg = got[5].transpose(0, 2, 3, 1).reshape(-1, 19)
    tgh = target.reshape(-1).astype(np.uint8)
    wref = w if w is not None else np.ones(19, np.float32)
    ce_ref = reference(lg, tgh, gen.IGNORE, wref)[0]
    l_ref = lov[0] * LR.lovasz_exact(lg, tgh, gen.IGNORE)
    live = tgh != gen.IGNORE
    tol = LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max())) + lov[0] * (1.0 / (2 * lov[1]) + 1e-6)
    print(f'head: CE + Lovasz {got[3]!r} ref {ce_ref + l_ref!r} error / bound = {abs(got[3] - ce_ref - l_ref) / tol:.3f}')
    assert abs(got[3] - (ce_ref + l_ref)) <= tol
    assert l_ref > 100 * tol


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


def test_train_step_with_lovasz_captured_equals_eager_and_validation_keeps_the_ce():
    (img, org), (tgt, _) = _batch()
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, lovasz=True)
        assert step.lovasz == (1.0, 1024)
        n = step.GRAPH_WARMUP + 2                                       # graph: the eager iterations, the capture, then a replay
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        if graph:
            assert step.graph_replays >= 1, 'the step with the Lovasz term was not captured and replayed'
        else:
            five, outs = _five(step, img, org, tgt, do_train=False)    # validation: the configured CE, no Lovasz term
            lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            tgh = tgt.cpu().numpy().reshape(-1)
            ce_ref = reference(lg, tgh, 255, np.ones(19, np.float32))[0]
            live = tgh != 255
            tol = LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max()))
            assert abs(float(five[0]) - ce_ref) <= tol, (five[0], ce_ref)
            assert LR.lovasz_exact(lg, tgh, 255) > 100 * tol
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


def test_the_training_ce_figure_includes_the_lovasz_term():
    (img, org), (tgt, _) = _batch()
    tgh = tgt.cpu().numpy().reshape(-1)
    lam, K = 0.5, 4096
    for fused in (True, False):
        model, step = _model_and_step(False, lovasz=(lam, K))
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
        ce_ref = reference(lg, tgh, 255, np.ones(19, np.float32))[0]
        l_ref = lam * LR.lovasz_exact(lg, tgh, 255)
        live = tgh != 255
        tol = LOSS_REL * abs(ce_ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max())) + lam * (1.0 / (2 * K) + 1e-6)
        print(f'fused_losses={fused}: CE + Lovasz {float(five[0])!r} ref {ce_ref + l_ref!r} error / bound = {abs(float(five[0]) - ce_ref - l_ref) / tol:.3f}')
        assert abs(float(five[0]) - (ce_ref + l_ref)) <= tol
        assert l_ref > 100 * tol
        step.release()


def test_off_is_the_step_built_without_the_argument():
    (img, org), (tgt, _) = _batch()
    res = []
    for kw in ({}, {'lovasz': None}, {'lovasz': False}, {'lovasz': 0}):
        model, step = _model_and_step(False, **kw)
        assert step.lovasz is None
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
    assert not any('lovasz' in c or c.endswith('_l') for c in res[0][1])


def test_check_lovasz_reads_the_dataset():
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    assert TR.check_lovasz({'settings': cs}) is None
    assert TR.check_lovasz({'settings': cs, 'lovasz': {'weight': 0.5}}) == (0.5, 1024)
    assert TR.check_lovasz({'settings': cs, 'lovasz': (2.0, 64)}) == (2.0, 64)

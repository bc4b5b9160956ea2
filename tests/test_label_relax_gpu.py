"""Boundary label relaxation on the GPU: dsrl_relax_mask against tests/label_relax_ref.mask_ref, exactly; the relaxed cross
entropy through the four paths of the training step against the float64 reference of label_relax_ref, inside bounds built from the weighted
suite's constants; and the step that uses it.

    A  dsrl_ce_fwd_r / dsrl_ce_bwd_r     HF.cross_entropy(label_relax=)
    B  dsrl_ce_fused_r                   the loss pass of HF.fused_losses(label_relax=)
    C  dsrl_convt2x2_fwd_ce_r            the value inside the last ConvTranspose forward (HF.logits_target(label_relax=))
    D  dsrl_convt2x2_bwd_ce_r            the gradient formed inside the ConvTranspose backward (HF.LogitsGrad.relax)

Bounds (label_relax_ref): loss LOSS_REL |L| + 2 M_ULPS ulp32(max |v| over live pixels) - the term carries two magnitudes, m and m_S; gradient
GRAD_TOL w[t_i] / D per summand, once on every class and once more on the classes of S_i; every element of every live pixel is checked, ignored
pixels are exactly 0.  B equals A bit for bit, D's dx / dw / db equal dsrl_ce_fused_r -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd bit for bit.

The identity: a mask of zeros (or of an image of one constant label) IS the weighted form.  Paths B, C and D are held to the bytes of their _w
siblings.  Path A is held to the bytes of path B's _w: the unfused weighted kernels (libm expf, (p - 1) sc) and the fused one (exp_nonpos,
e (sc / s) - sc) differ from each other in the parent already, and the relaxed form has ONE arithmetic for all paths - the fused one, which the
definition names."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gen                     # noqa: E402
import oracle as O             # noqa: E402
import label_relax_ref as RR   # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402
from ce_variant_runners import run_A, run_B, run_C, run_D, run_D_one, _convt_inputs   # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402
from dualsuperreslearningforsemseg_amd._lib import DsrlHipError  # noqa: E402

GUARD = 0x5A5A5A5A                     # the int32 pattern around a guarded buffer


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def weights_for(C, which):
    if which == 'ones':
        return np.ones(C, np.float32)
    w = np.random.RandomState(C).uniform(0.25, 8.0, C).astype(np.float32)
    w[C // 2] = 0.0                                  # one class of weight 0
    return w


def on_device(mask):
    return torch.tensor(np.ascontiguousarray(mask).astype(np.uint32).view(np.int32), device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------ the mask
def run_mask(tg, C, ii, r, stats=None, pad=64):
    """dsrl_relax_mask with `mask` between guard words -> (masks, the buffer); asserts the guards"""
    call, _ = _lib()
    N, H, W = tg.shape
    n = N * H * W
    buf = torch.full((n + 2 * pad,), GUARD, dtype=torch.int32, device=DEV)
    target = torch.tensor(tg, device=DEV)
    call('dsrl_relax_mask', target.data_ptr(), N, H, W, C, ii, r, buf.data_ptr() + 4 * pad, None if stats is None else stats.data_ptr(), HF._stream())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:pad] == GUARD) and np.all(h[pad + n:] == GUARD), 'wrote outside its N H W words'
    return h[pad:pad + n].view(np.uint32).reshape(N, H, W)


@pytest.mark.parametrize('r', [1, 2, 4])
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 3, 5), (2, 37, 130), (1, 64, 256), (3, 5, 1031)])
def test_mask_equals_the_reference_exactly(shape, r):
    for C, ii in ((19, 255), (3, 0), (32, -1)):
        for b in (2, 8):
            tg = RR.block_labels(*shape, C, b, 7 * r + b, ii if ii >= 0 else 255, p_bad=0.05)
            want, (live, multi) = RR.mask_ref(tg, C, ii, r)
            stats = torch.zeros(2, dtype=torch.int64, device=DEV)
            got = run_mask(tg, C, ii, r, stats)
            assert np.array_equal(got, want), (shape, r, C, ii, b)
            assert stats.cpu().tolist() == [live, multi]
            got2 = run_mask(tg, C, ii, r, stats)                # a second call ADDS to the counters and writes the same words
            assert np.array_equal(got2, want) and stats.cpu().tolist() == [2 * live, 2 * multi]
            assert np.array_equal(run_mask(tg, C, ii, r, None), want)          # without a record


def test_mask_sets_do_not_cross_an_image_or_wrap_a_row():
    tg = np.zeros((2, 20, 70), np.uint8); tg[1] = 5
    for r in (1, 2, 4):
        stats = torch.zeros(2, dtype=torch.int64, device=DEV)
        m = run_mask(tg, 19, 255, r, stats)
        assert np.all(m[0] == 1) and np.all(m[1] == 32) and stats.cpu().tolist() == [tg.size, 0]
    tg = np.zeros((1, 18, 66), np.uint8); tg[0, :, -1] = 3      # the last column's class never reaches the first column of the next row
    m = run_mask(tg, 19, 255, 4)
    assert np.array_equal(m, RR.mask_ref(tg, 19, 255, 4)[0]) and np.all(m[0, :, 0] == 1)


def test_mask_a_bad_argument_writes_nothing():
    call, _ = _lib()
    tg = torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV)
    out = torch.full((16,), 7, dtype=torch.int32, device=DEV)
    stats = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    for C, r in ((19, 0), (19, 5), (0, 1), (33, 1)):
        with pytest.raises(DsrlHipError, match='relax_mask'):
            call('dsrl_relax_mask', tg.data_ptr(), 1, 4, 4, C, 255, r, out.data_ptr(), stats.data_ptr(), HF._stream())
    with pytest.raises(DsrlHipError, match='relax_mask: bad arguments'):
        call('dsrl_relax_mask', None, 1, 4, 4, 19, 255, 1, out.data_ptr(), stats.data_ptr(), HF._stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((stats == 7).all())
    m = HF.relax_mask(tg, 19, 255, 2, None)
    assert m.dtype == torch.int32 and tuple(m.shape) == (1, 4, 4) and bool((m == 1).all())


# ------------------------------------------------------------------------------------------------------------------------------ paths A and B
def check_value_and_row(L, g, lg, tg, ii, w, mask, name):
    C = lg.shape[1]
    ref, gref, Dref = RR.relaxed_loss_and_grad(lg, tg, ii, w, mask)
    bound = RR.loss_bound(lg, tg, ii, ref)
    print(f'{name}: loss {L!r} ref {ref!r} error / bound = {abs(float(L) - ref) / bound:.3f}')
    assert abs(float(L) - ref) <= bound, f'{name}: loss {L!r} vs {ref!r}, bound {bound:.3e}'
    if g is None:
        return
    live = np.asarray(tg).astype(np.int64) != ii
    assert np.all(g[~live] == 0), f'{name}: nonzero gradient on an ignored pixel'
    gb = RR.grad_bound(tg, ii, w, mask, C)
    err = np.abs(g.astype(np.float64) - gref)
    assert not np.isnan(err[live]).any(), f'{name}: NaN in the gradient of a live pixel'
    ok = gb > 0
    print(f'{name}: max gradient error / bound = {float((err[ok] / gb[ok]).max(initial=0.0)):.3f}')
    assert np.all(err[live] <= gb[live]), f'{name}: gradient error beyond GRAD_TOL w / D per summand'


@pytest.mark.parametrize('P', [1, 63, 2048, 70001])
@pytest.mark.parametrize('C', [19, 3])
def test_paths_A_and_B_against_float64_and_each_other(C, P):
    for b, r in ((4, 1), (8, 2)) if P == 2048 else ((4, 1),):     # radius 2 needs the 8-grid for its one-class share; once is enough
        lg, tg, mask = RR.make_case(P, C, 100 + C + P % 97, b=b, r=r)
        if P >= 2048:
            s = RR.set_size_shares(mask, tg, C, 255)
            assert s[0] >= 0.2 and 1.0 - s[0] >= 0.2 and s[2] > 0 and (C < 4 or s[3] > 0), s
        mk = on_device(mask)
        for which in ('weights', 'ones'):
            w = weights_for(C, which)
            for layout in ('dense', 'slice'):
                name = f'C={C} P={P} b={b} r={r} {which} {layout}'
                La, Da, ga = run_A('_r', lg, tg, 255, w, mk.data_ptr(), layout)
                Lb, Db, fl, gb = run_B('_r', lg, tg, 255, w, mk.data_ptr(), layout)
                assert fl == 0
                assert _bits(La) == _bits(Lb) and _bits(Da) == _bits(Db) and ga.tobytes() == gb.tobytes(), f'{name}: fused and unfused differ'
                live = tg != 255
                if not live.any() or w[tg[live]].sum() == 0:
                    assert np.isnan(La)
                    continue
                check_value_and_row(La, ga, lg, tg, 255, w, mask, 'A/B ' + name)
                Lv, Dv, flv, none = run_B('_r', lg, tg, 255, w, mk.data_ptr(), layout, want_grad=False)
                assert none is None and _bits(Lv) == _bits(Lb) and _bits(Dv) == _bits(Db)


@pytest.mark.parametrize('C', [19, 3])
def test_arbitrary_words_give_the_result_of_the_cleaned_mask(C):
    P = 3001
    lg, tg, _ = RR.make_case(P, C, 55 + C)
    rs = np.random.RandomState(3)
    words = rs.randint(0, 2 ** 32, P, dtype=np.uint64).astype(np.uint32)
    words[::5] &= np.uint32(0x0000ffff if C == 19 else 0x6)      # some without high bits ...
    words[1::5] &= ~RR.clean(np.zeros(P, np.uint32), np.where(tg == 255, C, tg), C)[1::5]      # ... some without the own label's bit
    words[2::5] |= np.uint32(0xfff80000)                            # ... some with every bit >= 19
    cleaned = RR.clean(words, np.where(tg == 255, C, tg), C)
    assert (cleaned != words).mean() > 0.5 and not (cleaned >> np.uint32(C)).any()
    w = weights_for(C, 'weights')
    raw, cl = on_device(words), on_device(cleaned)
    for run in (run_A, run_B):
        a = run('_r', lg, tg, 255, w, raw.data_ptr())
        c = run('_r', lg, tg, 255, w, cl.data_ptr())
        assert _bits(a[0]) == _bits(c[0]) and a[-1].tobytes() == c[-1].tobytes()
    check_value_and_row(a[0], a[-1], lg, tg, 255, w, words, f'arbitrary words C={C}')


# ------------------------------------------------------------------------------------------------------------------------------ path C
def _convt_case(ii, N, H, W, seed, b=4, r=1):
    rs = np.random.RandomState(seed)
    x, wgt, bias, _ = _convt_inputs('randn', 255, rs, N, H, W)
    byte = 0 <= ii <= 255
    tg = RR.block_labels(N, 2 * H, 2 * W, 19, b, seed, ii if byte else 255, p_ignore=0.08 if byte else 0.0)      # no byte is ignored: no blocks of 255
    mask, _ = RR.mask_ref(tg, 19, ii, r)
    return x, wgt, bias, tg, mask


@pytest.mark.parametrize('ii', [255, 0, 18, -1])
def test_path_C_relaxed_value_inside_the_convT_forward(ii, monkeypatch):
    call, query = _lib()
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    N, H, W, C = 1, 3, 200, 19
    P = N * 4 * H * W
    x, wgt, bias, tg, mask = _convt_case(ii, N, H, W, 31 + (ii & 0xff))
    s = RR.set_size_shares(mask, tg, C, ii)
    assert s[0] >= 0.2 and 1.0 - s[0] >= 0.2 and s[2] > 0 and s[3] > 0, s
    mk = on_device(mask)
    for which in ('weights', 'ones'):
        w = weights_for(C, which)
        y0, Lw, Dw, flw = run_C('_w', x, wgt, bias, tg, ii, w)
        y1, L, Dg, fl = run_C('_r', x, wgt, bias, tg, ii, w, mk.data_ptr())
        assert _bits_equal(y0, y1) and fl == flw == 0 and _bits(Dg) == _bits(Dw)      # the logits themselves, and D, bit for bit
        lg = host(y1).reshape(P, C)
        LB, DB, flB, _ = run_B('_r', lg, tg.reshape(P), ii, w, mk.data_ptr(), want_grad=False)
        assert _bits(Dg) == _bits(DB) and flB == 0
        check_value_and_row(L, None, lg, tg.reshape(P), ii, w, mask.reshape(P), f'C ii={ii} {which}')
        check_value_and_row(LB, None, lg, tg.reshape(P), ii, w, mask.reshape(P), f'B on C ii={ii} {which}')
        assert abs(float(L) - float(Lw)) > 1e-3                  # ... and it is not the weighted value
        y2, L2, D2, fl2 = run_C('_r', x, wgt, bias, tg, ii, w, mk.data_ptr())
        assert _bits(L) == _bits(L2) and _bits(Dg) == _bits(D2) and fl == fl2


# ------------------------------------------------------------------------------------------------------------------------------ path D
def _path_D_inputs(N, H, ft, seed, W=128, C=19):
    rs = np.random.RandomState(seed)
    P = N * 4 * H * W
    tg = RR.block_labels(N, 2 * H, 2 * W, C, 4, seed)
    mask, _ = RR.mask_ref(tg, C, 255, 1)
    lg = (3.0 * rs.standard_normal((P, C))).astype(np.float32)
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    wgt = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor(lg.reshape(N, 2 * H, 2 * W, C), device=DEV)
    target = torch.tensor(tg, device=DEV)
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    return lg, tg, mask, x, wgt, logits, target, ftg, ftw


@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('N,H', [(1, 3), (2, 5)])
def test_path_D_relaxed_gradient_inside_the_convT_backward(N, H, ft, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
    W, C = 128, 19
    P = N * 4 * H * W
    lg, tg, mask, x, wgt, logits, target, ftg, ftw = _path_D_inputs(N, H, ft, 900 + 10 * N + ft)
    s = RR.set_size_shares(mask, tg, C, 255)
    assert s[0] >= 0.2 and 1.0 - s[0] >= 0.2 and s[2] > 0 and s[3] > 0, s
    mk = on_device(mask)
    for which in ('weights', 'ones'):
        w = weights_for(C, which)
        (dx, dw, db, dl_ce, fl), (dx2, dw2, db2) = run_D('_r', x, wgt, logits, target, 255, w, mk.data_ptr(), ftg, ftw, ft)
        assert fl == 0
        assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2), 'one call and three calls differ'
        (_, _, _, _, _), (dx3, dw3, db3) = run_D('_r', x, wgt, logits, target, 255, w, mk.data_ptr(), ftg, ftw, ft)      # twice: the same bytes
        assert _bits_equal(dx2, dx3) and _bits_equal(dw2, dw3) and _bits_equal(db2, db3)
        ref, g64, Dref = RR.relaxed_loss_and_grad(lg, tg.reshape(P), 255, w, mask.reshape(P))
        gb = RR.grad_bound(tg.reshape(P), 255, w, mask.reshape(P), C)
        row = host(dl_ce).reshape(P, C)
        live = tg.reshape(P) != 255
        err = np.abs(row.astype(np.float64) - g64)
        print(f'D N={N} H={H} ft={ft} {which}: max row error / bound = {float((err[gb > 0] / gb[gb > 0]).max()):.3f}')
        assert np.all(row[~live] == 0) and np.all(err[live] <= gb[live])
        g64 = g64.reshape(N, 2 * H, 2 * W, C)
        if ft:
            g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
        dxo, dwo, dbo = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(wgt).astype(np.float64),
                                                    g64.transpose(0, 3, 1, 2), has_bias=True)
        check(host(dx2).transpose(0, 3, 1, 2), dxo, 1e-5, 'dx'); check(host(dw2), dwo, 1e-5, 'dw'); check(host(db2), dbo, 1e-5, 'db')


# ------------------------------------------------------------------------------------------------------------------------------ the identity
@pytest.mark.parametrize('kind', ['zeros', 'constant_image'])
def test_singleton_masks_are_the_weighted_form_byte_for_byte(kind, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
    C = 19
    rs = np.random.RandomState(12)
    w = weights_for(C, 'weights')
    w[C // 2] = 1.5                                             # (the constant label below must carry weight)

    def labels(shape):
        if kind == 'constant_image':
            return np.full(shape, C // 2, np.uint8)
        t = rs.randint(0, C, shape).astype(np.uint8)
        t[rs.uniform(size=shape) < 0.1] = 255
        return t

    def mask_of(t):
        if kind == 'zeros':
            return torch.zeros(t.size, dtype=torch.int32, device=DEV)
        m = run_mask(t, C, 255, 2)
        assert np.all(m == np.uint32(1 << (C // 2)))
        return on_device(m)

    # paths A and B (A against B's weighted bytes: see the module docstring)
    for P, layout in ((1, 'dense'), (2048, 'dense'), (3001, 'slice')):
        t = labels((1, 1, P))
        lg = (3.0 * rs.standard_normal((P, C))).astype(np.float32)
        lg[::11] *= 30
        mk = mask_of(t)
        Lw, Dw, flw, gw = run_B('_w', lg, t.reshape(P), 255, w, None, layout)
        Lr, Dr, flr, gr = run_B('_r', lg, t.reshape(P), 255, w, mk.data_ptr(), layout)
        La, Da, ga = run_A('_r', lg, t.reshape(P), 255, w, mk.data_ptr(), layout)
        assert _bits(Lw) == _bits(Lr) == _bits(La) and _bits(Dw) == _bits(Dr) == _bits(Da) and flw == flr
        assert gw.tobytes() == gr.tobytes() == ga.tobytes()
    # path C
    x, wgt, bias, _ = _convt_inputs('randn', 255, rs)
    t = labels((1, 6, 400))
    mk = mask_of(t)
    yw, Lw, Dw, flw = run_C('_w', x, wgt, bias, t, 255, w)
    yr, Lr, Dr, flr = run_C('_r', x, wgt, bias, t, 255, w, mk.data_ptr())
    assert _bits_equal(yw, yr) and _bits(Lw) == _bits(Lr) and _bits(Dw) == _bits(Dr) and flw == flr
    # path D
    N, H, W = 2, 3, 128
    t = labels((N, 2 * H, 2 * W))
    mk = mask_of(t)
    xx = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    ww = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor((3.0 * rs.standard_normal((N, 2 * H, 2 * W, C))).astype(np.float32), device=DEV)
    target = torch.tensor(t, device=DEV)
    ftg = torch.tensor(rs.standard_normal((N, 1, 32)).astype(np.float32), device=DEV)
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV)
    (_, _, _, dlw, _), (dxw, dww, dbw) = run_D('_w', xx, ww, logits, target, 255, w, None, ftg, ftw, 8)
    (_, _, _, dlr, _), (dxr, dwr, dbr) = run_D('_r', xx, ww, logits, target, 255, w, mk.data_ptr(), ftg, ftw, 8)
    assert _bits_equal(dlw, dlr) and _bits_equal(dxw, dxr) and _bits_equal(dww, dwr) and _bits_equal(dbw, dbr)


# ------------------------------------------------------------------------------------------------------------------------------ edges
def test_edges_far_sets_infinities_equal_logits_and_flags():
    C = 5
    w = np.array([1.0, 2.0, 0.5, 1.5, 1.0], np.float32)
    ninf = -np.inf
    lg = np.array([[0.0, -200.0, -201.0, 3.0, -5.0],           # 0: the set {1, 2} lies 200 below the largest logit
                   [1.0, ninf, 0.5, 2.0, -1.0],                # 1: a -inf logit inside the set {1, 2}
                   [1.0, 0.5, ninf, 2.0, -1.0],                # 2: a -inf logit outside the set {0, 1}
                   [7.0, 2.5, 2.5, 2.5, -3.0],                 # 3: all set logits equal, {1, 2, 3}
                   [0.5, 0.25, 0.0, -0.25, 1.0]], np.float32)  # 4: a singleton
    tg = np.array([1, 2, 0, 2, 4], np.uint8)
    mask = np.array([0b00110, 0b00110, 0b00011, 0b01110, 0], np.uint32)
    mk = on_device(mask)
    La, Da, ga = run_A('_r', lg, tg, 255, w, mk.data_ptr())
    Lb, Db, fl, gb = run_B('_r', lg, tg, 255, w, mk.data_ptr())
    assert fl == 0 and _bits(La) == _bits(Lb) and ga.tobytes() == gb.tobytes()
    assert np.isfinite(La) and np.all(np.isfinite(gb))
    check_value_and_row(Lb, gb, lg, tg, 255, w, mask, 'edges')
    one = lambda i: run_B('_r', lg[i:i + 1], tg[i:i + 1], 255, w, on_device(mask[i:i + 1]).data_ptr())       # noqa: E731
    L0 = one(0)[0]
    assert 200.0 < L0 < 204.0, L0                               # finite where -log(sum_S e_c / s) on the shared terms is infinite
    g3 = gb[3]
    assert _bits(g3[1]) == _bits(g3[2]) == _bits(g3[3])        # equal logits in the set: equal elements
    # every pixel ignored: NaN loss (0 / 0), zero rows, no flag
    ig = np.full(5, 255, np.uint8)
    L, Dg, fl, g = run_B('_r', lg, ig, 255, w, mk.data_ptr())
    assert np.isnan(L) and Dg == 0.0 and fl == 0 and not g.any()
    # a NaN logit raises flag bit 1 in a live pixel only
    bad = lg.copy(); bad[4, 2] = np.nan
    assert run_B('_r', bad, tg, 255, w, mk.data_ptr())[2] == 1
    t2 = tg.copy(); t2[4] = 255
    L, _, fl, g = run_B('_r', bad, t2, 255, w, mk.data_ptr())
    flw = run_B('_w', bad, t2, 255, w, None)[2]
    assert fl == flw and np.isfinite(L) and not g[4].any()      # in an ignored pixel: the flag of the weighted form (its check covers every logit), a finite loss, a zero row
    # a label >= C that is not ignore_index: flag bit 2, NaN loss, weight 0 through the table
    t3 = tg.copy(); t3[4] = 9
    L, _, fl, g = run_B('_r', lg, t3, 255, w, mk.data_ptr())
    assert fl == 2 and np.isnan(L) and np.all(np.isfinite(g))
    Lw, _, flw, gw = run_B('_w', lg, t3, 255, w, None)
    assert flw == 2 and g[4].tobytes() == gw[4].tobytes()


def test_a_bad_argument_writes_nothing():
    C = 19
    lg, tg, mask = RR.make_case(63, C, 8)
    w = weights_for(C, 'ones')
    big = np.zeros((63, 40), np.float32)
    mk = on_device(mask)
    for run in (run_A, run_B):
        for out in (run('_r', lg, tg, 255, w, None, expect_error=True),                                         # no mask
                    run('_r', big, tg, 255, np.ones(40, np.float32), mk.data_ptr(), expect_error=True)):        # more than 32 classes
            assert out[0] == 7.0 and out[1] == 7.0 and np.all(out[-1] == 7.0)                                   # the pre-filled outputs stay
    rs = np.random.RandomState(5)
    x, wgt, bias, t = _convt_inputs('randn', 255, rs)
    y, L, Dg, fl = run_C('_r', x, wgt, bias, t, 255, w, None, expect_error=True)
    assert bool((y == 7.0).all()) and L == 7.0 and Dg == 7.0 and fl == 0
    xt = torch.tensor(x, device=DEV); wt = torch.tensor(wgt, device=DEV)
    logits = torch.zeros((1, 6, 400, C), device=DEV); target = torch.tensor(t, device=DEV)
    dx, dw, db = run_D_one('_r', xt, wt, logits, target, 255, w, None, torch.ones(8, device=DEV), None, None, 0, expect_error=True)
    assert bool((dx == 7.0).all()) and bool((dw == 7.0).all()) and bool((db == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------------ head: hand-over, gradients
def test_relaxed_fused_losses_on_the_head_hands_over_and_matches_autograd(monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    w = weights_for(19, 'weights')

    def step(mode, inputs):
        """'plain': no hand-over, HF.cross_entropy(label_relax=mask) + mse + FA through autograd; 'fused': fused_losses(label_relax=mask), the same mask
        given to logits_target; 'second': likewise while another consumer sends the logits a gradient of its own (zeros)"""
        x16, x4, target, org = inputs
        monkeypatch.setattr(HF, 'convt_ce_enabled', mode != 'plain')
        monkeypatch.setattr(HF, 'grad_slots_enabled', mode != 'plain')
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        tgt = dev(target); o = dev(org)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        mask = HF.relax_mask(tgt, 19, gen.IGNORE, 1)
        calls = []
        orig = HF.call
        monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
        if mode == 'plain':
            outs = head(a, b)
            ce = HF.cross_entropy(outs[0], tgt, gen.IGNORE, weight=w, label_relax=mask)
            total = ce + 0.1 * HF.mse_loss(outs[1], o) + 1.0 * D.FALoss()(outs[2], outs[3])
            total.backward()
            ce = float(ce.detach())
        else:
            with HF.logits_target(tgt, gen.IGNORE, flag, w, label_relax=mask):
                outs = head(a, b)
            vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=w, label_relax=mask)
            h = getattr(outs[0], '_dsrl_logits_grad', None)
            if mode == 'second':
                torch.autograd.backward([vals, outs[0]], [torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=DEV), torch.zeros_like(outs[0])])
            else:
                vals[3].backward()
            assert h is None or (not h.armed and h.relax is None and h.weight is None), 'holder left armed'
            ce = float(vals[0])
        monkeypatch.setattr(HF, 'call', orig)
        torch.cuda.synchronize()
        assert int(flag) == 0
        return {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad), ce, host(outs[0]), calls, mask.cpu().numpy()

    def inputs(seed, w16):
        x16, x4, target, org = gen.make_head_inputs(seed, 2, 2, w16, gen.SMALL)
        return x16, x4, RR.block_labels(*target.shape, 19, 8, seed), org     # labels with borders (the generator's are noise)

    big = inputs(303, 8)                                          # logits 64 x 256: the forward and the backward kernels both qualify
    ref = step('plain', big)
    assert 'dsrl_ce_fwd_r' in ref[5] and 'dsrl_ce_bwd_r' in ref[5]
    for mode in ('fused', 'second'):
        got = step(mode, big)
        calls = got[5]
        assert 'dsrl_convt2x2_fwd_ce_r' in calls, calls
        if mode == 'fused':
            assert 'dsrl_convt2x2_bwd_ce_r' in calls and 'dsrl_ce_fused_r' not in calls, calls
        else:                                                     # another consumer sent a gradient too: the relaxed row is written by dsrl_ce_fused_r
            assert 'dsrl_convt2x2_bwd_ce_r' not in calls and calls.count('dsrl_ce_fused_r') == 1, calls
        assert not any(c.startswith(('dsrl_ce_fused_w', 'dsrl_convt2x2_fwd_ce_w', 'dsrl_convt2x2_bwd_ce_w')) for c in calls), calls
        for k in ref[0]:
            check(got[0][k], ref[0][k], 1e-6, f'{mode} grad {k}')
        check(got[1], ref[1], 1e-6, 'dx16'); check(got[2], ref[2], 1e-6, 'dx4')
        lg = got[4].transpose(0, 2, 3, 1).reshape(-1, 19)
        tgh = big[2].reshape(-1)
        mask = got[6].view(np.uint32).reshape(-1)
        assert np.array_equal(mask, RR.mask_ref(big[2], 19, gen.IGNORE, 1)[0].reshape(-1))
        check_value_and_row(got[3], None, lg, tgh, gen.IGNORE, w, mask, f'head CE ({mode})')
    small = inputs(202, 4)                                        # logits too narrow for the backward kernel: the loss pass writes the row itself
    refs = step('plain', small)
    gots = step('fused', small)
    assert 'dsrl_convt2x2_bwd_ce_r' not in gots[5] and gots[5].count('dsrl_ce_fused_r') == 1, gots[5]
    for k in refs[0]:
        check(gots[0][k], refs[0][k], 1e-6, f'small grad {k}')


# ------------------------------------------------------------------------------------------------------------------------------ TrainStep, train_or_resume
def _model_and_step(graph, w, **kw):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(77)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    HF.set_dropout_seed(1234)
    return model, TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph, class_weights=w, **kw)


def _five(step, img, org, tgt, do_train=True):
    while step._pending:
        step.collect()
    outs = step.enqueue(img, org, tgt, 0.006, 0.9, 5e-4, do_train)
    hostbuf, ev = step._pending[-1]
    ev.synchronize()
    five = hostbuf.clone().numpy()
    step.collect()
    return five, outs


def _block_batch():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    tgt = torch.tensor(RR.block_labels(*tgt.shape, 19, 8, 5), device=DEV)      # labels with borders: the synthetic ones are noise
    return img, org, tgt


def test_train_step_with_label_relax_captured_equals_eager_and_validation_keeps_the_configured_ce(monkeypatch):
    img, org, tgt = _block_batch()
    w = weights_for(19, 'weights')
    tgh = tgt.cpu().numpy()
    want_mask, (live, multi) = RR.mask_ref(tgh, 19, 255, 1)
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, w, label_relax=1)
        assert step.label_relax == 1 and step.relax_classes == 19 and step._graph_key(img, org, tgt)[-2] == 1
        n = step.GRAPH_WARMUP + 3
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        assert step.relax_stats.cpu().tolist() == [n * live, n * multi]
        assert step.relax_fraction(reset=True) == multi / live and step.relax_stats.cpu().tolist() == [0, 0]
        if graph:
            assert step.graph_replays >= 2, 'the relaxed step was not captured and replayed'
        else:
            calls = []
            orig = HF.call
            monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
            five, outs = _five(step, img, org, tgt)                     # a training iteration: the relaxed kernels, the mask in front of the forward
            train_calls = list(calls); del calls[:]
            five_v, outs_v = _five(step, img, org, tgt, do_train=False)  # validation: the configured (weighted) CE
            monkeypatch.setattr(HF, 'call', orig)
            assert train_calls.count('dsrl_relax_mask') == 1, train_calls
            assert train_calls.index('dsrl_relax_mask') < train_calls.index('dsrl_convt2x2_fwd_ce_r')
            assert 'dsrl_convt2x2_bwd_ce_r' in train_calls and not any(c.startswith('dsrl_ce_fused') for c in train_calls), train_calls
            assert not any(c.endswith('_r') or c == 'dsrl_relax_mask' for c in calls), calls
            assert any(c.endswith('_w') for c in calls), calls
            lg = host(outs_v[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            ref_w, _, _ = RR.weighted_loss_and_grad(lg, tgh.reshape(-1), 255, w)
            assert abs(float(five_v[0]) - ref_w) <= RR.loss_bound(lg, tgh.reshape(-1), 255, ref_w)
            lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
            ref_r, _, _ = RR.relaxed_loss_and_grad(lg, tgh.reshape(-1), 255, w, want_mask.reshape(-1))
            assert abs(float(five[0]) - ref_r) <= RR.loss_bound(lg, tgh.reshape(-1), 255, ref_r)
            step.relax_stats.zero_()
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


def test_label_relax_none_is_the_step_built_without_the_argument(monkeypatch):
    img, org, tgt = _block_batch()
    w = weights_for(19, 'weights')
    seen = {}
    for tag, kw in (('without', {}), ('none', dict(label_relax=None)), ('zero', dict(label_relax=0))):
        model, step = _model_and_step(False, w, **kw)
        assert step.label_relax is None and step.relax_stats is None and step.relax_fraction() is None
        _five(step, img, org, tgt)                                      # (whatever a process does once is behind us)
        calls = []
        orig = HF.call
        monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
        five, _ = _five(step, img, org, tgt)
        monkeypatch.setattr(HF, 'call', orig)
        seen[tag] = (calls, five.tobytes(), step._graph_key(img, org, tgt))
        step.release()
    assert seen['without'] == seen['none'] == seen['zero']
    assert not any(c.endswith('_r') or c == 'dsrl_relax_mask' for c in seen['none'][0])


def test_unfused_losses_of_the_train_step_relax_too():
    img, org, tgt = _block_batch()
    w = weights_for(19, 'weights')
    tgh = tgt.cpu().numpy()
    mask = RR.mask_ref(tgh, 19, 255, 2)[0].reshape(-1)
    for fused in (True, False):
        model, step = _model_and_step(False, w, label_relax={'radius': 2})
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
        ref, _, _ = RR.relaxed_loss_and_grad(lg, tgh.reshape(-1), 255, w, mask)
        assert abs(float(five[0]) - ref) <= RR.loss_bound(lg, tgh.reshape(-1), 255, ref), (fused, five[0], ref)
        step.release()


def test_train_or_resume_passes_label_relax_on_and_writes_the_record_keys(tmp_path):
    from test_augment_gpu import _cache_tree
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import train_or_resume
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    data, _ = _cache_tree(tmp_path)

    def run(tag, **extra):
        torch.manual_seed(1234)
        HF.set_dropout_seed(77)
        kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                  dataset=dict({'path': data, 'settings': cs}, **extra), val_interval=1, checkpoint_interval=1, checkpoint_history=2,
                  init_weights=None, batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9, weights_decay=5e-4,
                  poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / tag), description='test',
                  early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))
        return train_or_resume(is_resuming_training=False, **kw)

    h0 = run('a')
    h1 = run('b', label_relax=2)
    assert 'train_ce_is_relaxed' not in h0[0] and 'relaxed_fraction' not in h0[0]
    assert h1[0]['train_ce_is_relaxed'] is True and 0.0 <= h1[0]['relaxed_fraction'] <= 1.0
    assert all(np.isfinite(v) for v in h1[0]['train'][:4]) and np.isfinite(h1[0]['val'][3])
    if h1[0]['relaxed_fraction'] > 0:
        assert h1[0]['train'][0] != h0[0]['train'][0]            # the relaxed CE is what the training iterations report

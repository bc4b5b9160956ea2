"""The memory-bound kernels of csrc/spatial.hip (3x3/2 max pool, align-corners bilinear resize, global average pool, image import) and the
tail of csrc/losses.hip (SGD update, validation counters) at their edges, each against the plain float64 reference of tests/spatial_ref.py
(which tests/test_spatial_refs_host.py holds against stock torch).  Every launch is a plain streaming one at a small shape.

u = 2^-24 is the unit roundoff of float32 (round to nearest: one operation errs by at most u times its result).  The library is built with
-ffp-contract=off, so the operation counts below are the ones written in the kernels.  Every tolerance-based test prints its largest observed
error / bound."""
import numpy as np
import pytest
import torch

import spatial_ref as R
from hip_helpers import DEV, HF, dev, host

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64 = np.float64


def worst_ratio(err, bound):
    """largest error / bound; an element whose bound is 0 has to be exact"""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert not np.isnan(err).any()
    assert not (err[bound == 0] != 0).any(), 'error on an element whose bound is 0'
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


def nhwc_view(a, width=None, lo=0, fill=0.0):
    """a (N, C, H, W) numpy float32 -> the logical (N, C, H, W) device view of channels lo : lo + C of a pixel-major buffer `width` channels wide
    (pixel stride `width`), the other channels holding `fill`.  width None: the dense pixel-major tensor."""
    N, C, H, W = a.shape
    if width is None:
        return dev(a)
    big = np.full((N, H, W, width), fill, np.float32)
    big[..., lo:lo + C] = a.transpose(0, 2, 3, 1)
    return torch.from_numpy(big).to(DEV).permute(0, 3, 1, 2)[:, lo:lo + C]


# ------------------------------------------------------------------------------------------------ max pool
POOL_SIZES = [(1, 1), (1, 7), (2, 2), (3, 3), (7, 10), (16, 9), (33, 34)]


def _check_max_pool(N, C, H, W, kind):
    rs = np.random.RandomState(1000 * H + 10 * W + C)
    x = R.maxpool_input(kind, (N, C, H, W), rs)
    Ho, Wo = R.pool_out(H), R.pool_out(W)
    dy = R.integer_grad(rs, (N, C, Ho, Wo))
    y_ref, tap = R.max_pool3x3s2(x)
    dx_ref = R.max_pool3x3s2_bwd((H, W), tap, dy)
    what = f'{kind} N={N} C={C} {H}x{W}'
    xt = dev(x).requires_grad_(True)
    y = HF.max_pool3x3s2(xt)
    y.backward(dev(dy))
    assert np.array_equal(host(y), y_ref, equal_nan=True), what + ': y'
    bad = np.argwhere(host(xt.grad) != dx_ref)
    assert bad.size == 0, f'{what}: dx differs at {len(bad)} elements, first (n, c, h, w) = {bad[0]}'
    # the forward without a backward pass: a null argmax pointer
    xd = HF.pm_dense(dev(x))
    y2 = HF.new_cl((N, C, Ho, Wo), xd)
    HF.call('dsrl_maxpool3x3s2_fwd', xd.data_ptr(), y2.data_ptr(), None, N, H, W, C, HF._stream())
    assert np.array_equal(host(y2), y_ref, equal_nan=True), what + ': y without argmax'


@pytest.mark.parametrize('kind', R.MAXPOOL_KINDS)
@pytest.mark.parametrize('C', [64, 8, 4, 5, 1, 19])
def test_max_pool_values_and_gradient_routing_are_torchs_bit_for_bit(C, kind):
    """C % 4 == 0: maxpool_fwd4_kernel / maxpool_bwd4_kernel (four argmax bytes in one word); else the scalar kernels.  y and dx bit-equal to
    the float64 reference with torch's scan (dy is integer-valued: the backward sums are exact), on tied windows, constant maps, -inf windows
    on the border and inside, +inf, single NaNs and several NaNs in one window, at H or W of 1, 2, 3 and odd / even sizes."""
    for H, W in POOL_SIZES:
        _check_max_pool(2, C, H, W, kind)


@pytest.mark.parametrize('kind', R.MAXPOOL_KINDS)
def test_max_pool_three_images_of_the_stem_width(kind):
    """N = 3, C = 64, 33x34: 55 blocks of the vector kernels, the e % C4 split over 16 channel groups"""
    _check_max_pool(3, 64, 33, 34, kind)


# ------------------------------------------------------------------------------------------------ bilinear
BILINEAR_SHAPES = [((2, 2), (65, 33)), ((5, 7), (13, 9)), ((13, 9), (5, 7)), ((33, 17), (4, 3)), ((9, 13), (9, 13)), ((7, 5), (1, 1)),
                   ((8, 6), (1, 11)), ((1, 1), (4, 8)), ((3, 64), (6, 127))]
# name: (channels, width of the buffer or None = dense, first channel)
BILINEAR_LAYOUTS = {'dense8': (8, None, 0), 'dense19': (19, None, 0), 'dense1': (1, None, 0),
                    'slice4:12': (8, 24, 4),       # 16-byte aligned base, pixel stride 24: the 16-byte path with a stride
                    'slice1:9': (8, 24, 1),        # C % 4 == 0 but a base that is not 16-byte aligned: the any-width path
                    'slice3:22': (19, 24, 3)}
SENTINEL = -12345.0


def _resize(x, dy, width, lo, size):
    xt = nhwc_view(x, width, lo, fill=3e7).detach().requires_grad_(True)
    y = HF.upsample_bilinear_ac(xt, size)
    y.backward(nhwc_view(dy, width, lo, fill=-3e7))
    torch.cuda.synchronize()
    return host(y), host(xt.grad)


@pytest.mark.parametrize('shape', BILINEAR_SHAPES, ids=lambda s: f'{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}')
def test_bilinear_resize_up_down_identity_and_strided(shape, monkeypatch):
    """HF.upsample_bilinear_ac forward and backward: upscaling, downscaling (ac_range with scale > 1), identity, output size 1 and large ratios
    (dozens of outputs gathered into one input pixel), dense and as channel slices of a 24-channel pixel-major buffer whose other channels hold
    3e7 (read by mistake they would swamp the result).  The reference has the kernels' float32 source coordinates, so what remains is the
    rounding of the blend; the bounds are written at the asserts."""
    (H, W), (Ho, Wo) = shape
    N = 2
    A, B = R.bilinear_matrices(H, W, Ho, Wo)
    T = R.max_taps(A, B)
    monkeypatch.setenv('DSRL_BILINEAR_G4', '1')
    worst_f = worst_b = 0.0
    for name, (C, width, lo) in BILINEAR_LAYOUTS.items():
        rs = np.random.RandomState(100 * H + Wo + C + lo)
        x = rs.standard_normal((N, C, H, W)).astype(np.float32)
        dy = rs.standard_normal((N, C, Ho, Wo)).astype(np.float32)
        y, dx = _resize(x, dy, width, lo, (Ho, Wo))
        what = f'{name} {H}x{W}->{Ho}x{Wo}'
        # forward: v = (1-lh) * ((1-lw) * x00 + lw * x01) + lh * ((1-lw) * x10 + lw * x11): every product term passes at most 6 roundings (1-lw, the
        # product, the inner sum, 1-lh, the product, the outer sum), (1 + u)^6 - 1 < 8 u of its magnitude: |y - ref| <= 8 u (|A| |x| |B|^T)
        rf = worst_ratio(np.abs(y - R.bilinear_fwd(A, B, x)), 8 * U * R.bilinear_fwd(np.abs(A), np.abs(B), np.abs(x)))
        # backward: two gathers, along W then along H; a gather of t taps rounds 1-l or nothing, each product and each of t additions: (t + 2) u of
        # the magnitude; the two in sequence with t_w + t_h <= T: |dx - ref| <= (T + 4) u (|A|^T |dy| |B|)
        rb = worst_ratio(np.abs(dx - R.bilinear_bwd(A, B, dy)), (T + 4) * U * R.bilinear_bwd(np.abs(A), np.abs(B), np.abs(dy)))
        assert rf <= 1.0, f'{what}: forward error {rf:.3f} x the bound'
        assert rb <= 1.0, f'{what}: backward error {rb:.3f} x the bound (T = {T})'
        worst_f, worst_b = max(worst_f, rf), max(worst_b, rb)
        if (H, W) == (Ho, Wo):
            assert np.array_equal(y, x), what + ': the identity resize changed the input'
        if name in ('dense19', 'slice1:9'):         # the same numbers from the one-element-per-thread kernels
            monkeypatch.setenv('DSRL_BILINEAR_G4', '0')
            y0, dx0 = _resize(x, dy, width, lo, (Ho, Wo))
            monkeypatch.setenv('DSRL_BILINEAR_G4', '1')
            assert np.array_equal(y0, y) and np.array_equal(dx0, dx), what + ': DSRL_BILINEAR_G4=0 differs'
        if name == 'slice1:9':                      # the same numbers as the 16-byte path gives the aligned slice of the same values
            ya, dxa = _resize(x, dy, 24, 4, (Ho, Wo))
            assert np.array_equal(ya, y) and np.array_equal(dxa, dx), what + ': differs from the aligned slice'
        if width is not None:
            # strided destinations (the library's own interface): the other channels of the buffers keep their sentinel
            xv, dyv = nhwc_view(x, width, lo, fill=3e7), nhwc_view(dy, width, lo, fill=-3e7)
            ybig = torch.full((N, Ho, Wo, width), SENTINEL, device=DEV).permute(0, 3, 1, 2)
            dxbig = torch.full((N, H, W, width), SENTINEL, device=DEV).permute(0, 3, 1, 2)
            yv, dxv = ybig[:, lo:lo + C], dxbig[:, lo:lo + C]
            HF.call('dsrl_bilinear_ac_fwd', xv.data_ptr(), width, yv.data_ptr(), width, N, H, W, C, Ho, Wo, HF._stream())
            ws = torch.empty(max(int(HF.cquery('dsrl_bilinear_ac_bwd_workspace_bytes', N, H, W, C, Ho, Wo)), 256), device=DEV, dtype=torch.uint8)
            HF.call('dsrl_bilinear_ac_bwd', dyv.data_ptr(), width, dxv.data_ptr(), width, N, H, W, C, Ho, Wo, ws.data_ptr(), ws.numel(), HF._stream())
            torch.cuda.synchronize()
            for got, want, s in ((host(ybig), y, 'y'), (host(dxbig), dx, 'dx')):
                assert np.array_equal(got[:, lo:lo + C], want), f'{what}: strided {s} differs from the dense one'
                assert (np.delete(got, np.s_[lo:lo + C], axis=1) == SENTINEL).all(), f'{what}: strided {s} wrote outside its channels'
    print(f'bilinear {H}x{W}->{Ho}x{Wo}: largest error / bound forward {worst_f:.3f}, backward {worst_b:.3f} (T = {T})')


# ------------------------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize('N,C,H,W,width,lo', [(2, 19, 1, 1, None, 0), (2, 65, 1, 3, None, 0), (3, 130, 5, 7, None, 0), (2, 64, 32, 64, None, 0),
                                              (2, 19, 5, 7, 24, 3)])
@pytest.mark.parametrize('offset', [False, True], ids=['noise', 'offset100'])
def test_global_average_pool_strided_ragged_and_single_pixel(N, C, H, W, width, lo, offset):
    """gap_fwd_kernel on HW = 1, on C that is no multiple of its 64-channel blocks with HW that is no multiple of its 4 pixel slots, and on a
    channel slice of a wider buffer; both backward kernels (C = 64: 16-byte stores, else the scalar one)."""
    rs = np.random.RandomState(C * 100 + H * W)
    HW = H * W
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    if offset:
        x += (100.0 * np.where(np.arange(C) % 2, -1.0, 1.0)).astype(np.float32).reshape(1, C, 1, 1)      # +100 / -100 by channel on top of the unit noise
    dy = rs.standard_normal((N, C, 1, 1)).astype(np.float32)
    xt = nhwc_view(x, width, lo, fill=3e7).detach().requires_grad_(True)
    y = HF.global_avg_pool(xt)
    y.backward(dev(dy))
    x64 = x.astype(F64)
    # forward: a slot adds its ceil(HW / 4) pixels in sequence (at most HW/4 roundings, each of at most u x the sum of magnitudes), three additions merge
    # the four slots and one division forms the mean: |y - mean| <= (HW/4 + 4) u mean|x|
    r = worst_ratio(np.abs(host(y) - x64.mean((2, 3), keepdims=True)), (HW / 4 + 4) * U * np.abs(x64).mean((2, 3), keepdims=True))
    print(f'global average pool N={N} C={C} {H}x{W} {"slice" if width else "dense"} {"offset" if offset else "noise"}: largest error / bound {r:.3f}')
    assert r <= 1.0
    inv = np.float32(1.0 / HW)
    assert inv == np.float32(1.0) / np.float32(HW)         # the kernel's float32 division gives the same factor
    assert np.array_equal(host(xt.grad), np.broadcast_to(dy * inv, x.shape))


# ------------------------------------------------------------------------------------------------ SGD
SGD_HYPER = [(0.006, 0.9, 5e-4, 1.0), (0.01, 0.0, 0.0, 0.125), (0.1, 0.9, 0.0, 3.0)]       # lr, momentum, weight decay, grad_scale
GUARD = 8


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 4 * 2 ** 20 + 4099])
def test_sgd_step_tails_wrapped_grid_and_grad_scale(n):
    """dsrl_sgd_step and dsrl_sgd_step_dev on n < 4 (scalar tail only), n % 4 != 0, and 4 * 2^20 + 4099 floats: more than 4096 blocks x 256 threads
    x 4 floats, so the grid-stride loop wraps, with a 3-float tail.  Two steps from a non-zero momentum buffer; each step is compared with the
    float64 update of the state the device held before it, with the hyper-parameters rounded to float32 as the kernels receive them."""
    rs = np.random.RandomState(n % 9973)
    p0, b0 = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    grads = [rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)]
    guard = np.float32([1e9, -2e9, 3e9, -4e9, 5e9, -6e9, 7e9, -8e9])

    def arena(a):
        return torch.from_numpy(np.concatenate([a, guard])).to(DEV)

    worst_p = worst_b = 0.0
    for hyper in SGD_HYPER:
        lr, mom, wd, gs = (float(v) for v in np.float32(hyper))
        hyper_dev = torch.tensor(hyper, dtype=torch.float32, device=DEV)
        P, Bf, P2, B2 = arena(p0), arena(b0), arena(p0), arena(b0)
        p_prev, b_prev = p0.astype(F64), b0.astype(F64)
        for g in grads:
            G = arena(g)
            HF.sgd_step_(P[:n], G[:n], Bf[:n], *hyper)
            HF.sgd_step_dev_(P2[:n], G[:n], B2[:n], hyper_dev)
            torch.cuda.synchronize()
            ph, bh = P.cpu().numpy(), Bf.cpu().numpy()
            assert torch.equal(P, P2) and torch.equal(Bf, B2), f'n={n} {hyper}: the two entry points differ'
            for a in (ph[n:], bh[n:], G[n:].cpu().numpy()):
                assert np.array_equal(a, guard), f'n={n} {hyper}: floats after the n-th element changed'
            p_ref, b_ref = R.sgd_step(p_prev, g, b_prev, lr, mom, wd, gs)
            g64 = np.abs(g.astype(F64) * gs)
            # buf = mom * buf + fma(wd, p, g * gs): four roundings (g * gs, the fma, mom * buf, the sum) over |mom buf| + wd |p| + |g gs|
            rb = worst_ratio(np.abs(bh[:n] - b_ref), 4 * U * (mom * np.abs(b_prev) + wd * np.abs(p_prev) + g64))
            # p -= lr * buf: two more (lr * buf, the difference): six float32 roundings over the magnitude of the terms,
            # |p - ref| <= 6 u (|p0| + lr (|buf0| + wd |p0| + |g gs|))
            rp = worst_ratio(np.abs(ph[:n] - p_ref), 6 * U * (np.abs(p_prev) + lr * (np.abs(b_prev) + wd * np.abs(p_prev) + g64)))
            assert rp <= 1.0 and rb <= 1.0, f'n={n} {hyper}: error / bound p {rp:.3f}, buf {rb:.3f}'
            worst_p, worst_b = max(worst_p, rp), max(worst_b, rb)
            p_prev, b_prev = ph[:n].astype(F64), bh[:n].astype(F64)
    print(f'sgd n={n}: largest error / bound p {worst_p:.3f}, buf {worst_b:.3f}')


# ------------------------------------------------------------------------------------------------ validation counters
@pytest.mark.parametrize('C,ld', [(19, 19), (19, 24), (3, 3), (3, 24)])
def test_seg_metrics_ties_stride_block_loop_and_foreign_labels(C, ld):
    """dsrl_seg_metrics as metrices/__init__.py calls it: rows with tied maxima and all-equal rows (the first maximum counts), pad channels holding
    1e30 behind ld > C (they would win the argmax if read), P that is no multiple of the 256-pixel block and P above 1024 x 256 pixels (the block loop
    with its barrier runs twice in some blocks), labels 255 (ignored) and 200 (>= C, counted nowhere), added to a table that already holds counts."""
    rs = np.random.RandomState(C * 100 + ld)
    for P in (1, 255, 257, 1024 * 256 + 300):
        buf = np.full((P, ld), 1e30, np.float32)
        buf[:, :C] = np.round(2.0 * rs.standard_normal((P, C))).clip(-2, 2) / 2.0
        buf[::7, :C] = 0.25
        tg = rs.randint(0, C, P)
        u = rs.uniform(size=P)
        tg[u < 0.1] = 255
        tg[u > 0.95] = 200
        if P == 1:
            tg[:] = C - 1
        tg = tg.astype(np.uint8)
        pre = np.arange(3 * C + 2, dtype=np.int64) * 1000 + 7
        logits, target, counts = torch.from_numpy(buf).to(DEV), torch.from_numpy(tg).to(DEV), torch.from_numpy(pre.copy()).to(DEV)
        HF.call('dsrl_seg_metrics', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, counts.data_ptr(), HF._stream())
        want = R.seg_counts(buf, tg, C, 255)
        assert want[3 * C + 1] == ((tg != 255) & (tg != 200)).sum()
        assert np.array_equal(counts.cpu().numpy(), pre + want), f'C={C} ld={ld} P={P}'
        if P == 257:        # nothing but ignored and foreign labels: a zero table
            target = torch.from_numpy(np.where(np.arange(P) % 2, 255, 200).astype(np.uint8)).to(DEV)
            counts = torch.zeros(3 * C + 2, dtype=torch.int64, device=DEV)
            HF.call('dsrl_seg_metrics', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, counts.data_ptr(), HF._stream())
            assert not counts.cpu().numpy().any()
            target = torch.full((P,), 255, dtype=torch.uint8, device=DEV)
            HF.call('dsrl_seg_metrics', logits.data_ptr(), ld, target.data_ptr(), P, C, 255, counts.data_ptr(), HF._stream())
            assert not counts.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ image import
@pytest.mark.parametrize('layout', ['nchw', 'channels_last', 'crop'])
def test_pad_image_import_from_any_input_strides(layout):
    """dsrl_pad_image_nhwc from a contiguous NCHW image, the same values stored channels-last and a crop of a larger NCHW tensor: pad 3, a zero
    fourth channel, and a bottom / right margin wider than the pad by different amounts, as _StemConv asks for.  Bit-equal to np.pad."""
    rs = np.random.RandomState(5)
    big = rs.standard_normal((2, 3, 16, 24)).astype(np.float32)
    vals = np.ascontiguousarray(big[:, :, 2:13, 3:20])
    N, Cc, H, W = vals.shape
    pad, Hp, Wp = 3, H + 2 * 3 + 2, W + 2 * 3 + 5
    if layout == 'nchw':
        x = torch.from_numpy(vals).to(DEV)
    elif layout == 'channels_last':
        x = torch.from_numpy(np.ascontiguousarray(vals.transpose(0, 2, 3, 1))).to(DEV).permute(0, 3, 1, 2)
    else:
        x = torch.from_numpy(big).to(DEV)[:, :, 2:13, 3:20]
    assert tuple(x.shape) == (N, Cc, H, W) and (x.is_contiguous() == (layout == 'nchw'))
    y = torch.full((N, Hp, Wp, 4), float('nan'), device=DEV)
    sn, sc, sh, sw = x.stride()
    HF.call('dsrl_pad_image_nhwc', x.data_ptr(), sn, sc, sh, sw, y.data_ptr(), N, Cc, H, W, 4, pad, pad, Hp, Wp, HF._stream())
    want = np.pad(vals.transpose(0, 2, 3, 1), ((0, 0), (pad, Hp - H - pad), (pad, Wp - W - pad), (0, 1)))
    assert np.array_equal(y.cpu().numpy(), want)

"""GPU parity tests: libdsrl_hip.so (through the ctypes C ABI and the autograd wrappers) against the golden vectors
captured from the reference and against the numpy oracle.  Tolerance: 1e-3 relative fp32 as BASELINE.json's north_star
states (most checks are held to 1e-4 or tighter: the convs run the fp32-equivalent 'f16x3' arithmetic in every pass by default,
see functional.set_conv_precision)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gen                     # noqa: E402
import oracle as O             # noqa: E402
from hip_helpers import *      # noqa: E402,F401,F403
from hip_helpers import DEV, HF, D, check, check_elementwise, dev, host, make_head, hip_losses, rel_err   # noqa: E402

TOL = 1e-3
HEAD_GRAD_BOUND, ARENA_GRAD_BOUND = 2e-3, 1e-1         # fixed bounds of test_full_model_total_loss_backward_with_fa_vs_oracle (measured: 3e-4 and 3.5e-2)


@pytest.fixture(autouse=True)
def _default_conv_precision():
    """Every test starts and ends in the library's default conv arithmetic (DSRL_CONV_PRECISION or 'f16x3')."""
    HF.set_conv_precision(None)
    yield
    HF.set_conv_precision(None)


def test_library_loaded_and_device():
    import ctypes
    from dualsuperreslearningforsemseg_amd import _lib
    lib = _lib.load()
    cu = ctypes.c_int(0)
    assert lib.dsrl_device_check(ctypes.byref(cu)) == 0, lib.dsrl_last_error()
    assert cu.value == 256


def test_cpu_tensor_is_refused():
    with pytest.raises(RuntimeError):
        HF.conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(4, 4, 1, 1))


# --------------------------------------------------------------------------------------------- micro ops vs golden
CONVS = ['conv_d6', 'conv_d12', 'conv_d18', 'conv_1x1', 'conv_3x3', 'conv_s2', 'conv_7x7s2', 'conv_1x1s2', 'conv_d2']


@pytest.mark.parametrize('name', CONVS)
def test_conv_golden(golden, name):
    g = golden('ops_micro')
    stride, pad, dil = [int(v) for v in g[f'{name}.cfg']]
    x = dev(g[f'{name}.x']).requires_grad_(True)
    w = dev(g[f'{name}.w']).requires_grad_(True)
    b = dev(g[f'{name}.b']).requires_grad_(True) if f'{name}.b' in g else None
    y = HF.conv2d(x, w, b, stride, pad, dil)
    check(host(y), g[f'{name}.y'], 1e-5, 'y')
    y.backward(dev(g[f'{name}.dy']))
    check(host(x.grad), g[f'{name}.dx'], 1e-5, 'dx')
    check(host(w.grad), g[f'{name}.dw'], 1e-5, 'dw')
    if b is not None:
        check(host(b.grad), g[f'{name}.db'], 1e-5, 'db')


@pytest.mark.parametrize('K', [192, 19, 48, 6])
def test_conv_bias_gradient_column_sums(K):
    """db of a biased conv = column sums of dy: the float4 kernel (K % 4 == 0: the 192-channel SISR conv, the 48-channel shortcut) and the
    one-float-per-lane kernel (19 classes), several row blocks, against fp64."""
    rs = np.random.RandomState(K)
    x = rs.standard_normal((2, 8, 40, 44)).astype(np.float32); w = (rs.standard_normal((K, 8, 1, 1)) * 0.3).astype(np.float32); b = rs.standard_normal(K).astype(np.float32)
    xt = dev(x).requires_grad_(True); wt = dev(w).requires_grad_(True); bt = dev(b).requires_grad_(True)
    y = HF.conv2d(xt, wt, bt, 1, 0, 1)
    dy = rs.standard_normal((2, K, 40, 44)).astype(np.float32)
    y.backward(dev(dy))
    check(host(bt.grad), dy.astype(np.float64).sum((0, 2, 3)), 1e-5, 'db')


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6', 'mixed', 'bf16x3', 'f16x3', 'f16x1'])
@pytest.mark.parametrize('shape', [(2, 304, 32, 64, 192, 3, 1, 1, 1), (2, 512, 16, 32, 256, 3, 1, 6, 6), (2, 256, 33, 47, 100, 3, 2, 1, 1),
                                   (4, 1024, 16, 32, 256, 1, 1, 0, 1)])
def test_conv_precision_modes(mode, shape):
    """The five arithmetic modes of the MFMA conv kernels against the fp64 oracle: exact-product fp32, bf16x6 and f16x3 are
    fp32-equivalent (3e-6 of the output range), bf16x3 carries 16 mantissa bits per operand (3e-5); 'mixed' = bf16x6 forward,
    bf16x3 backward.  Every one of them is far inside the 1e-3 gate.  'f16x1' is the reduced-precision arithmetic of apex O1 / O2 (one fp16
    term per operand = 11 significand bits, one MFMA per product, fp32 accumulation): 5e-4 of the output range on these shapes - what the
    reference's own mixed-precision runs compute, not an fp32-equivalent mode."""
    N, C, H, W, K, R, stride, pad, dil = shape
    rs = np.random.RandomState(sum(shape) + 1)
    x = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, dil)
    dy = rs.standard_normal(yo.shape).astype(np.float32)
    dxo, dwo = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, dil, False)[:2]
    HF.set_conv_precision(mode)
    assert HF.get_conv_precision() == mode
    xt = dev(x).requires_grad_(True); wt = dev(w).requires_grad_(True)
    y = HF.conv2d(xt, wt, None, stride, pad, dil)
    y.backward(dev(dy))
    tol_f = 5e-4 if mode == 'f16x1' else (3e-5 if mode == 'bf16x3' else 3e-6)
    tol_b = 5e-4 if mode == 'f16x1' else (3e-5 if mode in ('bf16x3', 'mixed') else 3e-6)
    e = (check(host(y), yo, tol_f, 'y'), check(host(xt.grad), dxo, tol_b, 'dx'), check(host(wt.grad), dwo, tol_b, 'dw'))
    print(mode, shape, ['%.1e' % v for v in e])


@pytest.mark.parametrize('case', ['tiny_heavy_tail', 'huge', 'outlier', 'zero_dy', 'nan'])
def test_f16x3_operand_ranges(case):
    """The per-tensor power-of-two scales of the f16x3 arithmetic: gradients of a mean-reduced loss (~1e-7 with a log-normal tail), operands
    around 1e+20, one element 1e+6 times the rest, an all-zero gradient, and a NaN (which must reach the outputs it touches, as in fp32
    arithmetic).  Against the fp64 oracle at the fp32-equivalent bound, row by row where the magnitudes of rows differ by orders."""
    N, C, H, W, K, R, stride, pad, dil = 2, 64, 16, 24, 96, 3, 1, 1, 1
    rs = np.random.RandomState(7)
    x = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    dy = rs.standard_normal((N, K, H, W)).astype(np.float32)
    if case == 'tiny_heavy_tail':
        dy = (dy * 1e-7 * np.exp(2.0 * rs.standard_normal(dy.shape))).astype(np.float32)
    elif case == 'huge':
        x = (x * 1e20).astype(np.float32); dy = (dy * 1e-25).astype(np.float32)
    elif case == 'outlier':
        dy = (dy * 1e-7).astype(np.float32); dy[0, 0, 0, 0] = 0.1; x[1, 3, 5, 5] = 3e5
    elif case == 'zero_dy':
        dy[:] = 0
    elif case == 'nan':
        x[1, 2, 3, 4] = np.nan
    HF.set_conv_precision('f16x3')
    xt = dev(x).requires_grad_(True); wt = dev(w).requires_grad_(True)
    y = HF.conv2d(xt, wt, None, stride, pad, dil)
    y.backward(dev(dy))
    if case == 'nan':
        yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, dil)
        assert np.array_equal(np.isnan(host(y)), np.isnan(yo)) and np.isnan(host(wt.grad)).any() and not np.isnan(host(xt.grad)).any()
        return
    yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, dil)
    dxo, dwo = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, dil, False)[:2]
    e = (check(host(y), yo, 3e-6, 'y'), check(host(xt.grad), dxo, 3e-6, 'dx'), check(host(wt.grad), dwo, 3e-6, 'dw'))
    print(case, ['%.1e' % v for v in e])
    if case == 'zero_dy':
        assert not host(xt.grad).any() and not host(wt.grad).any()


@pytest.mark.parametrize('mode', ['f16x3', 'bf16x6', 'fp32'])
def test_nan_at_first_element_stays_local_with_a_channel_tail(mode):
    """Padding taps and the channel tail of the last 32-channel chunk are both served by out-of-range buffer offsets; their sum must stay out of
    range (saturating add) instead of wrapping to offset 0: a NaN in x[0, 0:4, 0, 0] may only reach the outputs pixel (0, 0) touches, like in the
    fp64 oracle - not every border pixel (round 3)."""
    N, C, H, W, K, R, stride, pad, dil = 2, 48, 12, 16, 64, 3, 1, 1, 1
    rs = np.random.RandomState(11)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32); x[0, 0:4, 0, 0] = np.nan
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    HF.set_conv_precision(mode)
    try:
        y = host(HF.conv2d(dev(x), dev(w), None, stride, pad, dil))
    finally:
        HF.set_conv_precision(None)
    yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, dil)
    assert np.array_equal(np.isnan(y), np.isnan(yo)), (int(np.isnan(y).sum()), int(np.isnan(yo).sum()))


@pytest.mark.parametrize('shape', [(2, 64, 16, 24, 96, 3, 1, 1, 1), (2, 304, 16, 32, 192, 3, 1, 1, 1), (1, 256, 32, 64, 19, 1, 1, 0, 1), (4, 1024, 16, 32, 256, 1, 1, 0, 1),
                                   (2, 128, 16, 32, 128, 3, 2, 1, 1), (2, 512, 16, 32, 256, 3, 1, 6, 6)])
def test_f16x3_presplit_filters_match_on_the_fly(shape):
    """Forward and data gradient with the filter operand pre-split once (dsrl_conv2d_split_filters_batched: what ddp.FlatParams does per
    step) are BIT-identical to the same launches splitting the filter in every row tile: same scale, same two terms, same MFMA order.
    Odd K (19: the transposed filter is padded to 20), a channel tail (304 = 9.5 chunks), stride 2 and a dilated conv included."""
    N, C, H, W, K, R, stride, pad, dil = shape
    rs = np.random.RandomState(sum(shape))
    x = dev(np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32))
    w = dev((rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32))
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    dy, lddy = HF.pm_vec4(dev(rs.standard_normal((N, K, Ho, Wo)).astype(np.float32)))
    HF.set_conv_precision('f16x3')
    rec, wsp, wtsp, wtr = HF.split_filter(w)
    xa, dya = HF.amax_for(x), HF.amax_for(dy, dy, lddy)
    shp = (N, H, W, C, K, R, R, stride, pad, dil)
    st = HF._stream()
    outs = []
    for split in (False, True):
        y = torch.empty((N, K, Ho, Wo), device=DEV).contiguous(memory_format=torch.channels_last)
        dx = torch.empty((N, C, H, W), device=DEV).contiguous(memory_format=torch.channels_last)
        ws = HF._ws(HF.cquery('dsrl_conv2d_dgrad_workspace_bytes', *shp) + HF.cquery('dsrl_conv2d_fwd_workspace_bytes', *shp), x)
        HF.call('dsrl_conv2d_fwd_amax', x.data_ptr(), C, xa.data_ptr(), w.data_ptr(), rec.data_ptr(), wsp.data_ptr() if split else None, None, y.data_ptr(), K,
                *shp, ws.data_ptr(), ws.numel(), None, 0, st)
        HF.call('dsrl_conv2d_dgrad_amax', dy.data_ptr(), lddy, dya.data_ptr(), w.data_ptr(), wtr.data_ptr(), rec.data_ptr(), wtsp.data_ptr() if split else None,
                dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(), None, 0, None, 0, None, None, 0, None, 0, 0, st)
        outs.append((host(y), host(dx)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    yo = O.conv2d(host(x).astype(np.float64), host(w).astype(np.float64), None, stride, pad, dil)
    check(outs[1][0], yo, 3e-6, 'y')


# (N, C, H, W, K, R, stride, pad, dil), forced tile configuration (DSRL_FORCE_CFG: TileCfg of conv_igemm.hip; None = the planner's), K groups
_PLANES_CASES = [
    ((8, 256, 16, 32, 256, 3, 1, 1, 1), None, 0),         # layer3 3x3: 64x64 tiles, 4 K groups (the planner's choice at this size)
    ((2, 256, 16, 32, 256, 3, 1, 1, 1), 3, 2),            # 64x64, 2 K groups, ring of 4
    ((2, 1024, 16, 32, 256, 1, 1, 0, 1), 3, 1),           # 64x64, one group, three blocks per CU
    ((2, 304, 16, 64, 192, 3, 1, 1, 1), 0, 0),            # 128x128, channel tail (304 = 9.5 chunks), N tail (192 = 1.5 tiles)
    ((2, 48, 16, 64, 64, 3, 1, 6, 6), 4, 2),              # 128x64 with two K groups, dilation 6 (dead taps), C = 1.5 chunks
    ((2, 128, 16, 32, 256, 1, 2, 0, 1), 5, 1),            # 64x128, stride 2 forward (its dgrad stays on the register-staged kernel)
    ((1, 64, 64, 128, 64, 3, 1, 1, 1), 1, 0),             # 256x64
    ((2, 64, 64, 128, 256, 3, 1, 1, 1), 7, 0),            # 256x128, 8 waves
    ((4, 64, 64, 128, 256, 3, 1, 1, 1), 8, 0),            # 256x256, 8 waves
]


@pytest.mark.parametrize('shape,cfg,kg', _PLANES_CASES)
def test_planes_kernel_bit_identical_to_register_staged(shape, cfg, kg, monkeypatch):
    """conv_planes_kernel (both operands as fp16 planes, staged by LDS-DMA: dsrl_conv2d_fwd_planes / _dgrad_planes) against conv_igemm_split_kernel
    with pre-split filters under the SAME tile / K-group plan: the same terms meet the same MFMAs in the same order, so forward outputs, the
    BatchNorm partials of the forward epilogue, data gradients (plain and accumulating) and the BatchNorm-backward sums of the dgrad epilogue are
    BIT-identical.  The planes themselves are checked against the split the register-staged kernel performs (hi = f16(x 2^e), lo = f16(x 2^e - hi))."""
    N, C, H, W, K, R, stride, pad, dil = shape
    monkeypatch.setenv('DSRL_PLANES', '1')       # this test hands planes over explicitly, whatever DSRL_PLANES_MODE the suite runs under
    if cfg is not None:
        monkeypatch.setenv('DSRL_FORCE_CFG', str(cfg))
    if kg:
        monkeypatch.setenv('DSRL_FORCE_KG', str(kg))
    rs = np.random.RandomState(sum(shape))
    x = dev(np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32))
    w = dev((rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32))
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    dy = dev(rs.standard_normal((N, K, Ho, Wo)).astype(np.float32))
    HF.set_conv_precision('f16x3')
    rec, wsp, wtsp, wtr = HF.split_filter(w)
    wp, wtp = HF.filter_planes(w, rec)
    xa, dya = HF.amax_for(x), HF.amax_for(dy)
    xp, dyp = HF.planes_of(x, C, xa), HF.planes_of(dy, K, dya)
    # the planes are the two terms of the scaled values
    P = N * H * W
    ex = int((int(xa.cpu().numpy().view(np.uint32).max()) >> 23) & 0xff)
    xs = np.ldexp(host(x).transpose(0, 2, 3, 1).reshape(P, C).astype(np.float32), 14 - (ex - 127))
    hi = xs.astype(np.float16); lo = (xs - hi.astype(np.float32)).astype(np.float16)
    lo_off = int(HF.query('dsrl_planes_lo_offset', P * C))
    got = xp.cpu().numpy()
    assert np.array_equal(got[:P * C * 2].view(np.float16).reshape(P, C), hi) and np.array_equal(got[lo_off:lo_off + P * C * 2].view(np.float16).reshape(P, C), lo)
    shp = (N, H, W, C, K, R, R, stride, pad, dil)
    st = HF._stream()
    parts = int(HF.query('dsrl_conv2d_fwd_stats_parts', *shp)) if K % 32 == 0 else 0
    dparts = int(HF.query('dsrl_conv2d_dgrad_stats_parts', *shp)) if (C % 32 == 0 and stride == 1) else 0
    mean = dev(rs.standard_normal(C).astype(np.float32) * 0.1); invstd = dev((1.0 + rs.rand(C)).astype(np.float32))
    bnx = dev(rs.standard_normal((N, C, H, W)).astype(np.float32))
    dx0 = dev(rs.standard_normal((N, C, H, W)).astype(np.float32))
    outs = []
    for planes in (False, True):
        y = torch.empty((N, K, Ho, Wo), device=DEV).contiguous(memory_format=torch.channels_last)
        ws = HF._ws(HF.cquery('dsrl_conv2d_dgrad_workspace_bytes', *shp) + HF.cquery('dsrl_conv2d_fwd_workspace_bytes', *shp), x)
        stats = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 3, max(parts, 1), K)), device=DEV)
        HF.call('dsrl_conv2d_fwd_planes', x.data_ptr(), C, xa.data_ptr(), xp.data_ptr() if planes else None, w.data_ptr(), rec.data_ptr(), wsp.data_ptr(),
                wp.data_ptr() if planes else None, None, y.data_ptr(), K, *shp, ws.data_ptr(), ws.numel(), stats.data_ptr() if parts else None, parts, st)
        res = [host(y), host(stats[:3 * parts * K])]
        for acc in (0, 1):
            if cfg == 8 and not planes:
                res += [None, None]         # no register-staged 256x256 data-gradient build any more (it spilled 76-88 registers; round 5): oracle below
                continue
            dx = dx0.clone()
            bst = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 2, max(dparts, 1), C)), device=DEV)
            HF.call('dsrl_conv2d_dgrad_planes', dy.data_ptr(), K, dya.data_ptr(), dyp.data_ptr() if planes else None, w.data_ptr(), None, rec.data_ptr(), wtsp.data_ptr(),
                    wtp.data_ptr() if planes else None, dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(),
                    bnx.data_ptr() if dparts else None, C, x.data_ptr() if dparts else None, C, mean.data_ptr() if dparts else None,
                    invstd.data_ptr() if dparts else None, 1, bst.data_ptr() if dparts else None, dparts, acc, st)
            res += [host(dx), host(bst[:2 * dparts * C])]
        outs.append(res)
    for a_, b_ in zip(outs[0], outs[1]):
        if a_ is not None:
            assert np.array_equal(a_, b_, equal_nan=True)
    yo = O.conv2d(host(x).astype(np.float64), host(w).astype(np.float64), None, stride, pad, dil)
    check(outs[1][0], yo, 3e-6, 'y')
    if cfg == 8:
        dxo = O.conv2d_bwd(host(x).astype(np.float64), host(w).astype(np.float64), host(dy).astype(np.float64), stride, pad, dil)[0]
        check(outs[1][2], dxo, 3e-6, 'dx (planes kernel, 256x256)'); check(outs[1][4], dxo + host(dx0), 3e-6, 'dx accumulated')


@pytest.mark.parametrize('shape,splits', [((8, 256, 16, 32, 256, 3, 1, 1, 1), 4), ((8, 1024, 16, 32, 256, 1, 1, 0, 1), 4), ((4, 512, 16, 32, 512, 3, 1, 2, 2), 2),
                                          ((3, 200, 9, 20, 136, 3, 1, 1, 1), 3), ((8, 256, 16, 32, 256, 3, 1, 1, 1), 1)])
@pytest.mark.parametrize('mode', ['f16x3', 'f16x1'])
@pytest.mark.parametrize('kg', [2, 1])
def test_cooperative_splitk_matches_slabs_and_oracle(shape, splits, mode, kg, monkeypatch):
    """conv_sk.hip (round 5): 128x128 tiles, two K groups, split-K across workgroups with the reduction INSIDE the launch (arrival tickets in the spare
    words of the activation's amax record, last arriver sums in the order z = 0 .. splits-1) against the same plan with slabs + splitk_reduce_kernel:
    forward and data gradient (plain and accumulating) are BIT-identical; both match the fp64 oracle; the BatchNorm partials of the forward epilogue
    and the BatchNorm-backward sums of the dgrad epilogue - which only the cooperative launch can produce under split-K - reproduce the statistics of
    the tensors the launch wrote; the tickets are left zero (two launches in a row through the same record).  Ragged case: M, N and C off the tile sizes."""
    N, C, H, W, K, R, stride, pad, dil = shape
    # kg = 1 (DSRL_SK_COOP1): the planner's ordinary one-group 128x128 plan with only the reduction moved into the launch
    monkeypatch.setenv('DSRL_FORCE_CFG', '0'); monkeypatch.setenv('DSRL_FORCE_KG', str(kg)); monkeypatch.setenv('DSRL_FORCE_SPLITS', str(splits))
    monkeypatch.setenv('DSRL_SK_COOP1', '1')
    rs = np.random.RandomState(sum(shape) + splits)
    x = dev(np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32))
    w = dev((rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32))
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    dy = dev(rs.standard_normal((N, K, Ho, Wo)).astype(np.float32))
    HF.set_conv_precision(mode)
    try:
        rec, wsp, wtsp, wtr = HF.split_filter(w)
        xa, dya = HF.amax_for(x), HF.amax_for(dy)
        shp = (N, H, W, C, K, R, R, stride, pad, dil)
        st = HF._stream()
        mean = dev(rs.standard_normal(C).astype(np.float32) * 0.1); invstd = dev((1.0 + rs.rand(C)).astype(np.float32))
        bnx = dev(rs.standard_normal((N, C, H, W)).astype(np.float32))
        dx0 = dev(rs.standard_normal((N, C, H, W)).astype(np.float32))
        outs = {}
        for coop in ('1', '0'):
            monkeypatch.setenv('DSRL_SK_COOP', coop)
            HF._query_cache.clear()
            parts = int(HF.query('dsrl_conv2d_fwd_stats_parts', *shp)) if (K % 32 == 0 and coop == '1') else 0
            dparts = int(HF.query('dsrl_conv2d_dgrad_stats_parts', *shp)) if (C % 32 == 0 and coop == '1') else 0
            ws = torch.empty(int(HF.query('dsrl_conv2d_dgrad_workspace_bytes', *shp)) + int(HF.query('dsrl_conv2d_fwd_workspace_bytes', *shp)) + 4096, device=DEV, dtype=torch.uint8)
            res = []
            for rep in range(2):                        # twice: the second launch finds the tickets the first one left
                y = torch.full((N, K, Ho, Wo), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
                stats = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 3, max(parts, 1), K)), device=DEV)
                HF.call('dsrl_conv2d_fwd_planes', x.data_ptr(), C, xa.data_ptr(), None, w.data_ptr(), rec.data_ptr(), wsp.data_ptr(), None, None, y.data_ptr(), K, *shp,
                        ws.data_ptr(), ws.numel(), stats.data_ptr() if parts else None, parts, st)
            res += [host(y)]
            if parts:
                pt = host(stats[:3 * parts * K]).reshape(3, parts, K).astype(np.float64)
                n = pt[0].sum(0); mu = (pt[0] * pt[1]).sum(0) / n
                m2 = (pt[2] + pt[0] * (pt[1] - mu) ** 2).sum(0)
                yy = host(y).astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, K)
                assert np.all(n == yy.shape[0])
                check(mu, yy.mean(0), 1e-5, 'mean from the partials'); check(m2 / n, yy.var(0), 1e-4, 'variance from the partials')
            for acc in (0, 1):
                dx = dx0.clone()
                bst = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 2, max(dparts, 1), C)), device=DEV)
                HF.call('dsrl_conv2d_dgrad_planes', dy.data_ptr(), K, dya.data_ptr(), None, w.data_ptr(), None, rec.data_ptr(), wtsp.data_ptr(), None, dx.data_ptr(), C, *shp,
                        ws.data_ptr(), ws.numel(), bnx.data_ptr() if dparts else None, C, x.data_ptr() if dparts else None, C, mean.data_ptr() if dparts else None,
                        invstd.data_ptr() if dparts else None, 1, bst.data_ptr() if dparts else None, dparts, acc, st)
                res += [host(dx)]
                if dparts:
                    b2 = host(bst[:2 * dparts * C]).reshape(2, dparts, C).astype(np.float64).sum(1)
                    g = host(dx).astype(np.float64) * (host(x) > 0)
                    xh = (host(bnx).astype(np.float64) - host(mean)[None, :, None, None]) * host(invstd)[None, :, None, None]
                    check(b2[0], g.sum((0, 2, 3)), 2e-5, 'sum g'); check(b2[1], (g * xh).sum((0, 2, 3)), 2e-5, 'sum g xhat')
            outs[coop] = res
            assert int(xa.cpu().numpy().view(np.uint32).reshape(16, 16)[:, 1:].max()) == 0 and int(dya.cpu().numpy().view(np.uint32).reshape(16, 16)[:, 1:].max()) == 0, 'tickets left behind'
        for a_, b_ in zip(outs['1'], outs['0']):
            assert np.array_equal(a_, b_, equal_nan=True)
        tol = 1e-3 if mode == 'f16x1' else 3e-6          # f16x1: one 11-bit term per operand (2^-11 = 4.9e-4 per product term)
        check(outs['1'][0], O.conv2d(host(x).astype(np.float64), host(w).astype(np.float64), None, stride, pad, dil), tol, 'y')
        dxo = O.conv2d_bwd(host(x).astype(np.float64), host(w).astype(np.float64), host(dy).astype(np.float64), stride, pad, dil, has_bias=False)[0]
        check(outs['1'][1], dxo, tol, 'dx'); check(outs['1'][2], dxo + host(dx0), tol, 'dx accumulated')
    finally:
        HF.set_conv_precision(None)
        HF._query_cache.clear()


@pytest.mark.parametrize('shape,cfg,kg', [((8, 256, 16, 32, 256, 3, 1, 1, 1), None, 0), ((2, 304, 16, 64, 192, 3, 1, 1, 1), 0, 0), ((4, 64, 64, 128, 256, 3, 1, 1, 1), 8, 0)])
def test_one_plane_operands_bit_identical_to_f16x1_register_staged(shape, cfg, kg, monkeypatch):
    """Round 5: in 'f16x1' mode conv_planes_kernel takes ONE fp16 plane per operand (hi = f16(x 2^e): the operand of a 2-byte storage format) - the values
    the register-staged f16x1 kernel rounds to while staging - so forward and data gradient are BIT-identical to it for the same plan; deeper LDS rings
    (4 slots for the 64x64 / four-group and the 128x128 tiles, 3 for 256x256).  Against fp64: the 11-bit tolerance of the arithmetic."""
    N, C, H, W, K, R, stride, pad, dil = shape
    monkeypatch.setenv('DSRL_PLANES', '1')
    if cfg is not None:
        monkeypatch.setenv('DSRL_FORCE_CFG', str(cfg))
    rs = np.random.RandomState(sum(shape) + 1)
    x = dev(np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32))
    w = dev((rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32))
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    dy = dev(rs.standard_normal((N, K, Ho, Wo)).astype(np.float32))
    HF.set_conv_precision('f16x1')
    try:
        HF._query_cache.clear()
        rec, wsp, wtsp, wtr = HF.split_filter(w)
        wp, wtp = HF.filter_planes(w, rec)
        xa, dya = HF.amax_for(x), HF.amax_for(dy)
        xp, dyp = HF.planes_of(x, C, xa, 1), HF.planes_of(dy, K, dya, 1)
        shp = (N, H, W, C, K, R, R, stride, pad, dil)
        st = HF._stream()
        ws = torch.empty(int(HF.query('dsrl_conv2d_dgrad_workspace_bytes', *shp)) + int(HF.query('dsrl_conv2d_fwd_workspace_bytes', *shp)) + 4096, device=DEV, dtype=torch.uint8)
        outs = []
        for planes in (False, True):
            y = torch.empty((N, K, Ho, Wo), device=DEV).contiguous(memory_format=torch.channels_last)
            HF.call('dsrl_conv2d_fwd_planes', x.data_ptr(), C, xa.data_ptr(), xp.data_ptr() if planes else None, w.data_ptr(), rec.data_ptr(), wsp.data_ptr(),
                    wp.data_ptr() if planes else None, None, y.data_ptr(), K, *shp, ws.data_ptr(), ws.numel(), None, 0, st)
            res = [host(y)]
            if not (cfg == 8 and not planes):
                dx = torch.empty((N, C, H, W), device=DEV).contiguous(memory_format=torch.channels_last)
                HF.call('dsrl_conv2d_dgrad_planes', dy.data_ptr(), K, dya.data_ptr(), dyp.data_ptr() if planes else None, w.data_ptr(), None, rec.data_ptr(), wtsp.data_ptr(),
                        wtp.data_ptr() if planes else None, dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(), None, 0, None, 0, None, None, 0, None, 0, 0, st)
                res.append(host(dx))
            outs.append(res)
        for a_, b_ in zip(outs[0], outs[1]):
            assert np.array_equal(a_, b_, equal_nan=True)
        check(outs[1][0], O.conv2d(host(x).astype(np.float64), host(w).astype(np.float64), None, stride, pad, dil), 1e-3, 'y')
        check(outs[1][-1], O.conv2d_bwd(host(x).astype(np.float64), host(w).astype(np.float64), host(dy).astype(np.float64), stride, pad, dil)[0], 1e-3, 'dx')
    finally:
        HF.set_conv_precision(None)
        HF._query_cache.clear()


def test_pointwise_strided_golden(golden):
    g = golden('ops_micro')
    x = dev(g['conv_s8.x']).requires_grad_(True); w = dev(g['conv_s8.w']).requires_grad_(True)
    y = HF.pointwise_strided(x, w, 8)
    check(host(y), g['conv_s8.y'], 1e-5)
    y.backward(dev(g['conv_s8.dy']))
    check(host(x.grad), g['conv_s8.dx'], 1e-5); check(host(w.grad), g['conv_s8.dw'], 1e-5)


@pytest.mark.parametrize('shape', [(2, 128, 8, 64, 128, 3, 2, 1, 1), (2, 256, 8, 128, 512, 1, 2, 0, 1), (4, 64, 16, 64, 64, 3, 2, 1, 1),
                                   (8, 128, 64, 128, 128, 3, 2, 1, 1)])        # the last one: layer2.0.conv2 at full size (128x128 tiles, no K groups)
@pytest.mark.parametrize('accumulate', [False, True])
def test_strided_dgrad_parity_order(shape, accumulate, monkeypatch):
    """Data gradient of the stride-2 convs (layer2.0 / layer3.0 conv2 and downsample shapes at small N, H): with the GEMM rows ordered by
    parity class (ConvArgs::par) a tile runs only the taps that divide evenly for its class. The multiply-adds it drops act on zeros, so the
    gradient is BIT-identical to the row-major launch (DSRL_DGRAD_PARITY=0); the BatchNorm-backward partials of the epilogue
    (dsrl_conv2d_dgrad_bnstats) are sums over other row blocks: equal in total up to summation order. Also against the fp64 oracle."""
    N, C, H, W, K, R, stride, pad, dil = shape
    rs = np.random.RandomState(sum(shape))
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    dy = rs.standard_normal((N, K, Ho, Wo)).astype(np.float32)
    bx = rs.standard_normal((N, C, H, W)).astype(np.float32); by = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    mean = rs.standard_normal(C).astype(np.float32); invstd = rs.uniform(0.5, 2.0, C).astype(np.float32)
    old = rs.standard_normal((N, C, H, W)).astype(np.float32)
    wt, dyt = dev(w), dev(dy)
    bxt, byt, mt, it = dev(bx), dev(by), dev(mean), dev(invstd)
    shp = (N, H, W, C, K, R, R, stride, pad, dil)
    res = {}
    for par in ('1', '0'):
        monkeypatch.setenv('DSRL_DGRAD_PARITY', par)
        parts = int(HF.query('dsrl_conv2d_dgrad_stats_parts', *shp))      # 0: more than 256 row blocks (the full-size layer): plain data gradient
        dx = dev(old).clone(memory_format=torch.channels_last) if accumulate else torch.empty((N, C, H, W), device=DEV).contiguous(memory_format=torch.channels_last)
        bst = torch.zeros(2 * max(parts, 1) * C, device=DEV)
        ws = torch.empty(int(HF.cquery('dsrl_conv2d_dgrad_workspace_bytes', *shp)) + 256, dtype=torch.uint8, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        if parts > 0:
            HF.call('dsrl_conv2d_dgrad_bnstats', dyt.data_ptr(), K, wt.data_ptr(), None, dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(),
                    bxt.data_ptr(), C, byt.data_ptr(), C, mt.data_ptr(), it.data_ptr(), 1, bst.data_ptr(), parts, int(accumulate), st)
        else:
            HF.call('dsrl_conv2d_dgrad_accumulate' if accumulate else 'dsrl_conv2d_dgrad', dyt.data_ptr(), K, wt.data_ptr(), None, dx.data_ptr(), C, *shp,
                    ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        res[par] = (host(dx), bst.view(2, max(parts, 1), C).double().sum(1).cpu().numpy(), parts)
    assert np.array_equal(res['1'][0], res['0'][0])
    dxo = O.conv2d_bwd(np.zeros((N, C, H, W)), w.astype(np.float64), dy.astype(np.float64), stride, pad, dil)[0] + (old if accumulate else 0)
    check(res['1'][0], dxo, 1e-5, 'dx')
    g = dxo * (by > 0)
    xh = (bx.astype(np.float64) - mean[None, :, None, None]) * invstd[None, :, None, None]
    for par in ('1', '0'):
        if res[par][2] > 0:
            check(res[par][1][0], g.sum((0, 2, 3)), 1e-4, 'sum g'); check(res[par][1][1], (g * xh).sum((0, 2, 3)), 1e-4, 'sum g xhat')


@pytest.mark.parametrize('shape', [(2, 2048, 16, 32, 256, 3, 1, 12, 12), (2, 304, 64, 128, 256, 3, 1, 1, 1), (1, 256, 64, 128, 19, 1, 1, 0, 1),
                                   (2, 304, 32, 64, 192, 3, 1, 1, 1), (2, 256, 32, 64, 48, 1, 1, 0, 1), (3, 64, 33, 47, 64, 3, 2, 1, 1),
                                   (8, 2048, 1, 1, 256, 1, 1, 0, 1), (2, 128, 8, 64, 128, 3, 2, 1, 1), (2, 256, 8, 128, 512, 1, 2, 0, 1)])
def test_conv_vs_oracle_real_shapes(shape):
    """The shapes the DSRL head really launches (ASPP dilated, cat_conv, cls_conv, SISR, shortcut, a strided backbone conv,
    the pooled ASPP branch) against the fp64 oracle, forward and both gradients."""
    N, C, H, W, K, R, stride, pad, dil = shape
    rs = np.random.RandomState(sum(shape))
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    b = rs.standard_normal(K).astype(np.float32)
    yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), stride, pad, dil)
    dy = rs.standard_normal(yo.shape).astype(np.float32)
    dxo, dwo, dbo = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, dil, True)
    xt = dev(x).requires_grad_(True); wt = dev(w).requires_grad_(True); bt = dev(b).requires_grad_(True)
    y = HF.conv2d(xt, wt, bt, stride, pad, dil)
    check(host(y), yo, 2e-5, 'y')
    y.backward(dev(dy))
    check(host(xt.grad), dxo, 2e-5, 'dx'); check(host(wt.grad), dwo, 2e-5, 'dw'); check(host(bt.grad), dbo, 2e-5, 'db')


@pytest.mark.parametrize('mode', ['bf16x6', 'mixed', 'f16x3'])
def test_wgrad_group_vs_oracle_and_per_layer(mode):
    """dsrl_conv2d_wgrad_group_* (all weight gradients of a pass as a few grouped grids) against the fp64 oracle and against the
    per-layer dsrl_conv2d_wgrad: three tile configurations, dilated taps that never leave the padding (memset path), a strided conv,
    19 output channels with a padded gradient stride, a channel count that is no multiple of 32, and a layer long enough for several
    pixel ranges (slabs + the grouped reduce)."""
    HF.set_conv_precision(mode)
    shapes = [(2, 512, 16, 32, 256, 3, 1, 18, 18), (2, 304, 64, 128, 192, 3, 1, 1, 1), (3, 64, 33, 47, 64, 3, 2, 1, 1), (1, 256, 64, 128, 19, 1, 1, 0, 1),
              (4, 1024, 16, 32, 256, 1, 1, 0, 1), (2, 256, 32, 64, 48, 1, 1, 0, 1), (8, 64, 64, 128, 64, 1, 1, 0, 1), (2, 32, 40, 24, 128, 3, 1, 2, 2),
              (2, 20, 16, 16, 36, 3, 1, 1, 1)]
    q = HF.WgradQueue()
    refs = []
    for i, (N, C, H, W, K, R, stride, pad, dil) in enumerate(shapes):
        rs = np.random.RandomState(1000 + i)
        x = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
        w = np.zeros((K, C, R, R), np.float32)
        Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
        dy = rs.standard_normal((N, K, Ho, Wo)).astype(np.float32)
        dwo = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, dil, False)[1]
        xt, ldx = HF.pm_vec4(dev(x)); dyt, lddy = HF.pm_vec4(dev(dy))
        shp = (N, H, W, C, K, R, R, stride, pad, dil)
        dw_g = torch.full((K, C, R, R), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
        dw_l = torch.empty_like(dw_g)
        ws = HF._ws(HF.cquery('dsrl_conv2d_wgrad_workspace_bytes', *shp), xt)
        HF.call('dsrl_conv2d_wgrad', xt.data_ptr(), ldx, dyt.data_ptr(), lddy, dw_l.data_ptr(), *shp, ws.data_ptr(), ws.numel(), HF._stream())
        f16 = mode == 'f16x3'       # that arithmetic takes the operand magnitudes of every problem (the per-layer call above measured its own)
        q.add(xt, ldx, dyt, lddy, dw_g, shp, None, HF.amax_for(xt, xt, ldx) if f16 else None, HF.amax_for(dyt, dyt, lddy) if f16 else None)
        refs.append((dwo, dw_g, dw_l, shp))
    q.flush()
    tol = 3e-5 if mode == 'mixed' else 3e-6
    for dwo, dw_g, dw_l, shp in refs:
        e1 = check(host(dw_g), dwo, tol, f'grouped dw {shp}')
        e2 = check(host(dw_g), host(dw_l), tol, f'grouped vs per-layer {shp}')
        print(shp, '%.1e %.1e' % (e1, e2))


_W3_CASES = [
    (2, 64, 8, 32, 128, 1),          # one full tile pair per 64 channels
    (1, 304, 5, 64, 192, 1),         # decoder widths: ragged tile of in channels (304 = 4.75 x 64) and of out channels (192 = 1.5 x 128 rows of 64)
    (2, 128, 6, 32, 100, 2),         # dilation 2 (layer4), out channels no multiple of 32
    (3, 36, 2, 96, 96, 1),           # two image rows: every chunk sees a padding row; 36 in channels
]


@pytest.mark.parametrize('mode', ['f16x3', 'f16x1'])
@pytest.mark.parametrize('case', _W3_CASES)
def test_wgrad_all_taps_kernel_matches_per_tap_kernel(case, mode, monkeypatch):
    """conv_wgrad3_kernel (3x3 / stride 1: all nine taps of a 64 x 64 tile in one block, x rows staged once per chunk and read at nine offsets)
    against conv_wgrad_split_kernel (one tap per block) and the fp64 oracle.  With the same pixel ranges both kernels add the same products in
    the same order: equal values (a tap's all-padding chunks, which the per-tap kernel skips, add zeros).  Per-layer launches with 1 and 3 pixel
    ranges (slabs + reduce) and the grouped launch."""
    N, C, H, W, K, dil = case
    HF.set_conv_precision(mode)
    rs = np.random.RandomState(sum(case))
    x = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    dy = rs.standard_normal((N, K, H, W)).astype(np.float32)
    dwo = O.conv2d_bwd(x.astype(np.float64), np.zeros((K, C, 3, 3)), dy.astype(np.float64), 1, dil, dil, False)[1]
    xt, ldx = HF.pm_vec4(dev(x)); dyt, lddy = HF.pm_vec4(dev(dy))
    xa, dya = HF.amax_for(xt, xt, ldx), HF.amax_for(dyt, dyt, lddy)
    shp = (N, H, W, C, K, 3, 3, 1, dil, dil)
    tol = 3e-6 if mode == 'f16x3' else 2e-3
    got = {}
    for w3 in ('0', '1'):
        monkeypatch.setenv('DSRL_WGRAD3', w3)
        for sp in (1, 3):
            monkeypatch.setenv('DSRL_FORCE_PSPLITS', str(sp))
            dw = torch.full((K, C, 3, 3), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
            ws = HF._ws(int(HF.query('dsrl_conv2d_wgrad_workspace_bytes', *shp)), xt)
            HF.call('dsrl_conv2d_wgrad_amax', xt.data_ptr(), ldx, xa.data_ptr(), dyt.data_ptr(), lddy, dya.data_ptr(), dw.data_ptr(), *shp, ws.data_ptr(), ws.numel(), HF._stream())
            got[(w3, sp)] = host(dw)
            check(got[(w3, sp)], dwo, tol, f'dw all-taps={w3} ranges={sp}')
        monkeypatch.delenv('DSRL_FORCE_PSPLITS')
        q = HF.WgradQueue()
        dwg = torch.full((K, C, 3, 3), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
        q.add(xt, ldx, dyt, lddy, dwg, shp, None, xa, dya)
        q.flush()
        check(host(dwg), dwo, tol, f'grouped dw all-taps={w3}')
    for sp in (1, 3):
        assert np.array_equal(got[('0', sp)], got[('1', sp)]), (sp, float(np.abs(got[('0', sp)] - got[('1', sp)]).max()))


def test_conv_into_and_from_channel_slices():
    """ld > C: reading a channel slice of a wider buffer (the concat layout) gives the same result."""
    rs = np.random.RandomState(5)
    buf = dev(rs.standard_normal((2, 96, 8, 16)).astype(np.float32))
    w = dev((rs.standard_normal((32, 32, 3, 3)) * 0.1).astype(np.float32))
    a = HF.conv2d(buf[:, 32:64], w, None, 1, 1, 1)
    b = HF.conv2d(buf[:, 32:64].contiguous(memory_format=torch.channels_last), w, None, 1, 1, 1)
    assert torch.equal(a, b)


def test_convT_golden(golden):
    g = golden('ops_micro')
    x = dev(g['convT.x']).requires_grad_(True); w = dev(g['convT.w'], cl=False).requires_grad_(True); b = dev(g['convT.b']).requires_grad_(True)
    y = HF.conv_transpose2d_k2s2(x, w, b)
    check(host(y), g['convT.y'], 1e-5)
    y.backward(dev(g['convT.dy']))
    check(host(x.grad), g['convT.dx'], 1e-5); check(host(w.grad), g['convT.dw'], 1e-5); check(host(b.grad), g['convT.db'], 1e-5)


@pytest.mark.parametrize('mfma', ['1', '0'])
@pytest.mark.parametrize('shape', [(2, 19, 5, 150), (2, 19, 7, 200), (1, 19, 3, 64), (3, 19, 4, 12), (2, 8, 6, 72), (2, 19, 9, 328)])
def test_convT_vs_oracle_ragged(shape, mfma, monkeypatch):
    # mfma = 1: the fp32-MFMA segment kernels (default for W % 4 == 0; segments of 128 pixels), 0: the VALU kernels (both-rows forward with its
    # 16-byte path, fused backward over 64-pixel segments).  W = 150: the two-kernel backward (segments not 16-byte aligned); W % 4 == 0 with a
    # ragged last segment (200, 72, 12, 328 = 2 * 128 + 72) and with exactly one (64); 8 -> 8 channels: the second instantiation.
    # (2, 19, 9, 328) runs with at most 5 blocks for 54 (MFMA) / 108 (VALU) segments: every block walks several segments, the last one ragged,
    # so the cross-segment reuse of the prefetch registers and LDS buffers is checked against the fp64 oracle.
    rs = np.random.RandomState(9)
    C = shape[1]
    monkeypatch.setenv('DSRL_CONVT_MFMA', mfma)
    if shape[3] == 328:
        monkeypatch.setenv('DSRL_CONVT_MAX_BLOCKS', '5')
    x = rs.standard_normal(shape).astype(np.float32); w = rs.standard_normal((C, C, 2, 2)).astype(np.float32); b = rs.standard_normal(C).astype(np.float32)
    yo = O.conv_transpose2d_k2s2(x.astype(np.float64), w.astype(np.float64)) + b.astype(np.float64)[None, :, None, None]
    dy = rs.standard_normal(yo.shape).astype(np.float32)
    dxo, dwo, dbo = O.conv_transpose2d_k2s2_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), has_bias=True)
    grads = {}
    for fused in ('1', '0'):
        monkeypatch.setenv('DSRL_CONVT_FUSED_BWD', fused)
        xt = dev(x).requires_grad_(True); wt = dev(w, cl=False).requires_grad_(True); bt = dev(b).requires_grad_(True)
        y = HF.conv_transpose2d_k2s2(xt, wt, bt)
        check(host(y), yo, 1e-5)
        y.backward(dev(dy))
        check(host(xt.grad), dxo, 1e-5); check(host(wt.grad), dwo, 1e-5); check(host(bt.grad), dbo, 1e-5)
        grads[fused] = (host(xt.grad), host(wt.grad), host(bt.grad))
    for a, c in zip(grads['1'], grads['0']):
        check(a, c, 1e-5)


@pytest.mark.parametrize('shape,cap', [((1, 19, 3, 128), 0), ((2, 19, 5, 256), 3), ((2, 19, 9, 384), 2), ((3, 19, 4, 128), 5)])
def test_convT_backward_lds_dma_vs_oracle_and_register_staged(shape, cap, monkeypatch):
    # convt_dma.hip (W % 128 == 0, 19 -> 19): segments staged by LDS-DMA into a three-slot ring, one block per CU.  Against the fp64 oracle, and
    # bit-identical to convt2x2_bwd_mfma_kernel when both walk the segments with the same number of blocks (same MFMA order within a segment, same
    # segments per block, same merge).  cap = blocks allowed: 3 blocks for 20 segments / 2 for 54 wrap the ring many times, 5 for 12 leaves blocks
    # with 3 and with 2 segments (the tail of the counted waits), cap 0 = one segment per block.
    rs = np.random.RandomState(sum(shape))
    C = shape[1]
    monkeypatch.setenv('DSRL_CONVT_MFMA', '1')
    if cap:
        monkeypatch.setenv('DSRL_CONVT_MAX_BLOCKS', str(cap))
    x = rs.standard_normal(shape).astype(np.float32); w = rs.standard_normal((C, C, 2, 2)).astype(np.float32); b = rs.standard_normal(C).astype(np.float32)
    dy = rs.standard_normal((shape[0], C, 2 * shape[2], 2 * shape[3])).astype(np.float32)
    dxo, dwo, dbo = O.conv_transpose2d_k2s2_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), has_bias=True)
    grads = {}
    for dma in ('1', '0'):
        monkeypatch.setenv('DSRL_CONVT_DMA', dma)
        xt = dev(x).requires_grad_(True); wt = dev(w, cl=False).requires_grad_(True); bt = dev(b).requires_grad_(True)
        HF.conv_transpose2d_k2s2(xt, wt, bt).backward(dev(dy))
        check(host(xt.grad), dxo, 1e-5); check(host(wt.grad), dwo, 1e-5); check(host(bt.grad), dbo, 1e-5)
        grads[dma] = (xt.grad, wt.grad, bt.grad)
    for a, c in zip(grads['1'], grads['0']):
        assert torch.equal(a, c)


CONVT_CE_SHAPES = [((1, 4, 128), 0, 8), ((2, 6, 256), 3, 8), ((2, 9, 384), 2, 0), ((3, 4, 128), 5, 4)]


@pytest.mark.parametrize('shape,cap,ft', CONVT_CE_SHAPES)
def test_convT_backward_with_cross_entropy_inside_bit_identical_to_three_calls(shape, cap, ft, monkeypatch):
    # dsrl_convt2x2_bwd_ce: the ConvTranspose backward that forms d(CE)/d(logits) (+ the stride-s feature transformer's g * w_c) inside the kernel, against
    # the three calls it replaces - dsrl_ce_fused (writes the gradient), dsrl_pointwise_strided_bwd(accumulate = 1), dsrl_convt2x2_bwd - bit for bit:
    # dx, dw, db.  Ignored pixels (10 % + one whole row), block caps that make blocks walk many segments; and the CE gradient
    # itself against the fp64 oracle through dx.  The default build: the transform in four waves of its own.
    _convT_backward_with_cross_entropy_vs_three_calls(shape, cap, ft, None, monkeypatch)


@pytest.mark.parametrize('shape,cap,ft', CONVT_CE_SHAPES)
def test_convT_backward_with_cross_entropy_inside_8_wave_build_bit_identical_to_three_calls(shape, cap, ft, monkeypatch):
    # the same checks for the build selected by DSRL_CONVT_CE_WAVES=8: the transform inside the eight MFMA waves
    _convT_backward_with_cross_entropy_vs_three_calls(shape, cap, ft, '8', monkeypatch)


def _convT_backward_with_cross_entropy_vs_three_calls(shape, cap, ft, waves, monkeypatch):
    from dualsuperreslearningforsemseg_amd._lib import call, query
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')               # the path under test, whatever the suite's environment says
    if waves is None:
        monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
    else:
        monkeypatch.setenv('DSRL_CONVT_CE_WAVES', waves)
    N, H, W = shape
    C = 19
    rs = np.random.RandomState(N * 1000 + H * 10 + W)
    if cap:
        monkeypatch.setenv('DSRL_CONVT_MAX_BLOCKS', str(cap))
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    w = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor((rs.standard_normal((N, 2 * H, 2 * W, C)) * 3).astype(np.float32), device=DEV)
    tg = rs.randint(0, C, (N, 2 * H, 2 * W)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255; tg[0, 1, :] = 255
    target = torch.tensor(tg, device=DEV)
    P = N * 4 * H * W
    st = HF._stream()
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(query('dsrl_ce_fused_workspace_bytes', P), dtype=torch.uint8, device=DEV)
    wsb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=DEV)
    assert query('dsrl_convt2x2_bwd_ce_supported', x.data_ptr(), logits.data_ptr(), target.data_ptr(), N, H, W, C, C) == 1
    # the three calls
    scal = torch.zeros(8, device=DEV); dl = torch.empty_like(logits)
    call('dsrl_ce_fused', logits.data_ptr(), C, target.data_ptr(), P, C, 255, dl.data_ptr(), C, scal.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), st)
    dl_ce = dl.clone()
    if ft:
        dwf = torch.empty(C, device=DEV)
        wsf = torch.empty(query('dsrl_pointwise_strided_bwd_workspace_bytes', N, 2 * H, 2 * W, C, ft), dtype=torch.uint8, device=DEV)
        call('dsrl_pointwise_strided_bwd', logits.data_ptr(), ftw.data_ptr(), ftg.data_ptr(), dl.data_ptr(), dwf.data_ptr(), 1, N, 2 * H, 2 * W, C, ft,
             wsf.data_ptr(), wsf.numel(), st)
        dwf2 = torch.empty(C, device=DEV)
        call('dsrl_pointwise_strided_bwd', logits.data_ptr(), ftw.data_ptr(), ftg.data_ptr(), None, dwf2.data_ptr(), 2, N, 2 * H, 2 * W, C, ft,
             wsf.data_ptr(), wsf.numel(), st)
        assert torch.equal(dwf, dwf2)                       # accumulate = 2: the weight gradient alone
    dx = torch.empty_like(x); dw = torch.empty_like(w); db = torch.empty(C, device=DEV)
    call('dsrl_convt2x2_bwd', x.data_ptr(), w.data_ptr(), dl.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    # the one call: the loss pass writes no gradient
    scal2 = torch.zeros(8, device=DEV)
    call('dsrl_ce_fused', logits.data_ptr(), C, target.data_ptr(), P, C, 255, None, C, scal2.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert torch.equal(scal[:2], scal2[:2])
    dx2 = torch.full_like(x, 7.0); dw2 = torch.full_like(w, 7.0); db2 = torch.full((C,), 7.0, device=DEV)
    call('dsrl_convt2x2_bwd_ce', x.data_ptr(), w.data_ptr(), logits.data_ptr(), target.data_ptr(), 255, scal2.data_ptr() + 4,
         None if not ft else ftg.data_ptr(), None if not ft else ftw.data_ptr(), ft, dx2.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
         N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    # and against the oracle: d(CE)/d(logits) in fp64, pushed through the fp64 ConvTranspose backward
    lg64 = host(logits).astype(np.float64)
    z = lg64 - lg64.max(-1, keepdims=True); p = np.exp(z); p /= p.sum(-1, keepdims=True)
    live = tg != 255
    g64 = p.copy(); idx = np.where(live)
    g64[idx[0], idx[1], idx[2], tg[live]] -= 1.0
    g64 *= live[..., None] / live.sum()
    check(host(dl_ce), g64, 1e-5)
    if ft:
        g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
    dxo, dwo, dbo = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(w).astype(np.float64), g64.transpose(0, 3, 1, 2), has_bias=True)
    check(host(dx2).transpose(0, 3, 1, 2), dxo, 1e-5); check(host(dw2), dwo, 1e-5); check(host(db2), dbo, 1e-5)


@pytest.mark.parametrize('shape,cap', [((1, 3, 128), 0), ((2, 5, 200), 3), ((2, 9, 328), 5), ((3, 4, 12), 0)])
def test_convT_forward_with_cross_entropy_value_inside(shape, cap, monkeypatch):
    # dsrl_convt2x2_fwd_ce: the forward whose kernel also evaluates nn.CrossEntropyLoss of its output from the tile in LDS.  y bit-identical to
    # dsrl_convt2x2_fwd; loss and pixel count against dsrl_ce_fused on that y (1e-6: another summation order of the pixel losses) and the fp64 oracle;
    # ragged last segments (200, 328 = 2 * 128 + 72, 12), blocks walking several segments (cap); NaN input -> flag bit 0, label 200 -> NaN loss + bit 1.
    from dualsuperreslearningforsemseg_amd._lib import call, query
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    N, H, W = shape
    C = 19
    rs = np.random.RandomState(N * 1000 + H * 10 + W)
    if cap:
        monkeypatch.setenv('DSRL_CONVT_MAX_BLOCKS', str(cap))
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    w = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV); b = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV)
    tg = rs.randint(0, C, (N, 2 * H, 2 * W)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255; tg[0, 1, :] = 255
    target = torch.tensor(tg, device=DEV)
    st = HF._stream()
    P = N * 4 * H * W
    assert query('dsrl_convt2x2_fwd_ce_supported', x.data_ptr(), x.data_ptr(), N, H, W, C, C) == 1
    ws = torch.empty(query('dsrl_convt2x2_fwd_ce_workspace_bytes', N, H, W), dtype=torch.uint8, device=DEV)
    wsc = torch.empty(query('dsrl_ce_fused_workspace_bytes', P), dtype=torch.uint8, device=DEV)

    def run(xin, tgt):
        y0 = torch.empty((N, 2 * H, 2 * W, C), device=DEV); y1 = torch.full_like(y0, 7.0)
        f0 = torch.zeros(1, dtype=torch.int32, device=DEV); f1 = torch.zeros(1, dtype=torch.int32, device=DEV)
        s0 = torch.zeros(8, device=DEV); s1 = torch.zeros(8, device=DEV)
        call('dsrl_convt2x2_fwd', xin.data_ptr(), w.data_ptr(), b.data_ptr(), y0.data_ptr(), N, H, W, C, C, st)
        call('dsrl_ce_fused', y0.data_ptr(), C, tgt.data_ptr(), P, C, 255, None, C, s0.data_ptr(), f0.data_ptr(), wsc.data_ptr(), wsc.numel(), st)
        call('dsrl_convt2x2_fwd_ce', xin.data_ptr(), w.data_ptr(), b.data_ptr(), y1.data_ptr(), N, H, W, C, C, tgt.data_ptr(), 255, s1.data_ptr(), f1.data_ptr(),
             ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        return y0, y1, host(s0), host(s1), int(f0), int(f1)
    y0, y1, s0, s1, f0, f1 = run(x, target)
    assert torch.equal(y0, y1) and f0 == 0 and f1 == 0
    assert s0[1] == s1[1] == float((tg != 255).sum())
    assert abs(s0[0] - s1[0]) <= 1e-6 * abs(s0[0])
    lg64 = host(y1).astype(np.float64)
    lse = np.log(np.exp(lg64 - lg64.max(-1, keepdims=True)).sum(-1)) + lg64.max(-1)
    live = tg != 255
    ref = float((lse[live] - np.take_along_axis(lg64, np.where(live, tg, 0)[..., None].astype(np.int64), -1)[..., 0][live]).mean())
    assert abs(s1[0] - ref) <= 1e-5 * abs(ref)
    xb = x.clone(); xb[0, 0, 0, 0] = float('nan')
    _, _, s0, s1, f0, f1 = run(xb, target)
    assert f0 == 1 and f1 == 1 and np.isnan(s1[0])
    tb = target.clone(); tb[0, 0, 1] = 200
    _, _, s0, s1, f0, f1 = run(x, tb)
    assert f0 == 2 and f1 == 2 and np.isnan(s0[0]) and np.isnan(s1[0])


@pytest.mark.parametrize('name', ['up2', 'up4', 'up_bcast', 'up_odd'])
def test_bilinear_golden(golden, name):
    g = golden('ops_micro')
    x = dev(g[f'{name}.x']).requires_grad_(True)
    y = HF.upsample_bilinear_ac(x, g[f'{name}.y'].shape[2:])
    check(host(y), g[f'{name}.y'], 1e-5)
    y.backward(dev(g[f'{name}.dy']))
    check(host(x.grad), g[f'{name}.dx'], 1e-5)


@pytest.mark.parametrize('shape,r', [((2, 192, 5, 40), 8), ((1, 12, 3, 70), 2), ((2, 27, 4, 33), 3), ((1, 2048, 2, 3), 32)])
def test_pixel_shuffle_vs_oracle_ragged(shape, r):
    # the LDS-tiled kernel: tiles of 32 pixels with a ragged last tile (40 = 32 + 8, 70, 33), several upscale factors; r = 32 exceeds the
    # tile's LDS budget and takes the gather kernel. A permutation: exact.
    rs = np.random.RandomState(r)
    x = rs.standard_normal(shape).astype(np.float32)
    xt = dev(x).requires_grad_(True)
    y = HF.pixel_shuffle(xt, r)
    yo = O.pixel_shuffle(x, r)
    assert np.array_equal(host(y), yo)
    dy = rs.standard_normal(yo.shape).astype(np.float32)
    y.backward(dev(dy))
    N, C, H, W = shape
    c = C // (r * r)
    dxo = dy.reshape(N, c, H, r, W, r).transpose(0, 1, 3, 5, 2, 4).reshape(N, C, H, W)
    assert np.array_equal(host(xt.grad), dxo)


def test_pixel_shuffle_golden(golden):
    g = golden('ops_micro')
    x = dev(g['pixel_shuffle.x']).requires_grad_(True)
    y = HF.pixel_shuffle(x, 8)
    assert np.array_equal(host(y), g['pixel_shuffle.y'])
    y.backward(dev(g['pixel_shuffle.dy']))
    assert np.array_equal(host(x.grad), g['pixel_shuffle.dx'])


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_batchnorm_golden(golden, mode):
    g = golden('ops_micro')
    p = f'bn_{mode}'
    bn = D.nn_modules.HipBatchNorm2d(19).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(dev(g[f'{p}.gamma'])); bn.bias.copy_(dev(g[f'{p}.beta']))
        bn.running_mean.copy_(dev(g[f'{p}.rm0'])); bn.running_var.copy_(dev(g[f'{p}.rv0']))
    bn.train(mode == 'train')
    x = dev(g[f'{p}.x']).requires_grad_(True)
    y = bn(x)
    check(host(y), g[f'{p}.y'], 1e-5)
    y.backward(dev(g[f'{p}.dy']))
    check(host(x.grad), g[f'{p}.dx'], 1e-4); check(host(bn.weight.grad), g[f'{p}.dgamma'], 1e-5); check(host(bn.bias.grad), g[f'{p}.dbeta'], 1e-5)
    check(host(bn.running_mean), g[f'{p}.rm1'], 1e-5); check(host(bn.running_var), g[f'{p}.rv1'], 1e-5)
    assert int(bn.state_dict()['num_batches_tracked']) == (1 if mode == 'train' else 0)


@pytest.mark.parametrize('C', [1, 19, 48, 256, 304, 2048, (2, 19, 128, 128), (4, 6, 9, 10), (1, 1, 64, 128), (3, 19, 5, 7), (2, 3, 66, 34)])
def test_batchnorm_relu_dropout_residual_vs_oracle(C):
    # channel counts that are not multiples of 4 run the "flat" 16-byte kernels when the tensor is dense and P*C % 4 == 0 (19 classes with
    # several float4 strides per thread, 6 = the gcd-2 case, 1 and 3 channels) and the one-float-per-lane kernels otherwise ((3, 19, 5, 7))
    shape = C if isinstance(C, tuple) else (2, C, 6, 10)
    C = shape[1]
    rs = np.random.RandomState(C + shape[2])
    x = (rs.standard_normal(shape) * 2 + 0.5).astype(np.float32); res = rs.standard_normal(x.shape).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32); beta = rs.standard_normal(C).astype(np.float32)
    bn = D.nn_modules.HipBatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(dev(gamma)); bn.bias.copy_(dev(beta))
    bn.train()
    xt = dev(x).requires_grad_(True); rt = dev(res).requires_grad_(True)
    y = HF.batch_norm_act(xt, bn, relu=True, drop_p=0.2, seed=77, rng_stream=5, residual=rt)
    yo, (mean, invstd), _ = O.batchnorm_train(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    keep = O.dropout_mask(x.shape, 0.2, 77, 5)
    act = np.maximum(yo + res, 0)
    check(host(y), act * keep / 0.8, 1e-5, 'y')
    dy = rs.standard_normal(x.shape).astype(np.float32)
    y.backward(dev(dy))
    gpre = dy.astype(np.float64) * keep / 0.8 * (act > 0)
    dxo, dgo, dbo = O.batchnorm_train_bwd(x.astype(np.float64), gamma.astype(np.float64), mean, invstd, gpre)
    check(host(xt.grad), dxo, 1e-4, 'dx'); check(host(rt.grad), gpre, 1e-5, 'dres')
    check(host(bn.weight.grad), dgo, 1e-4, 'dgamma'); check(host(bn.bias.grad), dbo, 1e-4, 'dbeta')


@pytest.mark.parametrize('shape', [(8, 256, 16, 32), (8, 1024, 16, 32), (8, 64, 64, 128), (2, 512, 2, 4), (2, 256, 1, 1), (3, 128, 5, 7), (2, 32, 3, 3)])
@pytest.mark.parametrize('variant', ['relu+res+drop', 'plain'])
def test_batchnorm_fused_vs_three_kernel_path_and_oracle(shape, variant):
    """The single-kernel BN for small tensors (bn_fused_fwd/bwd_kernel: register-resident slabs + one device-wide barrier) against
    the statistics / finalize / apply kernels it replaces (DSRL_BN_FUSED=0 selects them per call) and against the fp64 oracle:
    layer3 / layer4 / layer1 shapes, one row per slab (2x4 maps), the pooled ASPP branch (one pixel per image), ragged row counts."""
    N, C, H, W = shape
    rs = np.random.RandomState(sum(shape))
    x = (rs.standard_normal(shape) * 2 + 0.5).astype(np.float32); res = rs.standard_normal(shape).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32); beta = rs.standard_normal(C).astype(np.float32)
    dy = rs.standard_normal(shape).astype(np.float32)
    full = variant != 'plain'
    out = {}
    for fused in ('1', '0'):
        os.environ['DSRL_BN_FUSED'] = fused
        try:
            bn = D.nn_modules.HipBatchNorm2d(C).to(DEV)
            with torch.no_grad():
                bn.weight.copy_(dev(gamma)); bn.bias.copy_(dev(beta))
            bn.train()
            xt = dev(x).requires_grad_(True); rt = dev(res).requires_grad_(True) if full else None
            y = HF.batch_norm_act(xt, bn, relu=full, drop_p=0.2 if full else 0.0, seed=77, rng_stream=5, residual=rt)
            y.backward(dev(dy))
            out[fused] = [host(y), host(xt.grad), host(bn.weight.grad), host(bn.bias.grad), host(bn.running_mean), host(bn.running_var)] + \
                         ([host(rt.grad)] if full else [])
        finally:
            os.environ.pop('DSRL_BN_FUSED', None)
    for a, b, name in zip(out['1'], out['0'], ('y', 'dx', 'dgamma', 'dbeta', 'running_mean', 'running_var', 'dres')):
        check(a, b, 2e-5 if name in ('y', 'running_mean', 'running_var', 'dres') else 2e-4, 'fused vs three-kernel ' + name)
    yo, (mean, invstd), (rm, rv) = O.batchnorm_train(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), np.zeros(C), np.ones(C))
    if full:
        keep = O.dropout_mask(x.shape, 0.2, 77, 5)
        act = np.maximum(yo + res, 0)
        yo = act * keep / 0.8
        gpre = dy.astype(np.float64) * keep / 0.8 * (act > 0)
    else:
        gpre = dy.astype(np.float64)
    dxo, dgo, dbo = O.batchnorm_train_bwd(x.astype(np.float64), gamma.astype(np.float64), mean, invstd, gpre)
    y, dx, dg, db = out['1'][:4]
    check(y, yo, 2e-5, 'y'); check(dx, dxo, 2e-4, 'dx'); check(dg, dgo, 2e-4, 'dgamma'); check(db, dbo, 2e-4, 'dbeta')
    check(out['1'][4], rm, 1e-5, 'running_mean'); check(out['1'][5], rv, 1e-5, 'running_var')


@pytest.mark.parametrize('C', [256, 48])
def test_batchnorm_frozen_statistics_backward(C):
    """--freeze-batch-norm training (train_or_resume.py:379-382): BN modules in eval mode, gradients still flow.  C = 256 takes the fused
    backward kernel (training = 0: no batch-statistics terms), C = 48 the three-kernel path; both against the oracle."""
    rs = np.random.RandomState(C)
    x = (rs.standard_normal((4, C, 16, 32)) * 1.5 + 0.3).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32); beta = rs.standard_normal(C).astype(np.float32)
    rm = rs.standard_normal(C).astype(np.float32) * 0.2; rv = rs.uniform(0.5, 2.0, C).astype(np.float32)
    dy = rs.standard_normal(x.shape).astype(np.float32)
    bn = D.nn_modules.HipBatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(dev(gamma)); bn.bias.copy_(dev(beta)); bn.running_mean.copy_(dev(rm)); bn.running_var.copy_(dev(rv))
    bn.eval()
    xt = dev(x).requires_grad_(True)
    y = HF.batch_norm_act(xt, bn, relu=True)
    y.backward(dev(dy))
    invstd = 1.0 / np.sqrt(rv.astype(np.float64) + bn.eps)
    yo = (x.astype(np.float64) - rm.reshape(1, -1, 1, 1)) * (invstd * gamma).reshape(1, -1, 1, 1) + beta.reshape(1, -1, 1, 1)
    g = dy.astype(np.float64) * (yo > 0)
    dxo, dgo, dbo = O.batchnorm_eval_bwd(x.astype(np.float64), gamma.astype(np.float64), rm.astype(np.float64), invstd, g)
    check(host(y), np.maximum(yo, 0), 1e-5, 'y'); check(host(xt.grad), dxo, 1e-5, 'dx')
    check(host(bn.weight.grad), dgo, 1e-4, 'dgamma'); check(host(bn.bias.grad), dbo, 1e-4, 'dbeta')
    check(host(bn.running_mean), rm, 0.0); check(host(bn.running_var), rv, 0.0)


@pytest.mark.parametrize('shape', [(8, 256, 16, 32, 256, 3, 1, 1, 1), (3, 64, 33, 47, 96, 3, 2, 1, 1), (2, 128, 9, 13, 64, 1, 1, 0, 1), (8, 64, 64, 128, 64, 3, 1, 1, 1),
                                   (8, 512, 16, 32, 512, 3, 1, 2, 2), (8, 2048, 16, 32, 256, 3, 1, 6, 6), (2, 1024, 9, 13, 512, 3, 1, 1, 1)])
def test_conv_epilogue_bn_statistics(shape):
    """conv2d_bn_act: BatchNorm batch statistics from the conv epilogue (dsrl_conv2d_fwd_stats -> dsrl_bn_train_fwd_from_stats) against
    the separate conv + BN path and the oracle; ragged row counts (33x47 maps), channel tails of the last tile (96 = 64 + 32), a shape
    with more than 256 row blocks (reduced to 32 by bn_stats_reduce_kernel first), residual + ReLU, and the backward pass through both. The last three shapes are
    split-K launches (layer4 conv2, a dilated ASPP branch, a ragged 9x13 map): their partials come from the slab reduce (splitk_reduce_stats_kernel)."""
    N, C, H, W, K, R, stride, pad, dil = shape
    rs = np.random.RandomState(sum(shape))
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, K).astype(np.float32); beta = rs.standard_normal(K).astype(np.float32)
    yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, dil)
    res = rs.standard_normal(yo.shape).astype(np.float32); dy = rs.standard_normal(yo.shape).astype(np.float32)
    out = {}
    old = HF.conv_bn_stats_enabled
    try:
        for enabled in (True, False):
            HF.conv_bn_stats_enabled = enabled
            bn = D.nn_modules.HipBatchNorm2d(K).to(DEV).train()
            with torch.no_grad():
                bn.weight.copy_(dev(gamma)); bn.bias.copy_(dev(beta))
            xt = dev(x).requires_grad_(True); wt = torch.nn.Parameter(dev(w)); rt = dev(res).requires_grad_(True)
            y = HF.conv2d_bn_act(xt, wt, None, stride, pad, dil, bn, relu=True, residual=rt)
            y.backward(dev(dy))
            out[enabled] = [host(v) for v in (y, xt.grad, wt.grad, rt.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)]
    finally:
        HF.conv_bn_stats_enabled = old
    names = ('y', 'dx', 'dw', 'dres', 'dgamma', 'dbeta', 'running_mean', 'running_var')
    for a, b, name in zip(out[True], out[False], names):
        check(a, b, 2e-5 if name in ('y', 'dres', 'running_mean', 'running_var') else 5e-4, 'epilogue statistics vs separate path: ' + name)
    bo, (mean, invstd), (rm, rv) = O.batchnorm_train(yo, gamma.astype(np.float64), beta.astype(np.float64), np.zeros(K), np.ones(K))
    check(out[True][0], np.maximum(bo + res, 0), 2e-5, 'y vs oracle'); check(out[True][6], rm, 1e-5, 'running_mean'); check(out[True][7], rv, 1e-5, 'running_var')


def test_batchnorm_fused_budget_and_timeout_counter():
    """Budget 0 selects the three-kernel path, 128 keeps the 256-block variant off; no launch of this suite ever timed out at the barrier."""
    rs = np.random.RandomState(11)
    x = rs.standard_normal((8, 512, 32, 64)).astype(np.float32)          # 8.4 M elements: 256-block variant when allowed
    outs = []
    try:
        for budget in (256, 128, 0):
            HF.set_bn_fused_max_blocks(budget)
            bn = D.nn_modules.HipBatchNorm2d(512).to(DEV).train()
            outs.append(host(HF.batch_norm_act(dev(x), bn, relu=True)))
    finally:
        HF.set_bn_fused_max_blocks(None)
    check(outs[0], outs[2], 2e-5); check(outs[1], outs[2], 2e-5)
    assert np.array_equal(outs[1], outs[2])          # budget 128 cannot hold this tensor: both ran the three-kernel path
    assert HF.bn_fused_barrier_timeouts() == 0


def test_dropout_matches_oracle_philox():
    x = np.random.RandomState(3).standard_normal((2, 19, 16, 32)).astype(np.float32)
    xt = dev(x).requires_grad_(True)
    y = HF.dropout(xt, 0.2, True, 1234, 3)
    keep = O.dropout_mask(x.shape, 0.2, 1234, 3)
    assert np.array_equal(host(y) != 0, keep & (x != 0))
    check(host(y), x * keep / 0.8, 1e-6)
    y.backward(torch.ones_like(y))
    check(host(xt.grad), keep / 0.8, 1e-6)


def test_pools_golden(golden):
    g = golden('ops_micro')
    x = dev(g['gap.x']).requires_grad_(True)
    y = HF.global_avg_pool(x); check(host(y), g['gap.y'], 1e-5)
    y.backward(dev(g['gap.dy'])); check(host(x.grad), g['gap.dx'], 1e-5)
    x = dev(g['maxpool.x']).requires_grad_(True)
    y = HF.max_pool3x3s2(x); assert np.array_equal(host(y), g['maxpool.y'])
    y.backward(dev(g['maxpool.dy'])); check(host(x.grad), g['maxpool.dx'], 1e-6)


@pytest.mark.parametrize('C', [2048, 19, 6])
def test_global_avgpool_backward_both_kernels(C):
    # the 16-byte kernel (C % 4 == 0) and the scalar one: dy / HW, exact
    rs = np.random.RandomState(C)
    x = rs.standard_normal((2, C, 5, 7)).astype(np.float32); dy = rs.standard_normal((2, C, 1, 1)).astype(np.float32)
    xt = dev(x).requires_grad_(True)
    y = HF.global_avg_pool(xt); check(host(y), x.mean((2, 3), keepdims=True), 1e-6)
    y.backward(dev(dy))
    assert np.array_equal(host(xt.grad), np.broadcast_to(dy * np.float32(1.0 / 35.0), x.shape))


def test_aspp_pooled_branch_publishes_the_shared_gradient():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 32, 6, 8)).astype(np.float32); w = (rs.standard_normal((16, 32, 1, 1)) * 0.2).astype(np.float32)
    dyp = rs.standard_normal((2, 32, 1, 1)).astype(np.float32); dyc = rs.standard_normal((2, 16, 6, 8)).astype(np.float32)
    xt = dev(x).requires_grad_(True); wt = dev(w).requires_grad_(True)
    xs, slot = HF.fork(xt), HF.GradSlot()
    a = HF.conv2d(xs, wt, None, 1, 0, 1, grad_slot=slot)
    b = HF.global_avg_pool(xs, slot)
    torch.autograd.backward([a, b], [dev(dyc), dev(dyp)])
    assert slot.buf is not None and not slot.closed            # one buffer: the pool's, completed by the conv (a leaf's .grad is autograd's copy of it)
    check(host(slot.buf), host(xt.grad), 0.0)
    ref = np.einsum('nkhw,kc->nchw', dyc.astype(np.float64), w[:, :, 0, 0].astype(np.float64)) + dyp.astype(np.float64) / 48.0
    check(host(xt.grad), ref, 1e-5)


def test_ce_mse_sgd_golden(golden):
    g = golden('ops_micro')
    lg = dev(g['ce.logits']).requires_grad_(True)
    loss = HF.cross_entropy(lg, dev(g['ce.target']), 255)
    check(host(loss), g['ce.loss'], 1e-5)
    loss.backward(); check(host(lg.grad), g['ce.dlogits'], 1e-5)
    a = dev(g['mse.a']).requires_grad_(True)
    loss = HF.mse_loss(a, dev(g['mse.b'])); check(host(loss), g['mse.loss'], 1e-5)
    loss.backward(); check(host(a.grad), g['mse.da'], 1e-5)
    p = dev(g['sgd.p0']).clone(); buf = torch.zeros_like(p)
    for step in range(2):
        HF.sgd_step_(p, dev(g[f'sgd.g{step}']), buf, 0.006, 0.9, 5e-4)
        check(host(p), g[f'sgd.p{step + 1}'], 1e-6)


def test_ce_all_ignored_is_nan_and_nan_check():
    lg = dev(np.zeros((1, 19, 4, 4), np.float32))
    loss = HF.cross_entropy(lg, torch.full((1, 4, 4), 255, dtype=torch.uint8, device=DEV), 255)
    assert torch.isnan(loss)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    HF.nan_check_(flag, lg); assert int(flag) == 0
    HF.nan_check_(flag, lg, loss.reshape(1)); assert int(flag) == 1


# --------------------------------------------------------------------------------------------- FA loss
@pytest.mark.parametrize('case', ['rand', 'c3', 'big', 'signed', 'relu_like', 'same', 'near_degenerate'])
def test_fa_golden(golden, case):
    g = golden('fa_loss')
    f1 = dev(g[f'{case}.fm1'], cl=False).requires_grad_(True); f2 = dev(g[f'{case}.fm2'], cl=False).requires_grad_(True)
    for red in ('mean', 'sum'):
        check(host(D.FALoss(reduction=red)(f1, f2)), g[f'{case}.{red}'], 2e-5, red)
    none = D.FALoss(reduction='none')(f1, f2)
    assert tuple(none.shape) == tuple(g[f'{case}.none_shape'])
    check(gen.strided_sample(host(none)), g[f'{case}.none_sample'], 1e-4, 'none')
    D.FALoss()(f1, f2).backward()
    tol = 2e-2 if case == 'near_degenerate' else 2e-3          # sign-count / degenerate sigma_1 sensitivity, as in the oracle test
    check(host(f1.grad), g[f'{case}.g1'], tol, 'g1'); check(host(f2.grad), g[f'{case}.g2'], 2e-3, 'g2')


def test_fa_zero_sample_nan_and_shape_asserts(golden):
    g = golden('fa_loss')
    assert torch.isnan(D.FALoss()(dev(g['zero_sample.fm1'], cl=False), dev(g['zero_sample.fm2'], cl=False)))
    with pytest.raises(AssertionError):
        D.FALoss()(torch.zeros(2, 1, 8, device=DEV), torch.zeros(2, 1, 8, device=DEV))
    with pytest.raises(AssertionError):
        D.FALoss()(torch.zeros(2, 1, 8, 8, device=DEV), torch.zeros(2, 1, 8, 16, device=DEV))


# --------------------------------------------------------------------------------------------- composite head
@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_head_small_golden(golden, mode):
    g = golden('head_small')
    head, _ = make_head(gen.SMALL, 3, 101, mode == 'train')
    x16, x4, target, org = gen.make_head_inputs(202, 2, 2, 4, gen.SMALL)
    a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
    outs = head(a, b)
    for n, o in zip(('SSSR', 'SISR', 'SSSR_ft', 'SISR_ft'), outs):
        check(host(o), g[f'{mode}.{n}'], 1e-4, n)
    L = hip_losses(outs, dev(target), dev(org), 3)
    check(np.array([float(v) for v in L]), g[f'{mode}.losses'], 1e-4, 'losses')
    L[3].backward()
    for k, p in head.named_parameters():
        tol = 2e-3 if 'branches.4.0' not in k else 5e-2       # global-pool branch: train BN over a batch of 2 is ill-conditioned
        check(host(p.grad), g[f'{mode}.grad.{k}'], tol, 'grad ' + k)
    check(host(a.grad), g[f'{mode}.grad.backbone_features'], 2e-3); check(host(b.grad), g[f'{mode}.grad.lowlevel_features'], 2e-3)
    if mode == 'train':
        sd = head.state_dict()
        for k, v in sd.items():
            if 'running_' in k:
                check(host(v), g[f'train.new.{k}'], 1e-4, k)


@pytest.mark.parametrize('stage', [1, 2])
def test_head_small_stage_gating(golden, stage):
    g = golden('head_small')
    head, _ = make_head(gen.SMALL, stage, 101, True)
    x16, x4, target, org = gen.make_head_inputs(202, 2, 2, 4, gen.SMALL)
    outs = head(dev(x16), dev(x4))
    check(host(outs[0]), g[f'stage{stage}.SSSR'], 1e-4)
    assert not outs[2].is_cuda and outs[2].shape == (1,) and (outs[1].is_cuda == (stage > 1))     # DSRL.py:172-174
    L = hip_losses(outs, dev(target), dev(org), stage)
    check(np.array([float(v) for v in L]), g[f'stage{stage}.losses'], 1e-4)
    L[3].backward()
    # batch-2 train-mode BN over 2x4 maps: one ReLU flip of a pre-activation that sits at ~1e-7 moves this gradient by 5e-3 (seen with
    # any change of summation order in the BN statistics), hence 1e-2 here; the smooth cases are held to 2e-3 in test_head_small_golden
    check(host(head.SSSR_decoder['cls_conv'].weight.grad), g[f'stage{stage}.grad.cls_w'], 1e-2)


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_head_fullwidth_golden(golden, mode):
    g = golden('head_fullwidth')
    head, _ = make_head(gen.FULL, 3, 303, mode == 'train')
    x16, x4, target, org = gen.make_head_inputs(404, 2, 4, 8, gen.FULL)
    outs = head(dev(x16), dev(x4))
    check(gen.strided_sample(host(outs[0]), 65536), g[f'{mode}.SSSR_sample'], TOL)
    lg = host(outs[0])
    flips = lg.argmax(axis=1) != g[f'{mode}.SSSR_argmax']
    top2 = np.sort(lg, axis=1)[:, -2:]
    # identical class map except at near-ties: a flip is tolerated only where the top-2 margin is below 1e-5 of the logit range
    assert flips.mean() < 1e-4 and not np.any(flips & ((top2[:, 1] - top2[:, 0]) > 1e-5 * np.abs(lg).max())), int(flips.sum())
    check(gen.strided_sample(host(outs[1]), 16384), g[f'{mode}.SISR_sample'], TOL)
    check(host(outs[2]), g[f'{mode}.SSSR_ft'], TOL); check(host(outs[3]), g[f'{mode}.SISR_ft'], TOL)
    L = hip_losses(outs, dev(target), dev(org), 3)
    check(np.array([float(v) for v in L]), g[f'{mode}.losses'], TOL)        # eval: FA (and total) are NaN in the reference too
    if mode == 'train':
        L[3].backward()
        for k, p in head.named_parameters():
            gr = host(p.grad)
            if f'train.grad.{k}' in g:
                check(gr, g[f'train.grad.{k}'], 3e-3, 'grad ' + k)
            else:
                check(gen.strided_sample(gr, 4096), g[f'train.gradsample.{k}'], 3e-3, 'gradsample ' + k)


@pytest.mark.parametrize('fixture,pseed,iseed,h16,w16', [('head_train_256x512', 909, 1010, 16, 32), ('head_train_512x1024', 1111, 1212, 32, 64)])
def test_head_train_golden(golden, fixture, pseed, iseed, h16, w16):
    """BASELINE's workload in TRAIN mode against vectors generated by the imported reference (round 3): 256x512 input (and config 5's 512x1024 ->
    1024x2048: the second fixture), B=2, BatchNorm batch
    statistics over 16x32 / 64x128 maps, Dropout modules in eval, stage 3.  Losses 1e-4 and logits 1e-3 (range-relative and per element)
    against the reference's fp32 run.  Gradients of the total loss w.r.t. EVERY head parameter and both backbone-feature tensors: the backward
    pass through batch-statistics BatchNorm cancels heavily, so the reference's own fp32 gradients sit 1e-4 .. 2e-2 of their range away from
    the same reference modules run in float64 (err32.* in the fixture: 2.2e-2 for the low-level features, 2e-3 for the shortcut and cat_conv
    weights); the HIP path is held to the float64 values within 3e-3, or - where the reference itself is further off - within 2.5 x the
    reference's own fp32 error (a 4096-element sample's max norm moves by that much between two fp32 summation orders: the reference's
    full cat_conv.0 gradient is 3.5e-3 off where its sample is 1.2e-3 off); over all tensors together the HIP errors must not exceed the
    reference's by more than 1.5 x in the geometric mean.  The arithmetic mode does not move these numbers (exact-product fp32 MFMA, bf16x6 and f16x3 agree to 10 %)."""
    g = golden(fixture)
    head, _ = make_head(gen.FULL, 3, pseed, True)
    x16, x4, target, org = gen.make_head_inputs(iseed, 2, h16, w16, gen.FULL)
    a, b = dev(x16).requires_grad_(True), dev(x4).requires_grad_(True)
    outs = head(a, b)
    L = hip_losses(outs, dev(target), dev(org), 3)
    L[3].backward()
    check(np.array([float(v.detach()) for v in L]), g['losses'], 1e-4, 'losses')
    check(np.array([float(v.detach()) for v in L]), g['losses64'], 1e-5, 'losses vs the float64 reference')
    ss = gen.strided_sample(host(outs[0]), 1 << 16)
    check(ss, g['SSSR_sample'], TOL, 'logits')
    # per element: against the float64 run of the reference modules (the exact values), and against the reference's fp32 run no further than that
    # run itself is from float64 (two fp32 evaluations of one dot product differ by their summation orders: at 1024x2048 the sample's worst element
    # is 1.04e-3 apart between the two fp32 runs while each is within 1e-3 of float64)
    e64 = check_elementwise(ss, g['SSSR_sample64'], TOL, name='logits vs the float64 reference')
    eref = check_elementwise(g['SSSR_sample'], g['SSSR_sample64'], 1.0, name='reference fp32 vs its float64 run')
    e32 = check_elementwise(ss, g['SSSR_sample'], max(TOL, 2.0 * eref), name='logits vs the fp32 reference')
    print('element-wise logits: HIP vs float64 %.2e, reference fp32 vs float64 %.2e, HIP vs reference fp32 %.2e' % (e64, eref, e32))
    check(ss, g['SSSR_sample64'], 2e-5, 'logits vs the float64 reference')
    check(gen.strided_sample(host(outs[1]), 1 << 14), g['SISR_sample'], TOL, 'SISR')
    check(host(outs[2]), g['SSSR_ft'], TOL); check(host(outs[3]), g['SISR_ft'], TOL)
    grads = {k: host(p.grad) for k, p in head.named_parameters()}
    grads['backbone_features'], grads['lowlevel_features'] = host(a.grad), host(b.grad)
    rows, bad = [], {}
    for k, gr in grads.items():
        got = gr if f'grad.{k}' in g else gen.strided_sample(gr, 4096)
        e64, eref = rel_err(got, g[f'grad64.{k}']), float(g[f'err32.{k}'])
        rows.append((k, e64, eref))
        if e64 > max(3e-3, 2.5 * eref):          # worst observed: 2.08 x (lowlevel_features at 512x1024: 2.9e-2 against the reference's own 1.4e-2)
            bad[k] = (e64, eref)
    assert len(rows) == len(grads) and len(rows) >= 40
    rows.sort(key=lambda r: -r[1])
    print('gradients vs float64 reference (HIP, reference fp32):', [(k, '%.1e' % e, '%.1e' % r) for k, e, r in rows[:6]])
    assert not bad, bad
    # as a whole the HIP gradients are as close to float64 as the reference's fp32 gradients are (geometric mean of the ratios)
    ratio = float(np.exp(np.mean([np.log(max(e, 1e-9) / max(r, 1e-9)) for _, e, r in rows])))
    assert ratio < 1.5, ratio
    for k, v in head.state_dict().items():
        if f'new.{k}' in g:
            check(host(v), g[f'new.{k}'], 1e-4, 'running statistic ' + k)


def test_head_256x512_golden(golden):
    """BASELINE.json's size: 256x512 input -> 512x1024 logits, B=2, eval: identical argmax map, logits within 1e-3."""
    g = golden('head_256x512')
    head, _ = make_head(gen.FULL, 3, 505, False)
    x16, x4, target, org = gen.make_head_inputs(606, 2, 16, 32, gen.FULL)
    with torch.no_grad():
        outs = head(dev(x16), dev(x4))
        L = hip_losses(outs, dev(target), dev(org), 3)
    sssr = host(outs[0])
    check(gen.strided_sample(sssr, 1 << 17), g['SSSR_sample'], TOL)
    print('logits element-wise', '%.1e' % check_elementwise(gen.strided_sample(sssr, 1 << 17), g['SSSR_sample'], TOL, name='logits'))     # north_star's 1e-3, per element
    am = sssr.argmax(axis=1).astype(np.uint8)
    diff = am != g['SSSR_argmax']
    # a flip is tolerated only where the reference's own top-2 margin is below fp32 resolution of the logits
    assert not np.any(diff & (g['margin_u8'] > 0)), f'{int(diff.sum())} argmax flips outside near-ties'
    assert diff.mean() < 1e-5
    check(gen.checksum(sssr)[:2], g['SSSR_sum'][:2], 1e-4)
    check(gen.strided_sample(host(outs[1]), 1 << 15), g['SISR_sample'], TOL)
    check(host(outs[2]), g['SSSR_ft'], TOL); check(host(outs[3]), g['SISR_ft'], TOL)
    check(np.array([float(v) for v in L]), g['losses'], TOL)
    pix, mean = O.miou_batch(am, target), O.miou_batch(g['SSSR_argmax'], target)
    assert abs(pix[0] - mean[0]) < 1e-3 and abs(pix[1] - mean[1]) < 1e-3      # "mIoU vs ref" on the argmax maps


def test_head_512x1024_golden(golden):
    """BASELINE.json config 5's size: 512x1024 input -> 1024x2048 logits, B=1, eval, against vectors from the imported reference:
    identical argmax map (flips only at the reference's own near-ties), logits / SISR / transformer maps / CE, MSE, FA (32x32
    similarity matrices: n = 1024 all-pairs terms) within 1e-3."""
    g = golden('head_512x1024')
    head, _ = make_head(gen.FULL, 3, 707, False)
    x16, x4, target, org = gen.make_head_inputs(808, 1, 32, 64, gen.FULL)
    with torch.no_grad():
        outs = head(dev(x16), dev(x4))
        L = hip_losses(outs, dev(target), dev(org), 3)
    sssr = host(outs[0])
    assert sssr.shape == (1, 19, 1024, 2048)
    check(gen.strided_sample(sssr, 1 << 17), g['SSSR_sample'], TOL)
    am = sssr.argmax(axis=1).astype(np.uint8)
    diff = am != g['SSSR_argmax']
    assert not np.any(diff & (g['margin_u8'] > 0)), f'{int(diff.sum())} argmax flips outside near-ties'
    assert diff.mean() < 1e-5
    check(gen.checksum(sssr)[:2], g['SSSR_sum'][:2], 1e-4)
    check(gen.strided_sample(host(outs[1]), 1 << 15), g['SISR_sample'], TOL)
    check(host(outs[2]), g['SSSR_ft'], TOL); check(host(outs[3]), g['SISR_ft'], TOL)
    check(np.array([float(v) for v in L]), g['losses'], TOL)
    pix, mean = O.miou_batch(am, target), O.miou_batch(g['SSSR_argmax'], target)
    assert abs(pix[0] - mean[0]) < 1e-3 and abs(pix[1] - mean[1]) < 1e-3


def test_f16x1_head_512x1024_against_reference(golden):
    """The reduced-precision arithmetic of BASELINE config 5 ('fp16 MFMA convs': one fp16 MFMA per product, fp32 accumulation - 'f16x1', what apex
    O1 / O2 select in the reference, train_or_resume.py:68-72) on that configuration's size against the imported reference's fp32 vectors: not an
    fp32-equivalent mode, so the stated tolerance is 3e-3 of the range on logits / SISR and on the losses (measured 5e-4 / 4e-4 / 1e-4), 6e-3 on the
    one-channel transformer maps (a 19 -> 1 projection of the logits: measured 2.9e-3 / 1.1e-3); every
    conv is 3e-4 of its range off, test_conv_precision_modes), argmax disagreement below 0.1 % of the pixels, mIoU within 2e-3.  No loss scaling is
    involved: every operand tensor carries its own power-of-two scale (the heavy-tailed 1e-7 gradients of test_f16x3_operand_ranges go through the
    same scaling)."""
    g = golden('head_512x1024')
    HF.set_conv_precision('f16x1')
    try:
        head, _ = make_head(gen.FULL, 3, 707, False)
        x16, x4, target, org = gen.make_head_inputs(808, 1, 32, 64, gen.FULL)
        with torch.no_grad():
            outs = head(dev(x16), dev(x4))
            L = hip_losses(outs, dev(target), dev(org), 3)
        sssr = host(outs[0])
    finally:
        HF.set_conv_precision(None)
    T = 3e-3
    e = [check(gen.strided_sample(sssr, 1 << 17), g['SSSR_sample'], T, 'logits'), check(gen.strided_sample(host(outs[1]), 1 << 15), g['SISR_sample'], T, 'SISR'),
         check(host(outs[2]), g['SSSR_ft'], 2 * T), check(host(outs[3]), g['SISR_ft'], 2 * T), check(np.array([float(v) for v in L]), g['losses'], T, 'losses')]
    am = sssr.argmax(axis=1).astype(np.uint8)
    flips = float((am != g['SSSR_argmax']).mean())
    pix, mean = O.miou_batch(am, target), O.miou_batch(g['SSSR_argmax'], target)
    print('f16x1 at 512x1024 vs the fp32 reference:', ['%.1e' % v for v in e], 'argmax flips %.2e' % flips, 'mIoU', pix, mean)
    assert flips < 1e-3 and abs(pix[0] - mean[0]) < 2e-3 and abs(pix[1] - mean[1]) < 2e-3


@pytest.mark.parametrize('mode', ['f16x3', 'bf16x6', 'bf16x3', 'f16x1'])          # f16x3: the default arithmetic; f16x1: config 5's reduced-precision one (both timed by bench.py's config5 object)
def test_full_size_train_step_properties_512x1024(mode):
    """Config-5 size end to end (whole model, 512x1024 -> 1024x2048, B=2, train mode with dropout), where no oracle finishes in seconds:
    size-independent properties instead.  (1) Determinism: the same step from the same state and dropout key gives bit-identical
    losses and gradients (no atomics, fixed reduction orders).  (2) The reduced-precision arithmetic of config 5 ('bf16x3': 16-bit
    operands on the matrix cores, fp32 storage and accumulation - no loss scaling needed, the exponent range is fp32's) stays
    within 2e-3 of the fp32-equivalent run on the losses, and its gradient arena keeps the direction (cosine > 0.99)."""
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(54321)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (512, 1024), torch.device(DEV), length=1)))
    p0, b0 = flat.p_flat.clone(), flat.b_flat.clone()
    runs = []
    for m_ in (mode, mode, 'bf16x6'):
        HF.set_conv_precision(m_)
        flat.p_flat.copy_(p0); flat.b_flat.copy_(b0); flat.m_flat.zero_()
        HF.set_dropout_seed(31337)
        step = TrainStep(model, flat, 3, 0.1, 1.0, 255, graph=False)
        losses, outs = step(img, org, tgt, 0.0, 0.9, 0.0, True)          # lr 0: the state stays put, the gradients are what we look at
        assert outs[0].shape == (2, 19, 1024, 2048) and outs[2].shape == (2, 1, 128, 256)
        runs.append((losses, flat.g_flat.clone()))
    assert all(np.isfinite(v) for v in runs[0][0]), runs[0][0]
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]), 'the step is not deterministic'
    ref = runs[2]
    # f16x1: 11 significand bits per operand (apex O1 / O2's arithmetic), 3e-4 of the range per conv, ~100 convs deep: CE / MSE move by 1e-4, the
    # feature-affinity loss (differences of normalised similarity matrices of the two heads) by 2 %
    ltol = 5e-2 if mode == 'f16x1' else 2e-3
    for a, b in zip(runs[0][0], ref[0]):
        assert abs(a - b) <= ltol * max(abs(b), 1e-3), (runs[0][0], ref[0])
    rel = float((runs[0][1] - ref[1]).norm() / ref[1].norm())
    cos = float(torch.dot(runs[0][1].double(), ref[1].double()) / (runs[0][1].double().norm() * ref[1].double().norm()))
    # a random-init 101-layer net with batch-2 BatchNorm amplifies 1e-5 perturbations (ReLU flips): the whole-arena gradient is held to
    # its direction, the per-op accuracy of the mode is pinned by test_conv_precision_modes (3e-5 per conv)
    # f16x1 (11 bits): the same amplification leaves a cosine of ~0.6 at this batch-2 random initialisation (measured 0.59) - the price of the
    # reference's O1 / O2 arithmetic on such a net, not of this implementation: per conv it is 3e-4 of the range (test_conv_precision_modes), and
    # every gradient TENSOR of the whole model is pinned at fixed bounds where that amplification is absent
    # (test_full_model_frozen_bn_every_gradient_vs_stock_torch_fp64[f16x1], round 5)
    assert cos > (0.4 if mode == 'f16x1' else 0.99), (cos, rel)
    print(mode, 'losses', runs[0][0], 'gradient arena vs bf16x6: L2 difference %.2e, cosine %.5f' % (rel, cos))


@pytest.mark.parametrize('stage', [1, 2])
def test_train_step_stage1_stage2_b8_256x512(stage):
    """BASELINE configs 2 and 3: TrainStep for stage 1 (SSSR only) and stage 2 (+ SISR) at batch 8, 256x512 -> 512x1024, default arithmetic.
    The hipGraph-replayed step equals the eager launches bit for bit (losses, parameters, BatchNorm buffers), the losses are finite, and the
    parameters a stage does not own are absent (models/DSRL.py:172-184: the SISR decoder from stage 2, the feature transformers from stage 3)."""
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    HF.set_conv_precision(None)
    res = {}
    for graph in (False, True):
        torch.manual_seed(1234)
        model = D.DSRL(stage, cs)
        names = [k for k, _ in model.named_parameters()]
        assert any(k.startswith('SSSR_decoder') for k in names)
        assert any(k.startswith('SISR_decoder') for k in names) == (stage >= 2)
        assert not any('feature_transformer' in k for k in names)
        model = model.to(DEV).to(memory_format=torch.channels_last).train()
        flat = FlatParams(model)
        HF.set_dropout_seed(2024)
        was = HF.overlap_wgrad
        HF.overlap_wgrad = False
        try:
            step = TrainStep(model, flat, stage, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph)
            batches = list(SyntheticCityscapes(8, (256, 512), torch.device(DEV), length=4, distinct=2))
            hist = []
            for (img, org), (tgt, _) in batches:
                losses, outs = step(img, org, tgt, 0.006, 0.9, 5e-4, True)
                hist.append(losses)
            # unused outputs are CPU zeros(1) (DSRL.py:172-174)
            assert outs[0].shape == (8, 19, 512, 1024) and (outs[1].numel() == 1) == (stage < 2) and outs[2].numel() == 1 and outs[3].numel() == 1
        finally:
            HF.overlap_wgrad = was
        torch.cuda.synchronize()
        if graph:
            assert step.graph_replays == 4 - step.GRAPH_WARMUP
        res[graph] = (hist, flat.p_flat.clone(), flat.b_flat.clone())
        step.release()
    assert all(np.isfinite(v) for h in res[True][0] for v in h), res[True][0]
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])
    ms, fa = [h[1] for h in res[True][0]], [h[2] for h in res[True][0]]
    assert all(v == 0.0 for v in fa) and (all(v == 0.0 for v in ms) if stage == 1 else all(v > 0.0 for v in ms))


@pytest.mark.parametrize('C', [19, 3, 5, 1])
def test_bilinear_any_width_groups_of_four_bit_identical_to_the_scalar_kernels(C, monkeypatch):
    """align_corners=True resize of a tensor whose width is no multiple of 4 (the 19-channel logits upsample, DSRL.py:54): groups of four channels per thread
    (index arithmetic and tap weights once per group, 4-byte accesses, a short last group) against the one-element-per-thread kernels (DSRL_BILINEAR_G4=0):
    forward and backward bit-identical, and against torch's own CPU interpolate."""
    rs = np.random.RandomState(C)
    x = rs.standard_normal((2, C, 9, 13)).astype(np.float32)
    dy = rs.standard_normal((2, C, 18, 26)).astype(np.float32)
    got = {}
    for g4 in ('1', '0'):
        monkeypatch.setenv('DSRL_BILINEAR_G4', g4)
        xt = dev(x).requires_grad_(True)
        y = HF.upsample_bilinear_ac(xt, (18, 26))
        y.backward(dev(dy))
        torch.cuda.synchronize()
        got[g4] = (host(y), host(xt.grad))
    assert np.array_equal(got['1'][0], got['0'][0]) and np.array_equal(got['1'][1], got['0'][1])
    xr = torch.from_numpy(x).requires_grad_(True)
    yr = torch.nn.functional.interpolate(xr, size=(18, 26), mode='bilinear', align_corners=True)
    yr.backward(torch.from_numpy(dy))
    check(got['1'][0], yr.detach().numpy(), 1e-6, 'y'); check(got['1'][1], xr.grad.numpy(), 1e-5, 'dx')


@pytest.mark.parametrize('widths,strided', [((256, 48), False), ((256, 256, 256, 256, 256), False), ((64, 32), True), ((19, 48), False)])
def test_channel_concatenation_in_one_launch_with_its_magnitude(widths, strided, monkeypatch):
    """torch.cat(dim=1) of ASPP.py:44 / DSRL.py:165 as ONE kernel (dsrl_cat_channels) that also leaves max |value| in the amax record the consuming convs
    scale their operand by: bit-identical to the per-source strided copies (DSRL_CAT_ONE_LAUNCH=0) and to numpy; the record equals the measured maximum;
    the gradient is the channel slices.  The last case (19 channels) does not qualify and takes the copies."""
    rs = np.random.RandomState(len(widths))
    N, H, W = 2, 16, 32
    xs = [rs.standard_normal((N, c, H, W)).astype(np.float32) * (i + 1) for i, c in enumerate(widths)]
    def make():
        ts = []
        for x in xs:
            t = dev(x)
            if strided:             # a channel slice of a wider pixel-major buffer (pixel stride 2c)
                t = torch.cat([t, t], 1).contiguous(memory_format=torch.channels_last)[:, :x.shape[1]]
            ts.append(t.requires_grad_(True))
        return ts
    got = {}
    dyh = rs.standard_normal((N, sum(widths), H, W)).astype(np.float32)
    for mode in (True, False):
        monkeypatch.setattr(HF, 'cat_one_launch', mode)
        ts = make()
        y = HF.cat_channels(ts)
        rec = HF.carried_amax(y)
        y.backward(dev(dyh))
        torch.cuda.synchronize()
        got[mode] = (host(y), [host(t.grad) for t in ts], rec)
    ref = np.concatenate(xs, 1)
    assert np.array_equal(got[True][0], ref) and np.array_equal(got[False][0], ref)
    off = 0
    for a, b, c in zip(got[True][1], got[False][1], widths):
        assert np.array_equal(a, b) and np.array_equal(a, dyh[:, off:off + c])
        off += c
    if all(c % 4 == 0 for c in widths) and HF.f16_mode():
        rec = got[True][2]
        assert rec is not None and got[False][2] is None
        assert float(rec.view(torch.float32).max()) == float(np.abs(ref).max())       # abs bits of non-negative floats order like the floats
    else:
        assert got[True][2] is None


def test_amax_record_goes_stale_with_the_tensor():
    """A magnitude record cached on a tensor (functional.amax_for) must not outlive what it describes: the step arena is rewound and zeroed by the
    next step (a zero record would scale by 2^140: Inf / NaN), and an in-place write changes the values under the record.  The
    same tensor convolved before and after amax_begin_step(), and after an in-place scale by 1024, gives the same / the scaled result."""
    HF.set_conv_precision('f16x3')
    rs = np.random.RandomState(11)
    x = dev(rs.standard_normal((2, 64, 16, 32)).astype(np.float32))
    w = dev((rs.standard_normal((64, 64, 3, 3)) / 24).astype(np.float32))
    HF.amax_begin_step(x.device)
    try:
        y0 = host(HF.conv2d(x, w, None, 1, 1, 1))
        rec0 = HF.carried_amax(x)
        assert rec0 is not None and rec0._dsrl_gen > 0
        HF.amax_begin_step(x.device)                    # the next step: the arena is zeroed, its records re-issued
        assert HF.carried_amax(x) is None
        y1 = host(HF.conv2d(x, w, None, 1, 1, 1))
        assert np.array_equal(y0, y1)
        x.mul_(1024.0)                                  # in place: same tensor object, other values
        assert HF.carried_amax(x) is None
        y2 = host(HF.conv2d(x, w, None, 1, 1, 1))
        assert np.isfinite(y2).all() and np.array_equal(y2, y0 * 1024.0)       # a power of two: the split terms are the same, scaled
    finally:
        HF.amax_end_step(x.device)
    x2 = dev(rs.standard_normal((2, 64, 16, 32)).astype(np.float32))
    HF.conv2d(x2, w, None, 1, 1, 1)
    assert HF.carried_amax(x2)._dsrl_gen == -1          # outside a step: the loose arena, never re-issued


def test_head_train_with_dropout_vs_oracle():
    """Full train mode (batch-stat BN AND the four Dropout(0.2) modules live): HIP vs the fp64 oracle driven by the same
    Philox keys - the case the reference itself cannot be compared on (torch's RNG stream differs)."""
    head, P = make_head(gen.SMALL, 3, 101, True, dropout=True)
    x16, x4, target, org = gen.make_head_inputs(202, 2, 2, 4, gen.SMALL)
    HF.set_dropout_seed(4242)
    seed = HF.peek_next_seed()
    a = dev(x16).requires_grad_(True)
    outs = head(a, dev(x4))
    L = hip_losses(outs, dev(target), dev(org), 3)
    L[3].backward()
    out = O.head_forward({k: v.astype(np.float64) for k, v in P.items()}, x16.astype(np.float64), x4.astype(np.float64), 3, True, dropout_seed=seed)
    Lo = O.total_loss(out, target, org.astype(np.float64), 3)
    check(host(outs[0]), out.SSSR.v, 1e-4, 'SSSR'); check(np.array([float(v) for v in L]), np.array(Lo), 1e-4, 'losses')
    for k, p in head.named_parameters():
        if 'branches.4.0' not in k:
            check(host(p.grad), out.params[k].g, 2e-3, 'grad ' + k)
    check(host(a.grad), out.inputs[0].g, 2e-3)


@pytest.mark.parametrize('stage', [1, 2, 3])
def test_fused_losses_match_separate_kernels_and_oracle(stage):
    """functional.fused_losses (CE forward + backward in one pass over the logits, MSE likewise, the NaN asserts folded in, the
    stride-8 feature transformers adding their sparse gradient into the published dense one) against the separate loss kernels and the
    fp64 oracle: same five scalars, same parameter and input gradients."""
    x16, x4, target, org = gen.make_head_inputs(202, 2, 2, 4, gen.SMALL)
    res = []
    for fused in (False, True):
        head, P = make_head(gen.SMALL, stage, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        outs = head(a, b)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        if fused:
            vals = HF.fused_losses(outs, dev(target), dev(org), gen.IGNORE, 0.1, 1.0, stage, flag)
            vals[3].backward()
            L = [float(v) for v in vals[:4]]
            assert float(vals[4]) == 0.0 and int(flag) == 0
            if stage > 2 and HF.grad_slots_enabled:
                assert outs[0]._dsrl_out_slot.buf is not None and not outs[0]._dsrl_out_slot.closed          # the transformers accumulated in place
        else:
            Lt = hip_losses(outs, dev(target), dev(org), stage)
            Lt[3].backward()
            L = [float(v) for v in Lt]
        res.append((L, {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad)))
    out = O.head_forward({k: v.astype(np.float64) for k, v in P.items()}, x16.astype(np.float64), x4.astype(np.float64), stage, True)
    Lo = O.total_loss(out, target, org.astype(np.float64), stage)
    check(np.array(res[1][0]), np.array(Lo), 1e-4, 'fused losses vs oracle')
    check(np.array(res[1][0]), np.array(res[0][0]), 1e-6, 'fused vs separate losses')
    for k in res[0][1]:
        check(res[1][1][k], res[0][1][k], 1e-5, 'grad ' + k)
    check(res[1][2], res[0][2], 1e-5, 'dx16'); check(res[1][3], res[0][3], 1e-5, 'dx4')


def test_fused_losses_nan_flag_and_eval_mode():
    """The fused kernels raise the NaN flag for a NaN logit / SISR value, and run forward-only (no gradient buffers) under no_grad."""
    rs = np.random.RandomState(5)
    sssr = dev(rs.standard_normal((2, 19, 16, 32)).astype(np.float32)); sisr = dev(rs.standard_normal((2, 3, 16, 32)).astype(np.float32))
    org = dev(rs.standard_normal((2, 3, 16, 32)).astype(np.float32))
    ft1 = dev(rs.uniform(0.1, 1, (2, 1, 16, 32)).astype(np.float32)); ft2 = dev(rs.uniform(0.1, 1, (2, 1, 16, 32)).astype(np.float32))
    tgt = dev(rs.randint(0, 19, (2, 16, 32)).astype(np.uint8))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        v = HF.fused_losses((sssr, sisr, ft1, ft2), tgt, org, 255, 0.1, 1.0, 3, flag, 8)
    ce = O.cross_entropy(host(sssr).astype(np.float64), host(tgt).astype(np.uint8), 255)
    ms = O.mse(host(sisr).astype(np.float64), host(org).astype(np.float64))
    fa = O.fa_loss(host(ft1).astype(np.float64), host(ft2).astype(np.float64), 8)
    check(host(v[:4]), np.array([ce, 0.1 * ms, fa, ce + 0.1 * ms + fa]), 1e-5)
    assert float(v[4]) == 0
    for which in (0, 1):
        flag.zero_()
        bad = [sssr.clone(), sisr.clone()]
        bad[which][1, 2, 3, 4] = float('nan')
        with torch.no_grad():
            v = HF.fused_losses((bad[0], bad[1], ft1, ft2), tgt, org, 255, 0.1, 1.0, 3, flag, 8)
        assert int(flag) == 1 and float(v[4]) == 1.0, which
    # a label outside [0, 19) that is not the ignore index: torch's CrossEntropyLoss asserts; here flag bit 1 and a NaN loss (TrainStep.collect raises)
    flag.zero_()
    tb = tgt.clone(); tb[1, 3, 5] = 200
    with torch.no_grad():
        v = HF.fused_losses((sssr, sisr, ft1, ft2), tb, org, 255, 0.1, 1.0, 3, flag, 8)
    assert int(flag) == 2 and np.isnan(float(v[0])) and np.isnan(float(v[3]))
    # the gradients are formed in the forward pass for d(total) = 1: a scaled loss (or another element as the root) must be refused, not served unscaled
    flag.zero_()
    a, b = sssr.clone().requires_grad_(True), sisr.clone().requires_grad_(True)
    HF._fused_losses_root_checked = False
    v = HF.fused_losses((a, b, ft1, ft2), tgt, org, 255, 0.1, 1.0, 3, flag, 8)
    with pytest.raises(Exception, match='only vals\\[3\\].backward'):
        (2.0 * v[3]).backward()
    v = HF.fused_losses((a, b, ft1, ft2), tgt, org, 255, 0.1, 1.0, 3, flag, 8)
    v[3].backward()
    assert HF._fused_losses_root_checked and a.grad is not None


def test_train_steps_golden(golden):
    """Two SGD steps of the small head on the flat-arena optimiser reproduce the reference's parameters."""
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    g = golden('train_steps')
    head, _ = make_head(gen.SMALL, 3, 101, True)
    flat = FlatParams(head)
    for step in range(2):
        x16, x4, target, org = gen.make_head_inputs(700 + step, 2, 2, 4, gen.SMALL)
        flat.zero_grad()
        outs = head(dev(x16), dev(x4))
        L = hip_losses(outs, dev(target), dev(org), 3)
        L[3].backward()
        flat.sgd_step(lr=0.006, momentum=0.9, weight_decay=5e-4)
        check(np.array([float(v) for v in L]), g[f'step{step}.losses'], 2e-4)
        for k, v in head.state_dict().items():
            if 'num_batches' not in k:
                check(host(v), g[f'step{step}.{k}'], 2e-4, f'step{step} {k}')


@pytest.mark.parametrize('graph', [False, True])
def test_gradient_arena_fill_skipped_only_because_every_slot_is_overwritten(graph, monkeypatch):
    """ddp.FlatParams.zero_grad() skips the 240 MB fill once a whole pass has written every parameter's gradient through the sink protocol (round 5).
    That is only sound if the kernels OVERWRITE their slots: poison the arena with NaN in front of a step and compare with a step that did zero it -
    every gradient finite and bit-identical; and the guard: a pass that leaves a parameter unwritten after a skipped fill is refused."""
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    res = {}
    for lazy in (True, False):
        torch.manual_seed(77)
        model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
        flat = FlatParams(model)
        flat.lazy_zero = lazy
        HF.set_dropout_seed(1234)
        step = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph)

        def poison(flat=flat):                  # every parameter's slot (the alignment padding between slots is written by nobody and stays zero)
            for p_ in flat.params:
                p_.grad.fill_(float('nan'))
        for it in range(step.GRAPH_WARMUP + 3 if graph else 3):
            if lazy and not graph and it >= 1:
                assert flat._all_claimed_last                      # the previous pass wrote all of them: this step will not fill
                poison()                                          # ... so whatever is in the slots must not matter
            losses, _ = step(img, org, tgt, 0.0, 0.9, 0.0, True)            # lr 0: the parameters stay put
        if graph:
            if lazy:
                poison()                                          # the captured step carries no fill either
            losses, _ = step(img, org, tgt, 0.0, 0.9, 0.0, True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(flat.g_flat).all()), 'a gradient slot kept what was in the arena'
        res[lazy] = (flat.g_flat.clone(), losses)
        if lazy and not graph:
            flat.zero_grad()
            assert flat._fill_skipped
            with pytest.raises(HF.DsrlHipError, match='not written by their kernels'):
                flat.settle_grads()                                # no backward pass in between: nothing was written
        step.release()
    assert torch.equal(res[True][0], res[False][0]) and res[True][1] == res[False][1]


def test_full_model_train_steps_run():
    """Whole DSRL (ResNet-101 on the same kernels: 7x7 s2 stem, strided/dilated bottlenecks, max-pool, residual BN) takes
    three SGD steps on a 64x128 batch through TrainStep: finite losses, every parameter receives a gradient."""
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(54321)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    step = TrainStep(model, flat, 3, 0.1, 1.0, 255)
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    hist = [step(img, org, tgt, 0.006, 0.9, 5e-4, True)[0] for _ in range(3)]
    assert all(np.isfinite(v) for h in hist for v in h), hist
    p0 = flat.p_flat.clone()
    step(img, org, tgt, 0.006, 0.9, 5e-4, True)
    assert float((flat.p_flat - p0).abs().max()) > 0
    assert all(float(p.grad.abs().sum()) > 0 for p in model.parameters())
    outs = model.eval()(img)
    assert outs[0].shape == (2, 19, 128, 256) and outs[1].shape == (2, 3, 128, 256) and outs[2].shape == (2, 1, 16, 32)


@pytest.mark.parametrize('shape', [(2, 3, 32, 64, 8, 7, 2, 3), (1, 3, 37, 51, 16, 7, 2, 3), (2, 3, 16, 24, 8, 3, 1, 1)])
def test_stem_rowfold_conv_vs_oracle(shape):
    """The row-folded image-stem path (7x7 stride 2 on RGB, ResNet101.py:28) against the oracle: output and weight gradient."""
    N, C, H, W, K, R, stride, pad = shape
    rs = np.random.RandomState(R * H)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32); w = (rs.standard_normal((K, C, R, R)) * 0.1).astype(np.float32)
    yo = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, 1)
    dy = rs.standard_normal(yo.shape).astype(np.float32)
    _, dwo, _ = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, 1)
    wt = dev(w).requires_grad_(True)
    y = HF.conv2d(dev(x, cl=False), wt, None, stride, pad, 1)         # NCHW image, no grad -> _StemConv
    assert y.grad_fn is not None and 'StemConv' in type(y.grad_fn).__name__
    check(host(y), yo, 1e-5, 'y')
    y.backward(dev(dy))
    check(host(wt.grad), dwo, 1e-5, 'dw')


def test_gradient_sink_matches_autograd_accumulation():
    """Conv / BN parameter gradients written straight into the FlatParams arena equal the ones autograd accumulates."""
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    x16, x4, target, org = gen.make_head_inputs(202, 2, 2, 4, gen.SMALL)
    grads = []
    for use_arena in (False, True):
        head, _ = make_head(gen.SMALL, 3, 101, True)
        flat = FlatParams(head) if use_arena else None
        if flat is not None:
            flat.zero_grad()
        outs = head(dev(x16), dev(x4))
        hip_losses(outs, dev(target), dev(org), 3)[3].backward()
        if flat is not None:
            flat.finish_reduction()              # joins the side stream the weight-gradient kernels ran on
            HF.amax_end_step(flat.device)        # no optimiser pass ends this step: close its amax arena, or every later test draws its records from it
            assert len(flat._claimed) >= 30
        grads.append({k: host(p.grad) for k, p in head.named_parameters()})
    # BN gradients: the same kernels either way - bit-identical.  Conv weight gradients: the arena path defers them into the grouped launch
    # (dsrl_conv2d_wgrad_group_*), whose pixel ranges are split differently from the per-layer launch - equal up to the summation order.
    for k in grads[0]:
        a, b = grads[0][k], grads[1][k]
        if a.ndim == 4 and 'upsample16_pred' not in k and 'feature_transformer' not in k:
            assert np.abs(a - b).max() <= 2e-6 * max(np.abs(a).max(), 1e-30), (k, float(np.abs(a - b).max()), float(np.abs(a).max()))
        else:
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


def test_batched_filter_transposes_match_per_layer_path():
    """ddp.FlatParams.refresh_transposed_filters (one dsrl_conv2d_transpose_filters_batched launch for every conv filter of the
    model) feeds the dgrad kernels the same transposed filters as the per-call transpose: bit-identical gradients; the copies
    are marked stale by the SGD update."""
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    from dualsuperreslearningforsemseg_amd.filter_operands import STALE
    x16, x4, target, org = gen.make_head_inputs(202, 2, 2, 4, gen.SMALL)
    grads = []
    for batched in (False, True):
        head, _ = make_head(gen.SMALL, 3, 101, True)
        flat = FlatParams(head)
        assert flat.filters.rows >= 10 and flat.filters.state == STALE
        flat.zero_grad()
        if batched:
            flat.refresh_transposed_filters()
            assert flat.filters.state != STALE
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        outs = head(a, b)
        hip_losses(outs, dev(target), dev(org), 3)[3].backward()
        flat.finish_reduction()
        g = {k: host(p.grad) for k, p in head.named_parameters()}
        g['x16'], g['x4'] = host(a.grad), host(b.grad)
        grads.append(g)
        flat.sgd_step(0.01, 0.9, 5e-4)
        assert flat.filters.state == STALE
    bad = {k: float(np.abs(grads[0][k] - grads[1][k]).max()) for k in grads[0] if not np.array_equal(grads[0][k], grads[1][k])}
    assert not bad, bad


def test_streaming_filter_amax_equals_transposing_pass(monkeypatch):
    """The per-step filter pass of the f16x3 arithmetic measures max |w| of every filter with one streaming launch (dsrl_conv2d_filters_amax_batched);
    its records must hold exactly the values the batched transpose leaves (the maximum over the 16 shards of a record, = max |w| of the filter)."""
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    head, _ = make_head(gen.FULL, 3, 909, True)
    flat = FlatParams(head)
    vals = {}
    for stream in ('1', '0'):
        monkeypatch.setenv('DSRL_FILTER_AMAX_STREAM', stream)
        flat.filters.invalidate()
        flat.refresh_transposed_filters()
        torch.cuda.synchronize()
        vals[stream] = flat.filters.amax.view(-1, HF.AMAX_WORDS).max(dim=1).values.cpu().numpy().copy()
    assert flat.filters.amax_segs > flat.filters.rows and np.array_equal(vals['1'], vals['0'])
    expect = np.array([np.abs(host(w)).max() for w in flat.filters.filters], dtype=np.float32).view(np.int32)
    assert np.array_equal(vals['1'].astype(np.int32), expect)


def test_grad_slots_match_autograd_accumulation():
    """Bottleneck inputs: the residual-branch gradient and conv1's (or the downsample conv's) data gradient accumulated in one buffer
    by the dgrad epilogue (functional.GradSlot, dsrl_conv2d_dgrad_accumulate) equal autograd's separate sum on the whole backbone +
    head (also the ASPP input and the concatenated decoder features, which use the same mechanism)."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    rs = np.random.RandomState(5)
    x = rs.standard_normal((2, 3, 32, 64)).astype(np.float32)
    tg = rs.randint(0, 19, (2, 64, 128)).astype(np.uint8)
    org = rs.standard_normal((2, 3, 64, 128)).astype(np.float32)
    grads, logits = [], []
    old = HF.grad_slots_enabled
    try:
        for enabled in (False, True):
            HF.grad_slots_enabled = enabled
            torch.manual_seed(3)
            model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
            for m in model.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.eval()
            outs = model(dev(x, cl=False))
            L = hip_losses(outs, dev(tg), dev(org), 3)
            (L[0] + L[1]).backward()
            torch.cuda.synchronize()
            grads.append({k: host(p.grad) for k, p in model.named_parameters() if p.grad is not None})
            logits.append(host(outs[0]))
    finally:
        HF.grad_slots_enabled = old
    assert np.array_equal(logits[0], logits[1])
    # two contributions sum bit-identically (a + b is commutative); the ASPP input has five, whose order differs from autograd's,
    # and that rounding difference reaches every earlier layer: equality to fp32 rounding, amplified by the batch-2 BNs
    bad = {k: rel_err(grads[1][k], grads[0][k]) for k in grads[0] if rel_err(grads[1][k], grads[0][k]) > 2e-4}
    assert not bad, bad
    for k in ('SSSR_decoder.cls_conv.weight', 'SSSR_decoder.cat_conv.0.weight', 'SISR_decoder.0.weight', 'feature_extractor.aspp.branches.5.0.weight'):
        assert np.array_equal(grads[0][k], grads[1][k]), k          # downstream of every shared buffer: untouched


@pytest.mark.parametrize('shape', [(2, 64, 16, 32), (1, 256, 50, 100), (8, 128, 32, 64)])
def test_bn_backward_leaves_the_sums_of_the_residual_branch_batchnorm(shape):
    """out = relu(bn3(a) + bn_ds(b)) (first bottleneck of a layer, ResNet101.py:67-89): the backward of bn3 from given sums (dsrl_bn_bwd_from_stats_res)
    writes the masked gradient g = dy * [out > 0] to dresidual - the output gradient of bn_ds - and leaves bn_ds's two backward sums per (row block,
    channel).  dx / dresidual bit-identical to dsrl_bn_bwd_from_stats; the sums against numpy; bn_ds's backward from those sums against the fp64 oracle."""
    N, C, H, W = shape
    P = N * H * W
    rs = np.random.RandomState(sum(shape))
    a, b = rs.standard_normal((N, C, H, W)).astype(np.float32), rs.standard_normal((N, C, H, W)).astype(np.float32) * 2 + 0.5
    out = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    dy = rs.standard_normal((N, C, H, W)).astype(np.float32)
    mean, invstd, gamma = rs.standard_normal(C).astype(np.float32), rs.uniform(0.5, 2, C).astype(np.float32), rs.standard_normal(C).astype(np.float32)
    mean2 = b.mean((0, 2, 3)).astype(np.float32); invstd2 = (1 / np.sqrt(b.astype(np.float64).var((0, 2, 3)) + 1e-5)).astype(np.float32)
    gamma2 = rs.standard_normal(C).astype(np.float32)
    g = dy * (out > 0)
    xh = (a.astype(np.float64) - mean[None, :, None, None]) * invstd[None, :, None, None]
    stats = np.stack([g.astype(np.float64).sum((0, 2, 3)), (g * xh).sum((0, 2, 3))]).astype(np.float32)       # one row block of partials
    at, bt, ot, dyt = dev(a), dev(b), dev(out), dev(dy)
    mt, it, gt, m2t, i2t, g2t, stt = dev(mean), dev(invstd), dev(gamma), dev(mean2), dev(invstd2), dev(gamma2), dev(stats.reshape(-1))
    st = torch.cuda.current_stream().cuda_stream
    rparts = int(HF.query('dsrl_bn_bwd_from_stats_res_parts', P, C, 1))
    assert rparts > 0
    res = {}
    for name in ('dsrl_bn_bwd_from_stats_res', 'dsrl_bn_bwd_from_stats_drop'):
        dx, dres = torch.empty_like(at), torch.empty_like(at)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        rst = torch.full((int(HF.query('dsrl_bn_stats_floats', 2, rparts, C)),), float('nan'), device=DEV)
        extra = (bt.data_ptr(), C, m2t.data_ptr(), i2t.data_ptr(), rst.data_ptr(), rparts) if name.endswith('_res') else ()
        HF.call(name, at.data_ptr(), C, ot.data_ptr(), C, dyt.data_ptr(), C, dx.data_ptr(), C, dres.data_ptr(), C, P, C, mt.data_ptr(), it.data_ptr(), gt.data_ptr(),
                dg.data_ptr(), db.data_ptr(), 1, 0.0, 1, stt.data_ptr(), 1, None, *extra, st)
        torch.cuda.synchronize()
        res[name] = (host(dx), host(dres), rst, dres)
    r, d = res['dsrl_bn_bwd_from_stats_res'], res['dsrl_bn_bwd_from_stats_drop']
    assert np.array_equal(r[0], d[0]) and np.array_equal(r[1], d[1]) and np.array_equal(r[1], g)
    sums = r[2][:2 * rparts * C].view(2, rparts, C).double().sum(1).cpu().numpy()
    xh2 = (b.astype(np.float64) - mean2[None, :, None, None]) * invstd2[None, :, None, None]
    check(sums[0], g.astype(np.float64).sum((0, 2, 3)), 1e-5, 'sum g'); check(sums[1], (g * xh2).sum((0, 2, 3)), 1e-5, 'sum g xhat2')
    # the downsample BatchNorm's backward from those sums (no ReLU, no residual of its own)
    dx2 = torch.empty_like(at)
    dg2, db2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    HF.call('dsrl_bn_bwd_from_stats', bt.data_ptr(), C, None, C, r[3].data_ptr(), C, dx2.data_ptr(), C, None, C, P, C, m2t.data_ptr(), i2t.data_ptr(), g2t.data_ptr(),
            dg2.data_ptr(), db2.data_ptr(), 0, 1, r[2].data_ptr(), rparts, None, st)
    torch.cuda.synchronize()
    dxo, dgo, dbo = O.batchnorm_train_bwd(b.astype(np.float64), gamma2.astype(np.float64), mean2.astype(np.float64), invstd2.astype(np.float64), g.astype(np.float64))
    check(host(dx2), dxo, 1e-5, 'dx of the downsample BatchNorm'); check(host(dg2), dgo, 1e-5, 'dgamma'); check(host(db2), dbo, 1e-5, 'dbeta')


@pytest.mark.parametrize('shared', [False, True])
def test_bn_backward_statistics_from_dgrad_epilogue(shared):
    """functional.BNLink: bn1 / bn2 of every bottleneck take their two backward sums from the partials the consuming conv's dgrad left
    (dsrl_conv2d_dgrad_bnstats -> dsrl_bn_bwd_from_stats). Same gradients as with the BN kernels' own reductions, up to summation order."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    if not (HF.grad_slots_enabled and HF.outer_grad_slot):
        pytest.skip('the launch counts below are those of the default configuration (shared gradient buffers on)')
    rs = np.random.RandomState(6)
    x = rs.standard_normal((2, 3, 96, 160)).astype(np.float32)
    tg = rs.randint(0, 19, (2, 192, 320)).astype(np.uint8)
    org = rs.standard_normal((2, 3, 192, 320)).astype(np.float32)
    grads, counts = [], []
    old, orig_call, old_shared = HF.bn_bwd_stats_enabled, HF.call, HF.bn_bwd_stats_shared

    def counting(name, *a):
        key = 'dsrl_conv2d_dgrad_bnstats' if (name == 'dsrl_conv2d_dgrad_planes_drop' and a[31] is not None) else name       # a[31]: the bstats argument
        key = 'dsrl_bn_bwd_from_stats' if name in ('dsrl_bn_bwd_from_stats_drop', 'dsrl_bn_bwd_from_stats_res') else key
        counts[-1][key] = counts[-1].get(key, 0) + 1
        if name == 'dsrl_bn_bwd_from_stats_res':
            counts[-1]['res'] = counts[-1].get('res', 0) + 1
        return orig_call(name, *a)

    try:
        HF.call = counting
        HF.set_conv_precision('mixed')       # the epilogue statistics exist in the split-precision kernels only
        HF.bn_bwd_stats_shared = shared      # also bn3, through the next block's accumulating dgrad (off by default: measured slower)
        for enabled in (False, True):
            HF.bn_bwd_stats_enabled = enabled
            counts.append({})
            torch.manual_seed(3)
            model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
            for m in model.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.eval()
            outs = model(dev(x, cl=False))
            L = hip_losses(outs, dev(tg), dev(org), 3)
            (L[0] + L[1]).backward()
            torch.cuda.synchronize()
            grads.append({k: host(p.grad) for k, p in model.named_parameters() if p.grad is not None})
    finally:
        HF.bn_bwd_stats_enabled, HF.call, HF.bn_bwd_stats_shared = old, orig_call, old_shared
    assert counts[0].get('dsrl_bn_bwd_from_stats', 0) == 0 and counts[0].get('dsrl_conv2d_dgrad_bnstats', 0) == 0
    # bn1, bn2 of 33 bottlenecks + bn3 of the blocks whose output feeds only the next block (completed by its accumulating dgrad)
    # (a BN whose output has a further consumer - layer1's output also feeds the decoder - receives a summed gradient and rightly ignores them)
    # (round 5: + the two decoder BatchNorms of cat_conv, whose outputs feed conv4 / cls_conv only)
    # (round 5: + the downsample BatchNorm of each layer's first bottleneck, whose sums bn3's backward leaves while it writes the residual gradient:
    #  dsrl_bn_bwd_from_stats_res - needs bn3 itself on the from-statistics path, i.e. `shared`)
    lo, hi = (92, 101) if shared else (68, 68)
    res = counts[1].get('res', 0)
    assert res == (4 if (shared and HF.bn_res_stats_enabled) else 0), counts[1]
    assert lo <= counts[1].get('dsrl_bn_bwd_from_stats', 0) - res <= counts[1].get('dsrl_conv2d_dgrad_bnstats', 0) <= hi
    bad = {k: rel_err(grads[1][k], grads[0][k]) for k in grads[0] if rel_err(grads[1][k], grads[0][k]) > 5e-4}
    assert not bad, bad


@pytest.mark.parametrize('mode', ['mixed', 'bf16x6', 'f16x3'])
def test_full_model_vs_oracle(mode):
    """Whole DSRL (ResNet-101 OS16 backbone + head) at 32x64, B=2, train-mode BN, dropout off: every kernel family in one graph
    (row-folded 7x7/2 stem, max-pool, strided and dilated bottlenecks with residual BN, ASPP, decoders, CE + MSE) against the
    oracle.  A random-init 101-layer net with train-mode BN over 2x(2x4) maps is ill-conditioned: the oracle run in fp32 differs
    from the same oracle in fp64 by ~4e-3 (logits) and 5-25 % (gradients).  The test is therefore self-calibrating - the HIP
    path must be as close to fp64 as the fp32 CPU oracle is: logits within x1.5 of the oracle's own fp32 error and within 5e-3;
    gradients in the L2 norm within x2.5 per tensor and x2 over all tensors together (a gradient that is 10 % off in an fp32 CPU
    run is rounding-pattern noise - layer4's BNs see 16 values per channel here - so the max norm of a single tensor is not a
    stable yardstick: exact-product fp32, bf16x6, 'mixed' and different summation orders of the BN statistics move it 0.1-0.4).
    The assembled backbone is not pinned by the reference (torchvision's Bottleneck is absent): its primitives are."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    HF.set_conv_precision(mode)
    gslack = 2.5
    torch.manual_seed(3)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    sd = {k: v.numpy() for k, v in model.state_dict().items() if 'num_batches' not in k}
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    rs = np.random.RandomState(0)
    x = rs.standard_normal((2, 3, 32, 64)).astype(np.float32)
    tg = rs.randint(0, 19, (2, 64, 128)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255
    org = rs.standard_normal((2, 3, 64, 128)).astype(np.float32)
    outs = model(dev(x, cl=False))
    L = hip_losses(outs, dev(tg), dev(org), 3)
    (L[0] + L[1]).backward()          # CE + w1*MSE (the FA gradient compares 4x4 entries here: one sign flip = 12 %; tested separately)
    ref = {}
    for dt in (np.float64, np.float32):
        out = O.model_forward({k: v.astype(dt) for k, v in sd.items()}, x.astype(dt), 3, True)
        Lo = O.total_loss(out, tg, org.astype(dt), 3, backward=False)
        O.total_loss(out, tg, org.astype(dt), 2, backward=True)
        ref[dt] = (out, Lo)
    o64, L64 = ref[np.float64]
    o32, L32 = ref[np.float32]
    P = dict(model.named_parameters())
    keys = ['feature_extractor.backbone.conv1.weight', 'feature_extractor.backbone.layer1.0.downsample.0.weight',
            'feature_extractor.backbone.layer2.0.conv2.weight', 'feature_extractor.backbone.layer2.0.downsample.0.weight',
            'feature_extractor.backbone.layer3.5.conv2.weight', 'feature_extractor.backbone.layer3.22.bn3.weight',
            'feature_extractor.backbone.layer4.1.conv2.weight', 'feature_extractor.backbone.bn1.bias',
            'feature_extractor.aspp.branches.2.0.weight', 'SSSR_decoder.cat_conv.0.weight', 'SSSR_decoder.upsample16_pred.6.weight']
    report = {}
    e_hip, e_f32 = rel_err(host(outs[0]), o64.SSSR.v), rel_err(o32.SSSR.v, o64.SSSR.v)
    report['SSSR'] = (e_hip, e_f32)
    assert e_hip <= 5e-3 and e_hip <= 1.5 * e_f32 + 1e-4, report
    check(np.array([float(v) for v in L]), np.array(L64), 1e-3, 'losses')
    assert (host(outs[0]).argmax(1) == o64.SSSR.v.argmax(1)).mean() >= (o32.SSSR.v.argmax(1) == o64.SSSR.v.argmax(1)).mean() - 1e-3
    def l2(a, b):
        a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))

    for k in keys:
        e_hip, e_f32 = l2(host(P[k].grad), o64.params[k].g), l2(o32.params[k].g, o64.params[k].g)
        report[k.replace('feature_extractor.', '')] = (e_hip, e_f32)
        assert e_hip <= gslack * e_f32 + 1e-4, (k, e_hip, e_f32)
    names = [k for k in P if P[k].grad is not None and k in o64.params]
    cat = lambda f: np.concatenate([np.asarray(f(k), np.float64).ravel() for k in names])
    g_hip, g_64, g_32 = cat(lambda k: host(P[k].grad)), cat(lambda k: o64.params[k].g), cat(lambda k: o32.params[k].g)
    report['all gradients (L2)'] = (l2(g_hip, g_64), l2(g_32, g_64))
    assert report['all gradients (L2)'][0] <= 2.0 * report['all gradients (L2)'][1] + 1e-4, report['all gradients (L2)']
    print({k: f'hip {a:.1e} / f32-oracle {b:.1e}' for k, (a, b) in report.items()})


def test_full_model_total_loss_backward_with_fa_vs_oracle():
    """The WHOLE loss (CE + w1 MSE + w2 FA, train_or_resume.py:435-438) back-propagated through the assembled model at 128x256 input, B=2
    (feature-transformer maps 32x64 -> 8x8 similarity matrices), through the production loss path (functional.fused_losses: fused CE/MSE
    kernels, sparse transformer gradient accumulated into the published dense one) against the fp64 oracle, default (fp32-equivalent)
    arithmetic, with FIXED bounds: losses 1e-3, logits 5e-3 of their range; gradients in the L2 norm over the whole arena and for the head tensors.

    Two backward passes (round 5).  The FA term is an all-pairs L1 of two similarity matrices: its gradient w.r.t. an entry is a SUM OF SIGNS over 64 pairs
    (FALoss.py:27-34), so a near-tie that lands on the other side in fp32 changes that entry by 2 of <= 64 - a last-bit change of any forward sum (a
    different BatchNorm merge order, measured this round) moved the head gradients from 3e-4 to 9e-3 of the oracle with both builds exact to 1e-8 in
    their statistics.  So: (1) the smooth part, CE + w1 MSE with the FA weight at zero, at the tight bound (2e-3, measured 2-5e-4); (2) the whole loss
    at a bound that admits a few flipped pairs (3e-2) - a wrong FA backward (sign, normalisation, pooling) is an error of order 1, not 1e-2."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    torch.manual_seed(11)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
        model.SSSR_feature_transformer[1].bias.fill_(0.3); model.SISR_feature_transformer[1].bias.fill_(0.3)     # away from FALoss's all-zero NaN corner
    sd = {k: v.numpy() for k, v in model.state_dict().items() if 'num_batches' not in k}
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    rs = np.random.RandomState(1)
    x = rs.standard_normal((2, 3, 128, 256)).astype(np.float32)
    tg = rs.randint(0, 19, (2, 256, 512)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255
    org = rs.standard_normal((2, 3, 256, 512)).astype(np.float32)

    def l2(a, b):
        a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    heads = ('SSSR_feature_transformer.0.weight', 'SISR_feature_transformer.0.weight', 'SSSR_decoder.upsample16_pred.6.weight', 'SISR_decoder.0.weight')
    FA_FLIP_BOUND = 3e-2
    for w2, bound in ((0.0, HEAD_GRAD_BOUND), (1.0, FA_FLIP_BOUND)):
        for p_ in model.parameters():
            p_.grad = None
        bn_state = {k: v.clone() for k, v in model.state_dict().items() if 'running' in k}
        outs = model(dev(x, cl=False))
        model.load_state_dict(bn_state, strict=False)            # both passes see the same running statistics (they do not enter a training forward anyway)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        vals = HF.fused_losses(outs, dev(tg), dev(org), 255, 0.1, w2, 3, flag)
        vals[3].backward()
        out = O.model_forward({k: v.astype(np.float64) for k, v in sd.items()}, x.astype(np.float64), 3, True)
        L64 = O.total_loss(out, tg, org.astype(np.float64), 3, w2=w2, backward=True)
        assert out.SSSR_ft.v.shape == (2, 1, 32, 64)
        check(host(vals[:4]), np.array(L64), 1e-3, 'losses (CE, MSE, FA, total)')
        check(host(outs[0]), out.SSSR.v, 5e-3, 'logits')
        check(host(outs[2]), out.SSSR_ft.v, 5e-3, 'SSSR_ft'); check(host(outs[3]), out.SISR_ft.v, 5e-3, 'SISR_ft')
        P = dict(model.named_parameters())
        tensors = heads + ('SSSR_decoder.cat_conv.0.weight', 'feature_extractor.aspp.branches.5.0.weight', 'feature_extractor.backbone.layer4.2.conv3.weight',
                           'feature_extractor.backbone.layer1.0.conv1.weight')
        rep = {k: l2(host(P[k].grad), out.params[k].g) for k in tensors if P[k].grad is not None and float(np.abs(out.params[k].g).max()) > 0}
        names = [k for k in P if P[k].grad is not None and k in out.params]
        cat = lambda f: np.concatenate([np.asarray(f(k), np.float64).ravel() for k in names])      # noqa: E731
        rep['all gradients (L2)'] = l2(cat(lambda k: host(P[k].grad)), cat(lambda k: out.params[k].g))
        print('w2 =', w2, {k: '%.2e' % v for k, v in rep.items()})
        if w2 == 0.0:
            g0 = P['SSSR_feature_transformer.0.weight'].grad
            assert g0 is None or float(g0.abs().max()) == 0.0                                           # no FA weight: the transformers receive no gradient
        else:
            assert float(L64[2]) > 0 and 'SSSR_feature_transformer.0.weight' in rep
        for k in heads:
            if k in rep:
                assert rep[k] <= bound, (w2, k, rep[k])
        assert rep['all gradients (L2)'] <= ARENA_GRAD_BOUND, rep


def test_logits_gradient_formed_inside_the_producer_is_bit_identical_in_the_whole_step(monkeypatch):
    """HF.LogitsGrad (round 5): with the CE gradient formed inside the last ConvTranspose's backward (dsrl_convt2x2_bwd_ce) every parameter gradient of the
    whole model, stage 3 with the FA term and the feature transformer's sparse contribution, equals the path that writes d(CE)/d(logits) to memory -
    bit for bit (128x256 input: the layer sees W = 256, a multiple of the 128-pixel segment; dropout active, same Philox key in both passes)."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    torch.manual_seed(5)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        model.SSSR_feature_transformer[1].bias.fill_(0.3); model.SISR_feature_transformer[1].bias.fill_(0.3)
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    assert model.SSSR_decoder['upsample16_pred'][6].logits_layer
    rs = np.random.RandomState(2)
    x = dev(rs.standard_normal((2, 3, 128, 256)).astype(np.float32), cl=False)
    tg = rs.randint(0, 19, (2, 256, 512)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255
    org = dev(rs.standard_normal((2, 3, 256, 512)).astype(np.float32))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads, vals_ = {}, {}
    launches = {}
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    for on in (True, False, 'value'):
        monkeypatch.setattr(HF, 'convt_ce_enabled', bool(on))
        model.load_state_dict(state)
        for p_ in model.parameters():
            p_.grad = None
        HF.set_dropout_seed(77)
        counts = {}
        orig = HF.call

        def counting(name, *a, _c=counts, _o=orig):
            _c[name] = _c.get(name, 0) + 1
            return _o(name, *a)
        monkeypatch.setattr(HF, 'call', counting)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        tgd = dev(tg)
        if on == 'value':                        # the loss value too comes from the producer: its forward kernel evaluates it (HF.logits_target)
            with HF.logits_target(tgd, 255, flag):
                outs = model(x)
        else:
            outs = model(x)
        vals = HF.fused_losses(outs, tgd, org, 255, 0.1, 1.0, 3, flag)
        vals[3].backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(HF, 'call', orig)
        launches[on] = counts
        grads[on] = {k: p_.grad.clone() for k, p_ in model.named_parameters() if p_.grad is not None}
        vals_[on] = vals.clone()
    assert launches[True].get('dsrl_convt2x2_bwd_ce', 0) == 1 and launches[True].get('dsrl_convt2x2_bwd', 0) == 1, launches[True]
    assert launches[False].get('dsrl_convt2x2_bwd_ce', 0) == 0 and launches[False].get('dsrl_convt2x2_bwd', 0) == 2, launches[False]
    assert launches['value'].get('dsrl_convt2x2_fwd_ce', 0) == 1 and launches['value'].get('dsrl_ce_fused', 0) == 0 and launches['value'].get('dsrl_convt2x2_bwd_ce', 0) == 1
    assert launches[True].get('dsrl_ce_fused', 0) == 1
    assert torch.equal(vals_[True], vals_[False])
    check(host(vals_['value']), host(vals_[True]), 1e-6)            # the pixel losses are summed in another order
    assert grads[True].keys() == grads[False].keys() == grads['value'].keys()
    for other in (False, 'value'):
        bad = [k for k in grads[True] if not torch.equal(grads[True][k], grads[other][k])]
        assert not bad, (other, bad[:5])


def test_full_model_vs_stock_torch_fp64():
    """The assembled network (ResNet-101 OS16 + head + CE / MSE / FA) against an INDEPENDENT implementation of the same graph: stock torch.nn
    CPU modules in float64 (oracle/torch_cpu_model.py: the ATen arithmetic the reference's `--device cpu` path executes, itself pinned to the
    reference's full-width head vectors by tests/test_oracle_vs_golden.py).  The backbone has no reference fixture (torchvision's Bottleneck is
    absent), so this is its second, ATen-side pin next to the numpy oracle.  128x256 input, B=2, train-mode BN, dropout off; fixed bounds."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from oracle.torch_cpu_model import TorchCpuDSRL, total_loss
    torch.manual_seed(21)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
        model.SSSR_feature_transformer[1].bias.fill_(0.3); model.SISR_feature_transformer[1].bias.fill_(0.3)
    ref = TorchCpuDSRL(3)
    missing, unexpected = ref.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    ref = ref.double().train()
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    for net in (model, ref):
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
    rs = np.random.RandomState(2)
    x = rs.standard_normal((2, 3, 128, 256)).astype(np.float32)
    tg = rs.randint(0, 19, (2, 256, 512)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255
    org = rs.standard_normal((2, 3, 256, 512)).astype(np.float32)
    outs = model(dev(x, cl=False))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    vals = HF.fused_losses(outs, dev(tg), dev(org), 255, 0.1, 1.0, 3, flag)
    vals[3].backward()
    r_outs = ref(torch.from_numpy(x).double())
    r_L = total_loss(r_outs, torch.from_numpy(tg), torch.from_numpy(org).double(), 3)
    r_L[3].backward()
    check(host(vals[:4]), np.array([float(v.detach()) for v in r_L]), 1e-3, 'losses (CE, MSE, FA, total)')
    check(host(outs[0]), r_outs[0].detach().numpy(), 5e-3, 'logits')
    check(host(outs[1]), r_outs[1].detach().numpy(), 5e-3, 'SISR')
    assert (host(outs[0]).argmax(1) == r_outs[0].detach().numpy().argmax(1)).mean() > 0.999

    def l2(a, b):
        a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    P, R = dict(model.named_parameters()), dict(ref.named_parameters())
    rep = {k: l2(host(P[k].grad), R[k].grad.numpy()) for k in ('SSSR_decoder.upsample16_pred.6.weight', 'SISR_decoder.0.weight', 'SSSR_decoder.cat_conv.0.weight',
                                                              'feature_extractor.aspp.branches.5.0.weight', 'feature_extractor.backbone.layer4.2.conv3.weight',
                                                              'feature_extractor.backbone.layer2.0.downsample.0.weight', 'feature_extractor.backbone.conv1.weight')}
    names = [k for k in P if P[k].grad is not None]
    cat = lambda f: np.concatenate([np.asarray(f(k), np.float64).ravel() for k in names])
    rep['all gradients (L2)'] = l2(cat(lambda k: host(P[k].grad)), cat(lambda k: R[k].grad.numpy()))
    print({k: '%.2e' % v for k, v in rep.items()})
    assert rep['SSSR_decoder.upsample16_pred.6.weight'] <= HEAD_GRAD_BOUND and rep['SISR_decoder.0.weight'] <= HEAD_GRAD_BOUND, rep
    assert rep['all gradients (L2)'] <= ARENA_GRAD_BOUND, rep


@pytest.mark.parametrize('mode', ['f16x3', 'f16x1'])
def test_full_model_frozen_bn_every_gradient_vs_stock_torch_fp64(mode):
    """mode 'f16x1' (round 5): the arithmetic of apex O1 / O2 - ONE fp16 term per operand, 11 significand bits - held per
    gradient TENSOR in the same well-conditioned setting, instead of by the whole-arena cosine of the batch-statistics test above (which a wrong-sign
    weight gradient of a single layer would pass).  Bounds from the operand error: a conv output carries 2^-11 relative operand rounding averaged over its
    K-term dot product, measured 3e-4 of the output range per conv (test_conv_precision_modes); forward and backward each stack ~100 such layers with
    independent errors (x sqrt(100)), so a gradient tensor may sit at a few 1e-3 .. 1e-2 of its range: every tensor within 4e-2, 95 % within 1.5e-2,
    logits within 1e-2 (a sign error or a dropped term in one layer is an error of order 1 in that layer's tensor and of >= 1e-1 in everything behind it).

    The well-conditioned whole-model pin (round 3): BatchNorm frozen as train_or_resume.py:379-382 does with --freeze-batch-norm (every BN
    module in eval: running statistics, no batch-statistics terms in the backward pass), 128x256 input, B=2, stage 3.  Without the 2-image batch
    statistics of a random-init net the assembled 101-layer backward is no longer ill-conditioned, so EVERY gradient tensor is held to a FIXED
    bound against the fp64 stock-torch graph: 5e-3 of its own range, 95 % of the tensors 2e-3 (the self-calibrating bounds of
    test_full_model_vs_oracle stay for the batch-statistics case)."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from oracle.torch_cpu_model import TorchCpuDSRL, total_loss
    torch.manual_seed(33)
    model = D.DSRL(3, cs)
    rs = np.random.RandomState(4)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):        # running statistics of a "trained" net: non-trivial, well scaled
                m.running_mean.copy_(torch.from_numpy(rs.standard_normal(m.num_features).astype(np.float32) * 0.1))
                m.running_var.copy_(torch.from_numpy(rs.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
        model.SSSR_feature_transformer[1].bias.fill_(0.3); model.SISR_feature_transformer[1].bias.fill_(0.3)
    ref = TorchCpuDSRL(3)
    missing, unexpected = ref.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    ref = ref.double().train()
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    for net in (model, ref):
        for m in net.modules():
            if isinstance(m, (torch.nn.Dropout, torch.nn.modules.batchnorm._BatchNorm)):
                m.eval()                                                    # freeze_batch_norm (and dropout off, as in every parity run)
    x = rs.standard_normal((2, 3, 128, 256)).astype(np.float32)
    tg = rs.randint(0, 19, (2, 256, 512)).astype(np.uint8); tg[rs.uniform(size=tg.shape) < 0.1] = 255
    org = rs.standard_normal((2, 3, 256, 512)).astype(np.float32)
    x1 = mode == 'f16x1'
    HF.set_conv_precision(mode)
    try:
        outs = model(dev(x, cl=False))
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        vals = HF.fused_losses(outs, dev(tg), dev(org), 255, 0.1, 1.0, 3, flag)
        vals[3].backward()
        torch.cuda.synchronize()
    finally:
        HF.set_conv_precision(None)
    r_outs = ref(torch.from_numpy(x).double())
    r_L = total_loss(r_outs, torch.from_numpy(tg), torch.from_numpy(org).double(), 3)
    r_L[3].backward()
    # the feature-affinity term (differences of normalised similarity matrices of two one-channel maps) amplifies the 11-bit error most: 5e-2 for it
    check(host(vals[:4]), np.array([float(v.detach()) for v in r_L]), 5e-2 if x1 else 1e-4, 'losses (CE, MSE, FA, total)')
    check(host(vals[:2]), np.array([float(v.detach()) for v in r_L[:2]]), 3e-3 if x1 else 1e-4, 'losses (CE, MSE)')
    check(host(outs[0]), r_outs[0].detach().numpy(), 1e-2 if x1 else 1e-3, 'logits')
    if not x1:
        check_elementwise(host(outs[0]), r_outs[0].detach().numpy(), 1e-3, name='logits')
    assert (host(outs[0]).argmax(1) == r_outs[0].detach().numpy().argmax(1)).mean() > (0.995 if x1 else 0.9999)
    P, R = dict(model.named_parameters()), dict(ref.named_parameters())
    errs = {k: rel_err(host(P[k].grad), R[k].grad.numpy()) for k in P if P[k].grad is not None and R[k].grad is not None}
    assert len(errs) >= 350, len(errs)
    every, most = (4e-2, 1.5e-2) if x1 else (5e-3, 2e-3)
    bad = {k: '%.1e' % v for k, v in errs.items() if v > every}
    worst = max(errs.items(), key=lambda kv: kv[1])
    vs = np.sort(np.array(list(errs.values())))
    print(mode, 'gradient tensors', len(errs), 'worst', worst, 'median %.1e 95%% %.1e above %.0e: %d' % (vs[len(vs) // 2], vs[int(0.95 * len(vs))], most, int((vs > most).sum())))
    # fixed bounds.  f16x3: every one of the 350+ tensors within 5e-3 of its range, 95 % of them within 2e-3 (measured: 2 tensors above 2e-3, worst 4.1e-3 -
    # one fp32 pass through 101 layers against float64); f16x1: 4e-2 / 1.5e-2 (docstring)
    assert not bad, bad
    assert vs[int(0.95 * len(vs))] <= most, vs[int(0.95 * len(vs))]
    if x1:
        # direction per tensor: a flipped sign or a missing term shows as a cosine far from 1 in exactly that tensor
        cos = {k: float(np.dot(host(P[k].grad).ravel().astype(np.float64), R[k].grad.numpy().ravel()) /
                        max(np.linalg.norm(host(P[k].grad).ravel().astype(np.float64)) * np.linalg.norm(R[k].grad.numpy().ravel()), 1e-300)) for k in errs}
        low = {k: '%.4f' % v for k, v in cos.items() if v < 0.995 and np.linalg.norm(R[k].grad.numpy().ravel()) > 0}
        assert not low, low


def test_train_or_resume_end_to_end(tmp_path):
    """The reference's entry point (command_handlers/train_or_resume.py:24-26 signature): two epochs on synthetic batches, a
    checkpoint in the reference's dict format, final.weights, then a resume that continues from the checkpoint."""
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, train_or_resume
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd import settings

    def factory(split, batch_size, device, rank, world):
        return SyntheticCityscapes(batch_size, (32, 64), device, rank=rank, length=2)

    kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
              dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': factory}, val_interval=1, checkpoint_interval=1,
              checkpoint_history=2, init_weights=None, batch_size=2, epochs=2, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9,
              weights_decay=5e-4, poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / 'exp'),
              description='test', early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))
    hist = train_or_resume(is_resuming_training=False, **kw)
    assert len(hist) == 3 and all(np.isfinite(v) for h in hist[:2] for v in h['train'][:4])
    assert abs(hist[1]['lr'] - ((0.006 - 0.0005) * (1 - 1 / 2) ** 0.9 + 0.0005)) < 1e-12 and 'val' in hist[0] and 0 <= hist[0]['val'][4] <= 100
    ckdir = os.path.join(str(tmp_path / 'exp'), settings.CHECKPOINTS_DIR.format(stage=3))
    ck = torch.load(os.path.join(ckdir, settings.CHECKPOINT_FILE.format(epoch=2)), map_location='cpu', weights_only=False)
    assert ck['epoch'] == 2 and ck['stage'] == 3 and len(ck['model_state_dict']) == 702
    # the reference reads back every key of settings.VARIABLES_IN_CHECKPOINT (main.py:51-52) and feeds optimizer_state_dict to torch.optim.SGD
    assert set(ck) == set(settings.VARIABLES_IN_CHECKPOINT)
    stock = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros_like(v)) for k, v in ck['model_state_dict'].items()
                                    if not any(s_ in k for s_ in ('running_', 'num_batches'))])
    opt = torch.optim.SGD(stock, lr=0.1, momentum=0.9)
    opt.load_state_dict(ck['optimizer_state_dict'])                    # torch's own loader accepts the layout
    assert len(opt.state_dict()['state']) == len(stock) and opt.param_groups[0]['momentum'] == 0.9 and opt.param_groups[0]['weight_decay'] == 5e-4
    names = sorted(os.listdir(ckdir))
    assert settings.CHECKPOINT_FILE.format(epoch=1) in names and any(n.endswith('_bestval.checkpoint') for n in names) == (ck['best_validation_dict']['epoch'] > 0), names
    fw = torch.load(os.path.join(str(tmp_path / 'exp'), settings.WEIGHTS_DIR.format(stage=3), settings.FINAL_WEIGHTS_FILE), map_location='cpu', weights_only=False)
    assert set(fw) == {'model_state_dict', 'mixed_precision', 'amp_state_dict'}
    kw['epochs'] = 3
    hist2 = train_or_resume(is_resuming_training=True, model_state_dict=ck['model_state_dict'], optimizer_state_dict=ck['optimizer_state_dict'],
                            epoch=ck['epoch'], best_validation_dict=ck['best_validation_dict'], **kw)
    assert hist2[0]['epoch'] == 3
    # checkpoint_history = 2, interval 1: writing epoch 3 prunes epoch 1 (train_or_resume.py:285-291); only one *_bestval file at a time
    names = sorted(os.listdir(ckdir))
    assert settings.CHECKPOINT_FILE.format(epoch=1) not in names and settings.CHECKPOINT_FILE.format(epoch=3) in names, names
    assert sum(n.endswith('_bestval.checkpoint') for n in names) <= 1
    # the momentum buffers really travelled: a resume from the SGD-layout state equals the state the first run ended epoch 2 with
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    m2 = D.DSRL(3, cs); m2.load_state_dict(ck['model_state_dict']); m2 = m2.to(DEV).to(memory_format=torch.channels_last)
    f2 = FlatParams(m2); f2.load_state_dict(ck['optimizer_state_dict'])
    assert float(f2.m_flat.abs().sum()) > 0
    rt = f2.state_dict(0.1, 0.9, 5e-4)
    for i, st in ck['optimizer_state_dict']['state'].items():
        assert torch.equal(rt['state'][i]['momentum_buffer'], st['momentum_buffer']), i
    # apex opt levels map onto the conv arithmetic (BASELINE config 5's reduced-precision path) and do not leak out of the call
    kw.update(epochs=1, mixed_precision='O2', experiment_id=str(tmp_path / 'exp_o2'))
    hist3 = train_or_resume(is_resuming_training=False, **kw)
    assert np.isfinite(hist3[0]['train'][3]) and HF.get_conv_precision() == 'f16x3'


def test_seg_metrics_golden(golden):
    """On-device mIoU / accuracy (dsrl_seg_metrics, argmax fused) vs the reference's metrices classes."""
    from dualsuperreslearningforsemseg_amd.metrices import Accuracy, mIoU
    g = golden('pipeline_metrics')
    m, a, m2 = mIoU(19), Accuracy(19), mIoU(19)
    rs = np.random.RandomState(1)
    for b in range(3):
        pred, target = g[f'metrics.pred{b}'], g[f'metrics.target{b}']
        logits = rs.uniform(0, 1, (2, 19, 24, 40)).astype(np.float32)
        np.put_along_axis(logits, pred[:, None].astype(np.int64), 2.0, axis=1)            # argmax(logits) == pred
        m.update_from_logits(dev(logits), dev(target)); a.update_from_logits(dev(logits), dev(target))
        m2.update(dev(pred.astype(np.int64)), dev(target), dev(target != 255))             # the reference's (pred, target, mask) call shape
    assert abs(m() - float(g['metrics.miou'])) < 1e-9 and abs(a() - float(g['metrics.acc'])) < 1e-9 and abs(m2() - float(g['metrics.miou'])) < 1e-9


def test_prepare_batch_golden(golden):
    """Device-side ToTensor+Normalize+label remap+dual-scale resize vs the reference's JointScaledImage output."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.models.transforms import DeviceBatchPreparation
    g = golden('pipeline_metrics')
    prep = DeviceBatchPreparation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, (16, 32))
    (img_in, img_org), (target, _) = prep(dev(g['prep.rgb']), dev(g['prep.labels']))
    check(host(img_in), g['prep.img_in'], 1e-5, 'img_in'); check(host(img_org), g['prep.img_org'], 1e-5, 'img_org')
    assert np.array_equal(host(target.float()).astype(np.uint8), g['prep.target'])
    assert img_in.shape == (2, 3, 16, 32) and HF._ld_of(img_in) == 4          # padded to the 4 channels the stem kernel reads

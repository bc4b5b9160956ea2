"""The float64 references of tests/spatial_ref.py against stock torch on the CPU, on the inputs and shapes test_spatial_edges_gpu.py uses, so that
a kernel that matches the references matches torch.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as O
import spatial_ref as R

POOL_SIZES = [(1, 1), (1, 7), (2, 2), (3, 3), (7, 10), (16, 9), (33, 34)]
BILINEAR_SHAPES = [((2, 2), (65, 33)), ((5, 7), (13, 9)), ((13, 9), (5, 7)), ((33, 17), (4, 3)), ((9, 13), (9, 13)), ((7, 5), (1, 1)),
                   ((8, 6), (1, 11)), ((1, 1), (4, 8)), ((3, 64), (6, 127))]


@pytest.mark.parametrize('kind', R.MAXPOOL_KINDS)
@pytest.mark.parametrize('hw', POOL_SIZES)
def test_max_pool_reference_and_oracle_are_torch(kind, hw):
    """values, recorded indices and the gradient of F.max_pool2d(3, 2, 1) in float64; the oracle's numpy pool on the same inputs"""
    H, W = hw
    rs = np.random.RandomState(1000 * H + W)
    x = R.maxpool_input(kind, (2, 5, H, W), rs)
    dy = R.integer_grad(rs, (2, 5, R.pool_out(H), R.pool_out(W)))
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    yt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    yt.backward(torch.from_numpy(dy.astype(np.float64)))
    for name, M in (('reference', R), ('oracle', O)):
        y, tap = M.max_pool3x3s2(x.astype(np.float64))
        assert np.array_equal(y, yt.detach().numpy(), equal_nan=True), name
        assert np.array_equal(R.tap_to_flat_index(tap, H, W), it.numpy()), name
        assert np.array_equal(M.max_pool3x3s2_bwd((H, W), tap, dy.astype(np.float64)), xt.grad.numpy()), name


def test_max_pool_all_minus_inf_map_sends_the_gradient_to_the_first_in_bounds_element():
    """the case an argmax over a -inf padded window gets wrong: indices [[0, 1], [4, 5]] on a 4x4 map, and the gradient arrives"""
    x = np.full((1, 1, 4, 4), -np.inf, np.float32)
    for y, tap in (R.max_pool3x3s2(x), O.max_pool3x3s2(x.astype(np.float64))):
        assert np.array_equal(R.tap_to_flat_index(tap, 4, 4)[0, 0], [[0, 1], [4, 5]]) and np.isneginf(y).all()
        assert R.max_pool3x3s2_bwd((4, 4), tap, np.ones((1, 1, 2, 2))).sum() == 4.0
        assert O.max_pool3x3s2_bwd((4, 4), tap, np.ones((1, 1, 2, 2))).sum() == 4.0


@pytest.mark.parametrize('shape', BILINEAR_SHAPES, ids=lambda s: f'{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}')
def test_bilinear_matrices_are_torch_float32_interpolate(shape):
    """A x B^T and A^T dy B against F.interpolate(align_corners=True) in float32.  The matrices hold torch's own float32 coordinates, so the
    difference is torch's blend rounding: a few ulp of the magnitude |A| |x| |B|^T forward; the backward scatters up to T float32 terms
    into one element in any order, (T + 4) ulp of |A|^T |dy| |B|."""
    (H, W), (Ho, Wo) = shape
    rs = np.random.RandomState(H * 1000 + Wo)
    x = rs.standard_normal((2, 3, H, W)).astype(np.float32)
    dy = rs.standard_normal((2, 3, Ho, Wo)).astype(np.float32)
    A, B = R.bilinear_matrices(H, W, Ho, Wo)
    assert np.allclose(A.sum(1), 1.0, atol=1e-15) and np.allclose(B.sum(1), 1.0, atol=1e-15) and (A >= 0).all() and (B >= 0).all()
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = F.interpolate(xt, size=(Ho, Wo), mode='bilinear', align_corners=True)
    yt.backward(torch.from_numpy(dy))
    u = 2.0 ** -24
    e = np.abs(R.bilinear_fwd(A, B, x) - yt.detach().numpy())
    assert (e <= 8 * u * R.bilinear_fwd(np.abs(A), np.abs(B), np.abs(x))).all(), e.max()
    e = np.abs(R.bilinear_bwd(A, B, dy) - xt.grad.numpy())
    assert (e <= (R.max_taps(A, B) + 4) * u * R.bilinear_bwd(np.abs(A), np.abs(B), np.abs(dy))).all(), e.max()
    if (H, W) == (Ho, Wo):
        assert np.array_equal(A, np.eye(H)) and np.array_equal(B, np.eye(W))


@pytest.mark.parametrize('lr,momentum,wd,scale', [(0.006, 0.9, 5e-4, 1.0), (0.01, 0.0, 0.0, 0.125), (0.1, 0.9, 0.0, 3.0)])
def test_sgd_reference_is_torch_optim_sgd(lr, momentum, wd, scale):
    """two steps of torch.optim.SGD in float64 on the scaled gradient, from a non-zero momentum buffer"""
    rs = np.random.RandomState(7)
    p0, b0 = rs.standard_normal(1027), rs.standard_normal(1027)
    gs = [rs.standard_normal(1027), rs.standard_normal(1027)]
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([pt], lr=lr, momentum=momentum, weight_decay=wd)
    if momentum:
        opt.state[pt]['momentum_buffer'] = torch.from_numpy(b0.copy())
    p, b = p0, b0
    for g in gs:
        pt.grad = torch.from_numpy(g * scale)
        opt.step()
        p, b = R.sgd_step(p, g, b, lr, momentum, wd, scale)
        assert np.allclose(p, pt.detach().numpy(), rtol=1e-14, atol=1e-15)
        if momentum:
            assert np.allclose(b, opt.state[pt]['momentum_buffer'].numpy(), rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize('C', [19, 3])
def test_seg_counts_is_the_oracle_metric_on_argmax_maps(C):
    """mean IoU and accuracy formed from the table equal oracle.seg_metrics_batch on the first-maximum class map (labels inside the classes or
    ignored: the reference metric has no notion of other labels); tied rows go to the lowest class; labels >= C count nowhere"""
    rs = np.random.RandomState(C)
    P = 4099
    lg = (np.round(2.0 * rs.standard_normal((P, C))).clip(-2, 2) / 2.0).astype(np.float32)
    lg[::7] = 0.25
    tg = rs.randint(0, C, P)
    tg[rs.uniform(size=P) < 0.1] = 255
    t = R.seg_counts(lg, tg, C, 255)
    pred = np.array([int(np.flatnonzero(row == row.max())[0]) for row in lg])
    assert (pred[::7] == 0).all()
    miou, acc = O.seg_metrics_batch(pred, tg, C, 255)
    inter, union = t[C:2 * C], t[:C] + t[2 * C:3 * C] - t[C:2 * C]
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.isclose(np.nanmean(inter / union), miou, rtol=1e-13) and np.isclose(t[3 * C] / t[3 * C + 1], acc, rtol=1e-13)
    assert t[:C].sum() == t[2 * C:3 * C].sum() == t[3 * C + 1] == (tg != 255).sum() and t[C:2 * C].sum() == t[3 * C]
    tg2 = tg.copy(); tg2[::5] = 200
    live = (tg2 != 255) & (tg2 != 200)
    assert np.array_equal(R.seg_counts(lg, tg2, C, 255), R.seg_counts(lg[live], tg2[live], C, 255))
    wide = np.concatenate([lg, np.full((P, 24 - C), 1e30, np.float32)], axis=1)
    assert np.array_equal(R.seg_counts(wide, tg, C, 255), t)
    assert not R.seg_counts(lg, np.full(P, 255), C, 255).any()

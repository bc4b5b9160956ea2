"""Reference of dsrl_sr_quality (include/dsrl_hip.h) for test_sr_quality_host.py and test_sr_quality_gpu.py, numpy only.

Semantics, as the header states them: every value is de-normalised in float32 as v = x * std[c] + mean[c] (a product, then a sum: two roundings)
and clamped to [0, 1] by comparisons, so that a NaN stays one.  sse = sum over all C*H*W values of (vp - vr)^2.  SSIM is the single-scale index of
Wang et al. at data range 1: the 11-tap window g[k] = exp(-(k - 5)^2 / 4.5), normalised in float64 and rounded to float32, applied separably (rows,
then columns) to x, y, x*x, x*y, y*y over the valid region (H-10) x (W-10) of each channel; per pixel
((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sxx + syy + C2)) with sab = E[ab] - ma mb, C1 = float32(1e-4), C2 = float32(9e-4).

reference64: the de-normalisation in float32, as the kernel does it, then everything in float64 (with the same eleven float32 taps).
restatement32: the same formula in float32 throughout, row pass then column pass, taps in ascending order, every product and sum rounded - what a
straightforward fp32 implementation gives; its distance from reference64 is the yardstick the kernel's error is measured with."""
import numpy as np

F32, F64 = np.float32, np.float64
WIN = 11
C1, C2 = F32(1e-4), F32(9e-4)


def window():
    """the eleven float32 taps"""
    k = np.arange(WIN, dtype=F64)
    g = np.exp(-(k - 5.0) ** 2 / 4.5)
    return (g / g.sum()).astype(F32)


def denormalise(x, mean=None, std=None):
    """(N,C,H,W) float32 -> float32 values in [0, 1], NaN kept"""
    x = np.asarray(x, F32)
    C = x.shape[1]
    mean = np.zeros(C, F32) if mean is None else np.asarray(mean, F32)
    std = np.ones(C, F32) if std is None else np.asarray(std, F32)
    v = (x * std.reshape(1, C, 1, 1)).astype(F32)
    v = (v + mean.reshape(1, C, 1, 1)).astype(F32)
    v = np.where(v < 0, F32(0), v)
    v = np.where(v > 1, F32(1), v)
    return v.astype(F32)


def filter_valid(a, g, axis):
    """valid correlation of `a` with the taps `g` along `axis`, taps ascending, in a's dtype (g is cast to it): out[i] = sum_k g[k] a[i + k]"""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1] - (WIN - 1)
    g = g.astype(a.dtype)
    out = g[0] * a[..., 0:n]
    for k in range(1, WIN):
        out = out + g[k] * a[..., k:k + n]
    return np.moveaxis(out.astype(a.dtype), -1, axis)


def _ssim_map(x, y, dtype):
    """x, y (N,C,H,W) of `dtype` -> the map (N,C,H-10,W-10) with every operation in `dtype`"""
    g = window()
    c1, c2, two = dtype(C1), dtype(C2), dtype(2)
    blur = lambda a: filter_valid(filter_valid(a, g, 3), g, 2)      # rows (along W), then columns (along H)
    mx, my = blur(x), blur(y)
    exx, exy, eyy = blur(x * x), blur(x * y), blur(y * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, sxy, syy = exx - mxx, exy - mxy, eyy - myy
    with np.errstate(invalid='ignore', divide='ignore'):
        out = ((two * mxy + c1) * (two * sxy + c2)) / (((mxx + myy) + c1) * ((sxx + syy) + c2))
    assert out.dtype == dtype
    return out


def reference64(pred, ref, mean=None, std=None):
    """-> dict: 'sse' (N,), 'ssim_map' (N,C,H-10,W-10), 'ssim_sum' (N,), all float64"""
    vp, vr = denormalise(pred, mean, std).astype(F64), denormalise(ref, mean, std).astype(F64)
    m = _ssim_map(vp, vr, F64)
    return {'sse': ((vp - vr) ** 2).sum(axis=(1, 2, 3)), 'ssim_map': m, 'ssim_sum': m.sum(axis=(1, 2, 3))}


def restatement32(pred, ref, mean=None, std=None):
    """-> the map (N,C,H-10,W-10) in float32 arithmetic throughout"""
    return _ssim_map(denormalise(pred, mean, std), denormalise(ref, mean, std), F32)


def figures(sse, ssim_sum, C, H, W):
    """-> (psnr dB, ssim) per image in float64"""
    with np.errstate(divide='ignore', invalid='ignore'):
        psnr = 10.0 * np.log10(F64(C * H * W) / np.asarray(sse, F64))
    return psnr, np.asarray(ssim_sum, F64) / F64(C * (H - WIN + 1) * (W - WIN + 1))


# ---------------------------------------------------------------------------------------------- the inputs both test files use
MEAN, STD = (0.28690, 0.32513, 0.28389, 0.3), (0.17614, 0.18099, 0.17772, 0.2)        # Cityscapes' three, and a fourth for C = 4
KINDS = ('noisy_copy', 'independent', 'complement', 'bright_flat', 'constants', 'normalised')


def make_case(kind, shape, seed=0):
    """-> (pred, ref, mean, std): float32 (N,C,H,W) arrays and the normalisation (None, None: values in [0, 1])"""
    rs = np.random.RandomState((seed * 7919 + sum(ord(ch) for ch in kind) * 31 + int(np.prod(shape))) % (2 ** 31))
    C = shape[1]
    if kind == 'noisy_copy':
        a = rs.uniform(0, 1, shape)
        return (a + rs.normal(0, 0.05, shape)).astype(F32), a.astype(F32), None, None
    if kind == 'independent':
        return rs.uniform(0, 1, shape).astype(F32), rs.uniform(0, 1, shape).astype(F32), None, None
    if kind == 'complement':
        a = rs.uniform(0, 1, shape).astype(F32)
        return a, (F32(1) - a).astype(F32), None, None
    if kind == 'bright_flat':           # the cancellation-heavy case: variances of 1e-6 taken as differences of moments near 0.96
        a = 0.98 + rs.uniform(-1e-3, 1e-3, shape)
        return (a + rs.uniform(-1e-3, 1e-3, shape)).astype(F32), a.astype(F32), None, None
    if kind == 'constants':
        return np.full(shape, 0.3, F32), np.full(shape, 0.7, F32), None, None
    if kind == 'normalised':            # N(0, 2.5^2) in normalised units: far more than a tenth of the values leave [0, 1]
        return (rs.normal(0, 2.5, shape)).astype(F32), (rs.normal(0, 2.5, shape)).astype(F32), MEAN[:C], STD[:C]
    raise KeyError(kind)

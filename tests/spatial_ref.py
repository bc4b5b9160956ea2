"""The memory-bound spatial operators, the SGD update and the validation counters of this project restated in float64 on the CPU, in the plainest
form that has torch's semantics (tests/test_spatial_refs_host.py holds every function against stock torch).  Logical NCHW numpy arrays throughout.

max pool 3x3 / stride 2 / pad 1 (torch max_pool2d on the CPU): the window is scanned row-major over its in-bounds taps only; the scan starts AT the
first in-bounds tap (its index is the answer when nothing beats -inf) and a later tap replaces the best on `v > best or isnan(v)`: the first of tied
maxima wins, the last of several NaNs wins, an all -inf window sends its gradient to its first in-bounds element.  The recorded tap is r * 3 + s.

align-corners bilinear resize: y = A x B^T per (n, c) plane with the two 1-D interpolation matrices A (Ho, H), B (Wo, W).  The source coordinates
(scale, scale * dst, the split into index and fraction) are evaluated in float32 exactly as torch float32 and the kernels define them
(oracle._ac_coords); everything after that - 1 - l, the products, the sums - is float64."""
import numpy as np

from oracle.dsrl_oracle import _ac_coords

F64 = np.float64


# ------------------------------------------------------------------------------------------------ max pool
def pool_out(n):
    return (n - 1) // 2 + 1


def _taps(H, W):
    """per tap t = r * 3 + s: (r, s, in-bounds mask (Ho, Wo))"""
    Ho, Wo = pool_out(H), pool_out(W)
    ho, wo = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    for r in range(3):
        for s in range(3):
            h, w = 2 * ho - 1 + r, 2 * wo - 1 + s
            yield r, s, (h >= 0) & (h < H) & (w >= 0) & (w < W)


def max_pool3x3s2(x):
    """x (N, C, H, W) -> (y float64 (N, C, Ho, Wo), tap int64 (N, C, Ho, Wo))"""
    x = np.asarray(x).astype(F64)
    N, C, H, W = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = np.zeros((N, C, 2 * Ho + 1, 2 * Wo + 1), F64)       # the padding's value is never looked at: the masks keep it out
    xp[:, :, 1:H + 1, 1:W + 1] = x
    best = np.full((N, C, Ho, Wo), -np.inf)
    tap = np.full((N, C, Ho, Wo), -1, np.int64)
    for r, s, inb in _taps(H, W):
        v = xp[:, :, r:r + 2 * Ho:2, s:s + 2 * Wo:2]
        with np.errstate(invalid='ignore'):
            take = inb & ((tap < 0) | (v > best) | np.isnan(v))
        best = np.where(take, v, best)          # at the scan's start a tap that beats nothing is -inf itself
        tap = np.where(take, r * 3 + s, tap)
    assert (tap >= 0).all()
    return best, tap


def max_pool3x3s2_bwd(in_hw, tap, dy):
    """dx (N, C, H, W) float64: every window's dy goes to the tap its forward pass recorded"""
    H, W = in_hw
    dy = np.asarray(dy).astype(F64)
    N, C, Ho, Wo = dy.shape
    dxp = np.zeros((N, C, 2 * Ho + 1, 2 * Wo + 1), F64)
    for r, s, _ in _taps(H, W):
        dxp[:, :, r:r + 2 * Ho:2, s:s + 2 * Wo:2] += np.where(tap == r * 3 + s, dy, 0.0)
    return dxp[:, :, 1:H + 1, 1:W + 1]


def tap_to_flat_index(tap, H, W):
    """the recorded taps as torch's return_indices (h * W + w of the input plane)"""
    Ho, Wo = tap.shape[2:]
    ho, wo = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    return (2 * ho - 1 + tap // 3) * W + (2 * wo - 1 + tap % 3)


def quantised_normal(rs, shape):
    """standard normal rounded to multiples of 0.5: a 3x3 window of it nearly always holds its maximum more than once"""
    return (np.round(2.0 * rs.standard_normal(shape)) / 2.0).astype(np.float32)


MAXPOOL_KINDS = ('ties', 'const', 'inf', 'nan')


def maxpool_input(kind, shape, rs):
    """The edge inputs of the max-pool tests -> float32 (N, C, H, W).
    ties:  ReLU of a quantised normal, the pool's input in the model: most windows hold several zeros or several equal maxima.
    const: one value everywhere: every window is a tie of all its taps.
    inf:   planes that are -inf throughout, planes with a -inf patch over the top-left (border and interior windows) or the bottom-right corner,
           and isolated +inf.
    nan:   isolated NaNs, and planes with a 2x2 NaN block in the corner and a 3x3 one inside (several NaNs in one window)."""
    N, C, H, W = shape
    if kind == 'ties':
        return np.maximum(quantised_normal(rs, shape), 0.0).astype(np.float32)
    if kind == 'const':
        return np.full(shape, -1.5, np.float32)
    x = quantised_normal(rs, shape)
    for n in range(N):
        for c in range(C):
            k = (n + c) % 3
            if kind == 'inf':
                if k == 0:
                    x[n, c] = -np.inf
                elif k == 1:
                    x[n, c, :5, :6] = -np.inf
                    x[n, c, H // 2, W // 2] = np.inf
                else:
                    x[n, c, max(H - 4, 0):, max(W - 5, 0):] = -np.inf
                    x[n, c, 0, W - 1] = np.inf
            else:
                x[n, c][rs.uniform(size=(H, W)) < 0.04] = np.nan
                if k == 0:
                    x[n, c, :2, :2] = np.nan
                elif k == 1:
                    x[n, c, H // 2:H // 2 + 3, W // 3:W // 3 + 3] = np.nan
    return x


def integer_grad(rs, shape):
    """integer-valued upstream gradient: every sum of up to four of them is exact in float32"""
    return rs.randint(-8, 9, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ bilinear
def interp_matrix(n_in, n_out):
    """(n_out, n_in) float64 align-corners interpolation matrix from float32 source coordinates"""
    i0, i1, l1 = _ac_coords(n_in, n_out, np.dtype('float32'))
    l1 = l1.astype(F64)
    A = np.zeros((n_out, n_in), F64)
    o = np.arange(n_out)
    np.add.at(A, (o, i0), 1.0 - l1)
    np.add.at(A, (o, i1), l1)
    return A


def bilinear_matrices(H, W, Ho, Wo):
    """-> A (Ho, H), B (Wo, W)"""
    return interp_matrix(H, Ho), interp_matrix(W, Wo)


def bilinear_fwd(A, B, x):
    """A x B^T per plane; with |A|, |B|, |x| the magnitude the rounding errors scale with"""
    return np.einsum('oh,nchw,pw->ncop', A, np.asarray(x).astype(F64), B, optimize=True)


def bilinear_bwd(A, B, dy):
    """A^T dy B per plane"""
    return np.einsum('oh,ncop,pw->nchw', A, np.asarray(dy).astype(F64), B, optimize=True)


def max_taps(A, B):
    """T of the backward bound: the longest gather along H plus the longest along W"""
    return int((A != 0).sum(0).max() + (B != 0).sum(0).max())


# ------------------------------------------------------------------------------------------------ SGD
def sgd_step(p, g, buf, lr, momentum, weight_decay, grad_scale=1.0):
    """torch.optim.SGD(momentum, weight_decay) with dampening 0, no nesterov and an existing momentum buffer, on the gradient g * grad_scale.
    -> (p, buf) float64"""
    p, g, buf = (np.asarray(a).astype(F64) for a in (p, g, buf))
    d = g * F64(grad_scale) + F64(weight_decay) * p
    buf = F64(momentum) * buf + d
    return p - F64(lr) * buf, buf


# ------------------------------------------------------------------------------------------------ validation counters
def seg_counts(logits, target, C, ignore):
    """logits (P, >= C) (only the first C columns are scores), target (P,) -> int64 [area_pred (C) | area_inter (C) | area_target (C) | correct, valid].
    The prediction is the FIRST maximum of a row; pixels labelled `ignore` or >= C count nowhere."""
    lg = np.asarray(logits)[:, :C].astype(F64)
    t = np.asarray(target).astype(np.int64).reshape(-1)
    live = (t != ignore) & (t < C)
    pred, t = lg[live].argmax(axis=1), t[live]
    out = np.zeros(3 * C + 2, np.int64)
    out[:C] = np.bincount(pred, minlength=C)
    out[C:2 * C] = np.bincount(t[pred == t], minlength=C)
    out[2 * C:3 * C] = np.bincount(t, minlength=C)
    out[3 * C], out[3 * C + 1] = int((pred == t).sum()), int(live.sum())
    return out

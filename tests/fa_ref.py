"""Plain float64 references of the loss kernels between the cross-entropy family and the SGD tail of csrc/losses.hip: the feature-affinity loss
(FALoss) for any (B, C, H, W), subsample factor and reduction, the MSE value and gradient, the five loss_mix outputs and the NaN flag; and the
case table tests/test_loss_edges_gpu.py and tests/test_fa_ref_host.py share, so that both see the same inputs.

FALoss, as the kernels compute it: X = floor k x k average pooling of one (b, c) slice, G = X^T X, lambda = the largest eigenvalue of G
(= sigma_1(X)^2, so S = G / lambda is the original module's (X / ||X||_2)^T (X / ||X||_2)), and the loss is the L1 distance between EVERY entry of S1
and EVERY entry of S2: 'none'[b, c, i * n + j] = |S1_i - S2_j| (repeat_interleave against repeat, n = (W // k)^2)."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = np.float64
U = 2.0 ** -24                      # unit roundoff of float32
GAP_FLOOR = 2e-5                    # a gradient case is valid only if every |S1_i - S2_j| is at least this (see min_gap)


# ------------------------------------------------------------------------------------------------ FA loss, numpy
def pool(f, k):
    """floor average pooling in float64: rows and columns past (H // k) * k, (W // k) * k take no part"""
    f = np.asarray(f, F64)
    B, C, H, W = f.shape
    hp, wp = H // k, W // k
    return f[:, :, :hp * k, :wp * k].reshape(B, C, hp, k, wp, k).sum((3, 5)) / float(k * k)


def gram(X):
    G = np.einsum('bcia,bcid->bcad', X, X)
    return 0.5 * (G + np.swapaxes(G, -1, -2))      # exactly symmetric: S_ab and S_ba tie exactly, as they do in the kernel


def top_eigenvalue(G):
    """(B, C) largest eigenvalue per slice; NaN for a slice with a non-finite entry (the original module divides the whole map by a NaN norm)"""
    lam = np.full(G.shape[:2], np.nan)
    for b in range(G.shape[0]):
        for c in range(G.shape[1]):
            if np.isfinite(G[b, c]).all():
                lam[b, c] = np.linalg.eigvalsh(G[b, c])[-1]
    return lam


def similarity(f, k):
    """S (B, C, n) in float64; 0 / 0 = NaN for an all-zero slice like the original module"""
    G = gram(pool(f, k))
    with np.errstate(divide='ignore', invalid='ignore'):
        S = G / top_eigenvalue(G)[:, :, None, None]
    return S.reshape(S.shape[0], S.shape[1], -1)


def fa_loss(f1, f2, k=8, reduction='mean'):
    assert f1.ndim == 4 and f1.shape == f2.shape
    S1, S2 = similarity(f1, k), similarity(f2, k)
    d = np.abs(S1[:, :, :, None] - S2[:, :, None, :])
    if reduction == 'mean':
        return d.mean()
    if reduction == 'sum':
        return d.sum()
    assert reduction == 'none'
    return d.reshape(d.shape[0], d.shape[1], -1)


def min_gap(f1, f2, k):
    """the smallest |S1_i - S2_j| over all pairs of all slices: with it above the float32 error of S every sign of the backward pass is determined"""
    S1, S2 = similarity(f1, k), similarity(f2, k)
    return float(np.abs(S1[:, :, :, None] - S2[:, :, None, :]).min())


# ------------------------------------------------------------------------------------------------ FA loss, torch
def _pool_t(x, k):
    B, C, H, W = x.shape
    hp, wp = H // k, W // k
    return x[:, :, :hp * k, :wp * k].reshape(B, C, hp, k, wp, k).sum((3, 5)) / float(k * k)


def fa_loss_torch64(f1, f2, k=8, reduction='mean'):
    """the formula of fa_loss in float64 torch (autograd gives the reference gradients); f1, f2 float64 tensors"""
    def sim(x):
        X = _pool_t(x, k)
        G = X.transpose(-1, -2) @ X
        G = 0.5 * (G + G.transpose(-1, -2))
        return (G / torch.linalg.eigvalsh(G)[..., -1][..., None, None]).flatten(2)
    d = (sim(f1)[:, :, :, None] - sim(f2)[:, :, None, :]).abs()
    return d.mean() if reduction == 'mean' else d.sum() if reduction == 'sum' else d.flatten(2)


def fa_loss_stock(f1, f2, k=8, reduction='mean'):
    """the original module's formula on stock torch ops in the dtype of its inputs: average pooling, division by the spectral norm, X^T X,
    repeat_interleave against repeat, l1_loss"""
    def sim(x):
        x = F.avg_pool2d(x, k)
        x = x / torch.linalg.matrix_norm(x, ord=2, dim=(-2, -1), keepdim=True)
        return (x.transpose(-2, -1) @ x).flatten(2)
    s1, s2 = sim(f1), sim(f2)
    n = s1.shape[-1]
    return F.l1_loss(s1.repeat_interleave(n, dim=2), s2.repeat(1, 1, n), reduction=reduction)


def _grads(fn, f1, f2, k, reduction, root, dtype):
    a = torch.from_numpy(np.ascontiguousarray(f1)).to(dtype).requires_grad_(True)
    b = torch.from_numpy(np.ascontiguousarray(f2)).to(dtype).requires_grad_(True)
    (root * fn(a, b, k, reduction)).backward()
    return a.grad.numpy().astype(F64), b.grad.numpy().astype(F64)


def fa_grads(f1, f2, k=8, reduction='mean', root=1.0):
    """float64 reference gradients of root * loss"""
    return _grads(fa_loss_torch64, f1, f2, k, reduction, root, torch.float64)


def fa_grads_stock32(f1, f2, k=8, reduction='mean', root=1.0):
    """what the original module's formula gives in float32 stock torch on the CPU: the yardstick of the gradient tolerance"""
    return _grads(fa_loss_stock, f1, f2, k, reduction, root, torch.float32)


def range_rel(a, b):
    """max |a - b| / max |b|"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


def grad_bound(f1, f2, k, reduction, root, ref=None):
    """(bound for d fm1, bound for d fm2), range-relative: 8 x the larger of the float32 stock-torch error against the float64 reference and 32 u.
    The backward pass is float32 arithmetic through sigma_1, whose conditioning depends on the spectral gap of each input, so no fixed number
    fits; 8 covers the kernel's other summation order and the float32 sigma, u and v it stores between its passes, the floor keeps a lucky
    stock run from failing a correct kernel."""
    ref = ref or fa_grads(f1, f2, k, reduction, root)
    got = fa_grads_stock32(f1, f2, k, reduction, root)
    return tuple(8.0 * max(range_rel(g, r), 32 * U) for g, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------ FA loss, forward bound
def forward_bounds(f1, f2, k):
    """-> (none_ref, none_bound, sum_ref, sum_bound) in float64, first order, from the kernel text.

    fa_pool: a cell is at most k^2 - 1 float32 additions and one multiplication by fl(1 / k^2), which itself carries one rounding:
    |dX| <= g * A with g = (k^2 + 3) u and A the average of |x| (not |average of x|: signed inputs cancel, their roundings do not).
    G = X^T X, the 20 squarings, the Rayleigh quotient and G / lambda are float64: they add ~1e-15, carried as 1e-13 below.
    dG = dX^T X + X^T dX:            |dG| <= E = 2 g A^T A, entry by entry
    dlambda = v^T dG v:              |dlambda| <= ||E||_2 = 2 g lambda_max(A^T A)
      and the power iteration: the Rayleigh quotient of a column of G^(2^20) misses lambda by at most lambda (1 - r) r^(2^21) per further
      eigenvalue, r = lambda_i / lambda (nothing unless two eigenvalues agree to 1e-6)
    S = G / lambda:                  |dS| <= E / lambda + |S| |dlambda| / lambda, and u |S| for the rounding of S to float32
    |S1_i - S2_j| in float32:        |d| <= dS1_i + dS2_j + u |S1_i - S2_j|
    the sum: a lane adds ceil(n / 8) terms of a row in float32 ((n / 8) u of the row), everything after that is float64, the result is rounded once."""
    g = (k * k + 3) * U
    S, dS = [], []
    for f in (f1, f2):
        X, A = pool(f, k), pool(np.abs(np.asarray(f, F64)), k)
        G, GA = gram(X), gram(A)
        ev = np.stack([[np.linalg.eigvalsh(G[b, c]) for c in range(G.shape[1])] for b in range(G.shape[0])])
        lam, lam_a = ev[..., -1], top_eigenvalue(GA)
        r = np.clip(ev[..., :-1] / lam[..., None], 0.0, 1.0)
        it = ((1.0 - r) * r ** float(2 ** 21)).sum(-1)
        s = G / lam[:, :, None, None]
        ds = 2 * g * GA / lam[:, :, None, None] + np.abs(s) * (2 * g * lam_a / lam + it + U + 1e-13)[:, :, None, None]
        S.append(s.reshape(s.shape[0], s.shape[1], -1)); dS.append(1.01 * ds.reshape(s.shape[0], s.shape[1], -1))     # 1 %: the second-order terms
    none = np.abs(S[0][:, :, :, None] - S[1][:, :, None, :])
    bound = dS[0][:, :, :, None] + dS[1][:, :, None, :] + U * none
    n = S[0].shape[-1]
    total = none.sum()
    return none.reshape(none.shape[0], none.shape[1], -1), bound.reshape(none.shape[0], none.shape[1], -1), total, bound.sum() + ((n + 7) // 8 + 1) * U * total


# ------------------------------------------------------------------------------------------------ MSE, loss mix, NaN flag
def mse(a, b):
    d = np.asarray(a, F64) - np.asarray(b, F64)
    return float((d * d).mean())


def mse_grad(a, b, scale=1.0):
    """d (scale * mse) / da = (a - b) 2 scale / n"""
    return (np.asarray(a, F64) - np.asarray(b, F64)) * (2.0 * scale / np.asarray(a).size)


def loss_mix(ce, mse_, fa, w1, w2, flag):
    """the five float32 values of loss_mix_kernel as written: c, w1 * m, w2 * f, (c + m) + f, the flag; a null term is 0"""
    f32 = np.float32
    with np.errstate(all='ignore'):
        c = f32(ce)
        m = f32(w1) * f32(mse_) if mse_ is not None else f32(0)
        f = f32(w2) * f32(fa) if fa is not None else f32(0)
        return np.array([c, m, f, f32(f32(c + m) + f), f32(flag) if flag is not None else f32(0)], np.float32)


def nan_flag(*arrays):
    return int(any(np.isnan(np.asarray(a)).any() for a in arrays if a is not None))


# ------------------------------------------------------------------------------------------------ the case table
# name: ((B, C, H, W), k, gradient case?).  n = 1024 is forward only: with 10^6 pairs per slice no seed keeps every pair GAP_FLOOR apart.
FA_CASES = {
    'vec64_T4': ((2, 1, 64, 64), 8, True),            # vector pooling, 64 cells, 4 lanes per cell
    'vec8_T8_C2': ((2, 2, 32, 16), 8, True),          # vector pooling, 8 cells, 8 lanes per cell, C > 1
    'wide_rank4': ((1, 1, 32, 128), 8, True),         # 64 cells, hp = 4 < wp = 16: G has rank 4
    'hp2_wp8': ((1, 2, 16, 64), 8, True),
    'pooled_1x1': ((3, 1, 8, 8), 8, True),            # S1 = S2 = 1: exact ties, exempt from the gap floor
    'ragged_scalar': ((2, 1, 29, 43), 8, True),       # row stride 43: scalar pooling; rows >= 24 and columns >= 40 take no part
    'ragged_vector': ((2, 1, 29, 44), 8, True),       # row stride 44: vector pooling with a ragged right and bottom edge
    'k4': ((2, 1, 24, 24), 4, True),
    'k3': ((1, 2, 17, 22), 3, True),
    'k1': ((1, 2, 8, 8), 1, True),
    'hp64': ((1, 1, 128, 16), 2, True),               # hp = 64, the limit
    'hp64_wp32': ((1, 1, 512, 256), 8, False),        # both limits, n = 1024
}
FA_KINDS = ('uniform', 'normal')
# Seeds found on the CPU (tests/test_fa_ref_host.py re-checks them): the first seed from 0 whose inputs keep every pair of every slice GAP_FLOOR
# apart by the float64 reference alone.  None: no seed below 400 does (the uniform 4 x 16 pooled map crowds its 256 S values into a band so narrow
# that the best seed reaches 2e-6); that kind is then checked forward only, on seed 0.
FA_SEEDS = {
    ('vec64_T4', 'uniform'): 720, ('vec64_T4', 'normal'): 0, ('vec8_T8_C2', 'uniform'): 0, ('vec8_T8_C2', 'normal'): 0,
    ('wide_rank4', 'uniform'): None, ('wide_rank4', 'normal'): 20, ('hp2_wp8', 'uniform'): 33, ('hp2_wp8', 'normal'): 0,
    ('ragged_scalar', 'uniform'): 0, ('ragged_scalar', 'normal'): 0, ('ragged_vector', 'uniform'): 0, ('ragged_vector', 'normal'): 0,
    ('k4', 'uniform'): 0, ('k4', 'normal'): 0, ('k3', 'uniform'): 4, ('k3', 'normal'): 0, ('k1', 'uniform'): 0, ('k1', 'normal'): 3,
    ('hp64', 'uniform'): 3, ('hp64', 'normal'): 0, ('pooled_1x1', 'uniform'): 0, ('pooled_1x1', 'normal'): 0,
    ('hp64_wp32', 'uniform'): 0, ('hp64_wp32', 'normal'): 0,
}


def fa_inputs(case, kind, seed=None):
    """the two float32 feature maps of a case"""
    shape, k, _ = FA_CASES[case]
    seed = FA_SEEDS.get((case, kind)) if seed is None else seed
    rs = np.random.RandomState(1000003 * (seed or 0) + sum(shape) * 131 + k * 7 + (kind == 'normal'))
    draw = (lambda: rs.uniform(size=shape)) if kind == 'uniform' else (lambda: rs.standard_normal(shape))
    return draw().astype(np.float32), draw().astype(np.float32)


def fa_exempt(case):
    return case == 'pooled_1x1'


def fa_gradient_cases():
    """[(case, kind)] whose gradients the GPU file checks"""
    return [(c, kd) for c, (_, _, grad) in FA_CASES.items() if grad for kd in FA_KINDS if fa_exempt(c) or FA_SEEDS.get((c, kd)) is not None]


def special_inputs(name):
    """(2, 1, 64, 64), k = 8: 'rank1' a constant map against a random one, 'same' two identical maps"""
    seed = {'rank1': 2, 'same': 5}[name]
    rs = np.random.RandomState(7700 + seed)
    b = rs.uniform(size=(2, 1, 64, 64)).astype(np.float32)
    if name == 'rank1':
        return np.full((2, 1, 64, 64), 0.5, np.float32), b
    return b, b.copy()

"""The soft Dice loss term of DESIGN.md 6.1.9 in numpy: the float64 definition (value, class sums, coefficients, closed-form gradient), a plain
fp32 restatement of the kernels' arithmetic, and the "overlap" case of the GPU tests.

    live_i = t_i != ignore_index and t_i < C         p = softmax of the pixel's logits
    I_c = sum_i p_ic [t_i = c]    P_c = sum_i p_ic    G_c = sum_i [t_i = c]    den_c = P_c + G_c + smooth    dice_c = (2 I_c + smooth) / den_c
    K = {c : G_c > 0}             L = 1 - mean_{c in K} dice_c      (K empty: L = 0 and every coefficient 0)
    a_c = -(lambda / |K|) 2 / den_c           b_c = (lambda / |K|) (2 I_c + smooth) / den_c^2          (c not in K: 0)
    d(lambda L) / d v_ik = live_i p_ik (g_ik - sum_j p_ij g_ij),   g_ij = b_j + a_j [j = t_i]
"""
import numpy as np

GRAD_TOL = 2.0 ** -20 + 2.0 ** -22          # x max_c (|a_c| + |b_c|), per gradient element: the weighted CE bound with Dice's own scale where w / D stands


def _live(tg, ii, C):
    t = np.asarray(tg).astype(np.int64)
    return (t != ii) & (t < C), t


def softmax64(lg):
    x = np.asarray(lg).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def sums64(lg, tg, ii):
    """-> (I (C,), P (C,), G (C,) int64) over the live pixels, float64"""
    P_, C = np.asarray(lg).shape
    live, t = _live(tg, ii, C)
    p = softmax64(lg)[live]
    tl = t[live]
    onehot = np.zeros((tl.size, C)); onehot[np.arange(tl.size), tl] = 1.0
    return (p * onehot).sum(axis=0), p.sum(axis=0), np.bincount(tl, minlength=C)[:C].astype(np.int64)


def coefficients64(I, Pc, G, lam, smooth):
    """-> (lambda L, |K|, a (C,), b (C,)) in float64"""
    present = G > 0
    K = int(present.sum())
    a = np.zeros(I.size); b = np.zeros(I.size)
    if K == 0:
        return 0.0, 0, a, b
    den = Pc + G + smooth
    num = 2.0 * I + smooth
    dice = np.where(present, num / np.where(present, den, 1.0), 0.0)
    a[present] = -(lam / K) * 2.0 / den[present]
    b[present] = (lam / K) * num[present] / den[present] ** 2
    return lam * (1.0 - dice.sum() / K), K, a, b


def dice_loss_and_grad(lg, tg, ii, lam=1.0, smooth=1.0):
    """-> (lambda L, gradient (P, C), |K|, a, b, G): float64 on the fp32 logits; rows of pixels that are not live are zero"""
    P_, C = np.asarray(lg).shape
    live, t = _live(tg, ii, C)
    I, Pc, G = sums64(lg, tg, ii)
    val, K, a, b = coefficients64(I, Pc, G, float(lam), float(smooth))
    p = softmax64(lg)
    g = np.broadcast_to(b, (P_, C)).copy()
    idx = np.where(live)[0]
    g[idx, t[idx]] += a[t[idx]]
    with np.errstate(invalid='ignore'):
        grad = p * (g - (p * g).sum(axis=1, keepdims=True))
    grad[~live] = 0.0
    return val, grad, K, a, b, G


def value64(lg64, tg, ii, lam=1.0, smooth=1.0):
    """lambda L of float64 logits (for central differences)"""
    C = lg64.shape[1]
    live, t = _live(tg, ii, C)
    x = lg64[live]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    tl = t[live]
    G = np.bincount(tl, minlength=C)[:C]
    I = np.zeros(C); np.add.at(I, tl, p[np.arange(tl.size), tl])
    return coefficients64(I, p.sum(axis=0), G, float(lam), float(smooth))[0]


def emulate_fp32(lg, tg, ii, lam=1.0, smooth=1.0):
    """The kernels' arithmetic restated plainly in numpy: m, e_c = exp(v_c - m), s = sum e_c (c ascending) and p_c = e_c (1 / s) in fp32; the class
    sums in double; the coefficients in double, rounded to fp32 once; the row p_k (g_k - sum_j p_j g_j) in fp32 with the sum in ascending j.
    np.exp in fp32 stands in for the device's exp (a few ulp).  -> (lambda L as fp32, gradient (P, C) fp32, a fp32, b fp32)"""
    f = np.float32
    lg = np.asarray(lg, f)
    P_, C = lg.shape
    live, t = _live(tg, ii, C)
    with np.errstate(invalid='ignore', over='ignore'):
        m = lg.max(axis=1, keepdims=True)
        e = np.exp((lg - m).astype(f)).astype(f)
        s = np.zeros(P_, f)
        for c in range(C):
            s = (s + e[:, c]).astype(f)
        inv_s = (f(1) / s).astype(f)
        p = (e * inv_s[:, None]).astype(f)
    pl = p[live].astype(np.float64)
    tl = t[live]
    I = np.zeros(C); np.add.at(I, tl, pl[np.arange(tl.size), tl])
    val, K, a, b = coefficients64(I, pl.sum(axis=0), np.bincount(tl, minlength=C)[:C], float(f(lam)), float(f(smooth)))
    a32, b32 = a.astype(f), b.astype(f)
    g = np.broadcast_to(b32, (P_, C)).copy()
    idx = np.where(live)[0]
    g[idx, t[idx]] = (g[idx, t[idx]] + a32[t[idx]]).astype(f)
    dot = np.zeros(P_, f)
    with np.errstate(invalid='ignore'):
        for c in range(C):
            dot = (dot + (p[:, c] * g[:, c]).astype(f)).astype(f)
        grad = (p * (g - dot[:, None]).astype(f)).astype(f)
    grad[~live] = 0
    return f(val), grad, a32, b32


def make_overlap(P, C, rs, ii=255):
    """-> (logits (P, C) float32, target (P,) uint8): logits of a few units; half the live labels are the pixel's arg-max, the others random; about
    10 % of the labels are `ii`; class C - 1 carries no pixel (its labels move to class 0), so that it is ABSENT from the mean."""
    lg = (rs.standard_normal((P, C)) * 3).astype(np.float32)
    tg = rs.randint(0, C, P).astype(np.int64)
    hit = rs.uniform(size=P) < 0.5
    tg[hit] = lg.argmax(axis=1)[hit]
    tg[tg == C - 1] = 0
    if 0 <= ii <= 255:
        tg[rs.uniform(size=P) < 0.1] = ii
    return lg, tg.astype(np.uint8)


def assert_overlap(lg, tg, ii, lam=1.0, smooth=1.0):
    """the conditions of the overlap case, on the float64 reference: 0.2 < L < 0.9, class C - 1 absent, and a gradient whose largest element is
    more than 100 x the gradient bound - a kernel that ignores Dice, or that counts the absent class, fails the checks that follow"""
    val, grad, K, a, b, G = dice_loss_and_grad(lg, tg, ii, lam, smooth)
    C = lg.shape[1]
    assert G[C - 1] == 0 and K == int((G > 0).sum()) < C
    assert 0.2 < val / lam < 0.9, f'L_dice = {val / lam}'
    bound = GRAD_TOL * float((np.abs(a) + np.abs(b)).max())
    assert np.abs(grad).max() > 100 * bound, (np.abs(grad).max(), bound)

"""Label-smoothed cross entropy, nn.CrossEntropyLoss(weight=, ignore_index=, label_smoothing=eps), restated in float64 numpy, the torch CPU call it
restates, a float32 emulation of the kernels' shared pixel function (smooth_pixel / smooth_grad, csrc/common.h), and the two error bounds the
tests hold the kernels (and the emulation) to.  Inputs: fp32 logits (P, C), uint8 / int labels (P,), fp32 class weights (C,).

With C real classes, table weights w, the live pixels i (label != ignore_index), m_i = max_c v_ic, s_i = sum_c exp(v_ic - m_i):
    nl_ic = (m_i - v_ic) + log s_i,   D = sum_i w[t_i],   W = sum_{c < C} w_c
    L = [ (1 - eps) sum_i w[t_i] nl_i,t_i  +  (eps / C) sum_i sum_{c < C, w_c > 0} w_c nl_ic ] / D
    dL / dv_ic = [ (1 - eps) w[t_i] (p_ic - [c == t_i])  +  (eps / C) (p_ic W - w_c) ] / D          (ignored pixels: exactly 0)
ONE deviation from torch: a class of weight 0 adds nothing to the smoothing sum, even where nl_ic is +inf (torch forms 0 * inf = NaN there).
What stays torch's: a live pixel whose target has weight 0 still contributes its smoothing term; D == 0 gives what IEEE division gives."""
import numpy as np
import torch
import torch.nn.functional as F

LOSS_REL = 1e-6                             # check_loss's relative part (tests/test_cross_entropy_edges.py), applied to each summand
M_ULPS = 2                                  # its m-ulp part
GRAD_TOL = 2.0 ** -20 + 2.0 ** -22          # the weighted test's gradient tolerance, applied to the magnitude of each summand


def _pixels(tg, ii):
    t = np.asarray(tg).astype(np.int64)
    return t != ii, t


def smooth_loss_and_grad(lg, tg, ii, w, eps):
    """-> (loss, gradient (P, C) with zero rows on ignored pixels, D, CE part, smoothing part), float64.  loss = CE part + smoothing part (the
    sum of the numerators divided once), the parts being (1 - eps) sum w[t] nl_t / D and (eps / C) sum sum w_c nl_c / D.  Labels must lie inside the classes or equal ii."""
    live, t = _pixels(tg, ii)
    P, C = lg.shape
    w64 = np.asarray(w).astype(np.float64)
    g = np.zeros((P, C), np.float64)
    tl = t[live]
    D = float(w64[tl].sum())
    W = 0.0
    for c in range(C):
        W += w64[c]
    v = np.asarray(lg)[live].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if v.shape[0] == 0:
            return float('nan'), g, D, float('nan'), float('nan')
        m = v.max(axis=1, keepdims=True)
        e = np.exp(v - m)
        s = e.sum(axis=1, keepdims=True)
        nl = (m - v) + np.log(s)
        n = np.arange(v.shape[0])
        ce_sum = float((w64[tl] * nl[n, tl]).sum())
        sm_sum = float(np.where(w64[None, :] > 0, w64[None, :] * nl, 0.0).sum())         # the zero-weight rule
        ce_part = float(np.float64((1.0 - eps) * ce_sum) / np.float64(D))        # D == 0: what IEEE division gives
        sm_part = float(np.float64((eps / C) * sm_sum) / np.float64(D))
        p = e / s
        hot = np.zeros_like(p); hot[n, tl] = 1.0
        g[live] = ((1.0 - eps) * w64[tl][:, None] * (p - hot) + (eps / C) * (p * W - w64[None, :])) / np.float64(D)
        loss = float(np.float64((1.0 - eps) * ce_sum + (eps / C) * sm_sum) / np.float64(D))      # one division of the sum: live pixels over D == 0 are +inf
    return loss, g, D, ce_part, sm_part


def torch_reference(lg, tg, ii, w, eps):
    """-> (loss, gradient (P, C)): F.cross_entropy(weight=, ignore_index=, label_smoothing=) on CPU float64, gradient from autograd"""
    x = torch.tensor(np.asarray(lg).astype(np.float64), requires_grad=True)
    t = torch.tensor(np.asarray(tg).astype(np.int64))
    loss = F.cross_entropy(x, t, weight=torch.tensor(np.asarray(w).astype(np.float64)), ignore_index=ii, label_smoothing=float(eps))
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def loss_bound(lg, tg, ii, w, eps):
    """LOSS_REL (|(1 - eps) CE part| + |smoothing part|) + M_ULPS ulp32(max |v| over the live pixels) ((1 - eps) + 2 eps (W / C) n_live / D): the
    relative part of check_loss on each summand, and its m-ulp part - the smoothing sum carries one m - v_c (up to 2 |m|) per class and weight,
    hence (eps / C) W n_live / D times two."""
    live, t = _pixels(tg, ii)
    _, _, D, ce_part, sm_part = smooth_loss_and_grad(lg, tg, ii, w, eps)
    C = lg.shape[1]
    W = float(np.asarray(w).astype(np.float64).sum())
    vmax = float(np.abs(np.asarray(lg)[live]).max())
    return LOSS_REL * (abs(ce_part) + abs(sm_part)) + M_ULPS * ulp32(vmax) * ((1.0 - eps) + 2.0 * eps * (W / C) * float(live.sum()) / D)


def grad_bound(tg, ii, w, eps, D):
    """(n_live, C) bounds of the live pixels' gradient elements: GRAD_TOL ((1 - eps) w[t] + (eps / C) (W + w_c)) / D"""
    live, t = _pixels(tg, ii)
    w64 = np.asarray(w).astype(np.float64)
    C = w64.size
    return GRAD_TOL * ((1.0 - eps) * w64[t[live]][:, None] + (eps / C) * (w64.sum() + w64[None, :])) / D


def emulate_fp32(lg, tg, ii, w, eps):
    """The arithmetic of smooth_pixel / smooth_grad as the kernels run it, in numpy float32 with the same operation order: m, e_c = exp(v_c - m) and
    s = sum e_c (c ascending) in fp32, nl_c = (m - v_c) + log s in fp32, the products with the weights and the sums over classes and pixels in double,
    D rounded to fp32 once, scale = 1 / D, omw = (1 - eps) w[t], inv = ((omw + (eps / C) W) scale) / s, g_c = e_c inv - (([c == t] ? omw : 0) +
    (eps / C) w_c) scale (the kernels read ((eps / C) w_c) scale of a class that is not the target from a per-block table: 0 + x is x, the same bits).  -> (loss as fp32, gradient (P, C) fp32).  np.exp / np.log in fp32 stand in for the device's exp and log (a few ulp)."""
    f = np.float32
    live, t = _pixels(tg, ii)
    P, C = lg.shape
    w32 = np.asarray(w).astype(f)
    g = np.zeros((P, C), f)
    v = np.asarray(lg)[live].astype(f)
    tl = t[live]
    n = np.arange(v.shape[0])
    d = 0.0
    cnt = np.bincount(tl, minlength=C)
    for c in range(C):
        d += float(cnt[c]) * float(w32[c])
    D32 = f(d)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        Wsum = f(0)
        for c in range(C):
            Wsum = f(Wsum + w32[c])
        m = v.max(axis=1)
        e = np.exp((v - m[:, None]).astype(f)).astype(f)
        s = np.zeros(v.shape[0], f)
        for c in range(C):
            s = (s + e[:, c]).astype(f)
        ls = np.log(s).astype(f)
        eps32 = f(eps)
        epsC = f(eps32 / f(C))
        omw = (f(f(1) - eps32) * w32[tl]).astype(f)
        sm = np.zeros(v.shape[0], np.float64)
        for c in range(C):
            nl = ((m - v[:, c]).astype(f) + ls).astype(f)
            if w32[c] > 0:
                sm += float(w32[c]) * nl.astype(np.float64)
        nlt = ((m - v[n, tl]).astype(f) + ls).astype(f)
        val = omw.astype(np.float64) * nlt.astype(np.float64) + float(epsC) * sm
        loss = f(np.float64(val.sum()) / np.float64(D32))
        scale = f(f(1) / D32)
        inv = (((omw + epsC * Wsum).astype(f) * scale).astype(f) / s).astype(f)
        gl = np.zeros_like(v)
        for c in range(C):
            sub = ((np.where(tl == c, omw, f(0)).astype(f) + f(epsC * w32[c])).astype(f) * scale).astype(f)
            gl[:, c] = ((e[:, c] * inv).astype(f) - sub).astype(f)
        g[live] = gl
    return loss, g

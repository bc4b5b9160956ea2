"""Reference for boundary label relaxation, numpy only: the class-set mask in two formulations, the relaxed cross entropy and
its gradient in float64, an fp32 restatement in the operation order of relax_pixel / relax_grad (csrc/common.h), a label generator on a coarse
block grid, and the bounds the GPU test holds the kernels to - built from the project's own constants, never from what the kernels give."""
import numpy as np

from label_smoothing_ref import GRAD_TOL, LOSS_REL, M_ULPS, ulp32  # noqa: F401  (the weighted suite's tolerances)


# ------------------------------------------------------------------------------------------------------------------------------ the mask
def _bits(tg, C, ii):
    tg = np.asarray(tg).astype(np.int64)
    ok = (tg != ii) & (tg < C)
    return np.where(ok, np.left_shift(np.uint64(1), np.where(ok, tg, 0).astype(np.uint64)), np.uint64(0)).astype(np.uint32), ok


def mask_ref(tg, C, ii, r, how='window'):
    """(N, H, W) labels -> ((N, H, W) uint32 masks, (live pixels, pixels with more than one class in their set)).  how = 'window': the OR over the
    (2r+1)^2 window written as a loop over its offsets; 'separable': a row pass, then a column pass.  Both clip at the image's borders."""
    tg = np.asarray(tg)
    N, H, W = tg.shape
    b, ok = _bits(tg, C, ii)
    pad = np.zeros((N, H + 2 * r, W + 2 * r), np.uint32)
    pad[:, r:r + H, r:r + W] = b
    if how == 'window':
        out = np.zeros((N, H, W), np.uint32)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                out |= pad[:, dy:dy + H, dx:dx + W]
    else:
        rows = np.zeros((N, H + 2 * r, W), np.uint32)
        for dx in range(2 * r + 1):
            rows |= pad[:, :, dx:dx + W]
        out = np.zeros((N, H, W), np.uint32)
        for dy in range(2 * r + 1):
            out |= rows[:, dy:dy + H, :]
    out = np.where(ok, out, np.uint32(0)).astype(np.uint32)
    live = tg.astype(np.int64) != ii
    return out, (int(live.sum()), int((popcount(out) > 1).sum()))


def popcount(m):
    m = np.asarray(m).astype(np.uint32)
    return sum(((m >> np.uint32(k)) & np.uint32(1)).astype(np.int64) for k in range(32))


def clean(mask, tg, C):
    """S_i = (mask_i & ((1 << C) - 1)) | bit(t_i): what every consumer makes of a word"""
    tg = np.asarray(tg).astype(np.int64).reshape(-1)
    m = np.asarray(mask).astype(np.uint32).reshape(-1) & np.uint32((1 << C) - 1)
    own = np.where(tg < C, np.left_shift(np.uint64(1), np.where(tg < C, tg, 0).astype(np.uint64)), np.uint64(0)).astype(np.uint32)
    return m | own


def members(S, C):
    """(P,) set words -> (P, C) bool"""
    return ((np.asarray(S).astype(np.uint32)[:, None] >> np.arange(C, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool)


# ------------------------------------------------------------------------------------------------------------------------------ the loss
def relaxed_loss_and_grad(lg, tg, ii, w, mask):
    """float64: (loss, gradient (P, C), D).  lg (P, C), tg (P,), w (C,) weights, mask (P,) words (cleaned here).  Labels must be < C or ii."""
    v = np.asarray(lg).astype(np.float64)
    tg = np.asarray(tg).astype(np.int64).reshape(-1)
    P, C = v.shape
    live = tg != ii
    t = np.where(live, tg, 0)
    w64 = np.asarray(w).astype(np.float64)
    wt = np.where(live, w64[t], 0.0)
    D = wt.sum()
    inS = members(clean(mask, np.where(live, tg, C), C), C)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        m = v.max(axis=1, keepdims=True)
        e = np.exp(v - m)
        s = e.sum(axis=1, keepdims=True)
        vs = np.where(inS, v, -np.inf)
        mS = vs.max(axis=1, keepdims=True)
        g = np.where(inS, np.exp(np.where(inS, v - mS, 0.0)), 0.0)
        z = g.sum(axis=1, keepdims=True)
        term = wt * ((m + np.log(s)) - (mS + np.log(z)))[:, 0]
        loss = term[live].sum() / D
        grad = np.where(live[:, None], (wt / D)[:, None] * (e / s - g / z), 0.0)
    return float(loss), grad, float(D)


def weighted_loss_and_grad(lg, tg, ii, w):
    """float64 class-weighted CE, the singleton case written on its own"""
    v = np.asarray(lg).astype(np.float64)
    tg = np.asarray(tg).astype(np.int64).reshape(-1)
    live = tg != ii
    t = np.where(live, tg, 0)
    w64 = np.asarray(w).astype(np.float64)
    wt = np.where(live, w64[t], 0.0)
    D = wt.sum()
    m = v.max(axis=1, keepdims=True)
    e = np.exp(v - m)
    s = e.sum(axis=1, keepdims=True)
    nll = (m + np.log(s))[:, 0] - v[np.arange(len(t)), t]
    onehot = np.zeros_like(v); onehot[np.arange(len(t)), t] = 1.0
    return float((wt * nll)[live].sum() / D), np.where(live[:, None], (wt / D)[:, None] * (e / s - onehot), 0.0), float(D)


def _exp32(x):
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return np.exp(x.astype(np.float32)).astype(np.float32)


def emulate_fp32(lg, tg, ii, w, mask):
    """The operation order of relax_pixel / relax_grad in numpy float32 (numpy's exp and log stand in for exp_nonpos and logf): m, e_c, s with c
    ascending; m_S, g_c, z with c ascending; term = (m + log s) - (m_S + log z); inv = sc / s, invz = sc / z, row = e inv - g invz; the products with
    the weight and the sum over the pixels in double, D one rounding of the double sum.  -> (loss, gradient (P, C), D) as float32 values."""
    f = np.float32
    v = np.asarray(lg).astype(f)
    tg = np.asarray(tg).astype(np.int64).reshape(-1)
    P, C = v.shape
    live = tg != ii
    t = np.where(live, tg, 0)
    w32 = np.asarray(w).astype(f)
    wt = np.where(live, w32[t], f(0))
    D = f(np.asarray(wt, np.float64).sum())
    inS = members(clean(mask, np.where(live, tg, C), C), C)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        m = v.max(axis=1)
        e = _exp32(v - m[:, None])
        s = np.zeros(P, f)
        for c in range(C):
            s = (s + e[:, c]).astype(f)
        mS = np.where(inS, v, f(-np.inf)).max(axis=1).astype(f)
        arg = np.where(v == mS[:, None], f(0), v - mS[:, None]).astype(f)
        g = np.where(inS, _exp32(arg), f(0)).astype(f)
        z = np.zeros(P, f)
        for c in range(C):
            z = (z + g[:, c]).astype(f)
        term = ((m + np.log(s).astype(f)).astype(f) - (mS + np.log(z).astype(f)).astype(f)).astype(f)
        loss = f((wt.astype(np.float64) * term.astype(np.float64))[live].sum() / np.float64(D))
        sc = (wt * (f(1) / D)).astype(f)
        inv = (sc / s).astype(f); invz = (sc / z).astype(f)
        row = ((e * inv[:, None]).astype(f) - (g * invz[:, None]).astype(f)).astype(f)
        row = np.where(live[:, None], row, f(0))
    return loss, row, D


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def block_labels(N, H, W, C, b, seed, ii=255, p_ignore=0.08, p_bad=0.0):
    """(N, H, W) uint8 labels: one class per b x b block of a coarse grid, some blocks ignored (and, with p_bad, some given a label >= C)"""
    rs = np.random.RandomState(seed)
    gh, gw = -(-H // b), -(-W // b)
    grid = rs.randint(0, C, (N, gh, gw)).astype(np.int64)
    u = rs.uniform(size=grid.shape)
    if 0 <= ii <= 255:
        grid[u < p_ignore] = ii
    if p_bad:
        bad = [x for x in range(C, 256) if x != ii]
        grid[(u >= p_ignore) & (u < p_ignore + p_bad)] = bad[0] if len(bad) == 1 else rs.choice(bad)
    return np.repeat(np.repeat(grid, b, axis=1), b, axis=2)[:, :H, :W].astype(np.uint8)


def set_size_shares(mask, tg, C, ii):
    """shares of the live pixels (label < C) whose set holds 1, 2, 3 and >= 4 classes"""
    tg = np.asarray(tg).reshape(-1)
    live = (tg.astype(np.int64) != ii) & (tg < C)
    n = popcount(clean(mask, tg, C))[live]
    return [float((n == 1).mean()), float((n == 2).mean()), float((n == 3).mean()), float((n >= 4).mean())]


def make_case(P, C, seed, b=8, r=1, ii=255, scale=3.0):
    """(logits (P, C) float32, labels (P,) uint8, masks (P,) uint32) for P pixels: block labels of an image wide enough, cut to its first P pixels in
    row-major order, the masks those of the whole image (a word of the image, whatever the cut)"""
    Wd = 96 if P >= 96 else max(P, 1)
    Hd = -(-P // Wd)
    tg = block_labels(1, Hd, Wd, C, b, seed, ii)
    mk, _ = mask_ref(tg, C, ii, r)
    rs = np.random.RandomState(seed + 1)
    lg = (scale * rs.standard_normal((P, C))).astype(np.float32)
    return lg, tg.reshape(-1)[:P].copy(), mk.reshape(-1)[:P].copy()


# ------------------------------------------------------------------------------------------------------------------------------ bounds
def loss_bound(lg, tg, ii, loss):
    """LOSS_REL |L| + 2 M_ULPS ulp32(max |v| over the live pixels): the term carries two magnitudes, m and m_S"""
    live = np.asarray(tg).reshape(-1).astype(np.int64) != ii
    v = np.abs(np.asarray(lg, np.float64)[live])
    v = v[np.isfinite(v)]                       # (an infinite logit has no ulp; the finite ones set the scale)
    vmax = float(v.max()) if v.size else 0.0
    return LOSS_REL * abs(loss) + 2 * M_ULPS * ulp32(vmax)


def grad_bound(tg, ii, w, mask, C):
    """(P, C): GRAD_TOL w[t_i] / D per summand - once on every class (e_c / s), once more on the classes of S_i (g_c / z); 0 on ignored pixels"""
    tg = np.asarray(tg).astype(np.int64).reshape(-1)
    live = tg != ii
    w64 = np.asarray(w).astype(np.float64)
    wt = np.where(live, w64[np.where(live, tg, 0)], 0.0)
    D = wt.sum()
    inS = members(clean(mask, np.where(live, tg, C), C), C)
    return GRAD_TOL * (wt / D)[:, None] * (1.0 + inS.astype(np.float64))

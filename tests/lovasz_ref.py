"""Reference of the Lovasz-Softmax term (include/dsrl_hip.h, "Lovasz-Softmax"), numpy float64 on fp32 logits taken to float64:

    lovasz_exact          the loss of Berman et al. (CVPR 2018): softmax, per class the errors sorted descending (stable), the Lovasz extension of
                          the Jaccard loss, classes = 'present' over the whole call, ignored pixels removed
    lovasz_extension      the extension at given errors with a stated tie order (foreground first), for the host test of the closed form
    binned                the quantised form by the closed formulas of the header: histograms, tables, value, gradient rows
    tables_from_hist      the closed form from given histograms (the device's own, in the GPU tests)
    rows_from_tables      the gradient rows from given tables, float64
    rows_fp32             a plain float32 numpy restatement of the same row (np.exp in float32, sums with c ascending): its error against
                          float64 times 4 is the bound of the device's row, the convention of tests/temperature_ref.py
    borderline            elements whose err K is within K 4e-6 of an integer: where a float32 softmax may legitimately move an element one level

A pixel is live when its label is neither ignore_index nor >= C."""
import numpy as np

MARGIN = 4e-6           # in units of the error: a float32 softmax (exp within 2 ulp, 19 additions, one reciprocal, one product) stays well inside


def live_mask(tg, C, ii):
    t = np.asarray(tg).astype(np.int64)
    return (t != ii) & (t < C)


def softmax64(lg):
    v = np.asarray(lg).astype(np.float64)
    m = v.max(axis=1, keepdims=True)
    e = np.exp(v - m)
    return e * (1.0 / e.sum(axis=1, keepdims=True))


def errors(lg, tg, ii):
    """-> (err (P, C) float64, fg (P, C) bool, live (P,) bool); rows of pixels that are not live are meaningless"""
    P, C = lg.shape
    live = live_mask(tg, C, ii)
    p = softmax64(lg)
    fg = np.zeros((P, C), bool)
    idx = np.where(live)[0]
    fg[idx, np.asarray(tg).astype(np.int64)[idx]] = True
    return np.abs(fg.astype(np.float64) - p), fg, live


def jaccard_increments(fg_sorted):
    """Berman's lovasz_grad: the gradient of the extension with respect to the sorted errors"""
    g = fg_sorted.astype(np.float64)
    gts = g.sum()
    inter = gts - np.cumsum(g)
    union = gts + np.cumsum(1.0 - g)
    jac = 1.0 - inter / union
    jac[1:] = jac[1:] - jac[:-1]
    return jac


def lovasz_extension(err, fg, fg_first=False):
    """The Lovasz extension of the Jaccard loss of one class at the errors `err` (n,) with foreground flags `fg` (n,).  Stable sort, descending;
    fg_first: among equal errors the foreground elements come first."""
    if fg_first:
        order = np.lexsort((~fg, -err))         # primary key -err, then foreground (False of ~fg) first; lexsort is stable
    else:
        order = np.argsort(-err, kind='stable')
    return float(np.dot(err[order], jaccard_increments(fg[order])))


def lovasz_exact(lg, tg, ii):
    """-> L (float64), the unquantised Lovasz-Softmax loss, classes = 'present', 0 when no class is present"""
    err, fg, live = errors(lg, tg, ii)
    err, fg = err[live], fg[live]
    losses = [lovasz_extension(err[:, c], fg[:, c]) for c in range(lg.shape[1]) if fg[:, c].any()]
    return float(np.mean(losses)) if losses else 0.0


def bins_of(err, K):
    return np.minimum(K - 1, np.maximum(0, np.floor(err * K))).astype(np.int64)


def histograms(lg, tg, ii, K):
    """-> (nf (C, K), nb (C, K)) int64 over the live pixels, bins (P, C)"""
    P, C = lg.shape
    err, fg, live = errors(lg, tg, ii)
    b = bins_of(err, K)
    nf = np.zeros((C, K), np.int64)
    nb = np.zeros((C, K), np.int64)
    for c in range(C):
        nf[c] = np.bincount(b[live & fg[:, c], c], minlength=K)
        nb[c] = np.bincount(b[live & ~fg[:, c], c], minlength=K)
    return nf, nb, b


def tables_from_hist(nf, nb, lam):
    """The closed form of the header from histograms (C, K): -> dict(value = lambda L, present, Lc (C,), wf, wb, gf, gb (C, K) float64)"""
    nf = np.asarray(nf).astype(np.float64)
    nb = np.asarray(nb).astype(np.float64)
    C, K = nf.shape
    G = nf.sum(axis=1)
    nf_incl = np.cumsum(nf[:, ::-1], axis=1)[:, ::-1]
    nb_incl = np.cumsum(nb[:, ::-1], axis=1)[:, ::-1]
    nb_above = nb_incl - nb
    present = G > 0
    Gs = np.where(present, G, 1.0)[:, None]
    wf = np.where(present[:, None], 1.0 / (Gs + nb_above), 0.0)
    wb = np.where(present[:, None], (Gs - nf_incl) / ((Gs + nb_above) * (Gs + nb_incl)), 0.0)
    e_hat = (np.arange(K) + 0.5) / K
    Lc = (e_hat[None, :] * (nf * wf + nb * wb)).sum(axis=1)
    npres = int(present.sum())
    L = float(Lc[present].sum() / npres) if npres else 0.0
    lk = lam / npres if npres else 0.0
    return dict(value=lam * L, present=npres, Lc=Lc, wf=wf, wb=wb, gf=-lk * wf, gb=lk * wb, G=G.astype(np.int64))


def rows_from_tables(lg, tg, ii, gf, gb, K):
    """d(lambda L) / d logits (P, C) float64 from tables (C, K): live p_k (g_k - sum_j p_j g_j), g_j = (j == t ? gf : gb)[j][b_j]; zeros elsewhere"""
    P, C = lg.shape
    err, fg, live = errors(lg, tg, ii)
    p = softmax64(lg)
    b = bins_of(err, K)
    cc = np.broadcast_to(np.arange(C)[None, :], (P, C))
    g = np.where(fg, np.asarray(gf, np.float64)[cc, b], np.asarray(gb, np.float64)[cc, b])
    row = p * (g - (p * g).sum(axis=1, keepdims=True))
    row[~live] = 0.0
    return row


def rows_fp32(lg, tg, ii, gf, gb, K):
    """The same row in plain float32 numpy: m = max, e = np.exp(v - m) in float32, s and the class sum with c ascending, p = e (1 / s)"""
    f = np.float32
    P, C = lg.shape
    v = np.asarray(lg, f)
    live = live_mask(tg, C, ii)
    t = np.asarray(tg).astype(np.int64)
    m = v.max(axis=1, keepdims=True)
    e = np.exp((v - m).astype(f)).astype(f)
    s = np.zeros(P, f)
    for c in range(C):
        s = (s + e[:, c]).astype(f)
    p = (e * (f(1) / s)[:, None]).astype(f)
    fg = np.zeros((P, C), bool)
    fg[np.where(live)[0], t[live]] = True
    err = np.where(fg, np.abs(f(1) - p), np.abs(p)).astype(f)
    b = np.minimum(K - 1, np.maximum(0, np.floor(err * f(K)))).astype(np.int64)
    cc = np.broadcast_to(np.arange(C)[None, :], (P, C))
    g = np.where(fg, np.asarray(gf, f)[cc, b], np.asarray(gb, f)[cc, b]).astype(f)
    dot = np.zeros(P, f)
    for c in range(C):
        dot = (dot + (p[:, c] * g[:, c]).astype(f)).astype(f)
    row = (p * (g - dot[:, None]).astype(f)).astype(f)
    row[~live] = 0
    return row


def borderline(lg, tg, ii, K):
    """(P, C) bool: live elements with |err K - round(err K)| < K MARGIN, decided in float64 alone"""
    err, _, live = errors(lg, tg, ii)
    x = err * K
    return (np.abs(x - np.round(x)) < K * MARGIN) & live[:, None]


def binned(lg, tg, ii, lam, K):
    """The quantised form end to end: dict of tables_from_hist + nf, nb, bins, rows, borderline (P, C), exact (the unquantised L)"""
    nf, nb, b = histograms(lg, tg, ii, K)
    out = tables_from_hist(nf, nb, lam)
    out.update(nf=nf, nb=nb, bins=b, rows=rows_from_tables(lg, tg, ii, out['gf'], out['gb'], K), borderline=borderline(lg, tg, ii, K),
               exact=lovasz_exact(lg, tg, ii), live=live_mask(tg, lg.shape[1], ii))
    return out


CS = (19, 3)
KS = (16, 1024, 4096)
PS = (1, 63, 2048, 70001)
LAYOUTS = ('dense', 'slice')
EXACT_SEED = {19: 1, 3: 0}     # seeds of make_case(2048, C, .) without a single borderline element at K = 16 (test_lovasz_host checks both)


def case_seed(C, K, P, layout):
    """The seed of make_case for a combination of the GPU test; test_lovasz_host checks on the CPU that every one leaves fewer than a quarter of
    its live pixels with a borderline element"""
    if K == 16 and P == 2048:
        return EXACT_SEED[C]
    return 1000 * C + K + P % 97 + (layout == 'slice')


def make_case(P, C, seed, ii=255):
    """fp32 logits (P, C) and uint8 labels.  Three classes of a pixel, drawn at random, are in play (uniform in [-2, 2]); the others sit at
    -8.8 +- 0.2 (p between 5e-6 and a few 1e-4: above MARGIN and, but for a rare pixel, inside level 0 at every K <= 4096, as most background
    errors of a trained model are - with every class in play, 19 classes at K = 4096 would leave half the pixels with a borderline element).
    Half the labels are the arg-max over the classes 0 .. C - 2, the others uniform over them: class C - 1 is never a label (C > 1), so it is
    absent; about 10 % ignored; a single pixel is live."""
    rs = np.random.RandomState(seed)
    lg = (-8.8 + 0.1 * np.clip(rs.standard_normal((P, C)), -2.0, 2.0))
    play = np.argsort(rs.rand(P, C), axis=1)[:, :3]
    lg[np.arange(P)[:, None], play] = rs.uniform(-2.0, 2.0, (P, play.shape[1]))
    lg = lg.astype(np.float32)
    hi = max(1, C - 1)
    tg = rs.randint(0, hi, P)
    am = lg[:, :hi].argmax(axis=1)
    pick = rs.rand(P) < 0.5
    tg = np.where(pick, am, tg)
    if P > 1:
        tg = np.where(rs.rand(P) < 0.1, ii, tg)
    return lg, tg.astype(np.uint8)

"""The focal cross entropy of this project restated in float64 on the CPU (no torch op exists for it).  Inputs: fp32 logits (P, C), uint8 / int
labels (P,), fp32 class weights (C,), all taken to float64.

For a live pixel (label t != ignore_index) with p = softmax(v)[t], q = 1 - p, nll = -log p:
    term = w[t] q^gamma nll,   loss = sum term / D,   D = sum over the live pixels of w[t]
    d loss / d v_c = (w[t] / D) mod (softmax_c - [c == t]),   mod = q^(gamma - 1) (q + gamma p nll)
with the limits q == 0 -> term = 0, mod = 0 and p == 0 -> p nll = 0.  q comes from -expm1(log_softmax), never from 1 - p.  The gradient is the
closed form, not autograd: with gamma < 1 autograd gives NaN on the pixels whose float64 q is exactly 0 (test_focal_host.py checks the closed
form against autograd where no such pixel exists)."""
import numpy as np
import torch


def make_graded(P, C, rs, ii=255):
    """The `graded` case: standard-normal logits and a margin from U(-4, 10) on the target's logit, so that p_t sweeps from about 1e-3 to about 1.
    -> logits (P, C) float32, labels (P,) uint8; 10 % of the labels are `ii` when a uint8 can hold it and P > 1."""
    lg = rs.standard_normal((P, C)).astype(np.float32)
    tg = rs.randint(0, C, P).astype(np.int64)
    lg[np.arange(P), tg] += rs.uniform(-4.0, 10.0, P).astype(np.float32)
    if 0 <= ii <= 255 and P > 1:
        tg[rs.uniform(size=P) < 0.1] = ii
    return lg, tg.astype(np.uint8)


def _pixels(tg, ii):
    """-> (mask of the live pixels, labels as int64)"""
    t = np.asarray(tg).astype(np.int64)
    return t != ii, t


def focal_terms(x, t, w, gamma):
    """x (n, C) float64 tensor, t (n,) int64 tensor, w (C,) float64 tensor -> (w[t] q^gamma nll, log-softmax rows, p, q, nll), all torch float64"""
    ls = torch.log_softmax(x, dim=1)
    lp = ls.gather(1, t[:, None])[:, 0]
    nll = -lp
    q = -torch.expm1(lp)
    p = torch.exp(lp)
    qg = torch.where(q > 0, q.clamp_min(1e-300) ** gamma, torch.zeros_like(q))
    term = torch.where(q > 0, qg * nll, torch.zeros_like(q))
    return w[t] * term, ls, p, q, nll


def focal_loss_and_grad(lg, tg, ii, w, gamma):
    """-> (loss, gradient (P, C) float64 with zero rows on ignored pixels, D).  Labels must lie inside the classes or equal ii.  D == 0: the loss is
    NaN (0 / 0) and the gradient is not defined (NaN rows on the live pixels)."""
    live, t = _pixels(tg, ii)
    P, C = lg.shape
    g = np.zeros((P, C), np.float64)
    w64 = torch.tensor(np.asarray(w).astype(np.float64))
    D = float(w64.numpy()[t[live]].sum())
    if not live.any():
        return float('nan'), g, D
    x = torch.tensor(np.asarray(lg)[live].astype(np.float64))
    tt = torch.tensor(t[live])
    wterm, ls, p, q, nll = focal_terms(x, tt, w64, gamma)
    with np.errstate(divide='ignore', invalid='ignore'):
        loss = float(wterm.sum()) / D if D != 0.0 else float('nan')
        pn = torch.where(p > 0, p * nll, torch.zeros_like(p))
        qg1 = torch.where(q > 0, q.clamp_min(1e-300) ** (gamma - 1.0), torch.zeros_like(q))
        mod = torch.where(q > 0, qg1 * (q + gamma * pn), torch.zeros_like(q))
        sm = torch.exp(ls)
        sm[torch.arange(sm.shape[0]), tt] -= 1.0
        g[live] = ((w64[tt] * mod)[:, None] * sm).numpy() / D
    return loss, g, D


def focal_autograd(lg, tg, ii, w, gamma):
    """The same loss through float64 autograd -> (loss, gradient (P, C)).  Only for inputs without a pixel whose float64 q is 0."""
    live, t = _pixels(tg, ii)
    x = torch.tensor(np.asarray(lg).astype(np.float64), requires_grad=True)
    w64 = torch.tensor(np.asarray(w).astype(np.float64))
    idx = torch.tensor(np.where(live)[0])
    tt = torch.tensor(t[live])
    wterm = focal_terms(x[idx], tt, w64, gamma)[0]
    loss = wterm.sum() / w64[tt].sum()
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def target_probability(lg, tg, ii):
    """p_t of the live pixels in float64"""
    live, t = _pixels(tg, ii)
    ls = torch.log_softmax(torch.tensor(np.asarray(lg)[live].astype(np.float64)), dim=1)
    return torch.exp(ls.gather(1, torch.tensor(t[live])[:, None])[:, 0]).numpy()

"""numpy restatement of one torch.optim.AdamW step (one group, decoupled decay, no amsgrad, no maximize) on flat arrays, in float64 and float32,
and the error measure the AdamW tests use (csrc/adamw.hip).

    gh = g * grad_scale
    p <- p (1 - lr wd);  m <- m + (1 - b1)(gh - m);  v <- b2 v + (1 - b2) gh gh;  p <- p - ss m / (sqrt(v) / sqrt(1 - b2^t) + eps),  ss = lr / (1 - b1^t)

The scalar factors are formed in Python doubles exactly as torch forms them (1 - lr * wd, 1 - beta, bias corrections, step size) and, for float32,
rounded once to float32 where torch hands them to a kernel.  float32 then performs every tensor operation of torch's single-tensor path
(mul_, lerp_ - from m for a weight below 1/2, from gh above -, mul_ + addcmul_, sqrt / div / add, addcdiv_) with one rounding per operation.

Errors are measured per element in units of u * S, u = 2^-24, with operand scales that account for cancellation - m + w (gh - m) and p - delta
cancel, so ulps of the RESULT read in the tens of thousands for a correct float32 implementation:

    S_m = |m| + |gh|          S_v = v + gh^2          S_p = |p| + ss / (sqrt(v') / sqrt(1 - b2^t) + eps) (|m| + |gh|)

(all from the float64 run on the inputs).  Where the scale is 0 the result must be exact."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24

# lr, beta1, beta2, eps, weight decay, grad_scale, t
CASES = [(1e-3, .9, .999, 1e-8, 1e-2, 1., 1),
         (6e-5, .9, .999, 1e-8, .05, .125, 7),
         (1e-2, .8, .99, 1e-6, 0., 1., 1000),
         (1e-3, .9, .999, 1e-8, 1e-2, .5, 100000)]


def factors(t, lr, b1, b2):
    """(step size lr / (1 - b1^t), sqrt(1 - b2^t)) in Python doubles, as torch.optim.adamw forms them"""
    return lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)


def adamw_step(p, g, m, v, t, lr, b1, b2, eps, wd, grad_scale, dtype=F64):
    """-> (p', m', v') after step number t (1-based), every array operation in `dtype`"""
    dt = np.dtype(dtype).type
    ss, bc2s = factors(t, lr, b1, b2)
    p, g, m, v = (np.asarray(a).astype(dt) for a in (p, g, m, v))
    with np.errstate(all='ignore'):
        gh = g * dt(grad_scale)
        p = p * dt(1.0 - lr * wd)
        w = dt(1.0 - b1)
        m = m + w * (gh - m) if w < 0.5 else gh - (gh - m) * (dt(1) - w)          # torch's lerp: from the nearer end
        v = v * dt(b2) + dt(1.0 - b2) * gh * gh
        denom = np.sqrt(v) / dt(bc2s) + dt(eps)
        p = p + dt(-ss) * (m / denom)
    return p, m, v


def scales(p, g, m, v, t, lr, b1, b2, eps, wd, grad_scale):
    """(S_p, S_m, S_v) of a step, float64"""
    p, g, m, v = (np.asarray(a).astype(F64) for a in (p, g, m, v))
    ss, bc2s = factors(t, lr, b1, b2)
    gh = g * grad_scale
    v1 = b2 * v + (1.0 - b2) * gh * gh
    s_m = np.abs(m) + np.abs(gh)
    with np.errstate(all='ignore'):
        s_p = np.abs(p) + ss / (np.sqrt(v1) / bc2s + eps) * s_m
    s_p = np.where(s_m == 0.0, np.abs(p), s_p)              # (eps = 0 and v' = 0: no update term to scale by)
    return s_p, s_m, v + gh * gh


def worst(got, ref, scale):
    """largest |got - ref| / (u * scale) over the elements; 0 / 0 counts as 0, anything else over a zero scale as inf"""
    err = np.abs(np.asarray(got).astype(F64) - ref)
    with np.errstate(all='ignore'):
        r = np.where(err == 0.0, 0.0, err / (U * scale))
    return float(r.max())


def errors(got, inputs, hyper):
    """got = (p', m', v') of some implementation, inputs = (p, g, m, v), hyper = a CASES row -> worst errors (p, m, v) against float64 in u * S"""
    lr, b1, b2, eps, wd, gs, t = hyper
    ref = adamw_step(*inputs, t, lr, b1, b2, eps, wd, gs, F64)
    s = scales(*inputs, t, lr, b1, b2, eps, wd, gs)
    return tuple(worst(a, r, sc) for a, r, sc in zip(got, ref, s))


def random_state(n, seed):
    """(p, g, m, v) float32: |p| in 1e-3 .. 10, |g| and |m| in 1e-6 .. 1 (log-uniform, random signs), v the square of such a number; zeros planted in
    each of the four alone, in g = m = v together, and in all four"""
    rs = np.random.RandomState(seed)

    def logu(lo, hi):
        return np.exp(rs.uniform(math.log(lo), math.log(hi), n))

    def sign():
        return np.where(rs.rand(n) < 0.5, -1.0, 1.0)

    p = (sign() * logu(1e-3, 10.0)).astype(F32)
    g = (sign() * logu(1e-6, 1.0)).astype(F32)
    m = (sign() * logu(1e-6, 1.0)).astype(F32)
    v = (logu(1e-6, 1.0) ** 2).astype(F32)
    for k, arrs in enumerate(((p,), (g,), (m,), (v,), (g, m, v), (p, g, m, v))):
        idx = np.arange(k, n, 13)[:max(1, n // 40)] if n > 13 else np.arange(0)
        for a in arrs:
            a[idx] = 0.0
    return p, g, m, v

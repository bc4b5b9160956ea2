"""Plain numpy reference of the weight average (csrc/ema.hip, ddp.FlatParams.enable_ema): the decay schedule in float32 exactly as the device
forms it, one update and the k-step recursion in float64, the closed form the recursion is held against (tests/test_ema_host.py), and the SGD step
of tests/spatial_ref.py the fused kernels shadow."""
import numpy as np

from spatial_ref import sgd_step  # noqa: F401  (the optimiser update the fused kernels apply before the average)

F32, F64 = np.float32, np.float64


def decay(t, decay_max, warmup):
    """d_t of update number t (0-based) in float32: min(decay_max, (1 + t) / (10 + t)) under warm-up, else decay_max - every operation a float32
    operation rounded to nearest, as dsrl_ema_advance evaluates it."""
    d = F32(decay_max)
    if warmup:
        tf = F32(t)
        d = min(d, F32(F32(1) + tf) / F32(F32(10) + tf))
    return F32(d)


def omd(t, decay_max, warmup):
    """1 - d_t in float32: the word the element kernels read"""
    return F32(F32(1) - decay(t, decay_max, warmup))


def ema_step(e, p, omd_):
    """e + omd (p - e) with the product and the sum in float64.  The difference is taken in the precision of the inputs: float32 arrays give the
    float32 difference the kernels form (then the only slack against the device's single fma is the second rounding of the float64 result to
    float32), float64 arrays the exact recursion."""
    e, p = np.asarray(e), np.asarray(p)
    diff = (p - e).astype(F64)
    return e.astype(F64) + F64(omd_) * diff


def ema_run(e0, snapshots, decay_max, warmup, t0=0):
    """The k-step recursion in float64: e_0, then e_{j+1} = e_j + (1 - d_{t0+j}) (p_j - e_j) over the snapshots p_0 .. p_{k-1}, with the float32
    schedule.  -> the list [e_1, ..., e_k]"""
    e = np.asarray(e0).astype(F64)
    out = []
    for j, p in enumerate(snapshots):
        e = ema_step(e, np.asarray(p).astype(F64), F64(omd(t0 + j, decay_max, warmup)))
        out.append(e)
    return out


def ema_closed_form(e0, snapshots, decay_max, warmup, t0=0):
    """e_k = prod_i d_i e_0 + sum_j (1 - d_j) prod_{i > j} d_i p_j in float64, with d_i = 1 - omd_i (the weights the recursion really applies)."""
    k = len(snapshots)
    d = [F64(1) - F64(omd(t0 + j, decay_max, warmup)) for j in range(k)]
    acc = np.prod(d) * np.asarray(e0).astype(F64)
    for j, p in enumerate(snapshots):
        acc = acc + (F64(1) - d[j]) * np.prod(d[j + 1:]) * np.asarray(p).astype(F64)
    return acc

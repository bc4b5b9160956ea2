"""AdamW on the device (`-m gpu`; csrc/adamw.hip, ddp.FlatParams.enable_adamw) against tests/adamw_ref.py: one step against
float64 in units of u S (adamw_ref: u = 2^-24, S the operand scale of each quantity), the six launch forms bit for bit against each other, the
edges, the device record, the training step eager and captured, the multi-range schedule and train_or_resume end to end.

Measured on the MI355X, worst error over the sizes and the four cases in u S: p 4.81, m 0.99, v 1.21 (the float32 restatement of torch's
operation sequence on the same inputs: 5.64, 1.12, 2.18; the bound is twice that), case by case at the largest size p 4.81 / 4.48 / 3.28 / 4.44
against 5.64 / 4.46 / 4.32 / 4.71, at n = 1027 p 3.25 / 2.65 / 2.12 / 2.69 against 4.77 / 2.22 / 2.36 / 3.44; the record's two factors 0.00 float32 ulp from the float64 formula at every t looked at."""
import functools
import math
import os
import socket

import numpy as np
import pytest
import torch

import adamw_ref as R
import ema_ref as E
from hip_helpers import DEV, HF

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIZES = [1, 3, 4, 5, 1027, 4 * 2 ** 20 + 4099]          # those of tests/test_ema_gpu.py: scalar tail only, n % 4 != 0, the grid wraps past 4096 x 256 x 4 floats
NMAX, SMALL = SIZES[-1], SIZES[-2]
GUARD = np.float32([1e9, -2e9, 3e9, -4e9, 5e9, -6e9, 7e9, -8e9])
BADARG = 'failed with code -1'                       # include/dsrl_hip.h: DSRL_E_BADARG


def arena(a):
    """`a` followed by guard floats nothing may touch"""
    return torch.from_numpy(np.concatenate([np.asarray(a, F32), GUARD])).to(DEV)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def record(hyper, t=None):
    """a device record for a CASES row at its t (or the given one), the factors written by the device"""
    _, b1, b2, eps, _, _, t0 = hyper
    rec = HF.adamw_record(b1, b2, eps, DEV)
    HF.adamw_set_step_(rec, t0 if t is None else t)
    return rec


def ema_record(omd):
    w = np.zeros(4, np.int32)
    w[:2] = np.array([omd, 0.9], F32).view(np.int32)
    w[2:] = np.array([3, 1], np.uint32).view(np.int32)
    return torch.from_numpy(w).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs():
    """the random state at the largest size; every smaller size takes its first n elements (the planted zeros start at element 0)"""
    return R.random_state(NMAX, 20)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(float64 result, scales, worst errors of the float32 restatement on the whole random state and on its first SMALL elements), once per case"""
    h = R.CASES[case]
    lr, b1, b2, eps, wd, gs, t = h
    ref = R.adamw_step(*inputs(), t, lr, b1, b2, eps, wd, gs, F64)
    s = R.scales(*inputs(), t, lr, b1, b2, eps, wd, gs)
    r32 = R.adamw_step(*inputs(), t, lr, b1, b2, eps, wd, gs, F32)
    return ref, s, tuple(R.worst(a, r, sc) for a, r, sc in zip(r32, ref, s)), tuple(R.worst(a[:SMALL], r[:SMALL], sc[:SMALL]) for a, r, sc in zip(r32, ref, s))


def run_host_form(n, hyper, rec, state=None):
    """dsrl_adamw_step on the first n elements -> the (p, m, v) arenas with their guards, on the host"""
    lr, _, _, _, wd, gs, _ = hyper
    p, g, m, v = (arena(a[:n]) for a in (state or inputs()))
    HF.adamw_step_(p[:n], g[:n], m[:n], v[:n], lr, wd, gs, rec)
    torch.cuda.synchronize()
    assert same_bits(g.cpu().numpy()[:n], (state or inputs())[1][:n])
    return tuple(a.cpu().numpy() for a in (p, m, v))


# ------------------------------------------------------------------------------------------------ value
@pytest.mark.parametrize('n', SIZES)
def test_one_step_against_float64(n):
    """p, m and v of one step from the random state against float64, per element in u S.  Bound per quantity: twice the worst error the float32
    restatement of torch's operation sequence shows on the same inputs (the precedent of tests/calibration_ref.py: the kernel rounds in other
    places - fma, one multiplication by 1 / sqrt(1 - b2^t) instead of a division, lr times the device's 1 / (1 - b1^t) - but no more often).
    "The same inputs" is taken literally at the two large sizes, 1027 and 4 2^20 + 4099.  At n = 1, 3, 4, 5 it cannot be: the restatement's error
    on a handful of elements is whatever those elements happen to give, down to 0, and says nothing about a bound.  Those sizes - the first
    elements of the same state - are held to the restatement's worst error over the first 1027 elements, which contain them: a stated departure
    from the letter of the rule, towards the nearest set of inputs on which the restatement's worst error means something."""
    for case, hyper in enumerate(R.CASES):
        ref, s, e_all, e_small = reference(case)
        e32 = e_small if n <= SMALL else e_all
        out = run_host_form(n, hyper, record(hyper))
        worst = [R.worst(a[:n], r[:n], sc[:n]) for a, r, sc in zip(out, ref, s)]
        print(f'n={n} case {hyper}: p {worst[0]:.2f} m {worst[1]:.2f} v {worst[2]:.2f} u S   (float32 restatement: {e32[0]:.2f} {e32[1]:.2f} {e32[2]:.2f})')
        for a in out:
            assert np.array_equal(a[n:], GUARD), f'n={n} {hyper}: floats after the n-th element changed'
        for w, e, what in zip(worst, e32, 'pmv'):
            assert w <= 2.0 * e, f'n={n} {hyper}: {what} is {w} u S from float64, the float32 restatement {e}'


# ------------------------------------------------------------------------------------------------ bit identities
def segment_table(n, amax, cut=None):
    """rows {first, floats, record} over [0, n - n % 4) cut at `cut` floats (default: the library's 32768); "filters" of three rows share a record"""
    cut = cut or int(HF.query('dsrl_conv2d_filters_amax_segment_floats'))
    rows, filt = [], []
    for i, o in enumerate(range(0, n - n % 4, cut)):
        f = i // 3
        rows.append([o, min(cut, n - n % 4 - o), amax[f].data_ptr() if f % 2 == 0 else 0])
        filt.append(f)
    return rows, filt


@pytest.mark.parametrize('n', SIZES)
def test_forms_are_bit_identical(n):
    """Host-hyper form == _dev form == segment form on p, m and v; each _ema twin == its plain form, its average within one ulp of ema_ref on the
    device's own p and bit-equal to dsrl_ema_update; the arena cut into ranges at multiples of 1024 == one launch; the segment form's records
    hold max |p_new| of their filter, as bit patterns; nothing behind the n-th float (or between the table's end and n) is touched."""
    hyper = R.CASES[1]
    lr, b1, b2, eps, wd, gs, t = hyper
    rec = record(hyper)
    rec0 = bits(rec).copy()
    hyper_dev = torch.tensor([lr, 123.0, wd, gs], dtype=torch.float32, device=DEV)           # slot 1 (SGD's momentum) is not read
    st = tuple(a[:n] for a in inputs())
    e0 = (st[0] + F32(0.1) * np.random.RandomState(n % 9973).standard_normal(n).astype(F32)).astype(F32)
    omd = float(E.omd(3, 0.9, True))
    erec = ema_record(omd)
    want = run_host_form(n, hyper, rec)

    def fresh(with_ema):
        return [arena(a) for a in st] + ([arena(e0)] if with_ema else [])

    def check(name, arenas, upto=n):
        torch.cuda.synchronize()
        p, g, m, v = arenas[:4]
        for a, w, what in ((p, want[0], 'p'), (m, want[1], 'm'), (v, want[2], 'v')):
            a = a.cpu().numpy()
            assert same_bits(a[:upto], w[:upto]), f'n={n} {name}: {what} differs from dsrl_adamw_step'
            assert same_bits(a[upto:n], np.asarray(st['pgmv'.index(what)])[upto:n]) and np.array_equal(a[n:], GUARD), f'n={n} {name}: {what} written out of range'
        assert same_bits(g.cpu().numpy()[:n], st[1])
        if len(arenas) == 5:
            e = arenas[4].cpu().numpy()
            ref = E.ema_step(e0[:upto], want[0][:upto], F32(omd))
            ulp = np.spacing(np.abs(ref).astype(F32)).astype(F64)
            worst = float((np.abs(e[:upto].astype(F64) - ref) / ulp).max()) if upto else 0.0
            assert worst <= 1.0, f'n={n} {name}: average {worst} ulp from ema_ref'
            assert same_bits(e[upto:n], e0[upto:n]) and np.array_equal(e[n:], GUARD)
            E5, Pn = arena(e0), arena(want[0][:n])
            HF.ema_update_(E5[:n], Pn[:n], erec)
            torch.cuda.synchronize()
            assert same_bits(bits(E5)[:upto], e[:upto].view(np.uint32)), f'n={n} {name}: fused and unfused averages differ'

    a = fresh(False); HF.adamw_step_dev_(a[0][:n], a[1][:n], a[2][:n], a[3][:n], hyper_dev, rec); check('adamw_step_dev', a)
    a = fresh(True); HF.adamw_step_ema_(a[0][:n], a[1][:n], a[2][:n], a[3][:n], lr, wd, gs, rec, a[4][:n], erec); check('adamw_step_ema', a)
    a = fresh(True); HF.adamw_step_dev_ema_(a[0][:n], a[1][:n], a[2][:n], a[3][:n], hyper_dev, rec, a[4][:n], erec); check('adamw_step_dev_ema', a)
    # ranges at multiples of 1024, each a launch of its own
    if n > 1024:
        cuts = [0, 1024, 1024 * 37, 1024 * 2049, n] if n > 1024 * 2049 else [0, 1024, n]
        a = fresh(True)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            HF.adamw_step_dev_ema_(a[0][lo:hi], a[1][lo:hi], a[2][lo:hi], a[3][lo:hi], hyper_dev, rec, a[4][lo:hi], erec)
        check('ranges', a)
    # the segment forms, on the whole float4 of the arena
    n4 = n - n % 4
    if n4:
        for with_ema in (False, True):
            nf = -(-n4 // (3 * 32768))
            amax = torch.zeros(nf, HF.AMAX_WORDS, dtype=torch.int32, device=DEV)
            rows, filt = segment_table(n, amax)
            assert max(r[1] for r in rows) <= 32768 and sum(r[1] for r in rows) == n4
            tab = torch.tensor(rows, dtype=torch.int64, device=DEV)
            a = fresh(with_ema)
            tail = (a[4].data_ptr(), erec.data_ptr()) if with_ema else ()
            HF.call('dsrl_adamw_step_dev_segments' + ('_ema' if with_ema else ''), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(),
                    tab.data_ptr(), len(rows), hyper_dev.data_ptr(), rec.data_ptr(), *tail, HF._stream())
            check('segments' + ('_ema' if with_ema else ''), a, upto=n4)
            got = amax.cpu().numpy().view(np.uint32).max(axis=1)
            for f in range(nf):
                lo, hi = f * 3 * 32768, min((f + 1) * 3 * 32768, n4)
                exp = int(np.abs(want[0][lo:hi]).max().view(np.uint32)) if f % 2 == 0 else 0
                assert int(got[f]) == exp, f'n={n}: amax record of filter {f}: {int(got[f]):#x}, max |p_new| {exp:#x}'
    assert np.array_equal(bits(rec), rec0) and np.array_equal(bits(erec), bits(ema_record(omd))), 'the records are read only'


# ------------------------------------------------------------------------------------------------ edges
def test_zero_state_and_zero_decay():
    """g = m = v = 0: p (1 - lr wd) bit for bit - the float32 product by the float32 difference 1 - lr wd -, m and v stay 0; with wd = 0 p keeps its
    bits, -0 and denormals included."""
    lr, b1, b2, eps, wd, gs, t = hyper = R.CASES[0]
    n = 1027
    p0 = inputs()[0][:n].copy()
    p0[:4] = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff], np.uint32).view(F32)
    z = np.zeros(n, F32)
    rec = record(hyper)
    p, m, v = run_host_form(n, hyper, rec, state=(p0, z, z, z))
    assert same_bits(p[:n], p0 * (F32(1) - F32(lr) * F32(wd))) and not bits(torch.from_numpy(m[:n])).any() and not bits(torch.from_numpy(v[:n])).any()
    p, m, v = run_host_form(n, (lr, b1, b2, eps, 0.0, gs, t), rec, state=(p0, z, z, z))
    assert same_bits(p[:n], p0) and not m[:n].any() and not v[:n].any()


def test_eps_zero_and_zero_betas():
    """eps = 0 with v > 0 stays finite; beta1 = 0 and beta2 = 0 are accepted: m = gh and v = gh^2 exactly, the update is lr sign(gh)."""
    n = 1027
    p0, g0, m0, v0 = (a[:n].copy() for a in inputs())
    v0 = np.maximum(v0, F32(1e-12))
    hyper = (1e-3, .9, .999, 0.0, 1e-2, 1., 7)
    out = run_host_form(n, hyper, record(hyper), state=(p0, g0, m0, v0))
    assert all(np.isfinite(a[:n]).all() for a in out)
    ref = R.adamw_step(p0, g0, m0, v0, 7, 1e-3, .9, .999, 0.0, 1e-2, 1., F64)
    e32 = R.errors(R.adamw_step(p0, g0, m0, v0, 7, 1e-3, .9, .999, 0.0, 1e-2, 1., F32), (p0, g0, m0, v0), hyper)
    got = R.errors(tuple(a[:n] for a in out), (p0, g0, m0, v0), hyper)
    assert all(a <= 2 * b for a, b in zip(got, e32)), (got, e32)
    assert np.isfinite(ref[0]).all()
    hyper = (1e-3, 0., 0., 1e-8, 0., 1., 5)
    rec = record(hyper)
    r = HF.adamw_record_read(rec)
    assert (r['ss_factor'], r['isq'], r['t']) == (1.0, 1.0, 5)
    g1 = np.where(g0 == 0, F32(0.5), g0)
    p, m, v = run_host_form(n, hyper, rec, state=(p0, g1, m0, v0))
    assert same_bits(m[:n], g1) and same_bits(v[:n], g1 * g1)
    big = np.abs(g1) > 1e-3                                  # eps = 1e-8 is below half an ulp of |gh|: the quotient is +-1 to the last bit or two
    big &= np.abs(p0) < 1                                    # ... and the update of 1e-3 is resolved to 1e-4 of itself in p
    assert big.sum() > 100 and np.abs((p0 - p[:n])[big] / F32(1e-3) - np.sign(g1[big])).max() < 1e-3


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_nonfinite_gradient_stays_in_its_element(bad):
    """A NaN or infinite gradient element: its own p, m and v are what the float64 reference makes of it (NaN everywhere for a NaN; m = +-inf,
    v = inf and p = NaN = inf / inf for an infinity), every other element is bit-equal to the run without it.  One in a float4 and one in the tail."""
    hyper = R.CASES[1]
    lr, b1, b2, eps, wd, gs, t = hyper
    n = 1027
    st = [a[:n].copy() for a in inputs()]
    rec = record(hyper)
    clean = run_host_form(n, hyper, rec, state=tuple(st))
    where = [518, 1025]
    st[1][where] = bad
    out = run_host_form(n, hyper, rec, state=tuple(st))
    ref = R.adamw_step(*st, t, lr, b1, b2, eps, wd, gs, F64)
    others = np.ones(n, bool); others[where] = False
    for a, c, r, what in zip(out, clean, ref, 'pmv'):
        assert same_bits(a[:n][others], c[:n][others]), f'{what}: a neighbour of the {bad} gradient changed'
        assert np.array_equal(np.isnan(a[:n][where]), np.isnan(r[where])) and np.array_equal(a[:n][where][~np.isnan(r[where])], r[where][~np.isnan(r[where])]), (what, a[:n][where], r[where])
    assert np.isnan(out[0][where]).all()


# ------------------------------------------------------------------------------------------------ record
@pytest.mark.parametrize('b1,b2', [(0.9, 0.999), (0.8, 0.99), (0.0, 0.0), (0.5, 0.9999)])
def test_advance_and_set_step(b1, b2):
    """k advances from a fresh record: t = k and both factors within one float32 ulp of the float64 formula rounded to float32 (checked at every k up
    to 40, then at a spread of k up to 3000); set_step(k) gives the bits of k advances, also far out (t = 10^5, 10^7) where beta^t has underflowed."""
    rec = HF.adamw_record(b1, b2, 1e-8, DEV)
    seen = {}
    look = set(range(1, 41)) | {100, 691, 1000, 2302, 3000}
    for k in range(1, 3001):
        HF.adamw_advance_(rec)
        if k in look:
            seen[k] = rec.clone()
    torch.cuda.synchronize()
    worst = 0.0
    for k, r in seen.items():
        got = HF.adamw_record_read(r)
        assert got['t'] == k and got['beta1'] == b1 and got['beta2'] == b2
        for name, exact in (('ss_factor', 1.0 / (1.0 - b1 ** k)), ('isq', 1.0 / math.sqrt(1.0 - b2 ** k))):
            want = F32(exact)
            d = abs(float(F32(got[name])) - float(want)) / float(np.spacing(want))
            worst = max(worst, d)
            assert d <= 1.0, (k, name, got[name], want)
        s = HF.adamw_record(b1, b2, 1e-8, DEV)
        HF.adamw_set_step_(s, k)
        assert np.array_equal(bits(s), bits(r)), f'set_step({k}) differs from {k} advances'
    print(f'betas ({b1}, {b2}): factors at most {worst:.2f} float32 ulp from the float64 formula')
    for k in (10 ** 5, 10 ** 7):
        s = HF.adamw_record(b1, b2, 1e-8, DEV)
        HF.adamw_set_step_(s, k - 1)
        HF.adamw_advance_(s)
        s2 = HF.adamw_record(b1, b2, 1e-8, DEV)
        HF.adamw_set_step_(s2, k)
        assert np.array_equal(bits(s), bits(s2)) and HF.adamw_record_read(s)['t'] == k
        assert HF.adamw_record_read(s)['ss_factor'] == 1.0


def test_bad_arguments_are_refused():
    n = 64
    z = [torch.zeros(n + 8, device=DEV) for _ in range(5)]
    hyper = R.CASES[0]
    lr, _, _, _, wd, gs, _ = hyper
    hyper_dev = torch.tensor([lr, 0.0, wd, gs], dtype=torch.float32, device=DEV)
    rec, erec = record(hyper), ema_record(0.1)
    rec0 = bits(rec).copy()
    odd = torch.zeros(20, dtype=torch.int32, device=DEV)[1:17]           # a record 4 bytes off
    odd_e = torch.zeros(8, dtype=torch.int32, device=DEV)[1:5]
    tab = torch.tensor([[0, n, 0]], dtype=torch.int64, device=DEV)
    S = HF._stream

    def every_form(a, r, er):
        """the six launches on arenas `a` (tensors, or None for a null pointer) and records r, er"""
        ptr = [0 if x is None else x.data_ptr() for x in a]
        r, er, hy = r.data_ptr(), er.data_ptr(), hyper_dev.data_ptr()
        return [lambda: HF.call('dsrl_adamw_step', *ptr[:4], n, lr, wd, gs, r, S()),
                lambda: HF.call('dsrl_adamw_step_dev', *ptr[:4], n, hy, r, S()),
                lambda: HF.call('dsrl_adamw_step_dev_segments', *ptr[:4], tab.data_ptr(), 1, hy, r, S()),
                lambda: HF.call('dsrl_adamw_step_ema', *ptr[:4], n, lr, wd, gs, r, ptr[4], er, S()),
                lambda: HF.call('dsrl_adamw_step_dev_ema', *ptr[:4], n, hy, r, ptr[4], er, S()),
                lambda: HF.call('dsrl_adamw_step_dev_segments_ema', *ptr[:4], tab.data_ptr(), 1, hy, r, ptr[4], er, S())]

    for k in range(5):                                                  # each arena in turn one float off, then null
        for broken in (z[k][1:n + 1], None):
            a = [broken if i == k else x[:n] for i, x in enumerate(z)]
            for j, launch in enumerate(every_form(a, rec, erec)):
                if k == 4 and j < 3:
                    continue                                            # the forms without an average do not take it
                with pytest.raises(HF.DsrlHipError, match=BADARG):
                    launch()
    a = [x[:n] for x in z]
    for launch in every_form(a, odd, erec) + every_form(a, rec, odd_e)[3:]:
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            launch()
    for nbad in (0, -4):
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.call('dsrl_adamw_step', *[x.data_ptr() for x in a[:4]], nbad, lr, wd, gs, rec.data_ptr(), S())
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.call('dsrl_adamw_step_dev_segments', *[x.data_ptr() for x in a[:4]], tab.data_ptr(), nbad, hyper_dev.data_ptr(), rec.data_ptr(), S())
    for r in (odd, ):
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.adamw_advance_(r)
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.adamw_set_step_(r, 3)
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.call('dsrl_adamw_advance', None, S())
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.adamw_set_step_(rec, -1)
    with pytest.raises(HF.DsrlHipError):
        HF.adamw_step_(z[0][:n], z[1][:n], z[2][:n], z[3][:n - 4], lr, wd, gs, rec)       # arenas of two sizes
    with pytest.raises(HF.DsrlHipError):
        HF.adamw_step_(z[0][:n], z[1][:n], z[2][:n], z[3][:n], lr, wd, gs, erec)          # a 16-byte record
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0.0 for x in z) and np.array_equal(bits(rec), rec0)      # nothing ran


# ------------------------------------------------------------------------------------------------ FlatParams and TrainStep
LR, MOM, WD = 1e-4, 0.9, 1e-2


def _model():
    """the fixture of tests/test_ema_gpu.py::_build: DSRL(3) on the Cityscapes settings"""
    import dualsuperreslearningforsemseg_amd as D
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    torch.manual_seed(54321)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    return model.to(DEV).to(memory_format=torch.channels_last).train(), cs


def _build(graph, adamw=True, clip=None, ema=None, world_claim=1):
    """the smallest training step the existing step tests use: DSRL(3), batch 2 at 64 x 128, SyntheticCityscapes"""
    from dualsuperreslearningforsemseg_amd import ddp
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    model, cs = _model()
    if world_claim > 1:
        real = ddp.dist.get_world_size
        ddp.dist.get_world_size = lambda group=None: world_claim       # the collectives still run on the 1-rank group
        try:
            flat = ddp.FlatParams(model, chunk_bytes=16 << 20)
        finally:
            ddp.dist.get_world_size = real
    else:
        flat = ddp.FlatParams(model)
    if adamw:
        flat.enable_adamw()
    if ema is not None:
        flat.enable_ema(*ema)
    if clip is not None:
        flat.enable_grad_clip(clip)
    HF.set_dropout_seed(4242)
    step = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph)
    batch = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    return model, flat, step, batch


def _one(step, batch, lr=LR):
    (img, org), (tgt, _) = batch
    return step(img, org, tgt, lr, MOM, WD, True)[0]


class _pinned:
    """one summation order in eager and captured steps (tests/test_rccl_gpu.py)"""

    def __enter__(self):
        self.was = HF.overlap_wgrad
        HF.overlap_wgrad = False
        HF.set_bn_fused_max_blocks(128)

    def __exit__(self, *exc):
        HF.overlap_wgrad = self.was
        HF.set_bn_fused_max_blocks(None)


def test_flat_params_forms_ranges_and_clipping():
    """FlatParams with AdamW on a gradient arena of known norm: the host form, the device form (the segment launch under the f16 arithmetics) and the
    four-range schedule give the same p, m and v, each pass advances t once; grad_clip = inf changes nothing; a small max_norm is the unclipped
    launch at grad_scale = coef, coef read from grad_clip_stats; the average follows when it is on."""
    from dualsuperreslearningforsemseg_amd import ddp
    model, _ = _model()
    flat = ddp.FlatParams(model)
    flat.enable_adamw((0.9, 0.999), 1e-8)
    with pytest.raises(HF.DsrlHipError, match='already enabled'):
        flat.enable_adamw()
    flat.enable_ema(0.9, True)
    gen = torch.Generator(device=DEV).manual_seed(77)
    flat.g_flat.copy_(torch.randn(flat.numel, device=DEV, generator=gen) * 0.01)
    flat.m_flat.copy_(torch.randn(flat.numel, device=DEV, generator=gen) * 0.01)
    flat.v_flat.copy_((torch.randn(flat.numel, device=DEV, generator=gen) * 0.01) ** 2)
    HF.adamw_set_step_(flat.adamw_rec, 6)
    p0, m0, v0, e0, erec0, arec0 = (a.clone() for a in (flat.p_flat, flat.m_flat, flat.v_flat, flat.e_flat, flat.ema_rec, flat.adamw_rec))
    hyper = torch.tensor([LR, MOM, WD, 1.0], dtype=torch.float32, device=DEV)

    def fresh():
        with torch.no_grad():
            for a, b in ((flat.p_flat, p0), (flat.m_flat, m0), (flat.v_flat, v0), (flat.e_flat, e0), (flat.ema_rec, erec0), (flat.adamw_rec, arec0)):
                a.copy_(b)

    def state():
        torch.cuda.synchronize()
        assert flat.adamw_step_count() == 7
        return tuple(a.clone() for a in (flat.p_flat, flat.m_flat, flat.v_flat, flat.e_flat))

    def same(a, b):
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

    flat.sgd_step(LR, MOM, WD, reduce=False)
    plain = state()
    assert not torch.equal(plain[0], p0) and not torch.equal(plain[3], e0)
    # against the element kernel on the arenas, at t = 7
    P, M, V, Ev = (a.clone() for a in (p0, m0, v0, e0))
    rec7 = arec0.clone(); HF.adamw_advance_(rec7)
    HF.adamw_step_ema_(P, flat.g_flat, M, V, LR, WD, 1.0, rec7, Ev, erec0.clone())
    torch.cuda.synchronize()
    assert same((P, M, V, Ev), plain)
    calls = {'device form': lambda: flat.sgd_step(0.0, 0.0, 0.0, hyper=hyper, reduce=False),
             'four ranges, host': lambda: flat.reduce_chunked_and_step(hp=(LR, MOM, WD), nchunks=4),
             'four ranges, device': lambda: flat.reduce_chunked_and_step(hyper=hyper, nchunks=4)}
    for name, call in calls.items():
        fresh()
        ranges = call()
        assert same(state(), plain), name
        assert ranges is None or (len(ranges) == 4 and all(a % 1024 == 0 for a, _ in ranges))
    if flat._fold_amax():
        # the segment launch left the filters' magnitudes: what the measuring sweep finds on the same parameters
        left = flat.filters.amax.clone()
        flat.filters.amax.zero_()
        flat.filters.measure(streaming=True)
        torch.cuda.synchronize()
        assert torch.equal(left.view(-1, HF.AMAX_WORDS).view(torch.int32).max(dim=1).values,
                           flat.filters.amax.view(-1, HF.AMAX_WORDS).view(torch.int32).max(dim=1).values)
    # --- monitoring only, then a threshold at a third of the norm
    true_norm = float(flat.g_flat.double().pow(2).sum().sqrt())
    flat.enable_grad_clip(float('inf'))
    for name, call in [('host form', lambda: flat.sgd_step(LR, MOM, WD, reduce=False))] + list(calls.items()):
        fresh()
        call()
        assert same(state(), plain), f'grad_clip = inf changed the step ({name})'
    flat.set_grad_clip_max_norm(true_norm / 3.0)
    fresh()
    flat.sgd_step(LR, MOM, WD, reduce=False)
    clipped = state()
    coef = flat.grad_clip_stats()['coef']
    assert 0.3 < coef < 0.34 and not same(clipped[:1], plain[:1])
    P, M, V, Ev = (a.clone() for a in (p0, m0, v0, e0))
    HF.adamw_step_ema_(P, flat.g_flat, M, V, LR, WD, coef, rec7, Ev, erec0.clone())
    torch.cuda.synchronize()
    assert same((P, M, V, Ev), clipped), 'the clipped step is not the unclipped kernel at grad_scale = coef'
    # ... and the reference on g * coef, in the units of the value test
    sl = slice(0, 1 << 20)
    st = tuple(a[sl].cpu().numpy() for a in (p0, flat.g_flat, m0, v0))
    h = (LR, 0.9, 0.999, 1e-8, WD, coef, 7)
    e32 = R.errors(R.adamw_step(*st, 7, LR, 0.9, 0.999, 1e-8, WD, coef, F32), st, h)
    got = R.errors(tuple(a[sl].cpu().numpy() for a in clipped[:3]), st, h)
    print('clipped step against the reference on g * coef (p, m, v) in u S:', ['%.2f' % x for x in got], ' float32 restatement:', ['%.2f' % x for x in e32])
    assert all(a <= 2 * b for a, b in zip(got, e32)), (got, e32)
    for name, call in calls.items():
        fresh()
        call()
        assert same(state(), clipped), name
    # the state dict carries what the arenas hold
    sd = flat.state_dict(LR, MOM, WD)
    ps = [p for p in model.parameters() if p.requires_grad]
    for i in (0, len(ps) // 2, len(ps) - 1):
        o = flat.offsets[flat._index[id(ps[i])]]
        assert float(sd['state'][i]['step']) == 7.0
        assert torch.equal(sd['state'][i]['exp_avg_sq'], flat.v_flat.as_strided(ps[i].shape, ps[i].stride(), o).cpu().contiguous())


@functools.lru_cache(maxsize=None)
def _scenario(graph, adamw=True, clip=None):
    """GRAPH_WARMUP + 2 training steps -> (losses, p, m, v or None, t or None after step 3 and after the last step, graph facts)"""
    with _pinned():
        model, flat, step, batch = _build(graph, adamw=adamw, clip=clip)
        hist, snaps = [], []
        for i in range(step.GRAPH_WARMUP + 2):
            hist.append(_one(step, batch))
            if i + 1 >= 3:
                torch.cuda.synchronize()
                snaps.append((flat.p_flat.cpu(), flat.m_flat.cpu(), None if flat.v_flat is None else flat.v_flat.cpu(),
                              flat.adamw_step_count() if adamw else None))
        (img, org), (tgt, _) = batch
        facts = (step.graph_replays, len(step._graphs), step._graph_key(img, org, tgt)[7])
        if adamw and flat._fold_amax() and flat._amax_key == flat._params_key():
            # the segment launch of the last step left max |p_new| of every filter: what the measuring sweep finds on the same parameters
            print(f'graph={graph}: filter magnitudes left by dsrl_adamw_step_dev_segments against the measuring sweep')
            left = flat.filters.amax.clone()
            flat.filters.amax.zero_()
            flat.filters.measure(streaming=True)
            torch.cuda.synchronize()
            per_filter = lambda a: a.view(-1, HF.AMAX_WORDS).max(dim=1).values
            assert torch.equal(per_filter(left), per_filter(flat.filters.amax)) and int(per_filter(left).max()) > 0
        if adamw and not graph:
            step.split = True
            with pytest.raises(HF.DsrlHipError, match='DSRL_GRAPH_SPLIT'):
                _one(step, batch)
            step.split = False
        step.release()
        return hist, snaps, facts


def _same_snap(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_train_step_eager_and_captured_agree():
    """TrainStep with AdamW, eager against the captured graph: losses, p, m and v bit-equal after the third iteration (the first replay) and the
    fourth; t counts every step, replays included; "AdamW enabled" is part of the graph key."""
    eager, graph = _scenario(False), _scenario(True)
    assert eager[0] == graph[0] and np.isfinite(eager[0]).all(), (eager[0], graph[0])
    for a, b, k in zip(eager[1], graph[1], (3, 4)):
        assert _same_snap(a, b), f'after step {k}'
        assert a[3] == k
    assert float(eager[1][-1][2].abs().sum()) > 0 and not torch.equal(eager[1][0][0], eager[1][1][0])
    assert eager[2] == (0, 0, True) and graph[2] == (2, 1, True)


def test_grad_clip_inf_with_adamw_is_adamw_alone():
    plain, mon = _scenario(True), _scenario(True, clip=float('inf'))
    assert plain[0] == mon[0] and all(_same_snap(a, b) for a, b in zip(plain[1], mon[1]))


def test_default_run_has_no_adamw():
    """dataset['optimizer'] absent: no v_flat, no record and not one AdamW entry point called; the step is the SGD one - p and m after an eager step
    are those of the SGD element kernel on the step's gradients, bit for bit -, and "AdamW enabled" in the graph key is False."""
    base = _scenario(True, adamw=False)
    assert base[2] == (2, 1, False) and base[1][0][2] is None and np.isfinite(base[0]).all()
    real = HF.call

    def no_adamw(name, *a):
        assert 'adamw' not in name, name
        return real(name, *a)
    with _pinned():
        model, flat, step, batch = _build(False, adamw=False)
        assert flat.v_flat is None and flat.adamw_rec is None and flat.adamw_config is None
        p0, m0 = flat.p_flat.clone(), flat.m_flat.clone()
        HF.call = no_adamw
        try:
            loss = _one(step, batch)
        finally:
            HF.call = real
        torch.cuda.synchronize()
        assert loss == base[0][0]
        HF.sgd_step_(p0, flat.g_flat, m0, LR, MOM, WD, 1.0)
        torch.cuda.synchronize()
        assert torch.equal(p0.view(torch.int32), flat.p_flat.view(torch.int32)) and torch.equal(m0.view(torch.int32), flat.m_flat.view(torch.int32))
        assert 'exp_avg' not in flat.state_dict(LR, MOM, WD)['state'][0]
        step.release()


def test_multi_rank_schedule_one_advance_per_step(monkeypatch):
    """A 1-rank 'nccl' group with a claimed world of 2 (tests/test_ema_gpu.py::test_multi_rank_schedule_one_omd_per_step), one captured graph per
    step and the exchange + update behind it in four ranges: one advance per step, in front of the four range launches, all of which therefore
    read the same t - p, m, v and the average are bit-equal to the same run with the update in ONE range."""
    import torch.distributed as dist
    monkeypatch.setenv('DSRL_GRAPH_SPLIT', '0')
    steps = 4
    out = {}
    with _pinned():
        s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
        dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1, device_id=torch.device(DEV))
        real = HF.call
        try:
            for nchunks in (4, 1):
                monkeypatch.setenv('DSRL_REDUCE_CHUNKS', str(nchunks))
                model, flat, step, batch = _build(True, ema=(0.9, True), world_claim=2)
                assert flat.world == 2
                log = []

                def logged(name, *a, _log=log):
                    if 'adamw' in name or 'sgd' in name:
                        _log.append(name)
                    return real(name, *a)
                HF.call = logged
                hist = []
                for _ in range(steps):
                    log.append('step')
                    hist.append(_one(step, batch))
                HF.call = real
                torch.cuda.synchronize()
                assert step.graph_replays == steps - step.GRAPH_WARMUP and flat.defer_collectives and not step.split
                launch = 'dsrl_adamw_step_dev_segments_ema' if flat._fold_amax() else 'dsrl_adamw_step_dev_ema'
                assert log == (['step', 'dsrl_adamw_advance'] + [launch] * nchunks) * steps, log
                assert flat.adamw_step_count() == steps and flat.ema_updates() == steps
                out[nchunks] = (hist, flat.p_flat.clone(), flat.m_flat.clone(), flat.v_flat.clone(), flat.e_flat.clone())
                step.release()
                del model, flat, step
        finally:
            HF.call = real
            dist.destroy_process_group()
    assert out[4][0] == out[1][0]
    for a, b in zip(out[4][1:], out[1][1:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ train_or_resume
def test_train_or_resume_with_adamw_and_resume(tmp_path, monkeypatch):
    """dataset['optimizer'] = 'adamw' with the weight average, two epochs of two iterations: the epoch records say so, momentum draws one warning,
    the checkpoint's optimizer_state_dict loads into a CPU torch.optim.AdamW and its tensors are the arenas', bit for bit; a resume from the epoch-1
    checkpoint ends with the p, m, v and t bits of the uninterrupted run."""
    import dualsuperreslearningforsemseg_amd as D
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as T
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs

    def factory(split, batch_size, device, rank, world):
        return T.SyntheticCityscapes(batch_size, (32, 64), device, rank=rank, length=2)

    def load(*parts):
        return torch.load(os.path.join(*parts), map_location='cpu', weights_only=False)

    def kw(exp, **dataset):
        return dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                    dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': factory, **dataset}, val_interval=1, checkpoint_interval=1,
                    checkpoint_history=2, init_weights=None, batch_size=2, epochs=2, learning_rate=1e-4, end_learning_rate=1e-5, momentum=0.9,
                    weights_decay=1e-2, poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / exp),
                    description='test', early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))

    flats, keys = [], {}
    real_flat, real_epoch = T.FlatParams, T._do_train_val

    def flat_spy(model, *a, **k):
        flats.append(real_flat(model, *a, **k))
        return flats[-1]

    def epoch_spy(do_train, epoch, *a, **k):
        if do_train:
            keys.setdefault(epoch, dict(HF._rng_state))               # the dropout key position at which the epoch's training starts
        return real_epoch(do_train, epoch, *a, **k)
    monkeypatch.setattr(T, 'FlatParams', flat_spy)
    monkeypatch.setattr(T, '_do_train_val', epoch_spy)
    with pytest.raises(ValueError, match='optimizer'):
        T.train_or_resume(is_resuming_training=False, **kw('bad', optimizer={'name': 'adamw', 'betas': (0.9, 1.0)}))
    assert not os.path.exists(str(tmp_path / 'bad')) and not flats
    with _pinned():
        HF.set_dropout_seed(777)
        with pytest.warns(UserWarning, match='momentum') as caught:
            hist = T.train_or_resume(is_resuming_training=False, **kw('exp', optimizer='adamw', ema=0.9))
        assert sum('momentum' in str(w.message) for w in caught) == 1
        assert len(hist) == 3 and all(h['optimizer'] == 'adamw' for h in hist[:2]) and all(np.isfinite(v) for h in hist[:2] for v in h['train'][:4])
        flat = flats[-1]
        torch.cuda.synchronize()
        assert flat.adamw_step_count() == 4 and flat.ema_updates() == 4
        ckdir = os.path.join(str(tmp_path / 'exp'), settings.CHECKPOINTS_DIR.format(stage=3))
        ck = load(ckdir, settings.CHECKPOINT_FILE.format(epoch=2))
        assert set(ck) == set(settings.VARIABLES_IN_CHECKPOINT) | {'ema_state_dict'} and ck['momentum'] == 0.9
        osd = ck['optimizer_state_dict']
        cpu_model = D.DSRL(3, cs)
        ps = [p for p in cpu_model.parameters() if p.requires_grad]
        opt = torch.optim.AdamW(ps, lr=1.0)
        opt.load_state_dict(osd)
        g = opt.param_groups[0]
        assert (g['betas'], g['eps'], g['weight_decay'], g['amsgrad'], g['initial_lr']) == ((0.9, 0.999), 1e-8, 1e-2, False, 1e-4)
        assert g['lr'] == hist[1]['lr'] and len(opt.state) == len(ps) == len(flat.params)
        live = [p for p in flat.model.parameters() if p.requires_grad]
        for cp, lp in zip(ps, live):
            st = opt.state[cp]
            o = flat.offsets[flat._index[id(lp)]]
            assert float(st['step']) == 4.0
            for key, arena_ in (('exp_avg', flat.m_flat), ('exp_avg_sq', flat.v_flat)):
                assert torch.equal(st[key].view(torch.int32), arena_.as_strided(lp.shape, lp.stride(), o).cpu().contiguous().view(torch.int32)), key
        assert float(flat.v_flat.abs().sum()) > 0
        end = tuple(a.cpu() for a in (flat.p_flat, flat.m_flat, flat.v_flat, flat.e_flat))
        # --- the same two epochs, the second one from the epoch-1 checkpoint
        ck1 = load(ckdir, settings.CHECKPOINT_FILE.format(epoch=1))
        assert float(ck1['optimizer_state_dict']['state'][0]['step']) == 2.0
        HF.set_dropout_seed(777)
        HF._rng_state.update(keys[2])
        with pytest.warns(UserWarning, match='momentum'):
            T.train_or_resume(is_resuming_training=True, model_state_dict=ck1['model_state_dict'], optimizer_state_dict=ck1['optimizer_state_dict'],
                              epoch=ck1['epoch'], best_validation_dict=ck1['best_validation_dict'], ema_state_dict=ck1['ema_state_dict'],
                              **kw('exp_resumed', optimizer='adamw', ema=0.9))
        flat2 = flats[-1]
        torch.cuda.synchronize()
        assert flat2 is not flat and flat2.adamw_step_count() == 4
        for a, b, what in zip((flat2.p_flat, flat2.m_flat, flat2.v_flat, flat2.e_flat), end, ('p', 'm', 'v', 'average')):
            assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), f'{what} after the resume differs from the uninterrupted run'
        # --- the other optimiser's state is refused
        with pytest.raises(ValueError, match=r'(?s)AdamW.*SGD'):
            T.train_or_resume(is_resuming_training=True, model_state_dict=ck1['model_state_dict'], optimizer_state_dict=ck1['optimizer_state_dict'],
                              epoch=ck1['epoch'], best_validation_dict=ck1['best_validation_dict'], **kw('exp_mixed'))

"""The weight average on the device (`-m gpu`; csrc/ema.hip, ddp.FlatParams.enable_ema) against tests/ema_ref.py: the fused SGD
launches bit for bit against their twins without the average, the average itself to one float32 ulp of the float64 update, the schedule kernel
bit for bit against the float32 formula, the in-place swap on every bit pattern, and the training step, the multi-rank schedule and
train_or_resume end to end.

u = 2^-24 is the unit roundoff of float32.  The library is built with -ffp-contract=off: the average is ONE float32 difference and ONE fma per
element and step."""
import functools
import os
import socket

import numpy as np
import pytest
import torch

import ema_ref as E
from hip_helpers import DEV, HF

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIZES = [1, 3, 4, 5, 1027, 4 * 2 ** 20 + 4099]          # scalar tail only, n % 4 != 0, and more than 4096 blocks x 256 threads x 4 floats (the grid wraps)
SGD_HYPER = [(0.006, 0.9, 5e-4, 1.0), (0.1, 0.9, 0.0, 0.125)]       # lr, momentum, weight decay, grad_scale
GUARD = np.float32([1e9, -2e9, 3e9, -4e9, 5e9, -6e9, 7e9, -8e9])
BADARG = 'failed with code -1'                       # include/dsrl_hip.h: DSRL_E_BADARG


def arena(a):
    """`a` followed by guard floats nothing may touch"""
    return torch.from_numpy(np.concatenate([np.asarray(a, F32), GUARD])).to(DEV)


def record(omd, decay_max=0.9, updates=0, warmup=1):
    """an EMA record with a given omd word"""
    w = np.zeros(4, np.int32)
    w[:2] = np.array([omd, decay_max], F32).view(np.int32)
    w[2:] = np.array([updates, warmup], np.uint32).view(np.int32)
    return torch.from_numpy(w).to(DEV)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def assert_one_ulp(e_dev, e0, p_new, omd, what):
    """the device's fma(omd, p_new - e0, e0) against the reference: float32 difference, then product and sum in float64 - the second rounding (of
    the float64 result to float32) is the only slack"""
    ref = E.ema_step(e0, p_new, F32(omd))
    err = np.abs(e_dev.astype(F64) - ref)
    ulp = np.spacing(np.abs(ref).astype(F32)).astype(F64)
    worst = float((err / ulp).max())
    print(f'{what}: largest error {worst:.3f} ulp')
    assert worst <= 1.0, f'{what}: {worst} ulp'


# ------------------------------------------------------------------------------------------------ element kernels
@pytest.mark.parametrize('n', SIZES)
def test_fused_sgd_ema_against_twins(n):
    """dsrl_sgd_step_ema and dsrl_sgd_step_dev_ema: p and buf bit-equal to dsrl_sgd_step / dsrl_sgd_step_dev on the same inputs, the average within
    one ulp of the float64 update of the device's own p_new, bit-equal between the two entry points and bit-equal to the twin followed by
    dsrl_ema_update; nothing behind the n-th float is touched."""
    rs = np.random.RandomState(n % 9973 + 1)
    p0, b0, g = (rs.standard_normal(n).astype(F32) for _ in range(3))
    e0 = (p0 + 0.1 * rs.standard_normal(n)).astype(F32)
    omd = float(E.omd(3, 0.9, True))
    rec = record(omd)
    for hyper in SGD_HYPER:
        hyper_dev = torch.tensor(hyper, dtype=torch.float32, device=DEV)
        G = arena(g)
        P, Bf = arena(p0), arena(b0)
        HF.sgd_step_(P[:n], G[:n], Bf[:n], *hyper)
        P2, B2 = arena(p0), arena(b0)
        HF.sgd_step_dev_(P2[:n], G[:n], B2[:n], hyper_dev)
        P3, B3, E3 = arena(p0), arena(b0), arena(e0)
        HF.sgd_step_ema_(P3[:n], G[:n], B3[:n], *hyper, E3[:n], rec)
        P4, B4, E4 = arena(p0), arena(b0), arena(e0)
        HF.sgd_step_dev_ema_(P4[:n], G[:n], B4[:n], hyper_dev, E4[:n], rec)
        E5 = arena(e0)
        HF.ema_update_(E5[:n], P[:n], rec)
        torch.cuda.synchronize()
        assert np.array_equal(bits(P3), bits(P)) and np.array_equal(bits(B3), bits(Bf)), f'n={n} {hyper}: dsrl_sgd_step_ema changed p or buf'
        assert np.array_equal(bits(P4), bits(P2)) and np.array_equal(bits(B4), bits(B2)), f'n={n} {hyper}: dsrl_sgd_step_dev_ema changed p or buf'
        assert np.array_equal(bits(E3), bits(E5)) and np.array_equal(bits(E4), bits(E5)), f'n={n} {hyper}: fused and unfused averages differ'
        for a in (P3, B3, E3, P4, B4, E4, E5, G):
            assert np.array_equal(a[n:].cpu().numpy(), GUARD), f'n={n} {hyper}: floats after the n-th element changed'
        assert np.array_equal(bits(rec), bits(record(omd))), 'the record is read only'
        assert_one_ulp(E3[:n].cpu().numpy(), e0, P[:n].cpu().numpy(), omd, f'n={n} {hyper}')


@pytest.mark.parametrize('n', SIZES)
def test_omd_zero_and_one(n):
    """omd = 0 leaves the average untouched, whatever p is.  omd = 1 gives e == p_new bit for bit where the float32 difference p_new - e is exact,
    i.e. for e between p_new / 2 and 2 p_new (Sterbenz) - the regime of an average that follows its parameter; fma(1, fl(p - e), e) of an
    unrelated pair rounds twice and is not p.  All three variants."""
    rs = np.random.RandomState(n % 9973 + 2)
    p0, b0, g = (rs.standard_normal(n).astype(F32) for _ in range(3))
    hyper = SGD_HYPER[0]
    hyper_dev = torch.tensor(hyper, dtype=torch.float32, device=DEV)
    G, P, Bf = arena(g), arena(p0), arena(b0)
    HF.sgd_step_(P[:n], G[:n], Bf[:n], *hyper)
    p_new = P[:n].cpu().numpy()
    e_far = (7.0 + rs.standard_normal(n)).astype(F32)
    e_near = (p_new * rs.uniform(0.51, 1.99, n)).astype(F32)
    assert ((p_new - e_near).astype(F64) == p_new.astype(F64) - e_near.astype(F64)).all()
    for omd, e0, want in ((0.0, e_far, e_far), (1.0, e_near, p_new)):
        rec = record(omd)
        P3, B3, E3 = arena(p0), arena(b0), arena(e0)
        HF.sgd_step_ema_(P3[:n], G[:n], B3[:n], *hyper, E3[:n], rec)
        P4, B4, E4 = arena(p0), arena(b0), arena(e0)
        HF.sgd_step_dev_ema_(P4[:n], G[:n], B4[:n], hyper_dev, E4[:n], rec)
        E5 = arena(e0)
        HF.ema_update_(E5[:n], P[:n], rec)
        torch.cuda.synchronize()
        for name, a in (('sgd_step_ema', E3), ('sgd_step_dev_ema', E4), ('ema_update', E5)):
            assert np.array_equal(bits(a[:n]), want.view(np.uint32)), f'n={n} omd={omd} {name}'
            assert np.array_equal(a[n:].cpu().numpy(), GUARD)
        assert np.array_equal(bits(P3), bits(P)) and np.array_equal(bits(P4), bits(P))


def test_misaligned_pointers_are_refused():
    n = 64
    z = [torch.zeros(n + 8, device=DEV) for _ in range(4)]
    hyper_dev = torch.tensor(SGD_HYPER[0], dtype=torch.float32, device=DEV)
    rec = record(0.1)
    odd = torch.zeros(8, dtype=torch.int32, device=DEV)[1:5]           # a record 4 bytes off
    tab = torch.tensor([[0, n, 0]], dtype=torch.int64, device=DEV)
    p, g, b, e = (a[:n] for a in z)
    for k in range(4):                                                  # each arena in turn one float off
        args = [a[1:n + 1] if i == k else a[:n] for i, a in enumerate(z)]
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.sgd_step_ema_(args[0], args[1], args[2], *SGD_HYPER[0], args[3], rec)
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.sgd_step_dev_ema_(args[0], args[1], args[2], hyper_dev, args[3], rec)
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.call('dsrl_sgd_step_dev_segments_ema', args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), tab.data_ptr(), 1, hyper_dev.data_ptr(),
                    args[3].data_ptr(), rec.data_ptr(), HF._stream())
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.sgd_step_ema_(p, g, b, *SGD_HYPER[0], e, odd)
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.sgd_step_dev_ema_(p, g, b, hyper_dev, e, odd)
    for a, c in ((z[0][1:n + 1], p), (e, z[1][1:n + 1])):
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.ema_update_(a, c, rec)
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.arena_swap_(a, c)
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.ema_update_(e, p, odd)
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.ema_advance_(odd)
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.arena_swap_(z[0][:16], z[0][8:24])                           # overlapping
    torch.cuda.synchronize()
    assert all(float(a.abs().sum()) == 0.0 for a in z)                  # nothing ran


# ------------------------------------------------------------------------------------------------ segment kernel
def test_segment_kernel_against_its_twin():
    """dsrl_sgd_step_dev_segments_ema on a table with segments of 4, 32768 and 4 x 1237 floats, gaps between them, rows with and without an amax
    record: p, buf and the records bit-equal to dsrl_sgd_step_dev_segments, the average as in the element kernels, the gaps untouched in all three
    arenas."""
    rs = np.random.RandomState(11)
    segs = [(8, 4), (40, 32768), (40 + 32768 + 12, 4 * 1237), (40 + 32768 + 12 + 4 * 1237 + 4, 4), (40 + 32768 + 12 + 4 * 1237 + 4 + 4, 32768)]
    n = segs[-1][0] + segs[-1][1] + 20
    with_record = [True, False, True, False, True]
    p0, b0, g = (rs.standard_normal(n).astype(F32) for _ in range(3))
    e0 = (p0 + 0.1 * rs.standard_normal(n)).astype(F32)
    omd = float(E.omd(5, 0.9999, True))
    rec = record(omd)
    hyper = SGD_HYPER[0]
    hyper_dev = torch.tensor(hyper, dtype=torch.float32, device=DEV)
    res = {}
    for fused in (False, True):
        amax = torch.zeros(len(segs), HF.AMAX_WORDS, dtype=torch.int32, device=DEV)
        rows = [[o, c, amax[i].data_ptr() if with_record[i] else 0] for i, (o, c) in enumerate(segs)]
        tab = torch.tensor(rows, dtype=torch.int64, device=DEV)
        P, G, Bf, Ev = (torch.from_numpy(a.copy()).to(DEV) for a in (p0, g, b0, e0))
        if fused:
            HF.call('dsrl_sgd_step_dev_segments_ema', P.data_ptr(), G.data_ptr(), Bf.data_ptr(), tab.data_ptr(), len(rows), hyper_dev.data_ptr(),
                    Ev.data_ptr(), rec.data_ptr(), HF._stream())
        else:
            HF.call('dsrl_sgd_step_dev_segments', P.data_ptr(), G.data_ptr(), Bf.data_ptr(), tab.data_ptr(), len(rows), hyper_dev.data_ptr(), HF._stream())
        torch.cuda.synchronize()
        res[fused] = tuple(a.cpu().numpy() for a in (P, Bf, Ev, amax))
    (p_t, b_t, e_t, a_t), (p_f, b_f, e_f, a_f) = res[False], res[True]
    assert np.array_equal(p_f.view(np.uint32), p_t.view(np.uint32)) and np.array_equal(b_f.view(np.uint32), b_t.view(np.uint32))
    assert np.array_equal(a_f, a_t), 'amax records differ from the twin\'s'
    assert np.array_equal(e_t, e0)                                       # the twin knows no average
    inside = np.zeros(n, bool)
    for i, (o, c) in enumerate(segs):
        inside[o:o + c] = True
        m = int(a_f[i].view(np.uint32).max())
        assert m == (int(np.abs(p_f[o:o + c]).max().view(np.uint32)) if with_record[i] else 0), f'record of segment {i}'
    assert inside.sum() < n
    for new, old, what in ((p_f, p0, 'p'), (b_f, b0, 'buf'), (e_f, e0, 'ema')):
        assert np.array_equal(new[~inside].view(np.uint32), old[~inside].view(np.uint32)), f'{what}: a gap between segments changed'
        assert (new[inside] != old[inside]).mean() > 0.99
    assert_one_ulp(e_f[inside], e0[inside], p_f[inside], omd, 'segments')
    # and bit-equal to the unfused update of the same p_new
    E5 = torch.from_numpy(e0.copy()).to(DEV)
    Pn = torch.from_numpy(p_f.copy()).to(DEV)
    HF.ema_update_(E5, Pn, rec)
    torch.cuda.synchronize()
    assert np.array_equal(bits(E5)[inside], e_f.view(np.uint32)[inside])


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize('decay_max,warmup', [(0.9, True), (0.9999, True), (0.5, True), (0.9, False), (0.9999, False)])
def test_advance_follows_the_float32_schedule(decay_max, warmup):
    """25 calls of dsrl_ema_advance from updates = 0: after every call `updates` and the BITS of omd are those of ema_ref.decay in numpy float32.
    With the rule d_t = (1 + t) / (10 + t) the warm-up of 0.9 ends at t = 80 and that of 0.9999 far later, so inside 25 steps both are still
    warming up; 0.5 (reached at t = 8) is here to cross the hand-over inside the window."""
    rec = HF.ema_record(decay_max, warmup, 0, DEV)
    seen = []
    for _ in range(25):
        HF.ema_advance_(rec)
        seen.append(rec.clone())
    torch.cuda.synchronize()
    for i, r in enumerate(seen):
        t = i + 1
        w = bits(r)
        want = np.array([E.omd(t, decay_max, warmup), F32(decay_max)], F32).view(np.uint32)
        assert w[2] == t and w[3] == int(warmup), (t, w)
        assert w[0] == want[0] and w[1] == want[1], (t, w[:2], want, w[:2].view(F32))
    if warmup and decay_max == 0.5:
        assert bits(seen[6])[0] != bits(seen[7])[0] and bits(seen[7])[0] == bits(seen[24])[0] == F32(0.5).view(np.uint32)


# ------------------------------------------------------------------------------------------------ swap
@pytest.mark.parametrize('n', SIZES)
def test_arena_swap_moves_bit_patterns(n):
    rs = np.random.RandomState(n % 9973 + 3)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00000000, 0xffffffff], np.uint32)
    a0 = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    b0 = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    k = min(n, len(special))
    a0[:k], b0[n - k:] = special[:k], special[:k][::-1]
    if n > 2 * len(special):
        a0[-7:] = special[:7]               # the scalar tail and the last float4 carry some too
    A, B = arena(a0.view(F32)), arena(b0.view(F32))
    HF.arena_swap_(A[:n], B[:n])
    torch.cuda.synchronize()
    assert np.array_equal(bits(A[:n]), b0) and np.array_equal(bits(B[:n]), a0)
    assert np.array_equal(A[n:].cpu().numpy(), GUARD) and np.array_equal(B[n:].cpu().numpy(), GUARD)
    HF.arena_swap_(A[:n], B[:n])
    torch.cuda.synchronize()
    assert np.array_equal(bits(A[:n]), a0) and np.array_equal(bits(B[:n]), b0)


# ------------------------------------------------------------------------------------------------ TrainStep level
STEPS = 6


def _build(world_claim=1, graph=False, ema=None):
    """the fixture of tests/test_rccl_gpu.py::_make: DSRL(3), batch 2 at 64 x 128, SyntheticCityscapes"""
    import dualsuperreslearningforsemseg_amd as D
    from dualsuperreslearningforsemseg_amd import ddp
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    torch.manual_seed(54321)
    model = D.DSRL(3, cs)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, 'bn3'):
                m.bn3.weight.fill_(0.5)
    model = model.to(DEV).to(memory_format=torch.channels_last).train()
    if world_claim > 1:
        real = ddp.dist.get_world_size
        ddp.dist.get_world_size = lambda group=None: world_claim       # the collectives still run on the 1-rank group
        try:
            flat = ddp.FlatParams(model, chunk_bytes=16 << 20)
        finally:
            ddp.dist.get_world_size = real
        assert flat.world == world_claim
    else:
        flat = ddp.FlatParams(model)
    if ema is not None:
        flat.enable_ema(*ema)
    HF.set_dropout_seed(4242)
    step = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph)
    batch = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    return model, flat, step, batch


def _one(step, batch, lr, wd):
    (img, org), (tgt, _) = batch
    return step(img, org, tgt, lr, 0.9, wd, True)[0]


def _recursion_bound_check(e0, e_after, snaps, decay_max, what):
    """e after step k against the float64 recursion over the snapshots, per element within 2 k 2^-23 max(|p_i|, |e_0|): one float32 difference and
    one fma per step, each an error of at most 2^-24 times a number no larger than twice that maximum, and no amplification since d < 1.  float64
    on the device: the same IEEE operations as numpy's, on 60 M elements."""
    e = e0.double()
    big = e0.abs().double()
    for k, (p, dev_e) in enumerate(zip(snaps, e_after), start=1):
        omd = float(E.omd(k - 1, decay_max, True))
        p64 = p.double()
        e = e + omd * (p64 - e)
        big = torch.maximum(big, p64.abs())
        excess = ((dev_e.double() - e).abs() - 2 * k * 2.0 ** -23 * big).max().item()
        assert excess <= 0.0, f'{what}: step {k} exceeds the bound by {excess}'
    # the same recursion through the numpy reference on a slice (the device float64 above IS ema_ref.ema_run, checked here)
    sl = slice(0, 4096)
    ref = E.ema_run(e0[sl].cpu().numpy(), [p[sl].cpu().numpy() for p in snaps], decay_max, True)[-1]
    assert np.array_equal(e[sl].cpu().numpy(), ref)


@functools.lru_cache(maxsize=None)
def _scenario(graph):
    """6 steps without and with the average, then the context manager and a 7th step; -> (e_flat, eb_flat) after step 6 on the host"""
    decay = 0.9
    was = HF.overlap_wgrad
    HF.overlap_wgrad = False            # a capture is linear; the eager launches take the same order (tests/test_rccl_gpu.py)
    HF.set_bn_fused_max_blocks(128)
    try:
        # --- without the average
        model0, flat0, step0, batch = _build(graph=graph)
        hist0 = [_one(step0, batch, 0.006, 5e-4) for _ in range(STEPS)]
        torch.cuda.synchronize()
        assert flat0.e_flat is None and np.isfinite(hist0).all()
        off = (flat0.p_flat.clone(), flat0.m_flat.clone(), flat0.b_flat.clone())
        hist0.append(_one(step0, batch, 0.006, 5e-4))                 # the twin that never enters the context: its 7th step
        torch.cuda.synchronize()
        off7 = (flat0.p_flat.clone(), flat0.b_flat.clone())
        replays0 = step0.graph_replays
        (img0, org0), (tgt0, _) = batch
        key_without = step0._graph_key(img0, org0, tgt0)
        assert key_without[5] is False
        step0.release()
        del model0, flat0, step0
        # --- with it
        model, flat, step, batch = _build(graph=graph, ema=(decay, True))
        e0, eb0 = flat.e_flat.clone(), flat.eb_flat.clone()
        assert torch.equal(e0, flat.p_flat) and torch.equal(eb0, flat.b_flat)
        hist, ps, bs, es, ebs = [], [], [], [], []
        for _ in range(STEPS):
            hist.append(_one(step, batch, 0.006, 5e-4))
            ps.append(flat.p_flat.clone()); bs.append(flat.b_flat.clone()); es.append(flat.e_flat.clone()); ebs.append(flat.eb_flat.clone())
        torch.cuda.synchronize()
        assert hist == hist0[:STEPS], (hist, hist0)
        assert torch.equal(flat.p_flat, off[0]) and torch.equal(flat.m_flat, off[1]) and torch.equal(flat.b_flat, off[2]), 'the average changed the training run'
        _recursion_bound_check(e0, es, ps, decay, f'e_flat graph={graph}')
        _recursion_bound_check(eb0, ebs, bs, decay, f'eb_flat graph={graph}')
        assert not torch.equal(es[-1], ps[-1]) and not torch.equal(es[-1], e0)
        rec = HF.ema_record_read(flat.ema_rec)
        assert rec['updates'] == STEPS == flat.ema_updates() and rec['omd'] == float(E.omd(STEPS, decay, True)), rec
        if graph:
            assert step.graph_replays == STEPS - step.GRAPH_WARMUP == replays0 - 1
            assert all(k[5] is True for k in step._graphs)              # "EMA enabled" is part of the graph key
            assert step._graph_key(img0, org0, tgt0) in step._graphs and key_without not in step._graphs
        else:
            assert step.graph_replays == 0
        del ps[:-1], bs[:-1], es[:-1], ebs[:-1]
        # --- the averaged model in place
        avg = flat.ema_state_dict()
        assert avg.pop('ema_updates') == STEPS and avg.pop('ema_decay') == float(F32(decay))
        p_before, b_before = flat.p_flat.clone(), flat.b_flat.clone()
        (img, org), (tgt, _) = batch
        with flat.ema_weights():
            assert flat.ema_swapped and flat._amax_key is None
            sd = model.state_dict()
            assert list(sd) == list(avg)
            for k, v in sd.items():
                assert torch.equal(v, avg[k]), k
            assert torch.equal(flat.p_flat, es[-1]) and torch.equal(flat.e_flat, p_before)
            # one validation forward (do_train=False) on the averaged weights: dropout off, so that it draws no dropout key and the 7th step below
            # stays the twin's.  The BatchNorms keep the batch's statistics: six steps from a random initialisation leave running statistics an
            # eval-mode ResNet-101 cannot normalise with - live or averaged, its FA loss overflows - (they move the running statistics they find in
            # place, the averaged model's)
            model.eval()
            for m in model.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.train()
            vals, _ = step(img, org, tgt, 0.006, 0.9, 5e-4, False)
            model.train()
            assert np.isfinite(vals).all(), vals
            for call in (lambda: step(img, org, tgt, 0.006, 0.9, 5e-4, True), lambda: flat.sgd_step(0.006, 0.9, 5e-4),
                         lambda: flat.reduce_chunked_and_step(hp=(0.006, 0.9, 5e-4))):
                with pytest.raises(HF.DsrlHipError, match='ema_weights'):
                    call()
        torch.cuda.synchronize()
        assert not flat.ema_swapped and flat._amax_key is None
        assert np.array_equal(bits(flat.p_flat), bits(p_before)) and np.array_equal(bits(flat.b_flat), bits(b_before))
        assert torch.equal(flat.e_flat, es[-1])                      # (eb_flat took the running-statistics update of the train-mode forward above)
        # --- and on with training: the 7th step is the twin's
        hist.append(_one(step, batch, 0.006, 5e-4))
        torch.cuda.synchronize()
        assert hist[-1] == hist0[-1], (hist[-1], hist0[-1])
        assert torch.equal(flat.p_flat, off7[0]) and torch.equal(flat.b_flat, off7[1])
        assert flat.ema_updates() == STEPS + 1
        if graph:
            assert step.graph_replays == STEPS + 1 - step.GRAPH_WARMUP
        out = (es[-1].cpu(), ebs[-1].cpu())
        step.release()
        return out
    finally:
        HF.overlap_wgrad = was
        HF.set_bn_fused_max_blocks(None)


@pytest.mark.parametrize('graph', [False, True])
def test_train_step_with_ema(graph):
    """The average does not touch the run it follows (losses, p, momentum, buffers bit-equal to the run without it), follows the float64 recursion
    over the per-step snapshots, counts its updates on the device - replayed steps included -, and ema_weights() puts the averaged model in place and
    the live one back, bit for bit, with the optimiser's filter magnitudes invalidated and training refused in between."""
    _scenario(graph)


def test_eager_and_graph_average_agree():
    e_eager, eb_eager = _scenario(False)
    e_graph, eb_graph = _scenario(True)
    assert torch.equal(e_eager, e_graph) and torch.equal(eb_eager, eb_graph)


# ------------------------------------------------------------------------------------------------ the multi-rank schedule on one GPU
def test_multi_rank_schedule_one_omd_per_step(monkeypatch):
    """A 1-rank 'nccl' group with a claimed world of 2 (tests/test_rccl_gpu.py), one captured graph per step and the exchange + update behind it in
    four ranges: every range's launch reads the same omd and the schedule advances once per step, so e_flat is bit-equal to a single-process run at
    half the learning rate (weight decay 0: sum over one rank, times 1/2, at lr IS lr / 2 exactly)."""
    import torch.distributed as dist
    monkeypatch.setenv('DSRL_GRAPH_SPLIT', '0')
    steps, decay = 5, 0.9
    was = HF.overlap_wgrad
    HF.overlap_wgrad = False
    HF.set_bn_fused_max_blocks(128)
    try:
        model, flat, step, batch = _build(graph=True, ema=(decay, True))
        hist1 = [_one(step, batch, 0.003, 0.0) for _ in range(steps)]
        torch.cuda.synchronize()
        single = (flat.p_flat.clone(), flat.e_flat.clone(), flat.eb_flat.clone(), flat.ema_updates())
        step.release()
        del model, flat, step
        s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
        dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1, device_id=torch.device(DEV))
        try:
            model, flat, step, batch = _build(world_claim=2, graph=True, ema=(decay, True))
            assert flat._amax_key is None                   # the constructor's broadcast invalidated it explicitly
            ranges = []
            real = flat.reduce_chunked_and_step
            flat.reduce_chunked_and_step = lambda *a, **k: ranges.append(real(*a, **k))
            hist2 = [_one(step, batch, 0.006, 0.0) for _ in range(steps)]
            torch.cuda.synchronize()
            assert len(ranges) == steps and all(len(r) == 4 for r in ranges), ranges
            assert step.graph_replays == steps - step.GRAPH_WARMUP and flat.defer_collectives and not step.split
            assert HF.bn_fused_barrier_timeouts() == 0
            assert flat.ema_updates() == steps == single[3]
            assert hist2 == hist1, (hist2, hist1)
            assert torch.equal(flat.p_flat, single[0])
            assert torch.equal(flat.e_flat, single[1]) and torch.equal(flat.eb_flat, single[2])
            step.release()
        finally:
            dist.destroy_process_group()
    finally:
        HF.overlap_wgrad = was
        HF.set_bn_fused_max_blocks(None)


# ------------------------------------------------------------------------------------------------ train_or_resume
def test_train_or_resume_with_ema(tmp_path):
    """dataset['ema'] = 0.9 end to end: the checkpoint carries 'ema_state_dict' beside exactly the usual keys, the final weights are the averaged
    ones, a resume continues the update count; without the key the files are what they were."""
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, train_or_resume
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs

    def factory(split, batch_size, device, rank, world):
        return SyntheticCityscapes(batch_size, (32, 64), device, rank=rank, length=2)

    def load(*parts):
        return torch.load(os.path.join(*parts), map_location='cpu', weights_only=False)

    def kw(exp, **dataset):
        return dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                    dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': factory, **dataset}, val_interval=1, checkpoint_interval=1,
                    checkpoint_history=2, init_weights=None, batch_size=2, epochs=2, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9,
                    weights_decay=5e-4, poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / exp),
                    description='test', early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))

    with pytest.raises(ValueError):
        train_or_resume(is_resuming_training=False, **kw('bad', ema=1.5))
    assert not os.path.exists(str(tmp_path / 'bad'))
    args = kw('exp', ema=0.9)
    hist = train_or_resume(is_resuming_training=False, **args)
    assert len(hist) == 3 and all(np.isfinite(v) for h in hist[:2] for v in h['train'][:4]) and all(0 <= h['val'][4] <= 100 for h in hist[:2])
    ckdir = os.path.join(str(tmp_path / 'exp'), settings.CHECKPOINTS_DIR.format(stage=3))
    ck = load(ckdir, settings.CHECKPOINT_FILE.format(epoch=2))
    assert set(ck) == set(settings.VARIABLES_IN_CHECKPOINT) | {'ema_state_dict'}
    avg = dict(ck['ema_state_dict'])
    assert avg.pop('ema_updates') == 4 and avg.pop('ema_decay') == float(F32(0.9))          # 2 epochs of 2 iterations
    assert list(avg) == list(ck['model_state_dict'])
    fw = load(str(tmp_path / 'exp'), settings.WEIGHTS_DIR.format(stage=3), settings.FINAL_WEIGHTS_FILE)
    assert set(fw) == {'model_state_dict', 'mixed_precision', 'amp_state_dict', 'ema'} and fw['ema'] == {'decay': float(F32(0.9)), 'updates': 4}
    assert list(fw['model_state_dict']) == list(avg)
    differ = 0
    for k, v in fw['model_state_dict'].items():
        assert torch.equal(v, avg[k]), k                                                       # the averaged weights ...
        differ += int(v.dtype == torch.float32 and not torch.equal(v, ck['model_state_dict'][k]))
    assert differ > 300, differ                                                                # ... not the live ones
    for x in os.listdir(ckdir):
        assert 'ema_state_dict' in load(ckdir, x), x                                           # the best-validation checkpoint too
    # resume with the average: two more iterations on top of the four
    args['epochs'] = 3
    hist2 = train_or_resume(is_resuming_training=True, model_state_dict=ck['model_state_dict'], optimizer_state_dict=ck['optimizer_state_dict'],
                            epoch=ck['epoch'], best_validation_dict=ck['best_validation_dict'], ema_state_dict=ck['ema_state_dict'], **args)
    assert hist2[0]['epoch'] == 3
    ck3 = load(ckdir, settings.CHECKPOINT_FILE.format(epoch=3))
    assert ck3['ema_state_dict']['ema_updates'] == ck['ema_state_dict']['ema_updates'] + 2 == 6
    assert load(str(tmp_path / 'exp'), settings.WEIGHTS_DIR.format(stage=3), settings.FINAL_WEIGHTS_FILE)['ema']['updates'] == 6
    # resume with the average switched on and no stored one: it starts from the loaded weights, with a warning
    args['experiment_id'] = str(tmp_path / 'exp_b')
    with pytest.warns(UserWarning, match='ema_state_dict'):
        train_or_resume(is_resuming_training=True, model_state_dict=ck['model_state_dict'], optimizer_state_dict=ck['optimizer_state_dict'],
                        epoch=ck['epoch'], best_validation_dict=ck['best_validation_dict'], **args)
    assert load(str(tmp_path / 'exp_b'), settings.WEIGHTS_DIR.format(stage=3), settings.FINAL_WEIGHTS_FILE)['ema']['updates'] == 2
    # the same run without dataset['ema']: today's key sets
    train_or_resume(is_resuming_training=False, **kw('exp_d'))
    ckd = load(str(tmp_path / 'exp_d'), settings.CHECKPOINTS_DIR.format(stage=3), settings.CHECKPOINT_FILE.format(epoch=2))
    assert set(ckd) == set(settings.VARIABLES_IN_CHECKPOINT)
    assert set(load(str(tmp_path / 'exp_d'), settings.WEIGHTS_DIR.format(stage=3), settings.FINAL_WEIGHTS_FILE)) == {'model_state_dict', 'mixed_precision', 'amp_state_dict'}

"""Gradient-norm clipping on the device (`-m gpu`; csrc/gradclip.hip, ddp.FlatParams.enable_grad_clip) against
tests/grad_clip_ref.py: the tile sums within the rounding of their double additions, their independence from the way the arena is cut into calls,
the finish (hyper-parameters, coefficient, record) on chosen tile arrays, NaN and inf, and FlatParams, TrainStep and train_or_resume with clipping.

A float square is exact in double, so a tile's sum carries the rounding of its 1023 double additions alone: relative 1024 * 2^-53 against the
correctly rounded reference (all terms are >= 0).  The finish adds ntiles such numbers: relative ntiles * 2^-53, far below a float32 ulp."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from hip_helpers import DEV, HF

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TILE = 1024
SIZES = [1, 3, 4, 1023, 1024, 1025, 5 * 1024 + 7, 4 * 2 ** 20 + 4099]     # scalar tail only, n % 4 != 0, a tile boundary -1 / 0 / +1, a short last tile, a grid that wraps
GUARD = np.float32([1e9, -2e9, 3e9, -4e9, 5e9, -6e9, 7e9, -8e9])
SENTINEL = -7.25                                      # what an untouched tile slot holds (a sum of squares is never negative)
BADARG = 'failed with code -1'                       # include/dsrl_hip.h: DSRL_E_BADARG
HYPER = (0.006, 0.9, 5e-4, 0.125)                     # lr, momentum, weight decay, grad_scale


def bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def mixed(rs, n):
    """magnitudes from 1e-20 to 1e15, both signs, some zeros"""
    g = (rs.choice([-1.0, 1.0], n) * 10.0 ** rs.uniform(-20, 15, n)).astype(F32)
    g[rs.rand(n) < 0.01] = 0.0
    return g


def arena(a, lead=0):
    """`lead` floats in front (the arena's earlier tiles), `a`, then guard floats nothing may touch"""
    return torch.from_numpy(np.concatenate([np.full(lead, 3.0, F32), np.asarray(a, F32), GUARD])).to(DEV)


def workspace(n, extra=4):
    """-> (whole buffer, tiles view, number of doubles the library asked for): every double a sentinel, `extra` guard doubles behind the workspace"""
    nt = -(-n // TILE)
    words = int(HF.query('dsrl_grad_clip_workspace_bytes', n)) // 8
    assert words >= nt
    buf = torch.full((words + extra,), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[:nt], words


def assert_tiles(dev_tiles, g, what):
    ref = R.tile_sums(g)
    got = dev_tiles.astype(F64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    bound = TILE * 2.0 ** -53 * ref
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f'{what}: largest tile error {worst:.3f} of the bound 1024 * 2^-53')
    assert (err <= bound).all(), f'{what}: {worst} x the bound'


# ------------------------------------------------------------------------------------------------ tile sums
@pytest.mark.parametrize('lead', [0, 2 * TILE])
@pytest.mark.parametrize('n', SIZES)
def test_tile_sums(n, lead):
    """tiles[first / 1024 + k] against the float64 reference; the guard floats behind the range, the tile slots in front of and behind the range's
    and the finish's scratch keep their bits."""
    rs = np.random.RandomState(n % 9973 + 1)
    g = mixed(rs, n)
    G = arena(g, lead)
    buf, _, words = workspace(lead + n)
    nt, t0 = -(-n // TILE), lead // TILE
    HF.grad_sumsq_(G[lead:lead + n], lead, buf[:t0 + nt])
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert_tiles(out[t0:t0 + nt], g, f'n={n} first={lead}')
    assert (out[:t0] == SENTINEL).all() and (out[t0 + nt:] == SENTINEL).all(), 'a tile slot outside the range was written'
    assert np.array_equal(G[lead + n:].cpu().numpy(), GUARD) and np.array_equal(G[:lead].cpu().numpy(), np.full(lead, 3.0, F32))
    assert np.array_equal(G[lead:lead + n].cpu().numpy().view(np.uint32), g.view(np.uint32)), 'the gradient is read only'


def test_tile_sums_of_simple_values_are_exact():
    """integers: every partial sum is exact, whatever the order - the tile sums are the integers themselves"""
    n = 3 * TILE + 5
    g = (np.arange(n) % 7 - 3).astype(F32)
    G = arena(g)
    buf, tiles, _ = workspace(n)
    HF.grad_sumsq_(G[:n], 0, tiles)
    torch.cuda.synchronize()
    assert np.array_equal(tiles.cpu().numpy(), [float((g[i:i + TILE].astype(F64) ** 2).sum()) for i in range(0, n, TILE)])


# ------------------------------------------------------------------------------------------------ independence from the cut
def test_independent_of_the_cut_and_of_the_run():
    """One arena summed in one call and in calls cut at multiples of 1024: tile arrays and finished records bit-equal; two runs bit-equal."""
    n = 7 * TILE + 300
    rs = np.random.RandomState(5)
    g = mixed(rs, n)
    G = arena(g)
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=DEV)
    res = []
    for cuts in ([], [], [TILE], [TILE, 3 * TILE], [TILE, 3 * TILE, 6 * TILE, 7 * TILE], [4 * TILE]):
        buf, tiles, _ = workspace(n)
        edges = [0] + cuts + [n]
        for a, b in reversed(list(zip(edges[:-1], edges[1:]))):            # (and not in ascending order)
            HF.grad_sumsq_(G[a:b], a, tiles)
        rec = HF.grad_clip_record(1.0, DEV)
        out = torch.zeros(4, device=DEV)
        HF.grad_clip_finish_(tiles, rec, out, hyper=hyper)
        torch.cuda.synchronize()
        res.append((bits(tiles), bits(rec), bits(out)))
    assert_tiles(res[0][0].view(F64), g, 'one call')
    for r in res[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, res[0]))


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_are_refused():
    n = 4 * TILE
    G = torch.ones(n + 8, device=DEV)
    buf, tiles, _ = workspace(n)
    for first in (1, 4, 512, 1023, 1025):
        with pytest.raises(HF.DsrlHipError, match=BADARG):
            HF.grad_sumsq_(G[first:first + TILE], first, tiles)
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.call('dsrl_grad_sumsq', G.data_ptr() + 4, 0, TILE, tiles.data_ptr(), HF._stream())         # the arena one float off
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.call('dsrl_grad_sumsq', G.data_ptr() + 8, TILE, TILE, tiles.data_ptr(), HF._stream())
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.call('dsrl_grad_sumsq', G.data_ptr(), 0, 0, tiles.data_ptr(), HF._stream())
    with pytest.raises(HF.DsrlHipError):
        HF.grad_sumsq_(G[:n], TILE, tiles)                      # more tiles than the array holds
    rec = HF.grad_clip_record(1.0, DEV)
    out = torch.zeros(4, device=DEV)
    odd = torch.zeros(20, dtype=torch.int32, device=DEV)[1:17]         # a record 4 bytes off
    with pytest.raises(HF.DsrlHipError, match=BADARG):
        HF.grad_clip_finish_(tiles, odd, out, hp=HYPER)
    with pytest.raises(HF.DsrlHipError):
        HF.grad_clip_finish_(torch.zeros(4, dtype=torch.float64, device=DEV), rec, out, hp=HYPER)      # no scratch behind the tiles
    with pytest.raises(HF.DsrlHipError):
        HF.grad_clip_finish_(tiles, rec, out)                    # neither device nor host hyper-parameters
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all() and float(out.abs().sum()) == 0.0
    assert np.array_equal(bits(rec), bits(HF.grad_clip_record(1.0, DEV)))                               # nothing ran
    assert HF.query('dsrl_grad_clip_workspace_bytes', 0) == 0 and HF.query('dsrl_grad_clip_workspace_bytes', 1) >= 8


# ------------------------------------------------------------------------------------------------ the finish
def finish(tile_values, max_norm, hyper=HYPER, device_hyper=True, rec=None):
    """-> (hyper_out bits, record as a dict, record tensor) of one finish on the given tile sums; checks that nothing but record and hyper_out moved"""
    nt = len(tile_values)
    buf, tiles, words = workspace(nt * TILE)
    tiles.copy_(torch.from_numpy(np.asarray(tile_values, F64)))
    rec = HF.grad_clip_record(max_norm, DEV) if rec is None else rec
    box = torch.from_numpy(np.concatenate([np.zeros(4, F32), GUARD])).to(DEV)
    hin = torch.from_numpy(np.concatenate([np.asarray(hyper, F32), GUARD])).to(DEV)
    if device_hyper:
        HF.grad_clip_finish_(tiles, rec, box[:4], hyper=hin[:4])
    else:
        HF.grad_clip_finish_(tiles, rec, box[:4], hp=hyper)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.array_equal(out[:nt].view(np.uint64), np.asarray(tile_values, F64).view(np.uint64)), 'the tiles are read only'
    assert (out[words:] == SENTINEL).all(), 'doubles behind the workspace changed'
    assert np.array_equal(box[4:].cpu().numpy(), GUARD) and np.array_equal(hin.cpu().numpy()[4:], GUARD)
    assert np.array_equal(hin[:4].cpu().numpy(), np.asarray(hyper, F32))
    return bits(box[:4]), HF.grad_clip_record_read(rec), rec


def one_ulp(got_bits, want):
    got = got_bits.view(F32)[0] if isinstance(got_bits, np.ndarray) else F32(got_bits)
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(F32(want))))


@pytest.mark.parametrize('nt', [1, 5, 1023, 1024, 1025, 3 * 1024 + 17, 58485])         # one block of the first level, its boundary, several, the size of the real arena's count (58470)
def test_finish_against_reference(nt):
    """hyper_out[0:3] bit-equal to the inputs, hyper_out[3] within one float32 ulp of the reference's (the relative error of S is at most
    ntiles 2^-53: one rounding boundary is the only slack), the device and the host form of the hyper-parameters bit-equal; norm <= max_norm and
    max_norm = inf both hand grad_scale through bit for bit."""
    rs = np.random.RandomState(nt % 9973)
    tv = (rs.uniform(0.0, 2.0, nt) * 10.0 ** rs.uniform(-3, 3, nt)).astype(F64)
    S = R.total(tv)
    norm = float(R.norm_coef(S, HYPER[3], 1.0)[0])
    want_in = np.asarray(HYPER, F32).view(np.uint32)
    for max_norm in (norm / 3.0, norm * 0.999, norm * 4.0, float('inf'), 1e-30):
        ref, k = R.record_step(R.new_record(max_norm), S, HYPER[3])
        out_d, rec_d, _ = finish(tv, max_norm, device_hyper=True)
        out_h, rec_h, _ = finish(tv, max_norm, device_hyper=False)
        assert np.array_equal(out_d, out_h) and rec_d == rec_h, 'device and host hyper-parameters give different bits'
        assert np.array_equal(out_d[:3], want_in[:3])
        assert one_ulp(out_d[3:4], k), (nt, max_norm, out_d[3:4].view(F32), k)
        if max_norm >= norm * 4.0:
            assert out_d[3] == want_in[3] and rec_d['coef'] == 1.0 and rec_d['clipped'] == 0
        else:
            assert rec_d['clipped'] == 1 and rec_d['coef'] < 1.0
        assert abs(rec_d['sumsq'] - float(S)) <= nt * 2.0 ** -53 * float(S)
        assert one_ulp(rec_d['norm'], ref['norm']) and one_ulp(rec_d['coef'], ref['coef'])
        assert rec_d['max_norm'] == ref['max_norm'] and (rec_d['steps'], rec_d['nonfinite']) == (1, 0)
        assert one_ulp(rec_d['norm_max'], ref['norm_max']) and abs(rec_d['norm_sum'] - ref['norm_sum']) <= (nt + 8) * 2.0 ** -53 * ref['norm_sum']


def test_zero_gradient():
    out, rec, _ = finish(np.zeros(3), 1.0)
    assert out[3] == F32(HYPER[3]).view(np.uint32) and rec['coef'] == 1.0 and rec['norm'] == 0.0 and rec['sumsq'] == 0.0 and rec['clipped'] == 0
    out, rec, _ = finish(np.zeros(3), 1e-9)            # torch's formula: 1e-9 / (0 + 1e-6) clips a zero gradient as well
    assert one_ulp(out[3:4], F32(F64(F32(HYPER[3])) * (F64(F32(1e-9)) / 1e-6))) and rec['clipped'] == 1


@pytest.mark.parametrize('poison,max_norm,want', [(float('nan'), 1.0, 'nan'), (float('inf'), 1.0, 'zero'), (-float('inf'), 1.0, 'zero'),
                                                  (float('nan'), float('inf'), 'nan'), (float('inf'), float('inf'), 'nan'), (1e30, 1.0, 'tiny')])
def test_nonfinite_gradients(poison, max_norm, want):
    """A NaN gradient gives a NaN coefficient - the optimiser's grad_scale is NaN, as torch's clipped gradients are -, an infinite one 0 (inf / inf:
    NaN, as in torch); both count in `nonfinite` and stay out of norm_sum and norm_max.  1e30 squares to 1e60: finite in double, where float32 overflows."""
    n = 2 * TILE + 9
    rs = np.random.RandomState(3)
    g = rs.standard_normal(n).astype(F32)
    g[TILE + 5] = poison
    G = arena(g)
    buf, tiles, _ = workspace(n)
    rec = HF.grad_clip_record(max_norm, DEV)
    out = torch.zeros(4, device=DEV)
    HF.grad_sumsq_(G[:n], 0, tiles)
    HF.grad_clip_finish_(tiles, rec, out, hp=HYPER)
    clean = g.copy(); clean[TILE + 5] = 2.0
    G2 = arena(clean)
    HF.grad_sumsq_(G2[:n], 0, tiles)
    HF.grad_clip_finish_(tiles, rec, out[:4].clone(), hp=HYPER)         # a finite step behind it: the running fields take it
    torch.cuda.synchronize()
    r = HF.grad_clip_record_read(rec)
    k = float(out.cpu().numpy()[3])
    assert np.array_equal(out.cpu().numpy()[:3], np.asarray(HYPER[:3], F32))
    clean_norm = HYPER[3] * math.sqrt(float((clean.astype(F64) ** 2).sum()))
    if want == 'tiny':
        assert 0.0 < k < 1e-28 and (r['steps'], r['nonfinite'], r['clipped']) == (2, 0, 2)
    else:
        assert (math.isnan(k) if want == 'nan' else k == 0.0), k
        assert (r['steps'], r['nonfinite']) == (2, 1), r
        assert abs(r['norm_sum'] - clean_norm) <= 1e-12 * clean_norm and one_ulp(r['norm_max'], F32(clean_norm))


def test_running_fields_over_three_calls():
    rs = np.random.RandomState(9)
    ref = R.new_record(2.0)
    rec = HF.grad_clip_record(2.0, DEV)
    for i, scale in enumerate((0.05, 300.0, 20.0)):
        tv = (rs.uniform(0.0, 1.0, 40) * scale).astype(F64)
        gs = (1.0, 0.5, 0.125)[i]
        out, got, rec = finish(tv, 2.0, hyper=(0.1, 0.9, 0.0, gs), rec=rec)
        ref, k = R.record_step(ref, R.total(tv), gs)
        assert one_ulp(out[3:4], k)
        assert (got['steps'], got['clipped'], got['nonfinite']) == (ref['steps'], ref['clipped'], ref['nonfinite']) == (i + 1, ref['clipped'], 0)
        assert abs(got['norm_sum'] - ref['norm_sum']) <= 1e-12 * ref['norm_sum'] and one_ulp(got['norm_max'], ref['norm_max'])
        assert one_ulp(got['norm'], ref['norm']) and one_ulp(got['coef'], ref['coef']) and got['max_norm'] == 2.0
    assert ref['clipped'] == 2


# ------------------------------------------------------------------------------------------------ FlatParams on the small model
LR, MOM, WD = 0.006, 0.9, 5e-4


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


@pytest.mark.parametrize('ema', [False, True])
def test_flat_params_step(ema):
    """sgd_step on a gradient arena of known norm: monitoring (max_norm = inf) is bit-equal to the FlatParams before clipping was enabled; with a
    threshold below the norm p and the momentum arena are those of the unclipped kernels run with grad_scale = coef, the clipped gradient's norm
    is max_norm, and the four-range schedule is bit-equal to the single launch.  With the weight average on, the same - and the average follows."""
    from dualsuperreslearningforsemseg_amd import ddp
    model, _ = _model()
    flat = ddp.FlatParams(model)
    if ema:
        flat.enable_ema(0.9, True)
    gen = torch.Generator(device=DEV).manual_seed(77)
    flat.g_flat.copy_(torch.randn(flat.numel, device=DEV, generator=gen) * 0.01)
    flat.m_flat.copy_(torch.randn(flat.numel, device=DEV, generator=gen) * 0.01)
    p0, m0 = flat.p_flat.clone(), flat.m_flat.clone()
    e0 = flat.e_flat.clone() if ema else None
    erec0 = flat.ema_rec.clone() if ema else None
    true_norm = float(flat.g_flat.double().pow(2).sum().sqrt())

    def fresh():
        with torch.no_grad():
            flat.p_flat.copy_(p0); flat.m_flat.copy_(m0)
            if ema:
                flat.e_flat.copy_(e0); flat.ema_rec.copy_(erec0)

    def state():
        torch.cuda.synchronize()
        return (flat.p_flat.clone(), flat.m_flat.clone()) + ((flat.e_flat.clone(),) if ema else ())

    def same(a, b):
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

    with pytest.raises(HF.DsrlHipError, match='not enabled'):
        flat.grad_clip_stats()
    flat.sgd_step(LR, MOM, WD, reduce=False)
    plain = state()
    assert not torch.equal(plain[0], p0)
    # --- monitor only
    fresh()
    flat.enable_grad_clip(float('inf'))
    with pytest.raises(HF.DsrlHipError, match='already enabled'):
        flat.enable_grad_clip(1.0)
    flat.sgd_step(LR, MOM, WD, reduce=False)
    assert same(state(), plain), 'max_norm = inf changed the step'
    st = flat.grad_clip_stats()
    assert (st['steps'], st['clipped'], st['nonfinite'], st['coef'], st['max_norm']) == (1, 0, 0, 1.0, float('inf'))
    assert abs(st['norm'] - true_norm) <= 2.0 ** -23 * true_norm and st['norm_mean'] == pytest.approx(true_norm, rel=1e-9) and st['norm_max'] == st['norm']
    assert np.array_equal(flat.hyper_eff.cpu().numpy(), np.asarray([LR, MOM, WD, 1.0], F32))
    # --- a threshold below the norm
    max_norm = true_norm / 3.0
    flat.set_grad_clip_max_norm(max_norm)
    fresh()
    flat.sgd_step(LR, MOM, WD, reduce=False)
    clipped = state()
    st = flat.grad_clip_stats()
    k = flat.hyper_eff.cpu().numpy()
    assert (st['steps'], st['clipped']) == (2, 1) and k[3] == F32(st['coef']) and 0.3 < st['coef'] < 0.34
    assert np.array_equal(k[:3], np.asarray([LR, MOM, WD], F32))
    clipped_norm = float((flat.g_flat.double() * float(k[3])).pow(2).sum().sqrt())
    print(f'norm {true_norm!r}, max_norm {max_norm!r}, clipped norm {clipped_norm!r}')
    assert abs(clipped_norm - max_norm) <= 1e-6 * max_norm
    fresh()
    if ema:
        HF.sgd_step_ema_(flat.p_flat, flat.g_flat, flat.m_flat, LR, MOM, WD, float(k[3]), flat.e_flat, flat.ema_rec)
    else:
        HF.sgd_step_(flat.p_flat, flat.g_flat, flat.m_flat, LR, MOM, WD, float(k[3]))
    assert same(state(), clipped), 'the clipped step is not the unclipped kernels at grad_scale = coef'
    assert not same(clipped[:1], plain[:1])
    # --- the device form of the hyper-parameters, and the exchange in four ranges (world 1: no collective)
    rec_single = bits(flat.clip_rec)
    hyper = torch.tensor([LR, MOM, WD, 1.0], dtype=torch.float32, device=DEV)
    for call in (lambda: flat.sgd_step(0.0, 0.0, 0.0, hyper=hyper, reduce=False),
                 lambda: flat.reduce_chunked_and_step(hp=(LR, MOM, WD), nchunks=4),
                 lambda: flat.reduce_chunked_and_step(hyper=hyper, nchunks=4)):
        fresh()
        flat.clip_rec.copy_(HF.grad_clip_record(max_norm, DEV))
        flat.clip_tiles.fill_(SENTINEL)
        ranges = call()
        assert same(state(), clipped)
        assert ranges is None or (len(ranges) == 4 and all(a % TILE == 0 for a, _ in ranges))
        r = bits(flat.clip_rec)
        assert np.array_equal(r[:2], rec_single[:2]) and np.array_equal(r[4:7], rec_single[4:7]), 'S, norm or coef depend on the schedule'
    if ema:
        assert flat.ema_updates() == 1
    st = flat.grad_clip_stats(reset=True)
    assert st['steps'] == 1 and st['clipped'] == 1
    after = flat.grad_clip_stats()
    assert (after['steps'], after['clipped'], after['nonfinite'], after['norm_max']) == (0, 0, 0, 0.0) and math.isnan(after['norm_mean'])
    assert after['max_norm'] == float(F32(max_norm)) and after['coef'] == st['coef']


# ------------------------------------------------------------------------------------------------ TrainStep level
def _build(graph, clip):
    from dualsuperreslearningforsemseg_amd import ddp
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, TrainStep
    model, cs = _model()
    flat = ddp.FlatParams(model)
    if clip is not None:
        flat.enable_grad_clip(clip)
    HF.set_dropout_seed(4242)
    step = TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph)
    batch = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    return model, flat, step, batch


def _one(step, batch):
    (img, org), (tgt, _) = batch
    return step(img, org, tgt, LR, MOM, WD, True)[0]


@functools.lru_cache(maxsize=None)
def _scenario(graph, clip):
    """GRAPH_WARMUP + 3 steps.  clip None: no clipping; 'inf': monitoring; 'low': monitoring for the first step, then max_norm = a hundredth of that
    step's norm written into the record, and for one more step at the end a quarter of that (on the randomly initialised network the unclipped norm
    falls by an order of magnitude within a few steps; a clipped run moves a hundred times less and stays where it was).  -> (losses, p, m, records after every step, graph facts)"""
    was = HF.overlap_wgrad
    HF.overlap_wgrad = False            # a capture is linear; the eager launches take the same order (tests/test_rccl_gpu.py)
    HF.set_bn_fused_max_blocks(128)
    try:
        model, flat, step, batch = _build(graph, None if clip is None else float('inf'))
        n = step.GRAPH_WARMUP + 3
        hist, recs = [], []
        for i in range(n):
            hist.append(_one(step, batch))
            if clip is not None:
                recs.append(HF.grad_clip_record_read(flat.clip_rec))
                assert recs[-1]['steps'] == i + 1, 'the record did not advance'
            if clip == 'low' and i == 0:
                flat.set_grad_clip_max_norm(recs[0]['norm'] / 100.0)
        if clip == 'low':
            flat.set_grad_clip_max_norm(recs[0]['norm'] / 400.0)
            hist.append(_one(step, batch))
            recs.append(HF.grad_clip_record_read(flat.clip_rec))
            step.split = True
            with pytest.raises(HF.DsrlHipError, match='DSRL_GRAPH_SPLIT'):
                _one(step, batch)
            step.split = False
        torch.cuda.synchronize()
        (img, org), (tgt, _) = batch
        facts = (step.graph_replays, len(step._graphs), step._graph_key(img, org, tgt)[6])         # "clip enabled", behind "EMA enabled"
        out = (hist, flat.p_flat.cpu(), flat.m_flat.cpu(), recs, facts)
        step.release()
        return out
    finally:
        HF.overlap_wgrad = was
        HF.set_bn_fused_max_blocks(None)


def test_monitoring_leaves_the_captured_run_alone():
    """max_norm = inf: losses, p and the momentum arena of the captured run bit-equal to the run without clipping; the norms are there."""
    hist0, p0, m0, _, facts0 = _scenario(True, None)
    hist, p, m, recs, facts = _scenario(True, 'inf')
    assert hist == hist0 and torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(m.view(torch.int32), m0.view(torch.int32))
    assert facts0[2] is False and facts[2] is True and facts[:2] == facts0[:2] == (3, 1)
    assert all(r['coef'] == 1.0 and r['norm'] > 0.0 and math.isfinite(r['norm']) for r in recs) and recs[-1]['clipped'] == 0
    assert recs[-1]['norm_sum'] == pytest.approx(sum(r['norm'] for r in recs), rel=1e-6)


def test_captured_and_eager_steps_clip_alike():
    """The captured step against the eager one: same losses, parameters and records, step for step; `steps` advances on every replay; a new max_norm
    in the record takes effect at the next replay without a re-capture."""
    eager, graph = _scenario(False, 'low'), _scenario(True, 'low')
    assert eager[0] == graph[0] and eager[3] == graph[3], (eager[0], graph[0], eager[3], graph[3])
    assert torch.equal(eager[1].view(torch.int32), graph[1].view(torch.int32)) and torch.equal(eager[2].view(torch.int32), graph[2].view(torch.int32))
    assert eager[4] == (0, 0, True) and graph[4] == (4, 1, True)           # 3 + 1 replays of ONE graph
    recs = graph[3]
    first = recs[0]['norm']
    print('norm, coefficient per step:', [(r['norm'], r['coef']) for r in recs])
    assert recs[0]['coef'] == 1.0 and recs[0]['max_norm'] == float('inf')
    for r in recs[1:]:
        assert r['max_norm'] == float(F32(first / 400.0 if r is recs[-1] else first / 100.0))
        norm = math.sqrt(r['sumsq'])
        assert one_ulp(r['norm'], F32(norm)) and one_ulp(r['coef'], F32(min(1.0, r['max_norm'] / (norm + 1e-6))))
    assert recs[-1]['coef'] < 1.0 and recs[-1]['clipped'] >= 1, recs          # (the last step at least is clipped)
    assert [r['steps'] for r in recs] == list(range(1, len(recs) + 1))


# ------------------------------------------------------------------------------------------------ train_or_resume
def test_train_or_resume_with_grad_clip(tmp_path):
    """dataset['grad_clip'] end to end on the tiny configuration of tests/test_ema_gpu.py: every epoch record carries the four figures, over the
    epoch's own iterations; without the key none of them is there; a bad value raises before a directory is made."""
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes, train_or_resume
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    keys = {'grad_norm_mean', 'grad_norm_max', 'grad_clipped_fraction', 'grad_nonfinite_steps'}

    def factory(split, batch_size, device, rank, world):
        return SyntheticCityscapes(batch_size, (32, 64), device, rank=rank, length=2)

    def kw(exp, **dataset):
        return dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                    dataset={'path': str(tmp_path / 'data'), 'settings': cs, 'loader_factory': factory, **dataset}, val_interval=1, checkpoint_interval=1,
                    checkpoint_history=2, init_weights=None, batch_size=2, epochs=2, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9,
                    weights_decay=5e-4, poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / exp),
                    description='test', early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))

    with pytest.raises(ValueError):
        train_or_resume(is_resuming_training=False, **kw('bad', grad_clip=0))
    assert not os.path.exists(str(tmp_path / 'bad'))
    hist = train_or_resume(is_resuming_training=False, **kw('exp', grad_clip=1.0))
    assert len(hist) == 3
    for h in hist[:2]:
        assert keys <= set(h) and all(np.isfinite(v) for v in h['train'][:4])
        assert 0.0 < h['grad_norm_mean'] <= h['grad_norm_max'] * (1 + 1e-6) and math.isfinite(h['grad_norm_max'])
        assert h['grad_clipped_fraction'] in (0.0, 0.5, 1.0) and h['grad_nonfinite_steps'] == 0           # 2 iterations per epoch
        assert (h['grad_clipped_fraction'] > 0.0) == (h['grad_norm_max'] + 1e-6 > 1.0)
    hist = train_or_resume(is_resuming_training=False, **kw('exp_d'))
    assert len(hist) == 3 and not any(keys & set(h) for h in hist)

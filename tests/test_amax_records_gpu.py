"""The amax records the f16x3 / f16x1 conv arithmetic scales its operands by (csrc/common.h: 256 words, max |x| as a bit pattern in the 16 shard
words), written as a side effect by the kernel that wrote the tensor.  The contract pinned here: A RECORD EQUALS, BIT FOR BIT, THE LARGEST MAGNITUDE
OF WHAT THE LAUNCH WROTE, WHEREVER THAT ELEMENT SITS - not the maximum of what it read, of what it computed before a ReLU or a Dropout, or of the rows
and channels its main loop covers.  A record that is too small turns an outlier into Inf in the fp16 split; one that is too large costs mantissa.

1. dsrl_amax (amax_kernel, the independent measurement of a tensor that carries no record) against numpy, on every path of launch_amax.
2. every amax_publish site of bn.hip and cat_channels_kernel: the record against the written tensor read back, with the unique maximum planted at each
   of amax_ref.PLANTS, kept and dropped by the Dropout; the written tensor itself against the fp64 oracle, per channel.
3. a conv fed by a producer's record gives the bits of a conv fed by a measured record, forward, weight gradient and data gradient.

Dispatch of the BatchNorm entry points (bn.hip: flat_stride, vec4_ok, fused_plan, dsrl_bn_apply, dsrl_bn_train_fwd, dsrl_bn_bwd), which the shapes of
amax_ref.FWD_CASES / BWD_CASES are chosen inside:
  float4 kernels (bn_apply4 / bn_bwd_apply4):  C % 4 == 0, every row stride % 4 == 0, every pointer 16-byte aligned;
  flat kernels (bn_apply_flat; the backward takes its sums from bn_bwd_partial_flat and applies with the scalar kernel):  C % 4 != 0, P * C % 4 == 0,
      every row stride == C, pointers aligned, C / gcd(C, 2) <= 256;
  scalar kernels (bn_apply / bn_bwd_apply):  everything else (P * C odd, or a row stride above C);
  fused kernels (bn_fused_fwd / bn_fused_bwd; dsrl_bn_train_fwd and dsrl_bn_bwd only):  the float4 conditions, a block budget of at least 128, C a
      multiple of 32 whose C / 32 groups divide 128 or 256 blocks, ceil(P / slabs) <= 1024 rows per slab; budget 0 sends (521, 256) to the float4 kernels;
      96 channels are three groups, which divide neither block count;
  from-statistics kernels (bn_stats_apply / bn_bwd_stats_apply, their own entry points):  C % 32 == 0; 1024 threads with >= 128 row blocks of partials
      over at most 2 M elements, else 512; more than 256 row blocks are reduced to 32 by a launch in front.
"""
import ctypes

import numpy as np
import pytest
import torch

import gen                     # noqa: F401
import oracle as O
import amax_ref as A
from hip_helpers import DEV, HF, D, dev, host
from test_bn_relu_mask_gpu import SHAPES as MASK_SHAPES, host_partials, pack_mask, stats_buffer

gpu = pytest.mark.gpu
Y_TOL, DX_TOL, CONV_TOL = 1e-5, 1e-4, 3e-6        # test_hip_parity.py: check(y, ., 1e-5), check(dx, ., 1e-4); the f16x3 bound of test_conv_precision_modes
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _default_conv_precision():
    HF.set_conv_precision(None)
    yield
    HF.set_conv_precision(None)


def test_shapes_are_those_of_the_mask_tests():
    assert A.STATS_SHAPES == MASK_SHAPES and A.AMAX_WORDS == HF.AMAX_WORDS


# ------------------------------------------------------------------------------------------------ helpers
def new_rec():
    return torch.zeros(HF.AMAX_WORDS, dtype=torch.int32, device=DEV)


def words(rec):
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(np.uint32).copy()


def bits(v):
    return int(np.float32(v).view(np.uint32)) & 0x7fffffff


def measure(t, ld, P, C, rec=None):
    rec = new_rec() if rec is None else rec
    HF.call('dsrl_amax', t.data_ptr(), ld, P, C, rec.data_ptr(), HF._stream())
    return rec


def assert_record(rec, values, what):
    """(a) the record is the magnitude of `values`, exactly; (b) the ticket words are untouched"""
    w = words(rec)
    got, want = int(A.record_max(w)), int(A.abs_bits_max(values))
    assert got == want, f'{what}: record {got:#010x} {"UNDER" if got < want else "OVER"}-reports the written maximum {want:#010x}'
    assert A.record_spare_words_zero(w), f'{what}: a word between the shards was written'
    return got


def padded(a, ld, fill):
    """[P][ld] device buffer holding a [P][C] in its first C columns"""
    P, C = a.shape
    if ld == C:
        return dev(a)
    buf = np.full((P, ld), fill, np.float32)
    buf[:, :C] = a
    return dev(buf)


# ------------------------------------------------------------------------------------------------ 1. dsrl_amax against numpy
SCALAR_SHAPES = [(1, 1), (1, 3), (7, 19), (105, 19)]           # C % 4 != 0: one float per thread
FLOAT4_SHAPES = [(1, 4), (64, 4), (65, 48), (300, 256)]


@gpu
@pytest.mark.parametrize('P,C', SCALAR_SHAPES + FLOAT4_SHAPES)
def test_amax_dense_with_the_maximum_planted_everywhere(P, C):
    """the unique maximum, a negative number, at each of PLANTS; and the tensor as drawn"""
    rs = np.random.RandomState(P + C)
    a = rs.standard_normal((P, C)).astype(np.float32)
    assert_record(measure(dev(a), C, P, C), a, 'as drawn')
    for pos in A.PLANTS(P, C):
        b = a.copy()
        b[pos] = -50.0
        assert assert_record(measure(dev(b), C, P, C), b, f'plant {pos}') == bits(50.0)


@gpu
@pytest.mark.parametrize('P,C', [((1 << 15) + 3, 256), ((1 << 22) + 1027, 1)])
def test_amax_grid_wrap(P, C):
    """more float4 (first case) / floats (second) than 2048 blocks x 256 threads x 4: every thread loops, the last elements belong to a partial round"""
    assert (P * C // 4 if C % 4 == 0 else P * C) > 2048 * 256 * 4
    rs = np.random.RandomState(C)
    a = rs.standard_normal((P, C)).astype(np.float32)
    t = dev(a)
    assert_record(measure(t, C, P, C), a, 'as drawn')
    for pos in ((P - 1, C - 1), (0, 0), (P - 2, C // 2)):
        a[pos] = -50.0
        t[pos] = -50.0
        assert assert_record(measure(t, C, P, C), a, f'plant {pos}') == bits(50.0)
        a[pos] = 0.5
        t[pos] = 0.5


@gpu
@pytest.mark.parametrize('P,C,ld', [(65, 48, 64), (105, 19, 24)])
@pytest.mark.parametrize('fill', [1e30, np.nan])
def test_amax_strided_ignores_the_padding_channels(P, C, ld, fill):
    rs = np.random.RandomState(ld)
    a = rs.standard_normal((P, C)).astype(np.float32)
    for pos in [None] + A.PLANTS(P, C):
        b = a.copy()
        if pos is not None:
            b[pos] = -50.0
        got = assert_record(measure(padded(b, ld, fill), ld, P, C), b, f'ld {ld} plant {pos}')
        assert got < bits(1e30)


@gpu
def test_amax_unaligned_base_takes_the_scalar_path():
    P, C = 65, 48
    a = np.random.RandomState(5).standard_normal((P, C)).astype(np.float32)
    for pos in [None] + A.PLANTS(P, C):
        b = a.copy()
        if pos is not None:
            b[pos] = -50.0
        buf = torch.full((P * C + 1,), 1e30, device=DEV)
        buf[1:] = dev(b).reshape(-1)
        t = buf[1:]
        assert t.data_ptr() % 16 == 4
        assert_record(measure(t, C, P, C), b, f'unaligned, plant {pos}')


@gpu
@pytest.mark.parametrize('P,C', [(7, 19), (65, 48)])
def test_amax_special_values(P, C):
    z = np.zeros((P, C), np.float32)

    def run(pos, value):
        b = z.copy()
        b[pos] = value
        return assert_record(measure(dev(b), C, P, C), b, f'{value!r} at {pos}')
    last = (P - 1, C - 1)
    assert assert_record(measure(dev(z), C, P, C), z, 'all zero') == 0
    assert run((P // 2, 1), -0.0) == 0                                  # -0.0 alone: the sign is cleared, the record stays 0
    assert run(last, -3.5) == bits(3.5)
    assert 0 < run(last, 1e-40) < 0x00800000                            # a subnormal maximum
    assert run((0, 0), np.inf) == A.INF_BITS and run(last, -np.inf) == A.INF_BITS
    assert run(last, np.nan) > A.INF_BITS                               # one NaN at the last element sorts above Inf
    b = np.random.RandomState(1).standard_normal((P, C)).astype(np.float32)
    b[0, 0], b[last] = np.inf, np.nan
    assert assert_record(measure(dev(b), C, P, C), b, 'Inf and NaN') > A.INF_BITS


@gpu
@pytest.mark.parametrize('P,C', [(7, 19), (65, 48)])
def test_amax_maxes_into_the_record_it_is_given(P, C):
    rs = np.random.RandomState(9)
    a, b = rs.standard_normal((P, C)).astype(np.float32), (rs.standard_normal((P, C)) * 8).astype(np.float32)
    for first, second in ((a, b), (b, a)):
        rec = measure(dev(first), C, P, C)
        measure(dev(second), C, P, C, rec)
        assert_record(rec, np.stack([a, b]), 'two tensors into one record')
    for seeded, want in ((1000.0, bits(1000.0)), (1e-3, int(A.abs_bits_max(a)))):
        rec = new_rec()
        rec[3 * 16] = bits(seeded)                                      # shard 3
        measure(dev(a), C, P, C, rec)
        w = words(rec)
        assert int(A.record_max(w)) == want and A.record_spare_words_zero(w), seeded
        assert w[3 * 16] >= bits(seeded)                                # a shard only ever grows


# ------------------------------------------------------------------------------------------------ 2. the producers
class Budget:
    """the block budget of the fused BatchNorm set to 0 around a launch, and back to the environment's"""

    def __init__(self, zero):
        self.zero = zero

    def __enter__(self):
        if self.zero:
            HF.set_bn_fused_max_blocks(0)

    def __exit__(self, *exc):
        if self.zero:
            HF.set_bn_fused_max_blocks(None)
        return False


def run_forward(case, v, d, seed, stats_of=None):
    """one forward launch of `case` on the inputs d; -> dict(y [P][C] on the host, rec, device y / mean / invstd, stats handed to dsrl_bn_apply)"""
    P, C, ld = case.P, case.C, case.ld
    x, r = padded(d['x'], ld, 1e30), padded(d['r'], ld, 1e30)
    gamma, beta = dev(d['gamma']), dev(d['beta'])
    y = torch.full((P, ld), SENTINEL, device=DEV)
    rec = new_rec()
    st = HF._stream()
    rp = r.data_ptr() if v.res else None
    given = None
    with Budget(case.budget0):
        if case.entry == 'dsrl_bn_apply':
            clean = np.nan_to_num(d['x']).astype(np.float64)
            given = (clean.mean(0).astype(np.float32), (1.0 / np.sqrt(clean.var(0) + A.EPS)).astype(np.float32))
            mean, invstd = dev(given[0]), dev(given[1])
            HF.call('dsrl_bn_apply', x.data_ptr(), ld, y.data_ptr(), ld, P, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rp, ld,
                    int(v.relu), float(v.drop), int(seed), A.RNG_STREAM, rec.data_ptr(), st)
        else:
            mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
            head = (x.data_ptr(), ld, y.data_ptr(), ld, P, C, A.EPS, A.MOM, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), gamma.data_ptr(),
                    beta.data_ptr(), rp, ld, int(v.relu), float(v.drop), int(seed), A.RNG_STREAM)
            if case.entry == 'dsrl_bn_train_fwd':
                ws = torch.empty(int(HF.query('dsrl_bn_workspace_bytes', P, C)) + 256, dtype=torch.uint8, device=DEV)
                HF.call(case.entry, *head, ws.data_ptr(), ws.numel(), rec.data_ptr(), st)
            else:
                part = host_partials(d['x'] if stats_of is None else stats_of, case.parts, 3)
                stats = stats_buffer(part, C)
                if case.entry.endswith('_mask'):
                    mask = torch.zeros(int(HF.query('dsrl_bn_mask_words', P, C)), dtype=torch.int32, device=DEV)
                    HF.call(case.entry, *head, stats.data_ptr(), case.parts, rec.data_ptr(), mask.data_ptr(), st)
                else:
                    HF.call(case.entry, *head, stats.data_ptr(), case.parts, rec.data_ptr(), st)
    torch.cuda.synchronize()
    yh = host(y)
    assert (yh[:, C:] == SENTINEL).all(), 'the launch wrote into the padding channels of y'
    return dict(y=np.ascontiguousarray(yh[:, :C]), rec=rec, y_dev=y, mean=mean, invstd=invstd, given=given)


@gpu
@pytest.mark.parametrize('case,v', A.FWD_PARAMS, ids=[A.case_id(c, v) for c, v in A.FWD_PARAMS])
def test_forward_record_equals_what_was_written(case, v):
    """every forward path (amax_ref.FWD_CASES), every variant, the unique maximum of y planted at every one of PLANTS; under
    Dropout once kept and once dropped - then the record is the runner-up's magnitude"""
    P, C = case.P, case.C
    worst = 0.0
    for pos in A.PLANTS(P, C):
        d = A.forward_inputs(P, C, v.res, pos)
        for seed, kept in A.seeds_of(P, C, pos, v.drop):
            out = run_forward(case, v, d, seed)
            what = f'{A.case_id(case, v)} plant {pos} seed {seed} ({"kept" if kept else "dropped"})'
            got = assert_record(out['rec'], out['y'], what)
            y = out['y']
            if kept:
                rest = np.abs(y)
                rest[pos] = 0.0
                assert got == bits(y[pos]) and abs(y[pos]) >= A.MARGIN * rest.max(), what
            else:
                assert y[pos] == 0.0 and got < bits(A.GAMMA_PLANT), what
            yref, _, _, rng = A.forward_reference(d, v, seed, out['given'])
            e = A.per_channel_error(y, yref, rng)
            worst = max(worst, e)
            assert e <= Y_TOL, f'{what}: y differs from the oracle by {e:.3e} of a channel\'s range'
    print(f'{A.case_id(case, v)}: record exact at {len(A.PLANTS(P, C))} positions, y within {worst:.2e} per channel')


@gpu
@pytest.mark.parametrize('case,v', A.FWD_LONG, ids=[A.case_id(c, v) for c, v in A.FWD_LONG])
def test_forward_record_of_long_slabs(case, v):
    """slabs of several passes (amax_ref.LONG_STATS_SHAPES): the rows behind a thread's first one, the unrolled group of four and the tail loop"""
    P, C = case.P, case.C
    for pos in A.long_plants(P, C):
        d = A.forward_inputs(P, C, v.res, pos)
        out = run_forward(case, v, d, 1)
        what = f'{A.case_id(case, v)} plant {pos}'
        assert assert_record(out['rec'], out['y'], what) == bits(out['y'][pos]), what
        yref, _, _, rng = A.forward_reference(d, v, 1)
        e = A.per_channel_error(out['y'], yref, rng)
        assert e <= Y_TOL, f'{what}: y differs from the oracle by {e:.3e} of a channel\'s range'


NAN_FWD = [c for c in A.FWD_CASES if not c.entry.endswith('_mask')]       # the sign-mask entry exists behind a ReLU only, and a ReLU stores 0 for a NaN


@gpu
@pytest.mark.parametrize('case', NAN_FWD, ids=['-'.join(map(str, c)) for c in NAN_FWD])
def test_forward_record_of_a_nan(case):
    """a NaN in x, no ReLU: it is stored (with batch statistics, in its whole channel) and the record sorts above Inf"""
    P, C = case.P, case.C
    pos = (P // 2, C // 2)
    v = A.FwdVariant(False, 0, 0.0)
    d = A.forward_inputs(P, C, False, pos, nan=True)
    out = run_forward(case, v, d, 1, stats_of=np.nan_to_num(d['x']))
    assert np.isnan(out['y'][pos])
    assert assert_record(out['rec'], out['y'], f'NaN at {pos}') > A.INF_BITS


def run_backward(case, v, d, fwd, g, nan=False):
    """one backward launch: x, dy of d; y / mean / invstd of the forward launch `fwd`; for the from-statistics entries the sums of the masked gradient g"""
    P, C = case.P, case.C
    x, dy, gamma = dev(d['x']), dev(d['dy']), dev(d['gamma'])
    dx, dres = torch.full((P, C), SENTINEL, device=DEV), torch.full((P, C), SENTINEL, device=DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    rec = new_rec()
    st = HF._stream()
    drp = dres.data_ptr() if v.dres else None
    y = fwd['y_dev']
    if case.entry == 'dsrl_bn_bwd':
        ws = torch.empty(int(HF.query('dsrl_bn_workspace_bytes', P, C)) + 256, dtype=torch.uint8, device=DEV)
        with Budget(case.budget0):
            HF.call('dsrl_bn_bwd', x.data_ptr(), C, None if y is None else y.data_ptr(), C, dy.data_ptr(), C, dx.data_ptr(), C, drp, C, P, C,
                    fwd['mean'].data_ptr(), fwd['invstd'].data_ptr(), gamma.data_ptr(), dg.data_ptr(), db.data_ptr(), int(v.relu), float(v.drop), int(v.training),
                    ws.data_ptr(), ws.numel(), rec.data_ptr(), st)
    else:
        part = A.bwd_partials(np.nan_to_num(g), np.nan_to_num(A.xhat_of(d)), case.parts)
        stats = stats_buffer(part, C)
        if v.relu == 2:
            mask = torch.from_numpy(pack_mask(host(y)).view(np.int32)).to(DEV)
            ym = (mask.data_ptr(), P)
        else:
            ym = (None if y is None else y.data_ptr(), C)
        extra, keepalive = (), None
        if case.entry.endswith('_res'):
            rs = np.random.RandomState(P + 7 * C)
            rparts = int(HF.query('dsrl_bn_bwd_from_stats_res_parts', P, C, case.parts))
            assert rparts > 0
            keepalive = (dev((rs.standard_normal((P, C)) * 2 + 0.5).astype(np.float32)), dev(rs.standard_normal(C).astype(np.float32)),
                         dev(rs.uniform(0.5, 2, C).astype(np.float32)), torch.zeros(int(HF.query('dsrl_bn_stats_floats', 2, rparts, C)), device=DEV))
            extra = (keepalive[0].data_ptr(), C, keepalive[1].data_ptr(), keepalive[2].data_ptr(), keepalive[3].data_ptr(), rparts)
        HF.call(case.entry, x.data_ptr(), C, ym[0], ym[1], dy.data_ptr(), C, dx.data_ptr(), C, drp, C, P, C, fwd['mean'].data_ptr(), fwd['invstd'].data_ptr(),
                gamma.data_ptr(), dg.data_ptr(), db.data_ptr(), int(v.relu), float(v.drop), int(v.training), stats.data_ptr(), case.parts, rec.data_ptr(), *extra, st)
    torch.cuda.synchronize()
    return dict(dx=host(dx), dres=host(dres) if v.dres else None, rec=rec, dx_dev=dx)


FWD_OF_BWD = A.Fwd('forward of a backward case', 'dsrl_bn_train_fwd', 0, 0, 0, 0, False)


@gpu
@pytest.mark.parametrize('case,v', A.BWD_PARAMS, ids=[A.case_id(c, v) for c, v in A.BWD_PARAMS])
def test_backward_record_equals_what_was_written(case, v):
    """every backward path (amax_ref.BWD_CASES); y, mean and invstd come from a forward launch of the same case, the masked
    gradient from that y as the kernels define it, and the from-statistics entries are handed the sums of that gradient"""
    P, C = case.P, case.C
    fv = A.backward_forward_variant(v)
    fcase = FWD_OF_BWD._replace(P=P, C=C, ld=C)
    worst = 0.0
    for pos in A.PLANTS(P, C):
        d = A.backward_inputs(P, C, pos)
        for seed, kept in A.seeds_of(P, C, pos, v.drop):
            fwd = run_forward(fcase, fv, d, seed)
            g = A.masked_gradient(d, v, fwd['y'].astype(np.float64))
            assert (g[pos] != 0.0) == kept
            out = run_backward(case, v, d, fwd, g)
            what = f'{A.case_id(case, v)} plant {pos} seed {seed} ({"kept" if kept else "dropped"})'
            got = assert_record(out['rec'], out['dx'], what)
            dx = out['dx']
            assert (got == bits(dx[pos])) == kept, what
            dxref = A.backward_reference(d, v, g)
            e = A.per_channel_error(dx, dxref)
            worst = max(worst, e)
            assert e <= DX_TOL, f'{what}: dx differs from the oracle by {e:.3e} of a channel\'s range'
            if v.dres:
                assert A.per_channel_error(out['dres'], g) <= Y_TOL, what
    print(f'{A.case_id(case, v)}: record exact at {len(A.PLANTS(P, C))} positions, dx within {worst:.2e} per channel')


@gpu
@pytest.mark.parametrize('case,v', A.BWD_LONG, ids=[A.case_id(c, v) for c, v in A.BWD_LONG])
def test_backward_record_of_long_slabs(case, v):
    """slabs of several passes (amax_ref.LONG_STATS_SHAPES): the loop behind a thread's first row"""
    P, C = case.P, case.C
    fcase = FWD_OF_BWD._replace(P=P, C=C, ld=C)
    for pos in A.long_plants(P, C):
        d = A.backward_inputs(P, C, pos)
        fwd = run_forward(fcase, A.backward_forward_variant(v), d, 1)
        g = A.masked_gradient(d, v, fwd['y'].astype(np.float64))
        out = run_backward(case, v, d, fwd, g)
        what = f'{A.case_id(case, v)} plant {pos}'
        assert assert_record(out['rec'], out['dx'], what) == bits(out['dx'][pos]), what
        e = A.per_channel_error(out['dx'], A.backward_reference(d, v, g))
        assert e <= DX_TOL, f'{what}: dx differs from the oracle by {e:.3e} of a channel\'s range'
        assert A.per_channel_error(out['dres'], g) <= Y_TOL, what


@gpu
@pytest.mark.parametrize('case', A.BWD_CASES, ids=['-'.join(map(str, c)) for c in A.BWD_CASES])
def test_backward_record_of_a_nan(case):
    """a NaN in x, no ReLU, frozen statistics: dx holds it in that one element, and the record sorts above Inf"""
    P, C = case.P, case.C
    pos = (P // 2, C // 2)
    v = A.BwdVariant(0, 0.0, case.entry.endswith('_res'), 0)
    d = A.backward_inputs(P, C, pos)
    clean = d['x'].astype(np.float64)
    fwd = dict(y_dev=None, mean=dev(clean.mean(0).astype(np.float32)), invstd=dev((1.0 / np.sqrt(clean.var(0) + A.EPS)).astype(np.float32)))
    d['x'][pos] = np.nan
    out = run_backward(case, v, d, fwd, d['dy'].astype(np.float64))
    assert np.isnan(out['dx'][pos]) and np.isnan(out['dx']).sum() == 1
    assert assert_record(out['rec'], out['dx'], f'NaN at {pos}') > A.INF_BITS


@gpu
@pytest.mark.parametrize('widths,strided', A.CAT_CASES)
def test_concatenation_record_equals_what_was_written(widths, strided):
    P, n, ctot = A.CAT_ROWS, len(widths), sum(widths)
    ld_dst = ctot + 8
    for plant in A.cat_plants(widths):
        xs = A.cat_inputs(widths, plant)
        ts = [padded(x, 2 * x.shape[1] if strided else x.shape[1], 1e30) for x in xs]
        y = torch.full((P, ld_dst), SENTINEL, device=DEV)
        rec = new_rec()
        srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        lds = (ctypes.c_int32 * n)(*[t.shape[1] for t in ts])
        cs = (ctypes.c_int32 * n)(*widths)
        assert HF.query('dsrl_cat_channels_supported', srcs, lds, cs, n, y.data_ptr(), ld_dst, P)
        HF.call('dsrl_cat_channels', srcs, lds, cs, n, y.data_ptr(), ld_dst, P, rec.data_ptr(), HF._stream())
        yh = host(y)
        ref = np.concatenate(xs, 1)
        assert np.array_equal(yh[:, :ctot], ref) and (yh[:, ctot:] == SENTINEL).all(), plant
        assert assert_record(rec, ref, f'cat {widths} plant {plant}') == bits(A.RES_PLANT)


# ------------------------------------------------------------------------------------------------ 3. a conv fed by a producer's record
@gpu
@pytest.mark.parametrize('C', [19, 48, 64])        # bn_apply_flat_kernel, bn_apply4_kernel, bn_fused_fwd_kernel
def test_conv_reads_a_producer_record_like_a_measured_one(C):
    """y = relu(bn(x) + r) with +4096 in the last channel of the last pixel carries the record its kernel left; a conv of y and a conv of a copy of y
    that carries nothing (measured by dsrl_amax) are bit-identical, output and weight gradient.  Against the fp64 oracle the output pixels whose 3x3
    window holds the planted element, and all the others, are each within the f16x3 bound of their own range (conv_common.h: an operand 2^12 below the
    tensor's maximum keeps its full precision inside the 2^18 window)."""
    HF.set_conv_precision('f16x3')
    N, H, W, K = 2, 6, 10, 32
    rs = np.random.RandomState(C)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    r = rs.standard_normal((N, C, H, W)).astype(np.float32)
    r[N - 1, C - 1, H - 1, W - 1] = A.RES_PLANT
    w0 = (rs.standard_normal((K, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    dz = rs.standard_normal((N, K, H, W)).astype(np.float32)
    bn = D.nn_modules.HipBatchNorm2d(C).to(DEV).train()
    for p in bn.parameters():
        p.requires_grad_(False)
    y = HF.batch_norm_act(dev(x), bn, relu=True, residual=dev(r))
    rec = HF.carried_amax(y)
    assert rec is not None
    yh = host(y)
    assert assert_record(rec, yh, f'batch_norm_act C = {C}') == bits(yh[N - 1, C - 1, H - 1, W - 1]) and yh.max() > 4000
    outs = []
    for src in (y, y.detach().clone(memory_format=torch.channels_last)):
        assert (src is y) == (HF.carried_amax(src) is not None)
        w = dev(w0).requires_grad_(True)
        z = HF.conv2d(src, w, None, 1, 1, 1)
        z.backward(dev(dz))
        torch.cuda.synchronize()
        outs.append((host(z), host(w.grad)))
    (z1, dw1), (z2, dw2) = outs
    assert np.isfinite(z1).all() and np.isfinite(dw1).all() and np.isfinite(z2).all() and np.isfinite(dw2).all()
    zo = O.conv2d(yh.astype(np.float64), w0.astype(np.float64), None, 1, 1, 1)
    near = np.zeros(zo.shape, bool)
    near[N - 1, :, H - 2:, W - 2:] = True
    errs = [(name, group, float(np.abs(z[m] - zo[m]).max() / np.abs(zo[m]).max()))
            for name, z in (('measured record', z2), ('producer record', z1))
            for group, m in (('window holds the planted element', near), ('all other pixels', ~near))]
    for name, group, e in errs:
        print(f'C = {C}, {name}, {group}: error {e:.3e} = {e / CONV_TOL:.3f} of the bound {CONV_TOL:.0e}')
    for name, group, e in errs:         # the measured-record run first: a miss there is a finding about the arithmetic, not about the record
        assert e <= CONV_TOL, f'C = {C}, {name}, {group}: {e:.3e} > {CONV_TOL:.0e}'
    assert np.array_equal(z1.view(np.uint32), z2.view(np.uint32)), 'the conv output depends on where the record came from'
    assert np.array_equal(dw1.view(np.uint32), dw2.view(np.uint32)), 'the weight gradient depends on where the record came from'


@gpu
def test_dgrad_reads_a_producer_record_like_a_measured_one():
    """dx of dsrl_bn_bwd (bn_bwd_apply4_kernel, C = 48, the maximum planted through dy in the last channel of the last pixel) is the dy operand of the
    conv in front of the BatchNorm: dsrl_conv2d_dgrad_amax with the record the kernel left and with one measured by dsrl_amax, bit for bit"""
    HF.set_conv_precision('f16x3')
    N, H, W, Cin, K = 2, 6, 10, 32, 48
    P = N * H * W
    case, v = A.Bwd('bn_bwd_apply4_kernel', 'dsrl_bn_bwd', P, K, 0, False), A.BwdVariant(0, 0.0, False, 1)
    pos = (P - 1, K - 1)
    d = A.backward_inputs(P, K, pos)
    fwd = run_forward(FWD_OF_BWD._replace(P=P, C=K, ld=K), A.backward_forward_variant(v), d, 1)
    out = run_backward(case, v, d, fwd, d['dy'].astype(np.float64))
    assert assert_record(out['rec'], out['dx'], 'dsrl_bn_bwd') == bits(out['dx'][pos])
    g = out['dx_dev']
    measured = measure(g, K, P, K)
    assert int(A.record_max(words(measured))) == int(A.record_max(words(out['rec'])))
    w = dev((np.random.RandomState(3).standard_normal((K, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32))
    wrec, _, wtsp, wtr = HF.split_filter(w)
    shp = (N, H, W, Cin, K, 3, 3, 1, 1, 1)
    ws = torch.empty(int(HF.query('dsrl_conv2d_dgrad_workspace_bytes', *shp)) + 256, dtype=torch.uint8, device=DEV)
    got = []
    for rec in (out['rec'], measured):
        dxc = torch.full((N, Cin, H, W), SENTINEL, device=DEV).contiguous(memory_format=torch.channels_last)
        HF.call('dsrl_conv2d_dgrad_amax', g.data_ptr(), K, rec.data_ptr(), w.data_ptr(), wtr.data_ptr(), wrec.data_ptr(), wtsp.data_ptr(), dxc.data_ptr(), Cin, *shp,
                ws.data_ptr(), ws.numel(), None, 0, None, 0, None, None, 0, None, 0, 0, HF._stream())
        torch.cuda.synchronize()
        got.append(host(dxc))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[0] != SENTINEL).all()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), 'the data gradient depends on where the record came from'

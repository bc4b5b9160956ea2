"""Plain references for the amax records (csrc/common.h: 256 uint32 words, max |x| as a bit pattern in 16 shard words, one every 16th word; the other
240 words belong to the split-K tickets) and the planted inputs of tests/test_amax_records_gpu.py.  numpy and the fp64 oracle only: importable without
a GPU, so that tests/test_amax_ref_host.py can prove on the CPU that every planted case has the maximum where the GPU test says it is.

Every tensor is a flat [P][C] float32 array (pixel-major, as the kernels see it); the oracle's (N, C, H, W) is (1, C, P, 1) of it, and the Dropout draw of
element (p, c) is the Philox word of linear index p * C + c (oracle/philox.py)."""
import collections
import functools

import numpy as np

import oracle as O

AMAX_WORDS, SHARDS, SHARD_STRIDE = 256, 16, 16
INF_BITS = 0x7f800000
EPS, MOM, RNG_STREAM = 1e-5, 0.1, 3
DROP_P = 0.2
RES_PLANT, X_PLANT, DY_PLANT, GAMMA_PLANT = 4096.0, 1000.0, 64.0, 64.0
MARGIN = 4.0


# ------------------------------------------------------------------------------------------------ records
def record_max(rec):
    """the value a reader takes from a record: the maximum of its 16 shard words"""
    rec = np.asarray(rec)
    assert rec.dtype == np.uint32 and rec.shape == (AMAX_WORDS,), (rec.dtype, rec.shape)
    return np.uint32(rec[0::SHARD_STRIDE].max())


def record_spare_words_zero(rec):
    """the 240 words between the shards (the split-K ticket words of conv_common.h) are zero: no producer may touch them"""
    rec = np.asarray(rec)
    assert rec.dtype == np.uint32 and rec.shape == (AMAX_WORDS,), (rec.dtype, rec.shape)
    spare = np.ones(AMAX_WORDS, bool)
    spare[0::SHARD_STRIDE] = False
    return bool((rec[spare] == 0).all())


def abs_bits_max(a):
    """max over a float32 array of the bit pattern with the sign cleared: what the kernels max into a record (NaN patterns sort above Inf)"""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return np.uint32((a.reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)).max()) if a.size else np.uint32(0)


def PLANTS(P, C):
    """The probed positions (row, channel) of a [P][C] tensor, all distinct and inside it (a one-channel or three-channel tensor has fewer): the four
    corners, the middle, the last full group of four in front of a channel tail, the row before last."""
    cand = [(0, 0), (0, C - 1), (P - 1, 0), (P - 1, C - 1), (P // 2, C // 2), (P - 1, C - 1 - (C % 4 or 4)), (P - 2, 1)]
    out = []
    for p, c in cand:
        if 0 <= p < P and 0 <= c < C and (p, c) not in out:
            out.append((p, c))
    return out


# ------------------------------------------------------------------------------------------------ Dropout
def uniform_at(P, C, pos, seed, stream=RNG_STREAM):
    """the uniform of element `pos` alone (one Philox block instead of the whole tensor's)"""
    e = pos[0] * C + pos[1]
    q = e >> 2
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = O.philox.philox4x32_10(np.array([q & 0xFFFFFFFF], np.uint32), np.array([q >> 32], np.uint32), np.uint32(stream), np.uint32(0), seed & 0xFFFFFFFF, seed >> 32)
    return float(np.float32(int(r[e & 3][0]) >> 8) * np.float32(2.0 ** -24))


@functools.lru_cache(maxsize=64)
def keep_mask(P, C, seed, p=DROP_P, stream=RNG_STREAM):
    """keep mask [P][C] of oracle.dropout_mask; cached, never modified"""
    m = np.ascontiguousarray(O.dropout_mask((1, C, P, 1), p, seed, stream)[0, :, :, 0].T)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def drop_seeds(P, C, pos, p=DROP_P, stream=RNG_STREAM):
    """(seed that keeps element `pos`, seed that drops it): the smallest of each from 1 up; both are confirmed against oracle.dropout_mask"""
    kept = dropped = None
    for seed in range(1, 200):
        keep = uniform_at(P, C, pos, seed, stream) >= np.float32(p)
        if keep and kept is None:
            kept = seed
        if not keep and dropped is None:
            dropped = seed
        if kept is not None and dropped is not None:
            break
    assert kept is not None and dropped is not None, (P, C, pos)
    assert keep_mask(P, C, kept, p, stream)[pos] and not keep_mask(P, C, dropped, p, stream)[pos]
    return kept, dropped


# ------------------------------------------------------------------------------------------------ case tables
# A forward path: the kernel the dispatch of bn.hip takes for this shape, the entry point, [P][C] with row stride ld, the row blocks of handed-in
# partials (from-statistics entries), and whether the fused budget is set to 0 around the launch.
Fwd = collections.namedtuple('Fwd', 'kernel entry P C ld parts budget0')
Bwd = collections.namedtuple('Bwd', 'kernel entry P C parts budget0')
STATS_SHAPES = [(70, 32, 3), (521, 96, 5), (256, 32, 128), (600, 64, 300)]       # the SHAPES of tests/test_bn_relu_mask_gpu.py (asserted equal there)


def _fwd_cases():
    out = []
    for entry in ('dsrl_bn_apply', 'dsrl_bn_train_fwd'):
        out += [Fwd('bn_apply_kernel', entry, 105, 19, 19, 0, False), Fwd('bn_apply_kernel', entry, 120, 19, 24, 0, False)]
        out += [Fwd('bn_apply_flat_kernel', entry, P, C, C, 0, False) for P, C in ((120, 19), (70, 6), (44, 3), (128, 1))]
        out += [Fwd('bn_apply4_kernel', entry, 105, 48, 48, 0, False), Fwd('bn_apply4_kernel', entry, 70, 96, 128, 0, False),
                Fwd('bn_apply4_kernel', entry, 521, 256, 256, 0, True)]
    out += [Fwd('bn_fused_fwd_kernel', 'dsrl_bn_train_fwd', P, C, C, 0, False) for P, C in ((70, 32), (521, 256), (2, 64))]
    for entry in ('dsrl_bn_train_fwd_from_stats', 'dsrl_bn_train_fwd_from_stats_mask'):
        out += [Fwd('bn_stats_apply_kernel', entry, P, C, C, parts, False) for P, C, parts in STATS_SHAPES]
    return out


def _bwd_cases():
    out = [Bwd('bn_bwd_apply_kernel', 'dsrl_bn_bwd', 105, 19, 0, False), Bwd('bn_bwd_apply_kernel', 'dsrl_bn_bwd', 120, 19, 0, False),
           Bwd('bn_bwd_apply4_kernel', 'dsrl_bn_bwd', 105, 48, 0, False), Bwd('bn_bwd_apply4_kernel', 'dsrl_bn_bwd', 521, 256, 0, True),
           Bwd('bn_fused_bwd_kernel', 'dsrl_bn_bwd', 70, 32, 0, False), Bwd('bn_fused_bwd_kernel', 'dsrl_bn_bwd', 521, 256, 0, False)]
    for entry in ('dsrl_bn_bwd_from_stats_drop', 'dsrl_bn_bwd_from_stats_res'):
        out += [Bwd('bn_bwd_stats_apply_kernel', entry, P, C, parts, False) for P, C, parts in STATS_SHAPES]
    return out


FWD_CASES, BWD_CASES = _fwd_cases(), _bwd_cases()
FwdVariant = collections.namedtuple('FwdVariant', 'res relu drop')
BwdVariant = collections.namedtuple('BwdVariant', 'relu drop dres training')      # relu: 0, 1, or 2 = the kernel reads the sign mask instead of y


def fwd_variants(case):
    """{no residual, residual} x {no ReLU, ReLU} x {p = 0, p = 0.2}; the entry that also leaves the sign mask exists behind a ReLU only"""
    vs = [FwdVariant(res, relu, drop) for res in (False, True) for relu in (0, 1) for drop in (0.0, DROP_P)]
    return [v for v in vs if v.relu or not case.entry.endswith('_mask')]


def bwd_variants(case):
    """what the entry allows: dsrl_bn_bwd takes a Dropout with or without a ReLU; the from-statistics entries take y or its sign mask behind a ReLU
    and a Dropout only with it; the _res entry always writes dresidual"""
    if case.entry == 'dsrl_bn_bwd':
        base = [(0, 0.0, False), (1, 0.0, False), (1, 0.0, True), (1, DROP_P, False), (1, DROP_P, True), (0, DROP_P, False)]
    elif case.entry == 'dsrl_bn_bwd_from_stats_drop':
        base = [(relu, drop, dres) for relu in (1, 2) for drop in (0.0, DROP_P) for dres in (False, True)]
    else:
        base = [(relu, drop, True) for relu in (1, 2) for drop in (0.0, DROP_P)]
    return [BwdVariant(*b, training) for b in base for training in (0, 1)]


def case_id(case, variant):
    return '-'.join(str(v) for v in tuple(case) + tuple(variant))


FWD_PARAMS = [(c, v) for c in FWD_CASES for v in fwd_variants(c)]
BWD_PARAMS = [(c, v) for c in BWD_CASES for v in bwd_variants(c)]

# Long slabs.  A from-statistics block streams its slab in passes of threads / 8 rows, and the launch cuts ceil(P / rows per pass) slabs until there are
# 4 * 256 * 256 / threads blocks - so in STATS_SHAPES no thread ever takes a second row, and the loops behind the first row (in the sign-mask kernel a
# hand-unrolled group of four passes and a tail loop) run on larger tensors only.  The smallest that reach them, (P, C, row blocks of partials):
#   (32805, 64, 5):    512 threads, 2 groups: 255 slabs of 129 rows = three passes, the last of one row; the last slab has 39 rows
#   (40000, 32, 128):  1024 threads (>= 128 partials, <= 2 M elements): 255 slabs of 157 rows = two passes of 128; the last slab has 122 rows
#   (7163, 1024, 5):   512 threads, 32 groups: 16 slabs of 448 rows = the first row, one unrolled group of four passes, two tail passes; 443 in the last
# Residual + ReLU without Dropout (a Philox draw per element of the oracle would take seconds); the largest shape forward only, the backward kernel has
# one loop.  Plants: the last row, rows of the tail passes and of the unrolled group of the last slab, the middle.
LONG_STATS_SHAPES = [(32805, 64, 5), (40000, 32, 128), (7163, 1024, 5)]
FWD_LONG = [(Fwd('bn_stats_apply_kernel', entry, P, C, C, parts, False), FwdVariant(True, 1, 0.0))
            for entry in ('dsrl_bn_train_fwd_from_stats', 'dsrl_bn_train_fwd_from_stats_mask') for P, C, parts in LONG_STATS_SHAPES]
BWD_LONG = [(Bwd('bn_bwd_stats_apply_kernel', entry, P, C, parts, False), BwdVariant(relu, 0.0, True, 1))
            for P, C, parts in LONG_STATS_SHAPES[:2]
            for entry, relu in (('dsrl_bn_bwd_from_stats_drop', 1), ('dsrl_bn_bwd_from_stats_drop', 2), ('dsrl_bn_bwd_from_stats_res', 1))]


def long_plants(P, C):
    return [(P - 1, C - 1), (P - 70, 1), (P - 300, 2), (P // 2, C // 2)]


def seeds_of(P, C, pos, drop):
    """the Dropout keys one plant runs under: [(seed, planted element kept?)]"""
    if drop == 0.0:
        return [(1, True)]
    kept, dropped = drop_seeds(P, C, pos)
    return [(kept, True), (dropped, False)]


# ------------------------------------------------------------------------------------------------ planted inputs
def _nchw(a):
    return np.ascontiguousarray(a.T)[None, :, :, None]


def _flat(a):
    return np.ascontiguousarray(a[0, :, :, 0].T)


@functools.lru_cache(maxsize=4)
def _base(P, C):
    """N(0,1)-scale tensors of one shape, drawn once and never modified (the builders copy)"""
    rs = np.random.RandomState(1000 * P + C)
    x = rs.standard_normal((P, C)).astype(np.float32)
    if P == 2:
        # two rows: a channel whose two values nearly coincide has invstd ~ 1 / sqrt(eps) and loses its digits to x - mean, the ill-conditioned
        # offset-channel case that is not this test's subject; the rows are kept at least 1 apart
        x[1] = x[0] + (rs.uniform(1.0, 2.0, C) * rs.choice([-1.0, 1.0], C)).astype(np.float32)
    d = dict(x=x, r=rs.standard_normal((P, C)).astype(np.float32), dy=rs.standard_normal((P, C)).astype(np.float32),
             gamma=rs.uniform(0.5, 1.5, C).astype(np.float32), beta=(rs.standard_normal(C) * 0.3).astype(np.float32))
    for v in d.values():
        v.setflags(write=False)
    return d


def forward_inputs(P, C, res, pos, nan=False):
    """x, r, gamma, beta of a forward case whose output has its unique maximum at `pos`: +4096 in the residual where there is one; else x[pos] = 1000
    (normalised: ~sqrt(P - 1), every other row of the channel ~ -1 / sqrt(P - 1)) with gamma = 64 in that channel and beta = 64 / sqrt(P - 1), which
    moves those other rows to ~0 (at P = 2 they would mirror the planted one).  nan: a NaN at `pos` instead, nothing else planted."""
    b = _base(P, C)
    d = {k: b[k].copy() for k in ('x', 'r', 'gamma', 'beta')}
    p, c = pos
    if nan:
        d['x'][p, c] = np.nan
    elif res:
        d['r'][p, c] = RES_PLANT
    else:
        d['x'][p, c] = X_PLANT
        d['gamma'][c] = GAMMA_PLANT
        d['beta'][c] = GAMMA_PLANT / np.sqrt(max(P - 1, 1))
    return d


def forward_reference(d, v, seed, stats=None):
    """fp64 y [P][C] of BatchNorm (batch statistics, or the given (mean, invstd)) + residual, ReLU, Dropout(p, seed); -> y, mean, invstd, and the range
    of every channel as the kernel computes it: max |y| in front of the Dropout, times 1 / (1 - p) (per_channel_error)"""
    x, g, b = _nchw(d['x'].astype(np.float64)), d['gamma'].astype(np.float64), d['beta'].astype(np.float64)
    if stats is None:
        y, (mean, invstd), _ = O.batchnorm_train(x, g, b, eps=EPS)
        y = _flat(y)
    else:
        mean, invstd = stats[0].astype(np.float64), stats[1].astype(np.float64)
        y = (d['x'].astype(np.float64) - mean) * (invstd * g) + b
    if v.res:
        y = y + d['r']
    if v.relu:
        y = O.relu(y)
    rng = np.abs(y).max(0)
    if v.drop > 0.0:
        P, C = d['x'].shape
        y = y * keep_mask(P, C, seed, v.drop) / (1.0 - v.drop)
        rng = rng / (1.0 - v.drop)
    return y, mean, invstd, rng


def backward_inputs(P, C, pos):
    """x, r, gamma, beta, dy of a backward case whose dx has its unique maximum at `pos`: dy[pos] = 64 and gamma = 64 in that channel (every other element of the channel carries 64 x its own N(0,1) gradient); x[pos] = 2 puts the
    forward output of the element at ~128, so a ReLU lets its gradient through"""
    b = _base(P, C)
    d = {k: b[k].copy() for k in ('x', 'r', 'gamma', 'beta', 'dy')}
    p, c = pos
    d['x'][p, c] = 2.0
    d['gamma'][c] = GAMMA_PLANT
    d['dy'][p, c] = DY_PLANT
    return d


def backward_forward_variant(v):
    """the forward pass whose output the backward case masks with: a residual where dresidual is asked for"""
    return FwdVariant(bool(v.dres), 1 if v.relu else 0, v.drop)


def masked_gradient(d, v, y):
    """g [P][C] fp64, the gradient behind ReLU / Dropout as the kernels define it from the stored output y: dy / (1 - p) where y > 0 (ReLU, with or without
    Dropout), where y != 0 (Dropout alone), dy itself without either"""
    ks = 1.0 / (1.0 - v.drop) if v.drop > 0.0 else 1.0
    dy = d['dy'].astype(np.float64)
    if v.relu:
        return dy * ks * (y > 0)
    if v.drop > 0.0:
        return dy * ks * (y != 0)
    return dy


def backward_reference(d, v, g):
    """fp64 dx [P][C] of the BatchNorm for the masked gradient g: batch statistics (training) or frozen ones"""
    x, gm = _nchw(d['x'].astype(np.float64)), d['gamma'].astype(np.float64)
    _, (mean, invstd), _ = O.batchnorm_train(x, gm, d['beta'].astype(np.float64), eps=EPS)
    fn = O.batchnorm_train_bwd if v.training else O.batchnorm_eval_bwd
    return _flat(fn(x, gm, mean, invstd, _nchw(g))[0])


def bwd_partials(g, xhat, parts):
    """[2][parts][C] float32: sum g and sum g * xhat over `parts` row blocks, the sums a data-gradient epilogue hands to dsrl_bn_bwd_from_stats_*"""
    P, C = g.shape
    out = np.zeros((2, parts, C), np.float32)
    for i, idx in enumerate(np.array_split(np.arange(P), parts)):
        out[0, i], out[1, i] = g[idx].sum(0), (g[idx] * xhat[idx]).sum(0)
    return out


def xhat_of(d):
    x = d['x'].astype(np.float64)
    return (x - x.mean(0)) / np.sqrt(x.var(0) + EPS)


def premise(ref, pos, kept):
    """(holds, text): with the planted element kept, |ref| has its unique maximum at `pos`, at least 4x above the runner-up; with it dropped, the maximum
    is somewhere else and the planted element holds less than a quarter of it"""
    a = np.abs(ref)
    top = np.unravel_index(int(np.argmax(a)), a.shape)
    planted = a[pos]
    rest = a.copy()
    rest[pos] = 0.0
    runner = rest.max()
    if kept:
        return (tuple(top) == tuple(pos) and planted >= MARGIN * runner), f'argmax {top} want {pos}, planted {planted:.4g} runner-up {runner:.4g}'
    return (tuple(top) != tuple(pos) and MARGIN * planted <= runner), f'argmax {top} must not be {pos}, planted {planted:.4g} runner-up {runner:.4g}'


def per_channel_error(a, b, rng=None):
    """largest over the channels of max |a - b| / (range of that channel) (a planted channel's range dwarfs the others, so the tensor-wide figure would
    check that channel alone).  The range is max |b| of the channel, or `rng` [C] where given: behind a Dropout the range of the channel in front of it
    (forward_reference).  The Dropout multiplies by 0 or 1 / (1 - p) exactly, so a kept element carries the error of the value in front of it, whose
    size is set by the channel as computed - with the planted element dropped, max |b| of what is left of its channel can be the residue of two
    cancelling terms (at P = 2: 64 * (-1 + delta) + 64), against which no fp32 evaluation holds 1e-5."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), 'NaN pattern differs'
    rng = np.abs(b).max(0) if rng is None else np.asarray(rng, np.float64)
    assert rng.shape == (b.shape[1],) and (rng >= np.abs(b).max(0)).all()
    return float((np.abs(a - b).max(0) / np.maximum(rng, 1e-30)).max())


# ------------------------------------------------------------------------------------------------ concatenation
CAT_CASES = [((256, 48), False), ((64, 32), True), ((4, 4, 4), False)]       # widths, sources strided (a channel slice of a buffer twice as wide)
CAT_ROWS = 70


def cat_plants(widths, P=CAT_ROWS):
    """(source, row, channel within the source): the first source's first element, the last source's last channel of the last pixel, the last float4 of
    a middle source (the one at index n // 2)"""
    n = len(widths)
    return [(0, 0, 0), (n - 1, P - 1, widths[-1] - 1), (n // 2, P // 2, widths[n // 2] - 3)]


def cat_inputs(widths, plant, P=CAT_ROWS):
    rs = np.random.RandomState(sum(widths))
    xs = [rs.standard_normal((P, c)).astype(np.float32) * (i + 1) for i, c in enumerate(widths)]
    s, p, c = plant
    xs[s][p, c] = -RES_PLANT
    return xs

"""Guarded buffers and the case lists of tests/test_conv_guard_gpu.py: every conv entry point run with each pointer it writes at EXACTLY the size its
query reported, between two guards (docs/next_round_notes.md §2: "whatever a size query reports must hold for every launch of that shape in that mode").

Importable without a GPU (numpy, torch tensors on any device, the fp64 oracle): tests/test_conv_guard_host.py proves on the CPU that the guards detect
a planted byte and that the case lists have the edges they claim (M tail, N tail, channel-chunk tail for every forced tile)."""
import collections
import functools

import numpy as np
import torch

import oracle as O

# TileCfg of csrc/conv_igemm.hip in DSRL_FORCE_CFG order: (rows, columns) of a block tile; 7 and 8 are the 8-wave tiles of the fp16 arithmetics
TILES = ((128, 128), (256, 64), (256, 32), (64, 64), (128, 64), (64, 128), (128, 32), (256, 128), (256, 256))
MODES = ('f16x3', 'f16x1', 'bf16x6', 'fp32')
F16 = ('f16x3', 'f16x1')
# range-relative bounds per arithmetic: 3e-6 for the fp32-equivalent modes (test_conv_precision_modes); f16x1 carries one 11-bit term per operand,
# 2^-11 = 4.9e-4 per factor of a product, 1e-3 in the direct-ABI tests of test_hip_parity.py (cooperative split-K, one-plane operands)
TOL = {'f16x3': 3e-6, 'bf16x6': 3e-6, 'fp32': 3e-6, 'f16x1': 1e-3}
STATS_MEAN_TOL, STATS_VAR_TOL, DGRAD_SUMS_TOL, COLSUM_TOL = 1e-5, 1e-4, 2e-5, 1e-5       # as in test_cooperative_splitk_matches_slabs_and_oracle / column sums
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3                                        # include/dsrl_hip.h
KNOBS = ('DSRL_FORCE_CFG', 'DSRL_FORCE_KG', 'DSRL_FORCE_SPLITS', 'DSRL_SK_COOP', 'DSRL_FORCE_PSPLITS')
DROP_P = 0.25

ALIGN, MIN_GUARD = 256, 64 * 1024
SENTINEL = np.float32(-7777.25)           # gap columns of a strided output
AMAX_WORDS, SHARD_STRIDE = 256, 16        # csrc/common.h: an amax record; every 16th word a shard of max |x|, the others split-K tickets


# ------------------------------------------------------------------------------------------------ guarded buffers
def guard_bytes(nbytes):
    """bytes of each guard: at least the payload (an extra slab, or twice the rows of partials, lands inside it) and at least 64 KiB"""
    return (max(int(nbytes), MIN_GUARD) + ALIGN - 1) // ALIGN * ALIGN


@functools.lru_cache(maxsize=None)
def _pattern_host(n):
    return torch.from_numpy(((np.arange(n, dtype=np.int64) * 131 + 89) % 251).astype(np.uint8))


_pattern_dev = {}


def pattern(n, device):
    """the fixed byte pattern of a guard of n bytes"""
    device = torch.device(device)
    if device.type == 'cpu':
        return _pattern_host(n)
    key = (n, str(device))
    if key not in _pattern_dev:
        if len(_pattern_dev) > 64:
            _pattern_dev.clear()
        _pattern_dev[key] = _pattern_host(n).to(device)
    return _pattern_dev[key]


class Guarded:
    """uint8 buffer [front guard | payload | back guard]: the payload is exactly `nbytes` long and starts 256-byte aligned, the guards hold pattern()."""

    def __init__(self, nbytes, device='cpu', name=''):
        self.nbytes, self.name = int(nbytes), name
        g = guard_bytes(self.nbytes)
        self.raw = torch.empty(2 * g + ALIGN + self.nbytes, dtype=torch.uint8, device=device)
        self.off = g + (-(self.raw.data_ptr() + g)) % ALIGN
        self.front, self.payload, self.back = self.raw[:self.off], self.raw[self.off:self.off + self.nbytes], self.raw[self.off + self.nbytes:]
        assert self.front.numel() >= g and self.back.numel() >= g and self.ptr % ALIGN == 0
        self.front.copy_(pattern(self.front.numel(), device))
        self.back.copy_(pattern(self.back.numel(), device))
        self.saved = None

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.off

    def put(self, a):
        """payload <- the bytes of a numpy array or a tensor of exactly nbytes"""
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.contiguous()
        t = t.reshape(-1).view(torch.uint8)
        assert t.numel() == self.nbytes, (self.name, t.numel(), self.nbytes)
        self.payload.copy_(t)
        return self

    def fill_nan(self):
        self.payload.view(torch.float32).fill_(float('nan'))
        return self

    def keep(self):
        """remembers the payload: assert_unchanged() compares against it"""
        self.saved = self.payload.clone()
        return self

    def f32(self):
        return self.payload.view(torch.float32).cpu().numpy()

    def u32(self):
        return self.payload.view(torch.int32).cpu().numpy().view(np.uint32)

    def damage(self):
        """None if both guards hold their pattern, else where the first changed byte of each damaged guard sits relative to the payload"""
        out = []
        for side, g in (('front', self.front), ('back', self.back)):
            want = pattern(g.numel(), g.device)
            if not torch.equal(g, want):
                bad = torch.nonzero(g != want).reshape(-1)
                first, last, n = int(bad[0]), int(bad[-1]), int(bad.numel())
                where = (f'{g.numel() - first} bytes in front of the payload' if side == 'front' else f'{first} bytes behind the payload')
                out.append(f'{side} guard of {self.name or "buffer"} ({self.nbytes} payload bytes): {n} bytes changed, the first {where}, spanning {last - first + 1}')
        return '; '.join(out) or None

    def assert_guards(self):
        d = self.damage()
        assert d is None, d

    def assert_unchanged(self):
        assert self.saved is not None, f'{self.name}: keep() was not called'
        assert torch.equal(self.payload, self.saved), f'{self.name}: the call changed the payload'


def of_bytes(a, device, name=''):
    """a guarded copy of an operand (numpy array or tensor), remembered for assert_unchanged()"""
    n = a.nbytes if isinstance(a, np.ndarray) else a.numel() * a.element_size()
    return Guarded(n, device, name).put(a).keep()


def span_floats(rows, ld, C):
    """floats of a [rows][ld] tensor with C channels in use: rows * ld minus the unused tail of the last row"""
    return (rows - 1) * ld + C


class Rows(Guarded):
    """A pixel-major float tensor [rows][ld] with C channels in use, behind guards, exactly span_floats() long.  data: its values ([rows][C], an
    operand: kept for assert_unchanged); None: an output, NaN in the C channels.  Gap columns (ld > C) hold SENTINEL either way."""

    def __init__(self, rows, ld, C, device='cpu', data=None, name=''):
        assert ld >= C
        super().__init__(4 * span_floats(rows, ld, C), device, name)
        self.rows, self.ld, self.C = rows, ld, C
        flat = np.full(span_floats(rows, ld, C), SENTINEL, np.float32)
        self.used = (np.arange(rows)[:, None] * ld + np.arange(C)[None, :]).reshape(-1)
        flat[self.used] = np.nan if data is None else np.asarray(data, np.float32).reshape(-1)
        self.gap = np.ones(flat.size, bool)
        self.gap[self.used] = False
        self.put(flat)
        if data is not None:
            self.keep()

    def matrix(self):
        return self.f32()[self.used].reshape(self.rows, self.C)

    def gaps_intact(self):
        return bool((self.f32()[self.gap].view(np.uint32) == SENTINEL.view(np.uint32)).all())

    def assert_gaps(self):
        assert self.gaps_intact(), f'{self.name}: a gap column behind the {self.C} channels (ld {self.ld}) was written'


def record_max(rec):
    """what a reader takes from an amax record: the largest of its shard words"""
    return np.uint32(np.asarray(rec, np.uint32)[0::SHARD_STRIDE].max())


def tickets_zero(rec):
    spare = np.ones(AMAX_WORDS, bool)
    spare[0::SHARD_STRIDE] = False
    return bool((np.asarray(rec, np.uint32)[spare] == 0).all())


def abs_bits_max(a):
    return np.uint32((np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)).max())


# ------------------------------------------------------------------------------------------------ shapes
# (N, C, H, W, K, R, stride, pad, dil): the smallest that still have an M tail, an N tail and a channel-chunk tail against every tile they are forced on
SHAPES = {
    's1': (1, 40, 9, 31, 136, 3, 1, 1, 1),            # 3x3 stride 1: M = 279 (two tiles of 256 rows), K = 136, C = 1.25 chunks
    'bn': (2, 72, 9, 20, 160, 3, 1, 1, 1),            # forward BatchNorm partials: K % 32 == 0, M = 360, C = 2.25 chunks
    'dbn': (2, 160, 9, 20, 72, 3, 1, 1, 1),           # dgrad BatchNorm-backward partials: C % 32 == 0, the reduction runs over K = 72 = 2.25 chunks
    's2': (2, 40, 17, 33, 136, 3, 2, 1, 1),           # 3x3 stride 2 on an odd map: 9 x 17 outputs, M = 306 forward and 1122 dgrad
    'p2': (2, 40, 17, 33, 136, 1, 2, 0, 1),           # 1x1 stride 2
    'dil': (10, 40, 5, 6, 136, 3, 1, 6, 6),           # dilation 6 on a 5x6 map: only the centre tap is live, dw of the other eight is zero
    'k19': (1, 40, 9, 31, 19, 1, 1, 0, 1),            # 19 classes: dgrad pads dy to 20 channels
    'w3': (2, 40, 9, 32, 136, 3, 1, 1, 1),            # W % 32 == 0: the all-taps 3x3 weight gradient of the fp16 arithmetics (conv_wgrad3.hip)
    'wide': (1, 40, 5, 7, 264, 3, 1, 1, 1),           # weight-gradient rows = K = 264: two tiles of 256
    'g128': (1, 136, 5, 7, 136, 1, 1, 0, 1),          # K, C >= 128: the weight gradient's 128x128 class
    'c24': (1, 24, 5, 7, 72, 1, 1, 0, 1),             # C <= 32: its 128x32 class
    'splitk': (8, 1024, 16, 32, 256, 3, 1, 1, 1),     # the planner's own split-K in the fp16 arithmetics (256x128 tiles, 8 slabs); unforced forward only
    'fp32sk': (3, 200, 9, 20, 136, 3, 1, 1, 1),       # 63 chunk steps: the fp32 planner splits K by itself (the others take K groups)
}
STEM = (2, 3, 33, 45, 72, 7, 2, 3)                    # N, C, H, W, K, R, stride, pad: the 7x7 stride-2 stem on an odd map, row-folded to 32 channels
GROUP = ('w3', 'k19', 'g128', 'c24', 'dil', 's2', 'wide')     # one grouped weight-gradient launch set: five tile classes, dead taps, an all-taps 3x3
COLSUMS = ((279, 136, 136), (279, 19, 20), (2000, 192, 200), (5000, 6, 8))     # (P, K, ld): float4 and scalar kernels, several row blocks


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def pad4(v):
    return (v + 3) & ~3


def dims(shape):
    N, C, H, W, K, R, stride, pad, dil = shape
    return out_size(H, R, stride, pad, dil), out_size(W, R, stride, pad, dil)


def gemm(op, shape):
    """(rows, columns, reduction channels per tap) of the implicit GEMM a pass runs: what a tile (bm, bn) and the 32-channel chunks cut"""
    N, C, H, W, K, R, stride, pad, dil = shape
    Ho, Wo = dims(shape)
    if op == 'fwd':
        return N * Ho * Wo, K, C
    if op == 'dgrad':
        return N * H * W, C, pad4(K)
    return K, C, None               # wgrad: rows = output channels, columns = input channels, the reduction runs over pixels


def stem_geometry():
    """(shp of the row-folded calls, Sp, Cf, Hp, Wp, Ho, Wo) as functional._StemConv lays the stem out"""
    N, C, H, W, K, R, stride, pad = STEM
    Sp = (R + 7) & ~7
    Ho, Wo = out_size(H, R, stride, pad, 1), out_size(W, R, stride, pad, 1)
    Hp, Wp = max(H + 2 * pad, (Ho - 1) * stride + R), max(W + 2 * pad, (Wo - 1) * stride + Sp) + 1
    return (N, Hp, Wp, Sp * 4, K, R, stride, Ho, Wo), Sp, Sp * 4, Hp, Wp, Ho, Wo


def tail_ok(op, shape, cfg):
    """the forced tile leaves an M tail and an N tail on this shape, and there are at least two tiles along M"""
    bm, bn = TILES[cfg]
    if op in ('rowfold_fwd', 'rowfold_wgrad'):
        shp, Sp, Cf = stem_geometry()[:3]
        M, Nc = (shp[0] * shp[7] * shp[8], shp[4]) if op == 'rowfold_fwd' else (shp[4], Cf)
    else:
        M, Nc, _ = gemm('wgrad' if op in ('wgrad', 'group') else op, shape)
    return M % bm != 0 and Nc % bn != 0 and -(-M // bm) >= 2


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple('Case', 'op mode shape cfg kg splits coop psplits operands bias stats acc gap drop refused')
# op: fwd, dgrad, wgrad, group, rowfold_fwd, rowfold_wgrad.  shape: a key of SHAPES ('stem' / 'group' for the row-folded and grouped calls).
# operands (fp16 arithmetics): 'planes' = amax records, pre-split filter and fp16 planes handed in; 'amax' = records and pre-split filter; 'null' = nothing, the
# library measures into the scratch at the end of the workspace (the other arithmetics take no records: always 'null').
# refused: None, or (status code, fragment of the message) of a combination the library refuses by design.


def case_id(c):
    s = f'{c.op}-{c.mode}-{c.shape}'
    for k, v in (('cfg', c.cfg), ('kg', c.kg), ('sp', c.splits), ('coop', c.coop), ('ps', c.psplits)):
        if v is not None:
            s += f'-{k}{v}'
    s += f'-{c.operands}'
    for k, v in (('bias', c.bias), ('stats', c.stats), ('acc', c.acc), ('gap', c.gap), ('drop', c.drop), ('refused', c.refused)):
        if v:
            s += f'-{k}'
    return s


def knobs(c):
    """the environment of a case: every plan knob either set or removed"""
    v = dict(DSRL_FORCE_CFG=c.cfg, DSRL_FORCE_KG=c.kg, DSRL_FORCE_SPLITS=c.splits, DSRL_SK_COOP=c.coop, DSRL_FORCE_PSPLITS=c.psplits)
    return {k: (None if v[k] is None else str(v[k])) for k in KNOBS}


def cfgs_of(mode, op):
    """tile configurations a pass has: 0..6 everywhere; 7, 8 in forward / dgrad of the fp16 arithmetics"""
    return tuple(range(9 if (mode in F16 and op in ('fwd', 'dgrad', 'rowfold_fwd')) else 7))


def planes_ok(op, shape):
    """would the launch take fp16 planes of this shape's operands? (both channel counts multiples of 8; data gradients of stride 1 only)"""
    N, C, H, W, K, R, stride, pad, dil = SHAPES[shape]
    return C % 8 == 0 and K % 8 == 0 and (op == 'fwd' or stride == 1)


def _variants(mode, op, shape):
    if mode not in F16:
        return ('null',)
    return (('planes',) if planes_ok(op, shape) else ()) + ('amax', 'null')


class _Builder:
    def __init__(self):
        self.out, self.i = [], 0

    def add(self, op, mode, shape, cfg=None, kg=None, splits=None, coop=None, psplits=None, operands='null', stats=False, refused=None, drop=0.0):
        """bias (forward), accumulate (dgrad) and a strided output alternate from case to case"""
        self.i += 1
        bias = op in ('fwd', 'rowfold_fwd') and self.i % 2 == 0
        acc = op == 'dgrad' and self.i % 2 == 1
        gap = op in ('fwd', 'dgrad', 'rowfold_fwd') and self.i % 3 == 0
        self.out.append(Case(op, mode, shape, cfg, kg, splits, coop, psplits, operands, bias, stats, acc, gap, drop, refused))


def _dgrad_stats_possible(mode, cfg, kg, splits, coop):
    """BatchNorm-backward sums of a stride-1 dgrad: every 16-bit arithmetic unless split-K reduces through slabs (only the cooperative launch of the fp16
    arithmetics - 128x128 tiles, DSRL_SK_COOP on - keeps them under split-K)"""
    if mode == 'fp32':
        return False
    if splits is None or splits == 1:
        return True
    return mode in F16 and cfg == 0 and coop == 1


def _conv_cases(op):
    """forward or data gradient.  Rules: the planner's own choice on every kind of shape with every operand variant; every tile on the plain 3x3 shape with
    every operand variant, on the strided 3x3 shape and (tiles at least 64 columns wide) on the shape with BatchNorm partials; K groups 1 and 2 with the
    tiles that have them; split-K 1, 2, 3 x cooperative on / off on 128x128 tiles and on the planner's tile, plain, strided and with partials."""
    b = _Builder()
    bnshape = 'bn' if op == 'fwd' else 'dbn'
    for mode in MODES:
        f16 = mode in F16
        fwd_stats = mode != 'fp32'          # forward partials: the epilogue of every 16-bit kernel, and the slab reduce under split-K
        stats = (lambda cfg=None, kg=None, sp=None, coop=None: fwd_stats) if op == 'fwd' else (lambda cfg=None, kg=None, sp=None, coop=None: _dgrad_stats_possible(mode, cfg, kg, sp, coop))
        j = 0
        for name in ('s1', 's2', 'p2', 'dil', 'k19', bnshape):
            for v in _variants(mode, op, name):
                j += 1
                b.add(op, mode, name, operands=v, stats=name == bnshape and stats(), drop=DROP_P if (op == 'dgrad' and j % 2) else 0.0)
        if op == 'fwd':
            b.add(op, mode, 'fp32sk' if mode == 'fp32' else 'splitk', operands='amax' if f16 else 'null')       # the planner's own split-K
        else:
            b.add(op, mode, 'fp32sk', operands='amax' if f16 else 'null')
        for cfg in cfgs_of(mode, op):
            for v in _variants(mode, op, 's1'):
                if op == 'dgrad' and cfg == 8 and v != 'planes':
                    if v == 'amax':     # no register-staged 256x256 data-gradient build: refused by design, once per arithmetic
                        b.add(op, mode, 's1', cfg=cfg, operands=v, refused=(E_UNSUPPORTED, 'no 256x256 data-gradient build'))
                    continue
                b.add(op, mode, 's1', cfg=cfg, operands=v)
            if not (op == 'dgrad' and cfg == 8):
                b.add(op, mode, 's2', cfg=cfg, operands='amax' if f16 else 'null')
            if TILES[cfg][1] >= 64:
                v = _variants(mode, op, bnshape)[cfg % len(_variants(mode, op, bnshape))]
                if op == 'dgrad' and cfg == 8:
                    v = 'planes'
                b.add(op, mode, bnshape, cfg=cfg, operands=v, stats=stats(cfg), drop=DROP_P if (op == 'dgrad' and cfg % 2) else 0.0)
        if mode != 'fp32':                  # the fp32 kernel has no K groups
            for kg in (1, 2):
                for cfg in ((None, 3, 4, 5, 0) if f16 else (None, 3, 4, 5)):
                    vs = _variants(mode, op, 's1')
                    b.add(op, mode, 's1', cfg=cfg, kg=kg, operands=vs[(kg + (cfg or 0)) % len(vs)])
                    vs = _variants(mode, op, bnshape)
                    b.add(op, mode, bnshape, cfg=cfg, kg=kg, operands=vs[(kg + (cfg or 0) + 1) % len(vs)], stats=stats(cfg, kg), drop=DROP_P if (op == 'dgrad' and kg == 2) else 0.0)
                b.add(op, mode, 's2', kg=kg, operands='amax' if f16 else 'null')
        for cfg in (0, None):
            for kg in ((None, 2) if (f16 and cfg == 0) else (None,)):
                for sp in (1, 2, 3):
                    for coop in ((1, 0) if f16 else (1,)):          # the switch only exists for the fp16 arithmetics' cooperative launch
                        vs = _variants(mode, op, 's1')
                        b.add(op, mode, 's1', cfg=cfg, kg=kg, splits=sp, coop=coop, operands=vs[(sp + coop) % len(vs)])
                        b.add(op, mode, 's2', cfg=cfg, kg=kg, splits=sp, coop=coop, operands='amax' if f16 else 'null')
                        vs = _variants(mode, op, bnshape)
                        b.add(op, mode, bnshape, cfg=cfg, kg=kg, splits=sp, coop=coop, operands=vs[(sp + coop + 1) % len(vs)], stats=stats(cfg, kg, sp, coop),
                              drop=DROP_P if (op == 'dgrad' and sp != 2) else 0.0)
    return b.out


def _wgrad_cases():
    """dsrl_conv2d_wgrad_amax: the planner's own choice on every kind of shape with records given and withheld; every tile on the 264-row shape, the tiles of
    at most 128 rows on the plain 3x3 shape as well; pixel splits 1 and 3 plain, with dead taps, all-taps 3x3 and on the wide shape."""
    b = _Builder()
    for mode in MODES:
        vs = ('amax', 'null') if mode in F16 else ('null',)
        for name in ('s1', 's2', 'p2', 'dil', 'k19', 'w3', 'wide'):
            for v in vs:
                b.add('wgrad', mode, name, operands=v)
        for cfg in cfgs_of(mode, 'wgrad'):
            b.add('wgrad', mode, 'wide', cfg=cfg, operands=vs[cfg % len(vs)])
            if TILES[cfg][0] <= 128:
                b.add('wgrad', mode, 's1', cfg=cfg, operands=vs[(cfg + 1) % len(vs)])
        for ps in (1, 3):
            for name in ('s1', 'dil', 'w3', 'wide', 's2'):
                b.add('wgrad', mode, name, psplits=ps, operands=vs[ps % len(vs)])
            b.add('wgrad', mode, 'wide', cfg=1, psplits=ps, operands=vs[0])
    return b.out


def _group_cases():
    """dsrl_conv2d_wgrad_group_*: GROUP in one launch set, the planner's tiles, every forced tile, pixel splits 1 and 3; fp32 has no grouped launch"""
    b = _Builder()
    for mode in MODES:
        if mode == 'fp32':
            b.add('group', mode, 'group', refused=(E_UNSUPPORTED, 'the grouped launch exists for the 16-bit MFMA arithmetics only'))
            continue
        b.add('group', mode, 'group', operands='amax')
        for cfg in cfgs_of(mode, 'group'):
            b.add('group', mode, 'group', cfg=cfg, operands='amax')
        for ps in (1, 3):
            b.add('group', mode, 'group', psplits=ps, operands='amax')
    return b.out


def _rowfold_cases():
    """the stem: forward under the planner's choice, every tile, K groups, split-K 1, 2, 3 (x cooperative switch); its weight gradient under the planner's
    choice, 64x64 tiles (the only tile with two row tiles and a column tail on K = 72 x 32 folded channels) and pixel splits 1 and 3"""
    b = _Builder()
    for mode in MODES:
        f16 = mode in F16
        b.add('rowfold_fwd', mode, 'stem')
        for cfg in cfgs_of(mode, 'rowfold_fwd'):
            b.add('rowfold_fwd', mode, 'stem', cfg=cfg)
        if mode != 'fp32':
            for kg in (1, 2):
                for cfg in ((None, 0) if f16 else (None,)):
                    b.add('rowfold_fwd', mode, 'stem', cfg=cfg, kg=kg)
        for sp in (1, 2, 3):
            for coop in ((1, 0) if f16 else (1,)):
                b.add('rowfold_fwd', mode, 'stem', cfg=0, splits=sp, coop=coop)
            b.add('rowfold_fwd', mode, 'stem', splits=sp)
        b.add('rowfold_wgrad', mode, 'stem')
        b.add('rowfold_wgrad', mode, 'stem', cfg=3)
        for ps in (1, 3):
            b.add('rowfold_wgrad', mode, 'stem', psplits=ps)
    return b.out


FWD_CASES, DGRAD_CASES = _conv_cases('fwd'), _conv_cases('dgrad')
WGRAD_CASES, GROUP_CASES, ROWFOLD_CASES = _wgrad_cases(), _group_cases(), _rowfold_cases()
ALL_CASES = FWD_CASES + DGRAD_CASES + WGRAD_CASES + GROUP_CASES + ROWFOLD_CASES


def plan_kind(c):
    if c.splits is not None:
        return f'splits{c.splits}/coop{c.coop}' if c.coop is not None else f'splits{c.splits}'
    if c.psplits is not None:
        return f'psplits{c.psplits}'
    if c.kg is not None:
        return f'kg{c.kg}'
    if c.cfg is not None:
        return f'cfg{c.cfg}'
    return 'planner'


def entry_points(c):
    """the entry points a case calls"""
    if c.op == 'fwd':
        return ('dsrl_conv2d_fwd_planes',)
    if c.op == 'dgrad':
        return ('dsrl_conv2d_dgrad_planes_drop',) if (c.stats and c.drop > 0) else ('dsrl_conv2d_dgrad_planes',)
    if c.op == 'wgrad':
        return ('dsrl_conv2d_wgrad_amax',)
    if c.op == 'group':
        return ('dsrl_conv2d_wgrad_group_plan+launch',)
    return ('dsrl_conv2d_' + c.op,)


def coverage():
    """{(entry point, mode): {plan kind: cases}} of ALL_CASES (refused combinations not counted)"""
    out = collections.OrderedDict()
    for c in ALL_CASES:
        if c.refused:
            continue
        for e in entry_points(c):
            cell = out.setdefault((e, c.mode), collections.Counter())
            kind = plan_kind(c).split('/')[0]
            kind = 'cfg' if kind.startswith('cfg') else kind
            cell[kind] += 1
    return out


# ------------------------------------------------------------------------------------------------ inputs and fp64 references (computed once, never modified)
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(name):
    """x >= 0 [N,C,H,W], w [K,C,R,R], bias [K], dy [N,K,Ho,Wo], previous dx content [N,C,H,W]: float32, drawn once per shape"""
    N, C, H, W, K, R, stride, pad, dil = shape = SHAPES[name]
    Ho, Wo = dims(shape)
    rs = np.random.RandomState(sum(shape) + 7)
    x = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    bias = rs.standard_normal(K).astype(np.float32)
    dy = rs.standard_normal((N, K, Ho, Wo)).astype(np.float32)
    dx0 = rs.standard_normal((N, C, H, W)).astype(np.float32)
    return _frozen(x, w, bias, dy, dx0)


@functools.lru_cache(maxsize=None)
def bn_inputs(name):
    """the BatchNorm in front of the conv, for the dgrad epilogue's sums: its input [P][C], mean and invstd [C]"""
    N, C, H, W = SHAPES[name][:4]
    rs = np.random.RandomState(C + H)
    return _frozen(rs.standard_normal((N * H * W, C)).astype(np.float32), (rs.standard_normal(C) * 0.1).astype(np.float32), (1.0 + rs.rand(C)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def ref_fwd(name):
    x, w = inputs(name)[:2]
    stride, pad, dil = SHAPES[name][6:]
    return _frozen(O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, dil))[0]


@functools.lru_cache(maxsize=None)
def ref_bwd(name):
    """(dx, dw) in fp64"""
    x, w, _, dy, _ = inputs(name)
    stride, pad, dil = SHAPES[name][6:]
    dx, dw, _ = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, dil, False)
    return _frozen(dx, dw)


@functools.lru_cache(maxsize=None)
def stem_inputs():
    N, C, H, W, K, R, stride, pad = STEM
    Ho, Wo = out_size(H, R, stride, pad, 1), out_size(W, R, stride, pad, 1)
    rs = np.random.RandomState(77)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((K, C, R, R)) / np.sqrt(C * R * R)).astype(np.float32)
    bias = rs.standard_normal(K).astype(np.float32)
    dy = rs.standard_normal((N, K, Ho, Wo)).astype(np.float32)
    return _frozen(x, w, bias, dy)


@functools.lru_cache(maxsize=None)
def stem_refs():
    """(y, dw) in fp64"""
    x, w, _, dy = stem_inputs()
    stride, pad = STEM[6:]
    y = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, 1)
    dw = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, 1, False)[1]
    return _frozen(y, dw)


def pixel_major(a):
    """[N,C,H,W] -> [N*H*W][C]"""
    N, C, H, W = a.shape
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(N * H * W, C)


def krsc(w):
    """[K,C,R,S] -> [K][R][S][C], the filter layout of the kernels"""
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1))


def live_taps(shape):
    """[R][R] bool: taps that see at least one pixel of the map (the others have a zero weight gradient)"""
    N, C, H, W, K, R, stride, pad, dil = shape
    Ho, Wo = dims(shape)

    def live(n, no, off):
        return any(0 <= o * stride - pad + off < n for o in range(no))
    return np.array([[live(H, Ho, r * dil) and live(W, Wo, s * dil) for s in range(R)] for r in range(R)])


def range_error(a, b):
    """max |a - b| / max |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30)) if b.size else 0.0


def tail_tiles(c):
    """tiles whose last row / column blocks get a check of their own: the forced one, or (the planner chose) every tile size"""
    return (TILES[c.cfg],) if c.cfg is not None else tuple(sorted(set(TILES)))


def check_matrix(got, want, tol, tiles, what):
    """got [M][..][N] against want: no NaN, the whole tensor within tol of its range, and the rows of the last M tile and the columns of the last N tile
    within tol of THEIR range (a tail error must not hide under the range of the body).  -> the three figures"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), f'{what}: {int(np.isnan(got).sum())} elements were never written (first at {tuple(np.argwhere(np.isnan(got))[0])})'
    e = [range_error(got, want), 0.0, 0.0]
    assert e[0] <= tol, f'{what}: {e[0]:.3e} of the range > {tol:.1e}'
    M, Nc = want.shape[0], want.shape[-1]          # a weight gradient comes as [K][taps][C]: rows first, columns last
    for bm, bn in tiles:
        r0, c0 = (M - 1) // bm * bm, (Nc - 1) // bn * bn
        er, ec = range_error(got[r0:], want[r0:]), range_error(got[..., c0:], want[..., c0:])
        assert er <= tol, f'{what}: rows {r0}.. (last tile of {bm} rows) {er:.3e} of their range > {tol:.1e}'
        assert ec <= tol, f'{what}: columns {c0}.. (last tile of {bn} columns) {ec:.3e} of their range > {tol:.1e}'
        e[1], e[2] = max(e[1], er), max(e[2], ec)
    return e

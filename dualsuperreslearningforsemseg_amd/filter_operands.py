"""Prepared operands of conv filters: the one place that knows which filters have them, how the tables of the batched filter kernels are laid out, and
whether what was written is still current.  Per filter: an amax record (max |w|, the filter-side operand scale of the f16 arithmetics), the pre-split
form and the fp16 planes in the forward layout [K][R][S][C], and - with `transposed` - the fp32 transpose [C][R][S][K padded to 4] the data-gradient
kernels read, and the split form and planes of that layout.  ddp.FlatParams refreshes a transposed set once per training step; inference.FrozenOperands
prepares a forward-only set once per conv arithmetic.  A filter points at its set through `w._dsrl_operands = (FilterOperands, index)`, which
functional.py reads.  The functions above the class are plain integer arithmetic (no device): tests/test_filter_operands_host.py pins them."""
from itertools import accumulate

import torch

from . import functional as HF

STALE, FP32, SPLIT, PLANES = range(4)       # FilterOperands.state: what of the operands is current, each level including the records


def align(n, a=4):
    return (n + a - 1) // a * a


def eligible(C, krsc):      # the batched filter kernels and the implicit-GEMM dgrad take [K][R][S][C] filters with C % 4 == 0: not the RGB stem, not the C -> 1 transformers
    return C % 4 == 0 and bool(krsc)


def plane_eligible(K, C):       # conv_planes_kernel takes filter planes when both channel counts are multiples of 8
    return K % 8 == 0 and C % 8 == 0


def padded_k(K):
    return (K + 3) & ~3


def wt_floats(K, RS, C):        # of one transposed filter [C][R][S][K padded to 4]
    return C * RS * padded_k(K)


def table_row(w, K, RS, C, first_tile, record, transposed_out=0, forward_out=0, pad_k=True):
    """One row of the int64 table dsrl_conv2d_transpose_filters_batched, _split_filters_batched and _filter_planes_batched read:
    {w, transposed-out, K, K-out, R*S, C, first tile, channel tiles, amax record, forward-out} (addresses; a null output is not written).  K-out is the
    K extent of the transposed output: padded to 4 for the fp32 and split forms, K itself for planes (pad_k=False).  -> (row, tiles of this filter)"""
    k_out = padded_k(K) if pad_k else K
    ct = (C + 31) // 32
    return [w, transposed_out, K, k_out, RS, C, first_tile, ct, record, forward_out], RS * ct * ((k_out + 31) // 32)


def table_rows(dims, w, records, transposed_out=None, forward_out=None, pad_k=True):
    """The table of the filters `dims` = [(K, R*S, C)] with their addresses, in launch order.  -> (rows, tiles of the launch)"""
    rows, tiles = [], 0
    for i, (K, RS, C) in enumerate(dims):
        row, n = table_row(w[i], K, RS, C, tiles, records[i], transposed_out[i] if transposed_out else 0, forward_out[i] if forward_out else 0, pad_k)
        rows.append(row)
        tiles += n
    return rows, tiles


def segment_rows(first, count, record, seg, scale=1):
    """{first + scale * a, floats, amax record} for a = 0, seg, 2 seg ..: `count` floats in segments of at most `seg` (the rows of
    dsrl_conv2d_filters_amax_batched with addresses, scale = 4, and of dsrl_sgd_step_dev_segments with arena indices)."""
    return [[first + scale * a, min(seg, count - a), record] for a in range(0, count, seg)]


def conv_filters(model):
    """The filters of `model` that have prepared operands: the weights of its eligible HipConv2d layers, in module order."""
    from .nn_modules import HipConv2d
    return [m.weight for m in model.modules() if isinstance(m, HipConv2d) and eligible(m.weight.shape[1], HF._is_krsc(m.weight))]


class FilterOperands:
    """The operands of `filters` (eligible (K,C,R,S) weights on `device`).  Its methods are launches on the current stream; the caller decides which
    to run and in which order (records first: the split forms and the planes are scaled by them).  Arenas and tables are only ever added, never
    replaced: a captured graph keeps reading the ones it was captured with for as long as this object lives."""

    def __init__(self, filters, device, transposed):
        W = HF.AMAX_WORDS
        self.filters, self.device, self.transposed = list(filters), device, bool(transposed)
        self.rows = len(self.filters)
        self.state = STALE
        self.dims = [(w.shape[0], w.shape[2] * w.shape[3], w.shape[1]) for w in self.filters]
        self.amax = torch.zeros(max(self.rows, 1) * W, device=device, dtype=torch.int32)          # one amax record per filter
        self.records = [self.amax[i * W:(i + 1) * W] for i in range(self.rows)]
        self._w = [w.data_ptr() for w in self.filters]
        self._rec = [self.amax.data_ptr() + 4 * W * i for i in range(self.rows)]
        self.record_ptr_of = {id(w): r for w, r in zip(self.filters, self._rec)}
        rows, self.tiles = table_rows(self.dims, self._w, self._rec)
        self._amax_only_table = self._table(rows) if self.rows else None          # null outputs: the transposing launch only measures
        self.wt, self.wsplit, self.wtsplit = ([None] * self.rows for _ in range(3))
        self.wt_flat = self.wsplit_flat = self.wtsplit_flat = None
        self._wt_table, self._split_table, self._amax_seg_table, self.amax_segs = None, None, None, 0
        self.plane_sets, self._planes = [], {}          # sets in launch order; filter index -> (planes, transposed planes or None)
        if self.transposed and self.rows:
            self.wt_flat, self.wt = self._arena([wt_floats(*d) for d in self.dims])
            self._wt_table = self._table(table_rows(self.dims, self._w, self._rec, transposed_out=[t.data_ptr() for t in self.wt])[0])

    def _arena(self, floats):
        """One fp32 arena with a 4-aligned view per filter"""
        offs = [0] + list(accumulate(align(n) for n in floats))
        flat = torch.empty(offs[-1], device=self.device, dtype=torch.float32)
        return flat, [flat[o:o + n] for o, n in zip(offs, floats)]

    def _table(self, rows):
        return torch.tensor(rows, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ the hook functional.py reads
    def attach(self):
        for i, w in enumerate(self.filters):
            w._dsrl_operands = (self, i)

    def detach(self):
        for w in self.filters:
            if getattr(w, '_dsrl_operands', (None,))[0] is self:
                del w._dsrl_operands

    # what a conv may read of filter i, or None: the record while the operands are current, the fp32 transpose if this step wrote it (the scaling
    # arithmetics write the split forms instead), the split forms with the record, the planes of the filters that are in a set
    def record(self, i):
        return self.records[i] if self.state != STALE else None

    def fp32_transpose(self, i):
        return self.wt[i] if self.state == FP32 else None

    def split(self, i, transposed=False):
        return (self.wtsplit if transposed else self.wsplit)[i] if self.state >= SPLIT else None

    def planes(self, i, transposed=False):
        p = self._planes.get(i) if self.state == PLANES else None
        return None if p is None else p[1 if transposed else 0]

    def invalidate(self):       # the filters changed: records, transposes, split forms and planes are stale until they are written again
        self.state = STALE

    def nbytes(self):
        held = [self.amax, self.wt_flat, self.wsplit_flat, self.wtsplit_flat] + [a for st in self.plane_sets for a in st['arenas']]
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    # ------------------------------------------------------------------ launches
    def measure(self, streaming):
        """max |w| of every filter into its record: by one streaming launch over segments of the filters' contiguous storage
        (dsrl_conv2d_filters_amax_batched), or by the transposing launch with null outputs.  This and transpose() MAX into `amax`: zero it first."""
        if streaming:
            if self._amax_seg_table is None:
                seg = int(HF.query('dsrl_conv2d_filters_amax_segment_floats'))
                rows = [r for w, p, rec in zip(self.filters, self._w, self._rec) for r in segment_rows(p, w.numel(), rec, seg, 4)]
                self._amax_seg_table, self.amax_segs = self._table(rows), len(rows)
            HF.call('dsrl_conv2d_filters_amax_batched', self._amax_seg_table.data_ptr(), self.amax_segs, HF._stream())
        else:
            HF.call('dsrl_conv2d_transpose_filters_batched', self._amax_only_table.data_ptr(), self.rows, self.tiles, HF._stream())

    def transpose(self):
        """Records and fp32 transposes by one launch (the arithmetics that do not scale their operands read these)."""
        HF.call('dsrl_conv2d_transpose_filters_batched', self._wt_table.data_ptr(), self.rows, self.tiles, HF._stream())
        self.state = FP32

    def write_split(self):
        """Every filter in pre-split form, forward layout and (transposed sets) transposed, scaled by its record; the arenas are allocated on first use."""
        if self._split_table is None:
            self.wsplit_flat, self.wsplit = self._arena([w.numel() for w in self.filters])
            if self.transposed:
                self.wtsplit_flat, self.wtsplit = self._arena([wt_floats(*d) for d in self.dims])
            self._split_table = self._table(table_rows(self.dims, self._w, self._rec, [t.data_ptr() for t in self.wtsplit] if self.transposed else None,
                                                       [t.data_ptr() for t in self.wsplit])[0])
        HF.call('dsrl_conv2d_split_filters_batched', self._split_table.data_ptr(), self.rows, self.tiles, HF._stream())
        self.state = SPLIT

    def add_plane_set(self, wanted=lambda w: True):
        """A new set of fp16 planes [K][R][S][C] (and [C][R][S][K]) for the plane-eligible filters the caller picks (`wanted(w)`) that no set holds yet,
        if there are any (host-side check) - never inside a graph capture.  Sets are only ever ADDED: a captured graph keeps launching the tables it was
        captured with and reading their arenas; filters that want planes later get a set of their own."""
        idx = [i for i, (K, _RS, C) in enumerate(self.dims) if plane_eligible(K, C) and i not in self._planes and wanted(self.filters[i])]
        if not idx:
            return
        nb = [2 * int(HF.cquery('dsrl_planes_lo_offset', self.filters[i].numel())) for i in idx]
        arenas = tuple(torch.empty(sum(nb), device=self.device, dtype=torch.uint8) if on else None for on in (True, self.transposed))
        outs = [tuple(None if a is None else a[o:o + n] for a in arenas) for o, n in zip([0] + list(accumulate(nb)), nb)]
        self._planes.update(zip(idx, outs))
        rows, tiles = table_rows([self.dims[i] for i in idx], [self._w[i] for i in idx], [self._rec[i] for i in idx],
                                 [o[1].data_ptr() for o in outs] if self.transposed else None, [o[0].data_ptr() for o in outs], pad_k=False)
        self.plane_sets.append({'table': self._table(rows), 'rows': len(rows), 'tiles': tiles, 'arenas': arenas, 'filters': list(idx)})

    def write_planes(self):
        """The planes of every set, scaled by the same records as the split forms (dsrl_conv2d_filter_planes_batched): one launch per set."""
        for st in self.plane_sets:
            HF.call('dsrl_conv2d_filter_planes_batched', st['table'].data_ptr(), st['rows'], st['tiles'], HF._stream())
        self.state = PLANES

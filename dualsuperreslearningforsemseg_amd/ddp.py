"""Data-parallel gradient reduction and the SGD update on flat fp32 arenas.

Replaces what the reference gets from `torch.nn.parallel.DistributedDataParallel(model)` + `torch.optim.SGD`
(command_handlers/train_or_resume.py:63-66, 105-106, 444-445) with a layout chosen for RCCL over xGMI:

  * all parameters live in ONE contiguous arena (and their gradients / momentum buffers in two more), ordered in reverse
    registration order, i.e. roughly the order in which backward produces gradients;
  * the gradient arena is all-reduced in a few large contiguous chunks (default 32 MiB) straight out of that memory - no
    bucket gather/scatter copies - and each chunk is launched asynchronously from an autograd hook as soon as every
    gradient in it has been accumulated, so RCCL overlaps with the rest of backward;
  * the mean (1/world) is folded into the fused SGD kernel (one launch over the whole arena);
  * BatchNorm running statistics sit in a fourth small arena that rank 0 broadcasts in one collective per step (DDP's
    broadcast_buffers=True default, which train_or_resume.py:106 relies on).

One process per GPU; `torch.distributed` backend 'nccl' is RCCL on ROCm.  With world size 1 (or no process group) the
collectives are skipped and only the arena + fused optimiser remain.
"""

import contextlib

import torch
import torch.distributed as dist

from . import functional as HF
from .filter_operands import FilterOperands, align as _align, conv_filters, segment_rows


def optimizer_state_kind(sd):
    """'sgd', 'adamw' or None (no per-parameter state to tell by) for an optimiser state_dict, from the keys of its per-parameter entries."""
    for st in (sd.get('state') or {}).values():
        if 'momentum_buffer' in st:
            return 'sgd'
        if 'exp_avg' in st or 'exp_avg_sq' in st:
            return 'adamw'
    return 'sgd' if 'momentum_arena' in sd else None


def adamw_param_group(lr, betas, eps, weight_decay, nparams):
    """The one param group of torch.optim.AdamW.state_dict() with the keys the installed torch writes (a one-scalar CPU optimiser is asked)."""
    probe = torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False)
    group = dict(probe.state_dict()['param_groups'][0])
    group['params'] = list(range(nparams))
    return group


class FlatParams:
    def __init__(self, model, chunk_bytes=32 << 20, process_group=None, broadcast_buffers=True):
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError('model has no trainable parameters')
        dev = params[0].device
        self.device = dev
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.params = list(reversed(params))                 # backward order first
        offs, off = [], 0
        for p in self.params:
            offs.append(off)
            off += _align(p.numel())
        self.offsets, self.numel = offs, off
        self.p_flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.g_flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.m_flat = torch.zeros(off, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                if p.dtype != torch.float32:
                    raise TypeError('fp32 parameters expected')
                if not (p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))):
                    p.data = p.data.contiguous()          # the arena views need dense storage
                view = self.p_flat.as_strided(p.shape, p.stride(), o)
                view.copy_(p.data)
                p.data = view
                p.grad = self.g_flat.as_strided(p.shape, p.stride(), o)
        # float buffers (BN running statistics) in their own arena
        self.buffers = []
        boff = 0
        for mod in model.modules():
            for name, b in list(mod._buffers.items()):
                if b is not None and b.dtype == torch.float32:
                    self.buffers.append((mod, name, boff, b))
                    boff += _align(b.numel())
        self.b_flat = torch.zeros(max(boff, 4), device=dev, dtype=torch.float32)
        with torch.no_grad():
            for mod, name, o, b in self.buffers:
                view = self.b_flat[o:o + b.numel()].view(b.shape)
                view.copy_(b)
                mod._buffers[name] = view
        self.broadcast_buffers_enabled = broadcast_buffers
        # chunks of the gradient arena, each a contiguous range of whole parameters
        per = max(1, chunk_bytes // 4)
        self.chunks, start, count = [], 0, 0
        self._chunk_of = {}
        for i, (p, o) in enumerate(zip(self.params, offs)):
            self._chunk_of[i] = len(self.chunks)
            count += 1
            end = o + _align(p.numel())
            if end - start >= per or i == len(self.params) - 1:
                self.chunks.append([start, end, count])
                start, count = end, 0
        self._pending = [c[2] for c in self.chunks]
        self._works = []
        self._reduced = set()
        self._hooks = []
        self.defer_collectives = False      # set while a step is captured into a hipGraph: reduce_all() runs the collectives after the replay
        # gradient sink: kernels may write a parameter's gradient straight into its arena slot (functional._sink)
        self._index = {id(p): i for i, p in enumerate(self.params)}
        self._claimed = set()
        # Round 5: zero_grad() skips the fill of the gradient arena (239.5 MB, 31 us) when every parameter's gradient kernel OVERWROTE its slot in the
        # previous pass (claim: all 354 parameters of the stage-3 step do) - the same kernels will overwrite them again.  settle_grads() checks the
        # assumption behind the skipped fill after the backward pass and refuses to go on if it did not hold (lazy_zero = False: always fill).
        self.lazy_zero = True
        self._all_claimed_last = False
        self._fill_skipped = False
        for p in self.params:
            p._dsrl_arena = self
        # the conv filters of the arena with their prepared operands: amax records, the [C][R][S][K] transposes the dgrad kernels read, split forms and planes
        mine = {id(p) for p in self.params}
        self.filters = FilterOperands([w for w in conv_filters(model) if id(w) in mine] if dev.type == 'cuda' else [], dev, transposed=True)
        self.filters.attach()
        self._seg_tables, self._amax_key = {}, None        # segment tables of the optimiser pass by arena range; key under which its filter magnitudes are valid
        # the weight average (enable_ema): arenas laid out as p_flat / b_flat, the 16-byte device record, and whether ema_weights() has them swapped in
        self.e_flat = self.eb_flat = self.ema_rec = self.ema_config = None
        self.ema_swapped = False
        # gradient-norm clipping (enable_grad_clip): the 64-byte device record, the tile sums at the start of their workspace, the hyper-parameters the
        # optimiser launches read once the coefficient is folded into grad_scale
        self.clip_rec = self.clip_ws = self.clip_tiles = self.hyper_eff = None
        # AdamW (enable_adamw): the second-moment arena laid out as p_flat (m_flat is the first moment), the 64-byte device record, (beta1, beta2, eps)
        self.v_flat = self.adamw_rec = self.adamw_config = None
        if self.world > 1 and self.device.type == 'cuda' and HF.knob('DSRL_BN_FUSED_BIG', None) is None:
            # RCCL kernels hold CUs while they wait for their peers: a 256-block fused-BN launch (one block on EVERY CU) could stall behind
            # them, the 128-block variant cannot
            HF.set_bn_fused_max_blocks(128)
        if self.world > 1:
            dist.broadcast(self.p_flat, 0, group=self.pg)          # DDP constructor semantics: rank 0's weights win
            dist.broadcast(self.b_flat, 0, group=self.pg)
            self.invalidate_filter_amax()                          # the collective wrote the parameters behind torch's version counters
            for i, p in enumerate(self.params):
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(i)))

    # ------------------------------------------------------------------ gradient reduction
    def _make_hook(self, i):
        def hook(_param):
            # torch runs the post-accumulate hook of a parameter even when its backward returned no gradient, i.e. also for a parameter
            # whose kernel writes straight into the arena (claim): that gradient is complete when the kernel has been ENQUEUED - for a
            # deferred weight gradient at the flush of the queue, long after this hook - and is reported by written() alone.  (Counting both
            # made a chunk look complete after half of its notifications: found by the two-phase reduction, round 3.)
            if i in self._claimed:
                return
            self._on_grad_ready(i)
        return hook

    # ------------------------------------------------------------------ gradient sink protocol
    def claim(self, p):
        """First gradient of `p` in this backward pass? Then the producing kernel may overwrite the (zeroed) arena slot."""
        i = self._index.get(id(p))
        if i is None or i in self._claimed or p.grad is None or p.grad.data_ptr() != self.g_flat.data_ptr() + 4 * self.offsets[i]:
            return False
        self._claimed.add(i)
        return True

    def written(self, p, stream=None):
        """The kernel that claimed `p` has been enqueued (on `stream`, default the current one): run the reducer hook autograd
        would have run. Gradients produced on a side stream are joined before the collective is launched."""
        if self.world > 1:
            self._on_grad_ready(self._index[id(p)])

    def _on_grad_ready(self, i):
        ci = self._chunk_of[i]
        self._pending[ci] -= 1
        if self._pending[ci] == 0 and not self.defer_collectives:
            a, b, _ = self.chunks[ci]
            if self.device.type == 'cuda' and HF.overlap_wgrad:
                # The chunk holds gradients written on the compute stream AND weight gradients written on the side stream.  Launch the
                # collective with the side stream current, after making that stream wait for the compute stream: the collective's own
                # stream then starts behind every producer of the chunk on both streams, and the compute stream itself never waits
                # (it used to join the side stream here, draining the weight-gradient backlog at every chunk boundary).
                cur = torch.cuda.current_stream(self.device)
                side = HF.side_stream(self.device)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    self._works.append(dist.all_reduce(self.g_flat[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
            else:
                self._works.append(dist.all_reduce(self.g_flat[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))

    # ------------------------------------------------------------------ optimiser pass that also measures the filters (round 5)
    def _params_key(self):
        """Changes whenever torch code writes a filter or the arena (load_state_dict, copy_, fill_ ...): the magnitudes the optimiser kernel left are
        trusted only while it is unchanged - the kernels themselves write through raw pointers and do not move it."""
        return (self.p_flat._version, sum(w._version for w in self.filters.filters))

    def _segments(self, a, b):
        """Device table {first float, floats, amax record address or 0} covering arena range [a, b) (multiples of 4) with segments of at most 32768
        floats, each inside one parameter; the filters with prepared operands carry their record (dsrl_sgd_step_dev_segments)."""
        key = (a, b)
        tab = self._seg_tables.get(key)
        if tab is not None:
            return tab
        seg = int(HF.query('dsrl_conv2d_filters_amax_segment_floats'))
        rows = []
        for p_, o in zip(self.params, self.offsets):
            lo, hi = max(o, a), min(o + _align(p_.numel()), b)
            rows += segment_rows(lo, hi - lo, self.filters.record_ptr_of.get(id(p_), 0), seg)
        tab = self._seg_tables[key] = (torch.tensor(rows, dtype=torch.int64, device=self.device), len(rows))
        return tab

    def _sgd_range(self, a, b, hyper, hp):
        """SGD on arena range [a, b): with device-resident hyper-parameters and the f16 arithmetics, by the segment kernel that also measures the filters.
        With the weight average enabled the same three launches in their _ema forms: e_flat follows in the launch that writes p_flat."""
        if self.v_flat is not None:
            return self._adamw_range(a, b, hyper, hp)
        if self.e_flat is not None:
            e, rec = self.e_flat, self.ema_rec
            if hyper is not None and self._fold_amax():
                tab, n = self._segments(a, b)
                HF.call('dsrl_sgd_step_dev_segments_ema', self.p_flat.data_ptr(), self.g_flat.data_ptr(), self.m_flat.data_ptr(), tab.data_ptr(), n, hyper.data_ptr(),
                        e.data_ptr(), rec.data_ptr(), HF._stream())
            elif hyper is not None:
                HF.sgd_step_dev_ema_(self.p_flat[a:b], self.g_flat[a:b], self.m_flat[a:b], hyper, e[a:b], rec)
            else:
                HF.sgd_step_ema_(self.p_flat[a:b], self.g_flat[a:b], self.m_flat[a:b], hp[0], hp[1], hp[2], 1.0 / self.world, e[a:b], rec)
        elif hyper is not None and self._fold_amax():
            tab, n = self._segments(a, b)
            HF.call('dsrl_sgd_step_dev_segments', self.p_flat.data_ptr(), self.g_flat.data_ptr(), self.m_flat.data_ptr(), tab.data_ptr(), n, hyper.data_ptr(), HF._stream())
        elif hyper is not None:
            HF.sgd_step_dev_(self.p_flat[a:b], self.g_flat[a:b], self.m_flat[a:b], hyper)
        else:
            HF.sgd_step_(self.p_flat[a:b], self.g_flat[a:b], self.m_flat[a:b], hp[0], hp[1], hp[2], 1.0 / self.world)

    def _adamw_range(self, a, b, hyper, hp):
        """AdamW on arena range [a, b): the launch of the form _sgd_range would have picked (host / device hyper-parameters / segment table, with or
        without the average), at the t the record holds.  `hyper` and `hp` are the SGD ones; the momentum in them is not read."""
        p, g, m, v, rec = self.p_flat, self.g_flat, self.m_flat, self.v_flat, self.adamw_rec
        ema = () if self.e_flat is None else (self.e_flat.data_ptr(), self.ema_rec.data_ptr())
        if hyper is not None and self._fold_amax():
            tab, n = self._segments(a, b)
            HF.call('dsrl_adamw_step_dev_segments_ema' if ema else 'dsrl_adamw_step_dev_segments', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                    tab.data_ptr(), n, hyper.data_ptr(), rec.data_ptr(), *ema, HF._stream())
        elif hyper is not None and ema:
            HF.adamw_step_dev_ema_(p[a:b], g[a:b], m[a:b], v[a:b], hyper, rec, self.e_flat[a:b], self.ema_rec)
        elif hyper is not None:
            HF.adamw_step_dev_(p[a:b], g[a:b], m[a:b], v[a:b], hyper, rec)
        elif ema:
            HF.adamw_step_ema_(p[a:b], g[a:b], m[a:b], v[a:b], hp[0], hp[2], 1.0 / self.world, rec, self.e_flat[a:b], self.ema_rec)
        else:
            HF.adamw_step_(p[a:b], g[a:b], m[a:b], v[a:b], hp[0], hp[2], 1.0 / self.world, rec)

    def ensure_filter_amax(self):
        """In front of a REPLAYED step: a graph captured while the optimiser's magnitudes were valid contains no measuring sweep and relies on the
        previous replay's optimiser pass.  If torch code wrote parameters since (a restored state, load_state_dict), measure eagerly once."""
        if self._fold_amax() and self._amax_key != self._params_key():
            self.filters.amax.zero_()
            self.filters.measure(streaming=True)
            self._amax_key = self._params_key()

    def _fold_amax(self):
        return (self.device.type == 'cuda' and self.filters.rows and HF.f16_mode() and HF.knob('DSRL_FILTER_AMAX_STREAM', True) and
                HF.knob('DSRL_SGD_AMAX', True) and self.filters.wsplit_flat is not None)

    # ------------------------------------------------------------------ the per-step filter pass
    def refresh_transposed_filters(self):
        """What the convs of this step read of every filter (filter_operands.FilterOperands runs the launches): under the f16 arithmetics the amax
        records, both split forms and - for the filters whose convs asked for them - the planes; else the records and the fp32 transposes."""
        ops = self.filters
        if not ops.rows:
            return
        if not HF.f16_mode():
            ops.amax.zero_()
            ops.transpose()
            return
        # with pre-split filters nothing reads the fp32 transposes: the first launch only measures (amax records) - round 5: unless the optimiser pass of
        # the previous step left max |w| of every filter it wrote (dsrl_sgd_step_dev_segments) -, the second writes both split forms
        if not (self._amax_key is not None and self._amax_key == self._params_key() and self._fold_amax()):
            ops.amax.zero_()
            ops.measure(HF.knob('DSRL_FILTER_AMAX_STREAM', True))
        ops.write_split()
        if HF.planes_mode != 'off' and HF.get_conv_precision() in ('f16x3', 'f16x1'):      # f16x1 reads the first plane only
            if HF.graph_keepalive is None:
                # 'auto': the filters whose convs asked for planes in an earlier step (functional._Conv2d marks them: operands large enough for the split
                # pass to pay); 'all': every eligible filter.  First use, or more filters asked since the last set was built - never inside a capture
                ops.add_plane_set(lambda w: HF.planes_mode == 'all' or getattr(w, '_dsrl_want_planes', False))
            ops.write_planes()

    def zero_grad(self):
        self._fill_skipped = self.lazy_zero and self._all_claimed_last
        if not self._fill_skipped:
            self.g_flat.zero_()
        self._claimed.clear()
        self._pending = [c[2] for c in self.chunks]
        self._works = []
        self._reduced = set()
        if self.device.type == 'cuda':
            # The convs of this step defer their weight gradients to grouped launches at the end of backward (functional.WgradQueue) - unless the
            # chunk all-reduces are launched from gradient-ready notifications DURING backward (world > 1, eager): a deferred weight gradient
            # would report ready only at the flush and every collective would start behind backward; that path keeps the per-layer
            # side-stream launches, which also free x / dy layer by layer.
            if self.world == 1 or self.defer_collectives:
                HF.open_wgrad_queue()
            else:
                HF.wgrad_queue = None
            if HF.f16_mode():
                HF.amax_begin_step(self.device)     # operand-magnitude slots of this step (functional.amax_slot)

    def settle_grads(self):
        """After the backward pass (every gradient kernel enqueued or recorded): was it right not to zero the arena?  Remembers whether the next
        zero_grad() may skip the fill."""
        complete = len(self._claimed) == len(self.params)
        if self._fill_skipped and not complete:
            missing = [i for i in range(len(self.params)) if i not in self._claimed]
            raise HF.DsrlHipError(f'{len(missing)} parameter gradients were not written by their kernels in this pass (first: parameter #{missing[0]}) although the '
                                  'previous pass wrote all of them, and the gradient arena was not zeroed: the graph of the step changed - set lazy_zero = False on this FlatParams')
        self._all_claimed_last = complete
        self._fill_skipped = False

    def finish_reduction(self):
        """Waits (stream-wise) for the chunk all-reduces launched during backward; chunks whose hooks did not all fire
        (parameters unused in this step) are reduced here so that every rank issues the same collectives."""
        if self.device.type == 'cuda':
            HF.flush_wgrad_queue()          # the deferred weight gradients of this backward pass, as grouped grids
            HF.join_side_streams()          # weight gradients written on the side stream (functional.overlap_wgrad)
        if self.world == 1:
            return
        for ci, left in enumerate(self._pending):
            if left > 0:
                a, b, _ = self.chunks[ci]
                self._works.append(dist.all_reduce(self.g_flat[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
                self._pending[ci] = 0
        for w in self._works:
            w.wait()
        self._works = []

    # ------------------------------------------------------------------ two-phase reduction (split hipGraph capture, world > 1)
    def _ranges(self, idx):
        """chunk indices -> merged (start, end) element ranges: neighbouring chunks travel as one collective (larger messages)"""
        out = []
        for ci in sorted(idx):
            a, b, _ = self.chunks[ci]
            if out and out[-1][1] == a:
                out[-1][1] = b
            else:
                out.append([a, b])
        return out

    def ready_chunks(self):
        """Chunks whose every gradient has been produced so far in this backward pass and that have not been reduced yet."""
        return [ci for ci, left in enumerate(self._pending) if left == 0 and ci not in self._reduced]

    def reduce_chunks(self, idx):
        """Launches (asynchronously, behind what the current stream holds) the all-reduce of the given chunks; reduce_rest() waits."""
        if self.world == 1:
            return
        for a, b in self._ranges(idx):
            self._works.append(dist.all_reduce(self.g_flat[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
        self._reduced.update(idx)

    def reduce_rest(self):
        """All chunks not reduced yet, then the current stream waits for every collective of the step."""
        if self.world == 1:
            return
        self.reduce_chunks([ci for ci in range(len(self.chunks)) if ci not in self._reduced])
        for w in self._works:
            w.wait()
        self._works = []
        self._pending = [0] * len(self.chunks)

    def reduce_all(self):
        """All chunk all-reduces of the gradient arena at once, behind whatever the current stream holds (the replay of a captured
        forward + backward); the caller's stream waits for them.  Used when backward ran from a hipGraph, where no hook fires."""
        if self.world == 1:
            return
        # nothing overlaps with these collectives, so they are as large as possible (ring all-reduce bandwidth over xGMI grows with the message
        # size): the whole 239.5 MB arena in one call
        dist.all_reduce(self.g_flat, op=dist.ReduceOp.SUM, group=self.pg, async_op=True).wait()

    def reduce_chunked_and_step(self, hyper=None, hp=None, nchunks=None):
        """The default exchange behind a replayed (or deferred eager) backward pass with more than one rank: the gradient arena is cut into
        `nchunks` contiguous ranges (DSRL_REDUCE_CHUNKS, default 4), every range's all-reduce is launched at once on the collective stream, and the
        SGD kernel of range k runs on the compute stream as soon as ITS all-reduce is done - under the all-reduces of ranges k+1 .. (round 5; the
        single 239.5 MB call of round 4 exposed the whole optimiser pass behind the exchange).  Only element-wise kernels touch the ranges, so they
        need no parameter alignment beyond 16 bytes; no barrier kernel is co-resident with RCCL here - those are all inside the graph that has
        finished.  Bit-identical to reduce_all() + one SGD launch (same element-wise arithmetic).  Returns the chunk ranges (tests).
        With gradient clipping enabled (enable_grad_clip) the update of EVERY range needs the norm of the WHOLE arena: what runs under the all-reduces
        of ranges k+1 .. is then the sum-of-squares pass of range k (ranges start at multiples of 1024, the tile of dsrl_grad_sumsq), and the SGD
        launches follow the last all-reduce and the finish - they no longer overlap the exchange.  Still bit-identical to the single-range step."""
        self._refuse_swapped('reduce_chunked_and_step')
        n = max(1, HF.knob('DSRL_REDUCE_CHUNKS', 4) if nchunks is None else int(nchunks))
        per = _align(-(-self.numel // n), 1024)
        ranges = [(a, min(a + per, self.numel)) for a in range(0, self.numel, per)]
        works = []
        if self.world > 1:
            works = [dist.all_reduce(self.g_flat[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True) for a, b in ranges]
        self._update(ranges, works, hyper, hp)
        self._pending = [0] * len(self.chunks)
        return ranges

    def sync_buffers(self):
        if self.world > 1 and self.broadcast_buffers_enabled:
            dist.broadcast(self.b_flat, 0, group=self.pg)

    # ------------------------------------------------------------------ optimiser
    def sgd_step(self, lr, momentum, weight_decay, hyper=None, reduce=True):
        """torch.optim.SGD(momentum, weight_decay).step() on the whole arena; gradients are averaged over ranks here.  `hyper`: a
        4-float device tensor (lr, momentum, weight_decay, 1/world) the kernel reads when it runs (graph-replayable) instead of the
        three host values.  After enable_adamw() the pass is torch.optim.AdamW's at the same lr and weight decay; the momentum is not read."""
        self._refuse_swapped('sgd_step')
        if reduce:
            self.finish_reduction()
        self._update([(0, self.numel)], [], hyper, (lr, momentum, weight_decay))

    def _update(self, ranges, works, hyper, hp):
        """SGD over `ranges` of the arena, range k as soon as works[k] (its all-reduce, if any) is done; then the step is over."""
        self._refuse_swapped('the optimiser step')
        if self.clip_rec is not None:
            hyper = self._clip(ranges, works, hyper, hp)        # waits for every range; the launches below read grad_scale * coef
            works = []
        fold = hyper is not None and self._fold_amax()
        if fold:
            self.filters.amax.zero_()
        if self.v_flat is not None:
            HF.adamw_advance_(self.adamw_rec)       # once per pass, on the device: every range below reads the factors of the same t (the first pass: 1)
        for i, (a, b) in enumerate(ranges):
            if works:
                works[i].wait()             # stream-ordered for RCCL: the compute stream waits for this range only
            self._sgd_range(a, b, hyper, hp)
        if self.e_flat is not None:
            # every range above read the same omd; the buffers' average follows (the step's forward has left the running statistics), then the
            # schedule moves on - once per step, on the device
            HF.ema_update_(self.eb_flat, self.b_flat, self.ema_rec)
            HF.ema_advance_(self.ema_rec)
        self._amax_key = self._params_key() if fold else None
        if self.device.type == 'cuda':
            HF.amax_end_step(self.device)       # records asked for between steps (validation) come from the loose arena, not from the step's
        self.filters.invalidate()       # the filters changed: transposed / split copies and amax records are stale until the next refresh

    def _trainable_in_model_order(self):
        return [p for p in self.model.parameters() if p.requires_grad]

    def state_dict(self, lr=0.0, momentum=0.0, weight_decay=0.0, initial_lr=None):
        """The optimiser state in torch.optim.SGD's state_dict layout (what the reference saves as `optimizer_state_dict`,
        train_or_resume.py:276, and loads back at main.py:51-52): one param group over model.parameters() order, per-parameter
        `momentum_buffer` tensors (copies of the arena views, channels-last parameters returned in their logical NCHW shape)."""
        if self.v_flat is not None:
            return self._adamw_state_dict(lr, weight_decay, initial_lr)
        ps = self._trainable_in_model_order()
        state = {}
        for i, p in enumerate(ps):
            o = self.offsets[self._index[id(p)]]
            state[i] = {'momentum_buffer': self.m_flat.as_strided(p.shape, p.stride(), o).detach().clone().contiguous().cpu()}
        group = {'lr': lr, 'momentum': momentum, 'dampening': 0, 'weight_decay': weight_decay, 'nesterov': False, 'params': list(range(len(ps)))}
        if initial_lr is not None:
            group['initial_lr'] = initial_lr            # what a torch LR scheduler leaves in the group (PolynomialLR in the reference)
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """Accepts torch.optim.SGD's layout (a reference checkpoint or our own) and the round-1 arena dump; with AdamW enabled torch.optim.AdamW's.
        State of the other optimiser raises ValueError."""
        kind = optimizer_state_kind(sd)
        if self.v_flat is not None:
            if kind == 'sgd':
                raise ValueError('optimizer state mix-up: the state is SGD\'s (momentum_buffer), this run uses AdamW (exp_avg, exp_avg_sq)')
            return self._load_adamw_state_dict(sd)
        if kind == 'adamw':
            raise ValueError('optimizer state mix-up: the state is AdamW\'s (exp_avg, exp_avg_sq), this run uses SGD (momentum_buffer)')
        if 'momentum_arena' in sd:
            if sd['numel'] != self.numel:
                raise ValueError('optimizer arena size mismatch')
            self.m_flat.copy_(sd['momentum_arena'])
            self.invalidate_filter_amax()
            return
        ps = self._trainable_in_model_order()
        ids = [i for g in sd['param_groups'] for i in g['params']]
        if len(ids) != len(ps):
            raise ValueError(f'optimizer state has {len(ids)} parameters, the model {len(ps)}')
        self.m_flat.zero_()
        self.invalidate_filter_amax()           # a restored state: whatever wrote the parameters beside it may not have moved the version counters
        with torch.no_grad():
            for p, i in zip(ps, ids):
                st = sd['state'].get(i)
                buf = None if st is None else st.get('momentum_buffer')
                if buf is None:
                    continue                          # torch creates the buffer lazily: a parameter that never stepped has none
                if tuple(buf.shape) != tuple(p.shape):
                    raise ValueError(f'momentum buffer {tuple(buf.shape)} does not match parameter {tuple(p.shape)}')
                o = self.offsets[self._index[id(p)]]
                self.m_flat.as_strided(p.shape, p.stride(), o).copy_(buf.to(self.device))

    # ------------------------------------------------------------------ AdamW
    def enable_adamw(self, betas=(0.9, 0.999), eps=1e-8):
        """torch.optim.AdamW(lr, betas, eps, weight_decay) - one group, decoupled decay, no amsgrad - in every optimiser pass from here on instead of
        SGD: v_flat (zeros, laid out as p_flat) beside m_flat (zeroed: it is the first moment now) and the 64-byte device record, t = 0.  lr, weight
        decay and grad_scale arrive as they do for SGD (the momentum among them is ignored), the launches keep their form - host / device
        hyper-parameters / segment table, with or without the average - and the step counter and its bias corrections live on the device, so a
        captured step advances them on every replay.  Call it once the weights are loaded, in front of load_state_dict (which then expects AdamW's
        layout and refuses SGD's) and of enable_ema / enable_grad_clip; a second call raises."""
        if self.v_flat is not None:
            raise HF.DsrlHipError('enable_adamw: AdamW of this FlatParams is already enabled')
        cfg = HF.adamw_value({'name': 'adamw', 'betas': tuple(betas), 'eps': eps})
        self.adamw_config = cfg
        self.m_flat.zero_()
        self.v_flat = torch.zeros_like(self.p_flat)
        self.adamw_rec = HF.adamw_record(cfg[0], cfg[1], cfg[2], self.device)

    def adamw_step_count(self):
        """Optimiser passes done so far (t), read from the device record (synchronises)."""
        if self.v_flat is None:
            raise HF.DsrlHipError('adamw_step_count: AdamW is not enabled (enable_adamw)')
        return HF.adamw_record_read(self.adamw_rec)['t']

    def _adamw_state_dict(self, lr, weight_decay, initial_lr):
        """torch.optim.AdamW's state_dict layout: per parameter `step` (a float tensor, the same t for all), `exp_avg`, `exp_avg_sq` (copies of the
        arena views in logical NCHW shape); one param group with the keys the installed torch writes."""
        ps = self._trainable_in_model_order()
        t = self.adamw_step_count()
        state = {}
        for i, p in enumerate(ps):
            o = self.offsets[self._index[id(p)]]
            state[i] = {'step': torch.tensor(float(t), dtype=torch.float32),
                        'exp_avg': self.m_flat.as_strided(p.shape, p.stride(), o).detach().clone().contiguous().cpu(),
                        'exp_avg_sq': self.v_flat.as_strided(p.shape, p.stride(), o).detach().clone().contiguous().cpu()}
        b1, b2, eps = self.adamw_config
        group = adamw_param_group(lr, (b1, b2), eps, weight_decay, len(ps))
        if initial_lr is not None:
            group['initial_lr'] = initial_lr
        return {'state': state, 'param_groups': [group]}

    def _load_adamw_state_dict(self, sd):
        ps = self._trainable_in_model_order()
        ids = [i for g in sd['param_groups'] for i in g['params']]
        if len(ids) != len(ps):
            raise ValueError(f'optimizer state has {len(ids)} parameters, the model {len(ps)}')
        steps = set()
        todo = []
        for p, i in zip(ps, ids):
            st = sd['state'].get(i)
            if not st:
                continue                              # torch creates the state lazily: a parameter that never stepped has none and stays zero
            m, v = st.get('exp_avg'), st.get('exp_avg_sq')
            if m is None or v is None or 'step' not in st:
                raise ValueError(f'AdamW state of parameter {i} lacks step, exp_avg or exp_avg_sq')
            if tuple(m.shape) != tuple(p.shape) or tuple(v.shape) != tuple(p.shape):
                raise ValueError(f'AdamW moments {tuple(m.shape)} / {tuple(v.shape)} do not match parameter {tuple(p.shape)}')
            steps.add(int(float(st['step'])))
            todo.append((p, m, v))
        if len(steps) > 1 or any(s < 0 for s in steps):
            raise ValueError(f'AdamW state with step counts {sorted(steps)}: one count >= 0 for all parameters expected (one group, one arena)')
        self.m_flat.zero_()
        self.v_flat.zero_()
        self.invalidate_filter_amax()
        with torch.no_grad():
            for p, m, v in todo:
                o = self.offsets[self._index[id(p)]]
                self.m_flat.as_strided(p.shape, p.stride(), o).copy_(m.to(self.device))
                self.v_flat.as_strided(p.shape, p.stride(), o).copy_(v.to(self.device))
        HF.adamw_set_step_(self.adamw_rec, steps.pop() if steps else 0)

    # ------------------------------------------------------------------ filter magnitudes left by the optimiser pass: explicit invalidation
    def invalidate_filter_amax(self):
        """The magnitudes the optimiser pass left (_amax_key) are trusted while torch's version counters stand still (_params_key); a writer those
        counters do not see - a collective on the arena, a raw-pointer kernel such as the swap of ema_weights(), `.data` writes - calls this, and
        the next step measures the filters again.  External code that writes parameters through `.data` must call it too."""
        self._amax_key = None

    # ------------------------------------------------------------------ gradient-norm clipping
    def enable_grad_clip(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) inside every optimiser pass from here on, on the device: a sum-of-squares pass over
        the gradient arena, one finish that forms coef = min(1, max_norm / (norm + 1e-6)) from the norm of the rank-averaged gradient and writes
        {lr, momentum, weight_decay, coef / world} to `hyper_eff`, and the usual SGD launches reading that.  No host read or write per step, so a
        captured step clips on every replay; the record holds max_norm (write a new value into it and the next step uses it) and the figures
        grad_clip_stats() reports.  max_norm = inf monitors only: the step is bit-identical to one without clipping.  A second call raises."""
        if self.clip_rec is not None:
            raise HF.DsrlHipError('enable_grad_clip: gradient clipping of this FlatParams is already enabled')
        v = HF.grad_clip_value(max_norm)
        if v is None:
            raise ValueError(f'enable_grad_clip: max_norm = {max_norm!r}')
        self.clip_ws = HF.grad_clip_workspace(self.numel, self.device)
        self.clip_tiles = self.clip_ws[:-(-self.numel // HF.GRAD_CLIP_TILE)]
        self.hyper_eff = torch.zeros(4, device=self.device, dtype=torch.float32)
        self.clip_rec = HF.grad_clip_record(v, self.device)

    def set_grad_clip_max_norm(self, max_norm):
        """A new threshold, written into the device record behind what the stream holds: captured steps follow it without a re-capture."""
        self._need_clip('set_grad_clip_max_norm')
        v = HF.grad_clip_value(max_norm)
        if v is None:
            raise ValueError(f'set_grad_clip_max_norm: max_norm = {max_norm!r}')
        self.clip_rec[6:7].copy_(HF.grad_clip_record(v, 'cpu')[6:7])

    def grad_clip_stats(self, reset=False):
        """One device read (synchronises): {'norm_mean', 'norm_max' over the steps with a finite norm since the last reset (NaN / 0 when there
        was none), 'norm', 'coef' of the last step, 'steps', 'clipped', 'nonfinite', 'max_norm'}.  reset=True starts the running figures again
        (max_norm stays)."""
        self._need_clip('grad_clip_stats')
        r = HF.grad_clip_record_read(self.clip_rec)
        finite = r['steps'] - r['nonfinite']
        out = {'norm_mean': r['norm_sum'] / finite if finite else float('nan'), 'norm_max': r['norm_max'], 'norm': r['norm'], 'coef': r['coef'],
               'steps': r['steps'], 'clipped': r['clipped'], 'nonfinite': r['nonfinite'], 'max_norm': r['max_norm']}
        if reset:
            self.clip_rec[2:4].zero_()          # norm_sum
            self.clip_rec[7:11].zero_()         # norm_max, steps, clipped, nonfinite; max_norm and the last step's figures stay
        return out

    def _need_clip(self, what):
        if self.clip_rec is None:
            raise HF.DsrlHipError(f'{what}: gradient clipping is not enabled (enable_grad_clip)')

    def _clip(self, ranges, works, hyper, hp):
        """The clipping part of an optimiser pass: the tile sums of range k as soon as works[k] (its all-reduce, if any) is done - under the
        all-reduces of ranges k+1 .. -, then one finish.  -> hyper_eff, the device hyper-parameters of every SGD launch of the pass."""
        for i, (a, b) in enumerate(ranges):
            if works:
                works[i].wait()
            HF.grad_sumsq_(self.g_flat[a:b], a, self.clip_tiles)
        if hyper is not None:
            HF.grad_clip_finish_(self.clip_tiles, self.clip_rec, self.hyper_eff, hyper=hyper)
        else:
            HF.grad_clip_finish_(self.clip_tiles, self.clip_rec, self.hyper_eff, hp=(hp[0], hp[1], hp[2], 1.0 / self.world))
        return self.hyper_eff

    # ------------------------------------------------------------------ exponential moving average of the weights
    def enable_ema(self, decay, warmup=True):
        """Starts the weight average from the CURRENT parameters and buffers: e_flat / eb_flat (copies of p_flat / b_flat) and the device record
        {omd = 1 - d_0, decay, updates = 0, warmup}.  From here every optimiser pass updates e_flat in the launch that writes p_flat, eb_flat
        behind it, and advances the schedule on the device (d_t = min(decay, (1 + t) / (10 + t)) under warm-up).  Call it after a state load, so
        that the average starts from the weights training starts from; a second call raises.  With several ranks every rank averages its own
        arenas: the parameters are identical, the buffers are rank 0's after every broadcast, and only rank 0's average is ever read."""
        if self.e_flat is not None:
            raise HF.DsrlHipError('enable_ema: the weight average of this FlatParams is already enabled')
        cfg = HF.ema_value((decay, warmup))
        if cfg is None:
            raise ValueError(f'enable_ema: decay = {decay!r}')
        self.ema_config = cfg
        self.e_flat = self.p_flat.detach().clone()
        self.eb_flat = self.b_flat.detach().clone()
        self.ema_rec = HF.ema_record(cfg[0], cfg[1], 0, self.device)

    def ema_updates(self):
        """Averages formed so far, read from the device record (synchronises)."""
        self._need_ema('ema_updates')
        return HF.ema_record_read(self.ema_rec)['updates']

    def _need_ema(self, what):
        if self.e_flat is None:
            raise HF.DsrlHipError(f'{what}: the weight average is not enabled (enable_ema)')

    def _refuse_swapped(self, what):
        if self.ema_swapped:
            raise HF.DsrlHipError(f'{what} inside ema_weights(): the parameters are the averaged ones, a training step would update the average as if it were the model')

    def _swap_ema(self):
        HF.arena_swap_(self.p_flat, self.e_flat)
        HF.arena_swap_(self.b_flat, self.eb_flat)
        # the kernels wrote behind torch's back: drop what was derived from the old values, and move every counter a watcher reads (_params_key,
        # inference.FrozenOperands).  A parameter's counter is its own, not the arena's
        self.invalidate_filter_amax()
        self.filters.invalidate()
        bump = torch.autograd.graph.increment_version
        bump(self.p_flat)
        bump(self.b_flat)
        for p in self.params:
            bump(p)
        for mod, name, _, _ in self.buffers:
            bump(mod._buffers[name])

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model IS the averaged model: p_flat <-> e_flat and b_flat <-> eb_flat are exchanged in place (two launches, no
        third buffer) and exchanged back on exit, bit for bit.  For validation and for writing weights; a training step inside raises."""
        self._need_ema('ema_weights')
        self._refuse_swapped('ema_weights (nested)')
        self._swap_ema()
        self.ema_swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self.ema_swapped = False

    def _ema_sources(self):
        """state_dict key -> the tensor of the averaged model: views of e_flat / eb_flat for what the arenas hold, the live tensor for the rest
        (integer buffers such as num_batches_tracked, parameters that do not train)."""
        src = {}
        pviews = {id(p): self.e_flat.as_strided(p.shape, p.stride(), o) for p, o in zip(self.params, self.offsets)}
        bviews = {(id(mod), name): self.eb_flat[o:o + b.numel()].view(b.shape) for mod, name, o, b in self.buffers}
        for prefix, mod in self.model.named_modules(remove_duplicate=False):
            dot = prefix + '.' if prefix else ''
            for name, p in mod._parameters.items():
                if p is not None:
                    src[dot + name] = pviews.get(id(p), p)
            for name, b in mod._buffers.items():
                if b is not None and name not in mod._non_persistent_buffers_set:
                    src[dot + name] = bviews.get((id(mod), name), b)
        return src

    def ema_state_dict(self):
        """The averaged model in the layout of model.state_dict() - same keys, logical NCHW shapes, tensors on the arena's device -, parameters and
        float buffers from the EMA arenas, integer buffers from the live model, plus 'ema_updates' (int) and 'ema_decay' (float)."""
        self._need_ema('ema_state_dict')
        if self.ema_swapped:
            raise HF.DsrlHipError('ema_state_dict inside ema_weights(): the arenas are exchanged')
        src = self._ema_sources()
        sd = {k: src[k].detach().clone() for k in self.model.state_dict().keys()}
        rec = HF.ema_record_read(self.ema_rec)
        sd['ema_updates'], sd['ema_decay'] = rec['updates'], rec['decay_max']
        return sd

    def load_ema_state_dict(self, sd):
        """Restores the average from ema_state_dict(): the arenas from the tensors, `updates` from 'ema_updates', and omd recomputed from it under
        the decay and warm-up this FlatParams was enabled with (the run's setting rules; 'ema_decay' records what the file was written with)."""
        self._need_ema('load_ema_state_dict')
        if self.ema_swapped:
            raise HF.DsrlHipError('load_ema_state_dict inside ema_weights(): the arenas are exchanged')
        src = self._ema_sources()
        keys = set(self.model.state_dict().keys())
        missing = keys - set(sd)
        if missing or 'ema_updates' not in sd:
            raise ValueError(f'ema state has no {sorted(missing)[:3] or "ema_updates"!r}: not an ema_state_dict of this model')
        with torch.no_grad():
            for k in keys:
                dst = src[k]
                if dst.dtype != torch.float32 or not (dst._base is self.e_flat or dst._base is self.eb_flat):
                    continue                    # lives in the model, not in the average
                if tuple(sd[k].shape) != tuple(dst.shape):
                    raise ValueError(f'ema state: {k} is {tuple(sd[k].shape)}, the model {tuple(dst.shape)}')
                dst.copy_(sd[k].to(self.device))
        updates = int(sd['ema_updates'])
        if not 0 <= updates < 2 ** 32:
            raise ValueError(f'ema state: ema_updates = {updates!r}')
        self.ema_rec.copy_(HF.ema_record(self.ema_config[0], self.ema_config[1], updates, self.device))

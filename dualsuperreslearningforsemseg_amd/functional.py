"""torch.autograd.Function wrappers over the C ABI of libdsrl_hip.so (include/dsrl_hip.h).

Tensors keep the reference's logical NCHW shapes; physically they are torch.channels_last ("pixel-major"
[P][ld] for the kernels), which the wrappers enforce with at most one strided copy at the boundary.  Every op
raises if its tensors are not on a HIP device: there is no CPU / stock-ATen fallback in this package.
"""
import contextlib
import ctypes
import math
import os
import sys
import weakref

import numpy as np

import torch

from . import _lib
from ._lib import call, knob, query, DsrlHipError

CL = torch.channels_last


# ------------------------------------------------------------------------------------------------ helpers
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    """hipStream_t of torch's current stream on the current device (what `with torch.cuda.stream(...)` selects).  The raw accessors
    cost ~0.3 us; torch.cuda.current_stream() builds a Stream object and re-checks device availability (~4 us) on each of the ~250
    calls of a step."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


# Weight-gradient kernels run on a side HIP stream so that they overlap with the data-gradient kernel of the same layer (both
# only read dy): the small backbone layers do not fill 256 CUs on their own. ddp.FlatParams joins the stream before it
# reduces / applies the gradients; without an arena the caller's stream waits right away.
_side = {}
overlap_wgrad = knob('DSRL_OVERLAP_WGRAD', True)     # measured: +10-13 % step throughput on one MI355X


CONV_PRECISION_MODES = {'fp32': 0, 'bf16x3': 1, 'bf16x6': 2, 'mixed': 3, 'f16x3': 4, 'f16x1': 5}
DEFAULT_CONV_PRECISION = 4


def set_conv_precision(mode):
    """Arithmetic of the conv kernels (include/dsrl_hip.h: dsrl_conv_precision): 'fp32' (exact fp32 MFMA products), 'bf16x3',
    'bf16x6' (fp32-equivalent), 'mixed' (forward bf16x6, backward bf16x3), 'f16x3' (two fp16 terms of the per-tensor scaled
    operands: fp32-equivalent at half the matrix work of bf16x6; the default since round 3) or 'f16x1' (ONE fp16 term, one MFMA per
    product, fp32 accumulation: apex O1 / O2's arithmetic, the reduced-precision mode); None follows DSRL_CONV_PRECISION.
    Returns the previous setting as the library reported it (an int, -1 = environment)."""
    code = -1 if mode is None else (CONV_PRECISION_MODES[mode] if isinstance(mode, str) else int(mode))
    if not -1 <= code <= 5:
        raise ValueError(f'conv precision mode {mode!r}')
    _mode_cache.clear()
    _query_cache.clear()        # workspace sizes and partial counts follow the arithmetic's tile / pixel-range plans
    return int(_lib.load().dsrl_conv_precision(code))


_mode_cache = {}


def _conv_precision_code():
    code = _mode_cache.get('code')
    if code is None:
        prev = int(_lib.load().dsrl_conv_precision(-2))          # out-of-range argument: query only
        code = prev if prev >= 0 else knob('DSRL_CONV_PRECISION', DEFAULT_CONV_PRECISION)
        code = _mode_cache['code'] = min(max(code, 0), 5)
    return code


def get_conv_precision():
    """Name of the mode the conv kernels currently run in."""
    code = _conv_precision_code()
    return [k for k, v in CONV_PRECISION_MODES.items() if v == code][0]


# ------------------------------------------------------------------------------------------------ operand magnitudes (f16x3 arithmetic)
# The f16x3 conv kernels scale every operand tensor by a power of two taken from max |x| of the whole tensor (include/dsrl_hip.h:
# dsrl_amax).  A magnitude is one amax record of 256 uint32 device words ("slot"); a tensor that has one carries it as the attribute `_dsrl_amax`, left by
# the kernel that wrote the tensor (BatchNorm apply / backward, the batched filter transpose) or by a dsrl_amax launch here, so that the
# forward conv and the weight gradient (x) and the data and weight gradients (dy) share one measurement.  Slots come from an arena that
# ddp.FlatParams.zero_grad() rewinds and zeroes at the start of every training step (one memset; static addresses under graph capture).
_AMAX_SLOTS, AMAX_WORDS = 2048, 256          # records per arena (a stage-3 step uses ~700); include/dsrl_hip.h: DSRL_AMAX_WORDS
# Two kinds of arenas per device.  The STEP arena belongs to training steps: ddp.FlatParams.zero_grad() rewinds and zeroes it (amax_begin_step),
# sgd_step() closes it (amax_end_step); a captured hipGraph bakes in its addresses (the zero fill, ~700 records the kernels max into and read), so a
# capture PINS it (amax_pin: the graph holds the tensor, and a pinned arena is never replaced).  Everything outside an open step - evaluation
# forwards between epochs, tools, tests - draws from a LOOSE arena that is simply replaced when it is full (views keep the old one alive for the
# tensors that still carry its records).  Round 3 had one arena for both: ten validation batches exhausted it, the replacement freed the memory a
# live graph kept writing to.
_amax_arena = {}            # device -> [int32 tensor, next free slot, generation, pinned]
_amax_loose = {}            # device -> [int32 tensor, next free slot]
_amax_open = set()          # devices whose step arena is open


def _new_arena(device):
    return torch.zeros(_AMAX_SLOTS * AMAX_WORDS, dtype=torch.int32, device=device)


def amax_begin_step(device):
    """Rewinds the step arena of `device` and zeroes it (stream-ordered): every record handed out of it before belongs to a finished step - the
    generation counter invalidates the `_dsrl_amax` attributes that still point into it (amax_for re-measures such tensors)."""
    ar = _amax_arena.get(device)
    if ar is None:
        ar = _amax_arena[device] = [_new_arena(device), 0, 1, False]
    else:
        ar[0].zero_()
        ar[1] = 0
        ar[2] += 1
    _amax_open.add(device)
    return ar


def amax_end_step(device):
    """The training step of `device` is over (its optimiser update has been enqueued, or it was abandoned): records asked for from here on come from
    the loose arena, and the fp16 planes cached on this step's operand tensors are released."""
    _amax_open.discard(device)
    drop_planes()


def amax_pin(device):
    """The step arena of `device`, marked as referenced by a captured graph (the caller keeps the tensor with the graph): never replaced from now on."""
    ar = _amax_arena.get(device)
    if ar is None:
        ar = amax_begin_step(device)
        amax_end_step(device)
    ar[3] = True
    return ar[0]


def amax_slot(device):
    """A zeroed amax record.  The returned view carries `_dsrl_gen`: the generation of the step arena it came from (-1: loose arena, never reused)."""
    ar = _amax_arena.get(device)
    if ar is not None and device in _amax_open:
        if ar[1] >= _AMAX_SLOTS:
            if ar[3]:
                raise DsrlHipError(f'amax arena exhausted inside a training step whose graph is captured ({_AMAX_SLOTS} records): raise functional._AMAX_SLOTS')
            ar[0], ar[1] = _new_arena(device), 0          # an eager step that needs more: views keep the old tensor alive for its kernels
        i = ar[1]
        ar[1] = i + 1
        slot = ar[0][i * AMAX_WORDS:(i + 1) * AMAX_WORDS]
        slot._dsrl_gen = ar[2]
        return slot
    lo = _amax_loose.get(device)
    if lo is None or lo[1] >= _AMAX_SLOTS:
        lo = _amax_loose[device] = [_new_arena(device), 0]
    i = lo[1]
    lo[1] = i + 1
    slot = lo[0][i * AMAX_WORDS:(i + 1) * AMAX_WORDS]
    slot._dsrl_gen = -1
    return slot


class amax_private:
    """with amax_private(arena): ... - every amax record asked for inside the block comes out of `arena`, a step-arena of the caller's own
    ([tensor from _new_arena, next free slot, generation, pinned]): inference.CompiledPredictor captures each of its graphs inside one, with the
    arena's zero fill as the graph's first node, so that a replay maxes into records of its own that are zero when it starts.  The step arena of
    the training steps and the loose arena are neither read nor written; on exit they are what they were."""

    def __init__(self, arena):
        self.arena = arena
        self.device = arena[0].device

    def __enter__(self):
        self.saved = (_amax_arena.get(self.device), self.device in _amax_open)
        _amax_arena[self.device] = self.arena
        _amax_open.add(self.device)
        return self.arena

    def __exit__(self, *exc):
        prev, was_open = self.saved
        if prev is None:
            _amax_arena.pop(self.device, None)
        else:
            _amax_arena[self.device] = prev
        if not was_open:
            _amax_open.discard(self.device)
        return False


def f16_mode():
    """The conv kernels scale their operands by per-tensor powers of two (amax records): 'f16x3' and 'f16x1'."""
    return _conv_precision_code() >= 4


def set_amax(t, slot):
    """Attaches the amax record `slot` to tensor `t` together with what makes it stale: the tensor's version counter (an in-place write) and the
    generation of the step arena the record lives in (amax_begin_step zeroes and re-issues those records)."""
    try:
        t._dsrl_amax = slot
        t._dsrl_amax_meta = (t._version, getattr(slot, '_dsrl_gen', -1))
    except Exception:           # noqa: BLE001
        pass


def carried_amax(t):
    """The record `t` carries if it still describes the tensor's values, else None."""
    slot = getattr(t, '_dsrl_amax', None)
    if slot is None:
        return None
    meta = getattr(t, '_dsrl_amax_meta', None)
    if meta is None or meta[0] != t._version:
        return None
    if meta[1] != -1:
        ar = _amax_arena.get(slot.device)
        if ar is None or ar[2] != meta[1]:
            return None
    return slot


def amax_for(t, data=None, ld=None):
    """The magnitude record of pixel-major tensor `t` (N,C,H,W): the one it carries (left by its producer or by an earlier measurement, and still
    valid: carried_amax), or a fresh measurement that it then carries.  `data`/`ld`: the pixel-major copy of `t` the kernels read, if the caller has it."""
    slot = carried_amax(t)
    if slot is not None:
        return slot
    if data is None:
        data, ld = pm(t)
    N, Cc, H, W = data.shape
    slot = amax_slot(data.device)
    call('dsrl_amax', data.data_ptr(), ld, N * H * W, Cc, slot.data_ptr(), _stream())
    set_amax(t, slot)
    return slot


def set_bn_fused_max_blocks(n):
    """Block budget of the single-kernel BatchNorm (include/dsrl_hip.h: dsrl_bn_fused_max_blocks): 0 = off, 128, 256; None = follow the
    environment. Its device-wide barrier needs all blocks resident at once, i.e. no other process on the GPU."""
    return int(_lib.load().dsrl_bn_fused_max_blocks(-1 if n is None else int(n)))


def bn_fused_barrier_timeouts():
    """Blocks of fused BN launches that gave up waiting at the barrier so far (their outputs were poisoned with NaN). Synchronises."""
    import ctypes
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().dsrl_bn_fused_barrier_timeouts(ctypes.byref(n)), 'dsrl_bn_fused_barrier_timeouts')
    return int(n.value)


def side_stream(device):
    st = _side.get(device)
    if st is None:
        st = _side[device] = torch.cuda.Stream(device=device)
    return st


def join_side_streams():
    if not _side:                   # no side stream was ever made (also: a host-only schedule test on CPU)
        return
    cur = torch.cuda.current_stream()
    for st in _side.values():
        if st.device == cur.device:
            cur.wait_stream(st)


# Deferred weight gradients: while a WgradQueue is open (ddp.FlatParams opens one per training step), a conv's backward only records
# its weight-gradient problem (x, dy, arena slot); flush() launches all of them as a few grouped grids (dsrl_conv2d_wgrad_group_*).
# Nothing but the optimiser reads a weight gradient, the small layers do not fill the chip on their own, and a pass-wide grid needs
# neither the side stream nor per-layer pixel splits.  Off: DSRL_WGRAD_GROUP=0 (per-layer launches, overlapped on the side stream).
group_wgrad = knob('DSRL_WGRAD_GROUP', True)
graph_keepalive = None          # a list while a hipGraph capture is in progress: host buffers the captured copies read on every replay
capture_host, capture_host_off = None, 0      # pinned arena for host tables written during a capture (allocated before it starts)
GRAPH_WARMUP = 2                # eager calls per graph key before its capture (lazy initialisation, allocator warm-up)


@contextlib.contextmanager
def capture_scope(table_bytes):
    """The host state of a hipGraph capture: the pinned arena of `table_bytes` for host tables, allocated BEFORE the capture starts (hipHostMalloc
    is not capturable), and the keep-alive list, which it yields: the caller keeps it as long as the graph - captured copies re-read those buffers."""
    global graph_keepalive, capture_host, capture_host_off
    capture_host, capture_host_off = torch.empty(table_bytes, dtype=torch.uint8, pin_memory=True), 0
    keep = graph_keepalive = [capture_host]
    try:
        yield keep
    finally:
        graph_keepalive = capture_host = None


def abandon_capture(device, e, what, then):
    """After a failed capture (nothing of it has executed): one line on stderr, then back to the default stream and an idle device; the caller goes on
    with eager launches."""
    global graph_keepalive, capture_host
    print(f'[dsrl] hipGraph capture{what} failed ({type(e).__name__}: {str(e)[:200]}); {then}', file=sys.stderr, flush=True)
    graph_keepalive = capture_host = None
    try:
        torch.cuda.set_stream(torch.cuda.default_stream(device))
        torch.cuda.synchronize(device)
    except Exception:           # noqa: BLE001
        pass


class WgradQueue:
    def __init__(self):
        self.items = []           # (x, ldx, dy, lddy, dw tensor, shp, on_written)

    def add(self, x, ldx, dy, lddy, dw, shp, on_written=None, x_amax=None, dy_amax=None):
        self.items.append((x, ldx, dy, lddy, dw, shp, on_written, x_amax, dy_amax))

    def flush(self):
        items, self.items = self.items, []
        if not items:
            return
        n = len(items)
        probs = (_lib.WgradProblem * n)()
        for q, (x, ldx, dy, lddy, dw, shp, _, xa, dya) in zip(probs, items):
            N, H, W, Cc, K, R, S, stride, pad, dil = shp
            q.x, q.dy, q.dw = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
            q.x_amax = None if xa is None else xa.data_ptr()
            q.dy_amax = None if dya is None else dya.data_ptr()
            q.ldx, q.lddy, q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad, q.dil = ldx, lddy, N, H, W, Cc, K, R, S, stride, pad, dil
        import ctypes
        lib = _lib.load()
        like = items[0][0]
        tbytes = int(lib.dsrl_conv2d_wgrad_group_table_bytes(n))
        ws = _ws(int(lib.dsrl_conv2d_wgrad_group_workspace_bytes(ctypes.addressof(probs), n)), like)
        if graph_keepalive is not None:
            # under capture no pinned memory may be allocated (hipHostMalloc is not capturable): the table comes out of the pinned arena
            # the capturing TrainStep set aside, and that arena lives as long as the graph (its copy node re-reads it on every replay)
            global capture_host_off
            off = (capture_host_off + 255) & ~255
            if capture_host is None or off + tbytes > capture_host.numel():
                raise DsrlHipError('WgradQueue.flush under graph capture: the pinned table arena is missing or too small')
            host = capture_host[off:off + tbytes]
            capture_host_off = off + tbytes
        else:
            host = torch.empty(tbytes, dtype=torch.uint8, pin_memory=True)
        dev = torch.empty(tbytes, dtype=torch.uint8, device=like.device)
        call('dsrl_conv2d_wgrad_group_plan', ctypes.addressof(probs), n, host.data_ptr(), tbytes, dev.data_ptr(), ws.data_ptr(), ws.numel())
        dev.copy_(host, non_blocking=True)
        if graph_keepalive is not None:
            graph_keepalive.append(host)          # a captured copy re-reads this pinned buffer on every replay
        call('dsrl_conv2d_wgrad_group_launch', host.data_ptr(), dev.data_ptr(), _stream())
        for it in items:
            if it[6] is not None:
                it[6]()


wgrad_queue = None              # the open queue, if any


def open_wgrad_queue():
    global wgrad_queue
    wgrad_queue = WgradQueue() if (group_wgrad and get_conv_precision() != 'fp32') else None
    return wgrad_queue


def flush_wgrad_queue(reopen=False):
    """Launches what the open queue holds and closes it: only a step that opened a queue (FlatParams.zero_grad) defers.  `reopen`: a new
    queue takes the weight gradients of the rest of the backward pass (two-phase backward: one grouped launch set per phase)."""
    global wgrad_queue
    q, wgrad_queue = wgrad_queue, None
    if q is not None:
        q.flush()
        if reopen:
            wgrad_queue = WgradQueue()


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise DsrlHipError('dualsuperreslearningforsemseg_amd ops run on the HIP device only (got a CPU tensor); '
                               'there is no CPU fallback - move the model and inputs to cuda')


def _f32(t):
    if t.dtype != torch.float32:
        raise DsrlHipError(f'fp32 tensors expected, got {t.dtype}')
    return t


def new_cl(shape, like):
    return torch.empty(shape, device=like.device, dtype=torch.float32, memory_format=CL)


# Workspaces come from the caching allocator, one per call: a growing buffer per (device, stream) was measured and made no difference.
_ws_none = {}


def _ws(nbytes, like):
    nbytes = int(nbytes)
    if nbytes <= 0:             # nothing to hand over: one persistent 256-byte placeholder per device instead of an allocator round trip
        buf = _ws_none.get(like.device)
        if buf is None:
            buf = _ws_none[like.device] = torch.empty(256, device=like.device, dtype=torch.uint8)
        return buf
    return torch.empty(max(nbytes, 256), device=like.device, dtype=torch.uint8)


_query_cache = {}


def cquery(name, *args):
    """workspace-size style queries are pure functions of the shape: memoise them"""
    key = (name, args)
    v = _query_cache.get(key)
    if v is None:
        v = _query_cache[key] = query(name, *args)
    return v


def _ld_of(t):
    """Pixel stride if `t` (N,C,H,W) is pixel-major (channel stride 1, dense pixels with stride ld), else None."""
    N, C, H, W = t.shape
    st = t.stride()
    if C > 1 and st[1] != 1:
        return None
    if W > 1:
        ld = st[3]
    elif H > 1:
        ld = st[2]
    elif N > 1:
        ld = st[0]
    else:
        ld = C
    if ld < C:
        return None
    if (W > 1 and st[3] != ld) or (H > 1 and st[2] != W * ld) or (N > 1 and st[0] != H * W * ld):
        return None
    return ld


def pm(t):
    """-> (tensor, ld): a pixel-major view of `t` (copying into channels_last only when needed)."""
    _need_gpu(t); _f32(t)
    if t.dim() != 4:
        raise DsrlHipError(f'4-D (N,C,H,W) tensor expected, got shape {tuple(t.shape)}')
    ld = _ld_of(t)
    if ld is None or (t.data_ptr() % 4) != 0:
        out = new_cl(tuple(t.shape), t)
        out.copy_(t)
        return out, t.shape[1]
    return t, ld


def pm_dense(t):
    """pixel-major with ld == C"""
    t, ld = pm(t)
    if ld != t.shape[1]:
        out = new_cl(tuple(t.shape), t)
        N, Cc, H, W = t.shape
        call('dsrl_copy2d', t.data_ptr(), ld, out.data_ptr(), Cc, N * H * W, Cc, _stream())
        return out
    return t


def pm_vec4(t):
    """pixel-major view the float4 loaders of the MFMA kernels accept: 16-byte aligned base, ld a multiple of 4;
    a channel count that is not a multiple of 4 (the 19 class logits) is copied into a zero-padded buffer."""
    t, ld = pm(t)
    N, Cc, H, W = t.shape
    if Cc % 4 == 0 and ld % 4 == 0 and t.data_ptr() % 16 == 0:
        return t, ld
    cp = (Cc + 3) & ~3
    buf = new_cl((N, cp, H, W), t)
    if cp != Cc:
        buf.zero_()
    call('dsrl_copy2d', t.data_ptr(), ld, buf.data_ptr(), cp, N * H * W, Cc, _stream())
    return buf[:, :Cc], cp


def _sink(param, like_shape=None):
    """If `param` is bound to a ddp.FlatParams arena (and has not received a gradient yet in this backward), returns the arena
    view its gradient kernel may write directly - this skips the temporary + accumulate launch autograd would otherwise need."""
    owner = getattr(param, '_dsrl_arena', None)
    if owner is None or not owner.claim(param):
        return None
    return param.grad


def _sink_flat(param, n):
    """The arena slot of `param` as the n-float output of its gradient kernel, when the parameter's memory is dense in logical order (biases,
    ConvTranspose weights, the 1xCx1x1 feature-transformer filters) and this is its first gradient of the pass - else None.  The caller
    launches the kernel into it and then calls _sunk(param): no temporary, no copy launch (they were 4-5 us each, ~10 per step)."""
    owner = getattr(param, '_dsrl_arena', None)
    if owner is None or not isinstance(param, torch.nn.Parameter) or param.grad is None:
        return None
    g = param.grad
    if not g.is_cuda or g.numel() != n or not g.is_contiguous() or not owner.claim(param):
        return None
    return g


def _sunk(param):
    param._dsrl_arena.written(param)


def _deliver(param, grad):
    """Hands a freshly computed parameter gradient to the arena instead of to autograd: when `param` lives in a ddp.FlatParams arena and this
    is its first gradient of the pass, the values are copied into its (zeroed) arena slot on the CURRENT stream, the reducer is told, and
    autograd gets nothing.  Besides saving autograd's own accumulation launch this keeps leaf accumulation off other streams: torch runs an
    AccumulateGrad node on the stream its parameter was created on, which under graph capture forks the capture across streams (the warning
    'AccumulateGrad node's stream does not match ...') - with every parameter gradient delivered here the captured step is one linear stream."""
    if grad is None or not isinstance(param, torch.nn.Parameter):
        return grad
    owner = getattr(param, '_dsrl_arena', None)
    if owner is None or not grad.is_cuda or tuple(grad.shape) != tuple(param.shape) or not owner.claim(param):
        return grad
    param.grad.copy_(grad)
    owner.written(param)
    return None


def _weight_amax(w):
    """The amax record its FilterOperands (filter_operands.py) keeps for a conv filter - measured in this step, or once for a frozen model - or None."""
    h = getattr(w, '_dsrl_operands', None)
    return None if h is None else h[0].record(h[1])


def _weight_split(w, transposed=False):
    """The pre-split form of a conv filter written in this step (forward layout, or transposed), or None."""
    h = getattr(w, '_dsrl_operands', None)
    return None if h is None else h[0].split(h[1], transposed)


def _weight_planes(w, transposed=False):
    """The fp16 planes of a conv filter written in this step ([K][R][S][C], or transposed [C][R][S][K]), or None."""
    h = getattr(w, '_dsrl_operands', None)
    return None if h is None else h[0].planes(h[1], transposed)


def split_filter(w):
    """(amax record, w_split, wt_split) of one [K][R][S][C] filter for the f16x3 kernels: what filter_operands.FilterOperands prepares for every
    filter of a model (dsrl_conv2d_transpose_filters_batched + dsrl_conv2d_split_filters_batched), here for a single tensor."""
    from .filter_operands import table_row, wt_floats           # that module sits above this one
    w = w_cl(w)
    K, C, R, S = w.shape
    rec = amax_slot(w.device)
    wt = torch.empty(wt_floats(K, R * S, C), device=w.device, dtype=torch.float32)
    wsp, wtsp = torch.empty(K * R * S * C, device=w.device, dtype=torch.float32), torch.empty_like(wt)
    r1, tiles = table_row(w.data_ptr(), K, R * S, C, 0, rec.data_ptr(), wt.data_ptr())
    r2, _ = table_row(w.data_ptr(), K, R * S, C, 0, rec.data_ptr(), wtsp.data_ptr(), wsp.data_ptr())
    t1, t2 = (torch.tensor([r], dtype=torch.int64, device=w.device) for r in (r1, r2))
    call('dsrl_conv2d_transpose_filters_batched', t1.data_ptr(), 1, tiles, _stream())
    call('dsrl_conv2d_split_filters_batched', t2.data_ptr(), 1, tiles, _stream())
    return rec, wsp, wtsp, wt


def planes_of(data, ld, amax, nplanes=2):
    """fp16 planes (include/dsrl_hip.h: dsrl_split_planes) of the pixel-major tensor `data` (N,C,H,W; pixel stride ld), scaled by the amax record
    `amax`: a uint8 buffer holding [P][ld] fp16 first terms and, dsrl_planes_lo_offset(P * ld) bytes further, the second terms."""
    N, Cc, H, W = data.shape
    P = N * H * W
    buf = torch.empty(int(cquery('dsrl_planes_bytes', P * ld, nplanes)), device=data.device, dtype=torch.uint8)
    call('dsrl_split_planes', data.data_ptr(), ld, P, Cc, amax.data_ptr(), buf.data_ptr(), nplanes, _stream())
    return buf


# fp16 planes of activation operands (round 4): 'off' = never, 'all' = a standalone split pass for every eligible operand that does not carry
# planes yet, 'auto' (default) = the split pass only where it pays by itself (tensors of >= DSRL_PLANES_MIN_ELEMS elements: the 65536-pixel decoder
# operands; a split launch costs ~6 us on the small ones, more than the planes kernel gains there) - producers that write planes beside their
# fp32 output are used in every mode but 'off'
planes_mode = knob('DSRL_PLANES_MODE', 'auto')
if planes_mode == 'off':
    os.environ.setdefault('DSRL_PLANES', '0')       # the library's planner then keeps the f16x3 forward off the 256x256 tile, whose register-staged build spills
planes_min_elems = knob('DSRL_PLANES_MIN_ELEMS', 8 << 20)
# Round 5: the reduced-precision 'f16x1' arithmetic (apex O1 / O2) takes ONE plane per operand - the conv a 2-byte storage format would run.  A one-plane split
# pass moves 6 instead of 8 bytes per element and the conv gains more (tools/fp16_slice.py at config 5's shapes: cat_conv.0 forward 593 -> 406 us, dgrad
# 772 -> 547 us; layer3 3x3 48 -> 35 us), so the pass pays from 2 Mi elements on, and for the data gradients of the >= 8 Mi-element operands as well.
planes_min_elems_x1 = knob('DSRL_PLANES_MIN_ELEMS_X1', 2 << 20)


def _planes_npl():
    """planes per operand of the current arithmetic: 2 (f16x3), 1 (f16x1), 0 (no plane operands)"""
    return {4: 2, 5: 1}.get(_conv_precision_code(), 0)


def planes_wanted(data, ld, C, K, taps=9):
    """Would a conv with this activation operand take planes if its filter had them? (planes_mode 'auto' / 'all'; both channel counts multiples of 8;
    'auto': long K loops over large operands only - the 3x3 decoder convs)"""
    npl = _planes_npl()
    if planes_mode == 'off' or not npl or C % 8 or K % 8 or ld % 8 or data.data_ptr() % 16:
        return False
    N, Cc, H, W = data.shape
    return planes_mode == 'all' or (N * H * W * Cc >= (planes_min_elems if npl == 2 else planes_min_elems_x1) and taps >= 9)


def planes_for(t, data, ld, amax, taps=9, split_ok=True):
    """fp16 planes of operand tensor `t` (pixel-major copy `data`, pixel stride ld) scaled by ITS record `amax`, or None: the planes the tensor
    carries (left by its producer or by an earlier consumer of the same tensor in this step), else a split pass when planes_mode allows one."""
    npl = _planes_npl()
    if planes_mode == 'off' or amax is None or not npl:
        return None
    gen = getattr(amax, '_dsrl_gen', -1)          # a step-arena record is re-issued (same address) by the next step: its generation is part of the key
    have = getattr(t, '_dsrl_planes', None)
    if (have is not None and have[1] == ld and have[2] == amax.data_ptr() and have[3] == data.data_ptr() and have[4] == t._version and have[5] == gen and
            have[6] >= npl):
        return have[0]
    N, Cc, H, W = data.shape
    if Cc % 8 or ld % 8 or data.data_ptr() % 16:
        return None
    if planes_mode != 'all' and (N * H * W * Cc < (planes_min_elems if npl == 2 else planes_min_elems_x1) or taps < 9 or not split_ok):
        return None
    buf = planes_of(data, ld, amax, npl)
    try:
        t._dsrl_planes = (buf, ld, amax.data_ptr(), data.data_ptr(), t._version, gen, npl)
        _planes_holders.append(weakref.ref(t))
    except Exception:           # noqa: BLE001
        pass
    return buf


# Tensors that carry cached planes.  The planes are as large as the fp32 tensor, the tensor is saved for backward, and in 'auto' mode no backward
# kernel reads x planes (weight gradients read fp32 x): without a release every large decoder operand would keep a dead full-size copy until its
# backward node ran (~1.3 GB for the 304-channel concat at 512x1024, B=8: ADVICE round 4).  drop_planes() runs when the forward consumers are
# done - at the root of backward (fused_losses_backward) and at the end of the step.
_planes_holders = []


def drop_planes():
    for r in _planes_holders:
        t = r()
        if t is not None and hasattr(t, '_dsrl_planes'):
            try:
                del t._dsrl_planes
            except Exception:           # noqa: BLE001
                pass
    _planes_holders.clear()


def filter_planes(w, rec):
    """(w_planes [K][R][S][C], wt_planes [C][R][S][K]) of one filter, scaled by its amax record `rec`: what filter_operands.FilterOperands prepares
    for the filters of a plane set (dsrl_conv2d_filter_planes_batched), here for a single tensor.  K and C must be multiples of 8."""
    from .filter_operands import table_row
    w = w_cl(w)
    K, C, R, S = w.shape
    nbytes = int(cquery('dsrl_planes_bytes', K * R * S * C, 2))
    wp = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    wtp = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    row, tiles = table_row(w.data_ptr(), K, R * S, C, 0, rec.data_ptr(), wtp.data_ptr(), wp.data_ptr(), pad_k=False)
    t = torch.tensor([row], dtype=torch.int64, device=w.device)
    call('dsrl_conv2d_filter_planes_batched', t.data_ptr(), 1, tiles, _stream())
    return wp, wtp


def _is_krsc(w):
    """Is the (K,C,R,S) filter physically [K][R][S][C]?  (torch does not call plain-strided 1x1 filters channels_last although the
    two layouts coincide for them)"""
    return w.is_contiguous(memory_format=CL) or (w.shape[2] == 1 and w.shape[3] == 1 and w.is_contiguous())


def w_cl(w):
    _need_gpu(w); _f32(w)
    return w if _is_krsc(w) else w.contiguous(memory_format=CL)


def _out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


_rng_state = {'seed': 0x5EED, 'step': 0, 'current': 0}


def set_dropout_seed(seed):
    """Base key of the Philox dropout generator; every forward pass (begin_forward) derives its own key from it."""
    _rng_state['seed'] = int(seed) & 0xFFFFFFFFFFFF
    _rng_state['step'] = 0


def _derive(step):
    return (_rng_state['seed'] * 1000003 + step) & 0xFFFFFFFFFFFFFFFF


def peek_next_seed():
    return _derive(_rng_state['step'] + 1)


def begin_forward(training=True):
    """Called once per model forward: all Dropout modules of that pass share one key and differ by stream id.  An evaluation pass draws no mask
    and does not advance the key (torch's generator is not consumed by eval-mode Dropout either): the key sequence of the training steps is the
    same with and without validation passes in between, and the same for eager launches and for a graph whose key lives on the device."""
    if not training:
        return _rng_state['current']
    _rng_state['step'] += 1
    _rng_state['current'] = _derive(_rng_state['step'])
    return _rng_state['current']


def current_seed():
    return _rng_state['current']


# ------------------------------------------------------------------------------------------------ shared gradient buffers
# A tensor that feeds two branches (the input of a ResNet bottleneck: conv1 and the residual add / the downsample conv) receives two
# gradient contributions that autograd would sum with an extra elementwise kernel.  With a GradSlot the first contribution's buffer
# is published and the later data-gradient kernel accumulates into it in its epilogue (dsrl_conv2d_dgrad_accumulate) and reports
# no gradient of its own.  Only sound when EVERY consumer of the tensor takes part, hence fork(): an alias node whose output is
# consumed inside the block only; other users of the original tensor see one ordinary gradient.  Any case the protocol does not
# cover falls back to returning a separate gradient (closed slot), which autograd sums as usual.
grad_slots_enabled = knob('DSRL_GRAD_SLOTS', True)
# one slot for the three consumers of layer1's output (ResNet101.forward / DSRL.forward_head, round 5)
outer_grad_slot = knob('DSRL_OUTER_SLOT', True)


class GradSlot:
    __slots__ = ('buf', 'closed', 'link')

    def __init__(self):
        self.buf, self.closed = None, False
        self.link = None            # the BNLink whose backward sums the LAST contributor leaves (set where both are created); a contributor without
                                    # that link arriving after the sums exist withdraws them (they would miss its part of the gradient)


# Backward counterpart of conv2d_bn_act: when y = relu(bn(x)) feeds exactly one conv, that conv's data-gradient kernel produces the
# gradient of y in registers and can leave the BatchNorm-backward partial sums with it (dsrl_conv2d_dgrad_bnstats); the BN backward
# then runs as one streaming kernel (dsrl_bn_bwd_from_stats).  A BNLink carries what the conv needs from the BN's forward and the
# partials back; the BN only trusts them if the gradient it receives is the very buffer that conv wrote.
bn_bwd_stats_enabled = knob('DSRL_BN_BWD_STATS', True)
# the same for bn3 via the next block's accumulating dgrad.  Rounds 3-4: correct but slower (the wide 1x1 data gradients spent 11-17 us in an epilogue of
# 4-byte loads of x / y).  Round 5: on since that epilogue reads float4 rows through LDS (conv_split_kernel.h, bn_fast): +0.65 % step throughput, 29 of the 45
# device-wide-barrier BatchNorm launches become streaming from-sums launches (profiles/round5_ab.txt)
bn_bwd_stats_shared = knob('DSRL_BN_BWD_STATS_SHARED', True)
# Backward needs y = relu(bn(x)) only for the test y > 0.  The from-statistics forward leaves that bit per element (uint32 [C / 32][P], dsrl_bn_train_fwd_from_stats_mask)
# and the from-statistics backward and the linked data-gradient epilogues read it instead of y (relu == 2): a 32nd of the bytes, the same gradients bit for bit.
# 0: no mask is allocated and backward reads y.
bn_mask_enabled = knob('DSRL_BN_MASK', True)


class BNLink:
    __slots__ = ('x', 'y_ptr', 'y_shape', 'mean', 'invstd', 'relu', 'valid', 'stats', 'parts', 'dx_ptr', 'shared', 'drop_p', 'mask')

    def __init__(self, shared=False):
        self.x = self.mean = self.invstd = self.stats = None      # the BN output itself is NOT kept (it may carry this link: no cycles)
        self.y_ptr, self.y_shape = 0, None
        self.relu, self.valid, self.parts, self.dx_ptr = False, False, 0, 0
        self.shared = shared        # y feeds the two consumers of a GradSlot: the accumulating (= last) dgrad completes its gradient
        self.drop_p = 0.0           # a Dropout(p) behind the BN's ReLU (round 5): y is the tensor behind it, its zeros are the combined mask
        self.mask = None            # the sign mask of y the forward left (bn_mask_enabled), or None: the data gradient reads y; P * C / 8 bytes kept
                                    # alive until the next forward overwrites the link


class _Fork(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g


def fork(x):
    y = _Fork.apply(x)
    a = carried_amax(x)
    if a is not None:
        set_amax(y, a)              # the alias holds the same values: it keeps the magnitude record of the tensor it aliases
    return y


# ------------------------------------------------------------------------------------------------ conv2d
class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil, gslot=None, stats_parts=0, in_link=None):
        ctx.set_materialize_grads(False)       # no zero tensor for the (non-differentiable) statistics output's gradient
        ctx.gslot = gslot
        ctx.in_link = in_link
        x_in = x
        x, ldx = pm_vec4(x)
        w_param = w
        w = w_cl(w)
        N, Cc, H, W = x.shape
        K, Cw, R, S = w.shape
        if Cw != Cc:
            raise DsrlHipError(f'conv2d: input has {Cc} channels, weight expects {Cw}')
        Ho, Wo = _out_size(H, R, stride, pad, dil), _out_size(W, S, stride, pad, dil)
        y = new_cl((N, K, Ho, Wo), x)
        shp = (N, H, W, Cc, K, R, S, stride, pad, dil)
        ws = _ws(cquery('dsrl_conv2d_fwd_workspace_bytes', *shp), x)
        if bias is not None:
            _need_gpu(bias)
        stats = None
        xa = wa = None
        if f16_mode():              # operand magnitudes of the f16x3 arithmetic (the library measures what it is not given)
            xa = amax_for(x_in, x, ldx)
            wa = _weight_amax(w_param)
        ctx.amax = (xa, wa)
        if stats_parts > 0:         # BatchNorm partials of y from the conv epilogue (include/dsrl_hip.h: dsrl_conv2d_fwd_stats)
            stats = torch.empty(cquery('dsrl_bn_stats_floats', 3, int(stats_parts), K), device=x.device, dtype=torch.float32)
        wsp = _weight_split(w_param) if wa is not None else None        # the filter pre-split by its FilterOperands (same step, same record)
        wpl = _weight_planes(w_param) if wa is not None else None       # ... and as fp16 planes; with planes of x the launch stages by LDS-DMA
        if wpl is None and wa is not None and planes_wanted(x, ldx, Cc, K, R * S):
            w_param._dsrl_want_planes = True            # ddp.FlatParams adds this filter to a plane set at the next step
        xp = planes_for(x_in, x, ldx, xa, R * S) if wpl is not None else None
        call('dsrl_conv2d_fwd_planes', x.data_ptr(), ldx, None if xa is None else xa.data_ptr(), None if xp is None else xp.data_ptr(), w.data_ptr(),
             None if wa is None else wa.data_ptr(), None if wsp is None else wsp.data_ptr(), None if wpl is None else wpl.data_ptr(),
             None if bias is None else bias.data_ptr(), y.data_ptr(), K, *shp, ws.data_ptr(), ws.numel(),
             None if stats is None else stats.data_ptr(), int(stats_parts), _stream())
        ctx.save_for_backward(x, w)
        ctx.shp = shp
        ctx.has_bias = bias is not None
        ctx.bparam = bias if isinstance(bias, torch.nn.Parameter) else None
        ctx.wparam = w_param if isinstance(w_param, torch.nn.Parameter) else None
        if stats is not None:
            ctx.mark_non_differentiable(stats)
            return y, stats
        return y

    @staticmethod
    def backward(ctx, dy, *_unused):
        if dy is None:
            return (None,) * 9
        x, w = ctx.saved_tensors
        shp = ctx.shp
        N, H, W, Cc, K, R, S, stride, pad, dil = shp
        dy_in = dy
        dy, lddy = pm_vec4(dy)
        ldx = _ld_of(x)
        dx = dw = db = None
        st = _stream()
        xa, wa = ctx.amax
        dya = None
        if f16_mode():
            dya = amax_for(dy_in, dy, lddy)          # one measurement for the data and the weight gradient
            if xa is None:
                xa = amax_for(x, x, ldx)
            if wa is not None and ctx.wparam is not None and _weight_amax(ctx.wparam) is None:
                wa = None                             # the filter changed since its magnitude was taken
        p_ = lambda t_: None if t_ is None else t_.data_ptr()       # noqa: E731
        wtsp = _weight_split(ctx.wparam, True) if (wa is not None and ctx.wparam is not None) else None
        wtpl = _weight_planes(ctx.wparam, True) if (wa is not None and ctx.wparam is not None) else None
        # 'auto' never pays a split pass for a gradient (measured: the data-gradient launches gain less than the pass costs); planes a producer left are used
        # f16x1 (round 5): the one-plane split of a large gradient does pay (cat_conv.0 dgrad 772 -> 547 us at config 5's size for a ~60 us pass)
        dy_split_ok = planes_mode == 'all' or (_planes_npl() == 1 and dy.shape[0] * dy.shape[1] * dy.shape[2] * dy.shape[3] >= planes_min_elems)
        dyp = planes_for(dy_in, dy, lddy, dya, R * S, split_ok=dy_split_ok) if (wtpl is not None and ctx.needs_input_grad[0] and stride == 1 and K % 8 == 0) else None
        if ctx.needs_input_grad[1]:
            sink = _sink(ctx.wparam) if ctx.wparam is not None and _is_krsc(ctx.wparam) else None
            if sink is not None and wgrad_queue is not None:
                # deferred: all weight gradients of this backward pass run as a few grouped grids when the pass is over
                wp = ctx.wparam
                wgrad_queue.add(x, ldx, dy, lddy, sink, shp, lambda wp=wp: wp._dsrl_arena.written(wp), xa, dya)
            elif sink is not None and overlap_wgrad and ctx.needs_input_grad[0]:
                cur, side = torch.cuda.current_stream(), side_stream(x.device)
                side.wait_stream(cur)                                   # dy (and x) are ready on the compute stream
                with torch.cuda.stream(side):
                    ws = _ws(cquery('dsrl_conv2d_wgrad_workspace_bytes', *shp), x)
                    call('dsrl_conv2d_wgrad_amax', x.data_ptr(), ldx, p_(xa), dy.data_ptr(), lddy, p_(dya), sink.data_ptr(), *shp, ws.data_ptr(), ws.numel(), side.cuda_stream)
                x.record_stream(side); dy.record_stream(side)
                ctx.wparam._dsrl_arena.written(ctx.wparam, side)
            else:
                dw = sink if sink is not None else torch.empty((K, Cc, R, S), device=x.device, dtype=torch.float32, memory_format=CL)
                ws = _ws(cquery('dsrl_conv2d_wgrad_workspace_bytes', *shp), x)
                call('dsrl_conv2d_wgrad_amax', x.data_ptr(), ldx, p_(xa), dy.data_ptr(), lddy, p_(dya), dw.data_ptr(), *shp, ws.data_ptr(), ws.numel(), st)
                if sink is not None:
                    ctx.wparam._dsrl_arena.written(ctx.wparam)
                    dw = None
        if ctx.needs_input_grad[0]:
            slot = ctx.gslot
            acc = (slot is not None and not slot.closed and slot.buf is not None and tuple(slot.buf.shape) == (N, Cc, H, W)
                   and slot.buf.is_contiguous(memory_format=CL))
            dx = slot.buf if acc else new_cl((N, Cc, H, W), x)
            if slot is not None and slot.link is not None and slot.link is not ctx.in_link and slot.link.stats is not None:
                slot.link.stats = None      # sums left by an earlier contributor do not contain this gradient: that BatchNorm takes its own path
            ws = _ws(cquery('dsrl_conv2d_dgrad_workspace_bytes', *shp), x)
            wt_ptr = None
            if ctx.wparam is not None:
                # ddp.FlatParams keeps a transposed copy of every filter, refreshed by one batched launch per training step
                h = getattr(ctx.wparam, '_dsrl_operands', None)
                wt = None if h is None else h[0].fp32_transpose(h[1])
                if wt is not None:
                    wt_ptr = wt.data_ptr()
            link = ctx.in_link
            parts = 0
            # only the launch that completes the gradient may produce the sums: a plain dgrad when x has this single consumer, or the
            # accumulating dgrad that adds the last contribution to a shared buffer (GradSlot with two consumers)
            final = (not acc and ctx.gslot is None) or (acc and getattr(link, 'shared', False))
            if (link is not None and link.valid and final and link.y_ptr == x.data_ptr() and link.y_shape == (N, Cc, H, W) and Cc % 32 == 0):
                parts = int(query('dsrl_conv2d_dgrad_stats_parts', *shp))
            if parts > 0:
                # x is y = relu(bn(.)) of a BatchNorm that feeds only this conv: leave its backward partial sums with the data gradient
                bstats = torch.empty(cquery('dsrl_bn_stats_floats', 2, parts, Cc), device=x.device, dtype=torch.float32)
                _, bld = pm(link.x)
                # the BatchNorm's ReLU mask: its sign bits when the forward left them (relu == 2: pointer and row length of the mask), else y itself
                ym = (link.mask.data_ptr(), N * H * W, 2) if (link.mask is not None and link.relu) else (x.data_ptr(), ldx, int(link.relu))
                call('dsrl_conv2d_dgrad_planes_drop', dy.data_ptr(), lddy, p_(dya), p_(dyp), w.data_ptr(), wt_ptr, p_(wa), p_(wtsp), p_(wtpl), dx.data_ptr(), Cc, *shp,
                     ws.data_ptr(), ws.numel(), link.x.data_ptr(), bld, ym[0], ym[1], link.mean.data_ptr(), link.invstd.data_ptr(), ym[2],
                     float(link.drop_p), bstats.data_ptr(), parts, int(acc), st)
                link.stats, link.parts, link.dx_ptr = bstats, parts, dx.data_ptr()
            else:
                call('dsrl_conv2d_dgrad_planes', dy.data_ptr(), lddy, p_(dya), p_(dyp), w.data_ptr(), wt_ptr, p_(wa), p_(wtsp), p_(wtpl), dx.data_ptr(), Cc, *shp,
                     ws.data_ptr(), ws.numel(), None, 0, None, 0, None, None, 0, None, 0, int(acc), st)
            if acc:
                dx = None                   # the contribution went into the buffer autograd already holds for this input
            elif slot is not None:
                if slot.buf is None:
                    slot.buf = dx
                else:
                    slot.closed = True      # a separate gradient is on its way to autograd: nobody may touch the published buffer any more
        if ctx.has_bias and ctx.needs_input_grad[2]:
            P = dy.shape[0] * dy.shape[2] * dy.shape[3]
            bsink = _sink_flat(ctx.bparam, K)
            db = bsink if bsink is not None else torch.empty(K, device=x.device, dtype=torch.float32)
            ws = _ws(cquery('dsrl_colsum_workspace_bytes', P, K), x)
            call('dsrl_colsum', dy.data_ptr(), lddy, P, K, db.data_ptr(), ws.data_ptr(), ws.numel(), st)
            if bsink is not None:
                _sunk(ctx.bparam); db = None
            else:
                db = _deliver(ctx.bparam, db)
        if dw is not None:
            dw = _deliver(ctx.wparam, dw)
        return dx, dw, db, None, None, None, None, None, None


class _StemConv(torch.autograd.Function):
    """kernel-R x kernel-S, stride-s conv of a few-channel image (the 7x7/2 RGB stem, ResNet101.py:28) as a row-folded
    implicit GEMM: the image is zero-padded physically to 4 channels and `pad` pixels, and the S (rounded up to 8) horizontal
    taps x 4 channels of one filter row form one contiguous 32-float K chunk."""

    @staticmethod
    def forward(ctx, x, w, stride, pad):
        _need_gpu(x, w); _f32(x); _f32(w)
        N, Cc, H, W = x.shape
        K, _, R, S = w.shape
        Sp = (S + 7) & ~7 if S > 4 else 4
        Cf = Sp * 4
        Ho, Wo = _out_size(H, R, stride, pad, 1), _out_size(W, S, stride, pad, 1)
        Hp = max(H + 2 * pad, (Ho - 1) * stride + R)
        Wp = max(W + 2 * pad, (Wo - 1) * stride + Sp) + 1
        st = _stream()
        xp = torch.empty((N, Hp, Wp, 4), device=x.device, dtype=torch.float32)
        sn, sc, sh, sw = x.stride()
        call('dsrl_pad_image_nhwc', x.data_ptr(), sn, sc, sh, sw, xp.data_ptr(), N, Cc, H, W, 4, pad, pad, Hp, Wp, st)
        # zero-padded [K][R][Sp][4] copy of the filter: the padding never changes, so the buffer is kept with the weight and only the filter taps are
        # re-copied (one launch instead of a fill + a copy per step)
        w2 = getattr(w, '_dsrl_stem_pad', None)
        if w2 is None or tuple(w2.shape) != (K, R, Sp, 4) or w2.device != x.device:
            w2 = torch.zeros((K, R, Sp, 4), device=x.device, dtype=torch.float32)
            if isinstance(w, torch.nn.Parameter):
                w._dsrl_stem_pad = w2
        w2[:, :, :S, :Cc] = w.detach().permute(0, 2, 3, 1)
        y = new_cl((N, K, Ho, Wo), x)
        macs = cquery('dsrl_conv2d_inbounds_macs', N, H, W, Cc, K, R, S, stride, pad, 1)
        shp = (N, Hp, Wp, Cf, K, R, stride, Ho, Wo)
        ws = _ws(cquery('dsrl_conv2d_rowfold_fwd_workspace_bytes', *shp), x)
        call('dsrl_conv2d_rowfold_fwd', xp.data_ptr(), 4, w2.data_ptr(), None, y.data_ptr(), K, *shp, macs, ws.data_ptr(), ws.numel(), st)
        ctx.save_for_backward(xp)
        ctx.cfg = (shp, macs, tuple(w.shape), Sp)
        ctx.wparam = w if isinstance(w, torch.nn.Parameter) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        xp, = ctx.saved_tensors
        shp, macs, wshape, Sp = ctx.cfg
        K, Cc, R, S = wshape
        if ctx.needs_input_grad[0]:
            raise DsrlHipError('the image stem has no input-gradient kernel (the reference never differentiates w.r.t. the image)')
        dy, lddy = pm_vec4(dy)
        dw2 = torch.empty((K, R, Sp, 4), device=dy.device, dtype=torch.float32)
        ws = _ws(cquery('dsrl_conv2d_rowfold_wgrad_workspace_bytes', *shp), dy)
        call('dsrl_conv2d_rowfold_wgrad', xp.data_ptr(), 4, dy.data_ptr(), lddy, dw2.data_ptr(), *shp, macs, ws.data_ptr(), ws.numel(), _stream())
        dw = _deliver(ctx.wparam, dw2[:, :, :S, :Cc].permute(0, 3, 1, 2))
        return None, dw, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, grad_slot=None, in_link=None):
    """nn.Conv2d arithmetic (square stride/padding/dilation) on the MFMA implicit-GEMM kernels."""
    if grad_slot is not None and x.shape[1] % 4 != 0:
        grad_slot.closed = True             # the padded-channel fallback reports its own gradient: the shared buffer must not be used
        grad_slot = None
    if x.shape[1] < 4 and bias is None and dilation == 1 and not x.requires_grad:
        return _StemConv.apply(x, weight, int(stride), int(padding))
    if x.shape[1] % 4 != 0:
        padc = 4 - x.shape[1] % 4           # generic fallback: pad input and filter channels to a multiple of 4 (zeros contribute nothing)
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, padc))
        weight = torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, padc))
    if in_link is not None and x.shape[1] % 4 == 0 and bn_bwd_stats_enabled:
        return _Conv2d.apply(x, weight, bias, int(stride), int(padding), int(dilation), grad_slot, 0, in_link)
    return _Conv2d.apply(x, weight, bias, int(stride), int(padding), int(dilation), grad_slot)


# ------------------------------------------------------------------------------------------------ BatchNorm (+res, relu, dropout)
class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, relu, drop_p, seed, rng_stream, residual, rslot=None,
                stats=None, stats_parts=0, out_link=None, res_link=None):
        ctx.rslot = rslot
        ctx.out_link = out_link
        # the residual is the output of a BatchNorm without ReLU (downsample branch) that feeds only this add: our backward leaves that BatchNorm's sums
        ctx.res_link = res_link if (res_link is not None and res_link.valid and not res_link.relu and residual is not None
                                    and res_link.y_ptr == residual.data_ptr() and res_link.y_shape == tuple(x.shape)) else None
        x, ldx = pm(x)
        _need_gpu(gamma, beta, running_mean, running_var)
        N, Cc, H, W = x.shape
        P = N * H * W
        st = _stream()
        y = new_cl((N, Cc, H, W), x)
        # f16x3 conv arithmetic: the kernel leaves max |y| while it writes y (functional.amax_for finds it on the tensor)
        ya = amax_slot(x.device) if f16_mode() else None
        ya_ptr = None if ya is None else ya.data_ptr()
        res_ptr, ldr = None, 0
        if residual is not None:
            residual, ldr = pm(residual)
            res_ptr = residual.data_ptr()
        mask = None                 # sign bits of y, left by the from-statistics forward behind a ReLU (bn_mask_enabled)
        if training:
            if P <= 1:
                raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
            ws = _ws(cquery('dsrl_bn_workspace_bytes', P, Cc), x)
            mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
            invstd = torch.empty_like(mean)
            if stats is not None and stats_parts > 0:
                if relu and bn_mask_enabled and Cc % 32 == 0:
                    mask = torch.empty(cquery('dsrl_bn_mask_words', P, Cc), device=x.device, dtype=torch.int32)
                call('dsrl_bn_train_fwd_from_stats' if mask is None else 'dsrl_bn_train_fwd_from_stats_mask', x.data_ptr(), ldx, y.data_ptr(), Cc, P, Cc,
                     float(eps), float(momentum), mean.data_ptr(), invstd.data_ptr(),
                     None if running_mean is None else running_mean.data_ptr(), None if running_var is None else running_var.data_ptr(),
                     gamma.data_ptr(), beta.data_ptr(), res_ptr, ldr, int(relu), float(drop_p), int(seed), int(rng_stream),
                     stats.data_ptr(), int(stats_parts), ya_ptr, *(() if mask is None else (mask.data_ptr(),)), st)
            else:
                call('dsrl_bn_train_fwd', x.data_ptr(), ldx, y.data_ptr(), Cc, P, Cc, float(eps), float(momentum), mean.data_ptr(), invstd.data_ptr(),
                     None if running_mean is None else running_mean.data_ptr(), None if running_var is None else running_var.data_ptr(),
                     gamma.data_ptr(), beta.data_ptr(), res_ptr, ldr, int(relu), float(drop_p), int(seed), int(rng_stream),
                     ws.data_ptr(), ws.numel(), ya_ptr, st)
        else:
            mean = running_mean
            invstd = frozen_invstd(running_var, eps)
            if invstd is None:
                invstd = torch.empty(Cc, device=x.device, dtype=torch.float32)
                call('dsrl_bn_invstd_from_var', running_var.data_ptr(), Cc, float(eps), invstd.data_ptr(), st)
            call('dsrl_bn_apply', x.data_ptr(), ldx, y.data_ptr(), Cc, P, Cc, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                 res_ptr, ldr, int(relu), float(drop_p), int(seed), int(rng_stream), ya_ptr, st)
        if ya is not None:
            set_amax(y, ya)
        ctx.save_for_backward(x, y, mean, invstd, gamma)
        ctx.mask = mask
        if out_link is not None and (drop_p == 0.0 or relu) and Cc % 32 == 0 and ldx == Cc:
            out_link.x, out_link.mean, out_link.invstd, out_link.relu, out_link.valid = x, mean, invstd, bool(relu), True
            out_link.mask = mask
            out_link.y_ptr, out_link.y_shape, out_link.drop_p = y.data_ptr(), tuple(y.shape), float(drop_p)
        ctx.cfg = (bool(training), bool(relu), float(drop_p), residual is not None)
        ctx.gb = (gamma, beta) if isinstance(gamma, torch.nn.Parameter) and isinstance(beta, torch.nn.Parameter) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, invstd, gamma = ctx.saved_tensors
        training, relu, drop_p, has_res = ctx.cfg
        dy, lddy = pm(dy)
        _, ldx = pm(x)
        N, Cc, H, W = x.shape
        P = N * H * W
        dx = new_cl((N, Cc, H, W), x)
        dres = new_cl((N, Cc, H, W), x) if has_res else None
        sg = sb = None
        if ctx.gb is not None and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
            sg = _sink(ctx.gb[0])
            sb = _sink(ctx.gb[1]) if sg is not None else None
        dgamma = sg if sg is not None else torch.empty(Cc, device=x.device, dtype=torch.float32)
        dbeta = sb if sb is not None else torch.empty(Cc, device=x.device, dtype=torch.float32)
        dxa = amax_slot(x.device) if f16_mode() else None       # max |dx|, left by the kernel: dx is the dy operand of the conv in front of this BN
        dxa_ptr = None if dxa is None else dxa.data_ptr()
        link = ctx.out_link
        if link is not None and link.stats is not None and link.dx_ptr == dy.data_ptr() and lddy == Cc and (drop_p == 0.0 or relu):
            # the gradient we received is the buffer the consuming conv's dgrad wrote, and it left our two per-channel sums with it
            rl = ctx.res_link
            ym = (ctx.mask.data_ptr(), P, 2) if (ctx.mask is not None and relu) else (y.data_ptr(), Cc, int(relu))       # relu == 2: the sign mask and its row length in y's place
            rparts = int(query('dsrl_bn_bwd_from_stats_res_parts', P, Cc, int(link.parts))) if (rl is not None and dres is not None and bn_res_stats_enabled) else 0
            if rparts > 0:
                # ... and the masked gradient we write to dres is the output gradient of the downsample branch's BatchNorm: leave its sums as well
                rstats = torch.empty(cquery('dsrl_bn_stats_floats', 2, rparts, Cc), device=x.device, dtype=torch.float32)
                _, rld = pm(rl.x)
                call('dsrl_bn_bwd_from_stats_res', x.data_ptr(), ldx, ym[0], ym[1], dy.data_ptr(), lddy, dx.data_ptr(), Cc, dres.data_ptr(), Cc, P, Cc,
                     mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ym[2], float(drop_p), int(training),
                     link.stats.data_ptr(), int(link.parts), dxa_ptr, rl.x.data_ptr(), rld, rl.mean.data_ptr(), rl.invstd.data_ptr(), rstats.data_ptr(), rparts, _stream())
                rl.stats, rl.parts, rl.dx_ptr = rstats, rparts, dres.data_ptr()
            else:
                call('dsrl_bn_bwd_from_stats_drop', x.data_ptr(), ldx, ym[0], ym[1], dy.data_ptr(), lddy, dx.data_ptr(), Cc,
                     None if dres is None else dres.data_ptr(), Cc, P, Cc, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                     dgamma.data_ptr(), dbeta.data_ptr(), ym[2], float(drop_p), int(training), link.stats.data_ptr(), int(link.parts), dxa_ptr, _stream())
        else:
            ws = _ws(cquery('dsrl_bn_workspace_bytes', P, Cc), x)
            call('dsrl_bn_bwd', x.data_ptr(), ldx, y.data_ptr(), Cc, dy.data_ptr(), lddy, dx.data_ptr(), Cc,
                 None if dres is None else dres.data_ptr(), Cc, P, Cc, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                 dgamma.data_ptr(), dbeta.data_ptr(), int(relu), drop_p, int(training), ws.data_ptr(), ws.numel(), dxa_ptr, _stream())
        if dxa is not None:
            set_amax(dx, dxa)
        if sg is not None:
            ctx.gb[0]._dsrl_arena.written(ctx.gb[0]); dgamma = None
        if sb is not None:
            ctx.gb[1]._dsrl_arena.written(ctx.gb[1]); dbeta = None
        if dres is not None and ctx.rslot is not None:
            if ctx.rslot.buf is None:
                ctx.rslot.buf = dres            # published: a later dgrad of the same input accumulates into it (GradSlot)
            else:
                ctx.rslot.closed = True
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None, dres, None, None, None, None, None


bn_res_stats_enabled = knob('DSRL_BN_RES_STATS', True)      # 0: the downsample BatchNorm reduces its own backward sums (until round 5)


def frozen_invstd(running_var, eps):
    """1 / sqrt(var + eps) of an eval-mode BatchNorm as inference.FrozenOperands computed it once (by dsrl_bn_invstd_from_var: the same bits), if one
    is attached to the buffer and still describes it - else None, and the caller launches that kernel itself."""
    held = getattr(running_var, '_dsrl_invstd', None)
    if held is not None and held[1] == float(eps) and held[2] == running_var._version and held[0].device == running_var.device:
        return held[0]
    return None


def batch_norm_act(x, bn, relu=False, drop_p=0.0, seed=0, rng_stream=0, residual=None, residual_grad_slot=None, stats=None, out_link=None, res_link=None):
    """BatchNorm2d `bn` (an nn.BatchNorm2d holding the parameters/buffers) + optional residual add, ReLU, Dropout."""
    training = bn.training or bn.running_mean is None
    if training and bn.running_mean is not None:
        bn._dsrl_batches = getattr(bn, '_dsrl_batches', 0) + 1      # flushed into num_batches_tracked by HipBatchNorm2d.state_dict
        if getattr(bn.running_var, '_dsrl_invstd', None) is not None:
            bn.running_var._dsrl_invstd = None                      # the kernel rewrites the statistics through a raw pointer: a frozen invstd is stale
    momentum = 0.1 if bn.momentum is None else bn.momentum
    return _BNAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps, relu,
                        drop_p if training or drop_p == 0.0 else 0.0, seed, rng_stream, residual, residual_grad_slot if residual is not None else None,
                        stats[0] if (stats is not None and training) else None, stats[1] if (stats is not None and training) else 0,
                        out_link if bn_bwd_stats_enabled else None, res_link if (bn_bwd_stats_enabled and residual is not None) else None)


# BatchNorm statistics from the conv epilogue: the conv that feeds a training-mode BN leaves (n, mean, M2) partials of its output, and
# the BN becomes one streaming kernel without a statistics pass (dsrl_conv2d_fwd_stats + dsrl_bn_train_fwd_from_stats)
conv_bn_stats_enabled = knob('DSRL_CONV_BN_STATS', True)


def conv2d_bn_act(x, weight, bias, stride, padding, dilation, bn, relu=False, drop_p=0.0, seed=0, rng_stream=0, residual=None,
                  grad_slot=None, residual_grad_slot=None, in_link=None, out_link=None, res_link=None):
    """batch_norm_act(conv2d(x, ...), bn, ...) with the BN batch statistics taken from the conv epilogue when the launch can provide
    them (split-precision kernels, no split-K, <= 256 row blocks, out channels a multiple of 32)."""
    training = bn.training or bn.running_mean is None
    K, C = weight.shape[0], x.shape[1]
    if conv_bn_stats_enabled and training and x.is_cuda and C % 4 == 0 and K % 32 == 0:
        N, _, H, W = x.shape
        parts = int(query('dsrl_conv2d_fwd_stats_parts', N, H, W, C, K, weight.shape[2], weight.shape[3], int(stride), int(padding), int(dilation)))
        if parts > 0:
            y, stats = _Conv2d.apply(x, weight, bias, int(stride), int(padding), int(dilation), grad_slot, parts, in_link)
            return batch_norm_act(y, bn, relu=relu, drop_p=drop_p, seed=seed, rng_stream=rng_stream, residual=residual,
                                  residual_grad_slot=residual_grad_slot, stats=(stats, parts), out_link=out_link, res_link=res_link)
    y = (_Conv2d.apply(x, weight, bias, int(stride), int(padding), int(dilation), grad_slot, 0, in_link)
         if (in_link is not None and x.is_cuda and C % 4 == 0) else conv2d(x, weight, bias, stride, padding, dilation, grad_slot=grad_slot))
    return batch_norm_act(y, bn, relu=relu, drop_p=drop_p, seed=seed, rng_stream=rng_stream, residual=residual,
                          residual_grad_slot=residual_grad_slot, out_link=out_link, res_link=res_link)


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, rng_stream):
        x, ldx = pm(x)
        N, Cc, H, W = x.shape
        y = new_cl((N, Cc, H, W), x)
        call('dsrl_dropout_fwd', x.data_ptr(), ldx, y.data_ptr(), Cc, N * H * W, Cc, float(p), int(seed), int(rng_stream), _stream())
        ctx.cfg = (float(p), int(seed), int(rng_stream))
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, rng_stream = ctx.cfg
        dy, ld = pm(dy)
        N, Cc, H, W = dy.shape
        dx = new_cl((N, Cc, H, W), dy)
        call('dsrl_dropout_bwd', dy.data_ptr(), ld, dx.data_ptr(), Cc, N * H * W, Cc, p, seed, rng_stream, _stream())
        return dx, None, None, None


def dropout(x, p, training, seed, rng_stream):
    if not training or p == 0.0:
        return x
    return _Dropout.apply(x, p, seed, rng_stream)


# ------------------------------------------------------------------------------------------------ resize / pools / concat
class _UpsampleAC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo):
        x, ldx = pm(x)
        N, Cc, H, W = x.shape
        y = new_cl((N, Cc, Ho, Wo), x)
        call('dsrl_bilinear_ac_fwd', x.data_ptr(), ldx, y.data_ptr(), Cc, N, H, W, Cc, Ho, Wo, _stream())
        ctx.shp = (N, Cc, H, W, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, Cc, H, W, Ho, Wo = ctx.shp
        dy, ld = pm(dy)
        dx = new_cl((N, Cc, H, W), dy)
        ws = _ws(cquery('dsrl_bilinear_ac_bwd_workspace_bytes', N, H, W, Cc, Ho, Wo), dy)
        call('dsrl_bilinear_ac_bwd', dy.data_ptr(), ld, dx.data_ptr(), Cc, N, H, W, Cc, Ho, Wo, ws.data_ptr(), ws.numel(), _stream())
        return dx, None, None


def upsample_bilinear_ac(x, size):
    return _UpsampleAC.apply(x, int(size[0]), int(size[1]))


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gslot=None):
        ctx.gslot = gslot
        x, ldx = pm(x)
        N, Cc, H, W = x.shape
        y = new_cl((N, Cc, 1, 1), x)
        call('dsrl_global_avgpool_fwd', x.data_ptr(), ldx, y.data_ptr(), N, H * W, Cc, _stream())
        ctx.shp = (N, Cc, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, Cc, H, W = ctx.shp
        dy = dy.contiguous().view(N, Cc)
        dx = new_cl((N, Cc, H, W), dy)
        call('dsrl_global_avgpool_bwd', dy.data_ptr(), dx.data_ptr(), Cc, N, H * W, Cc, _stream())
        slot = ctx.gslot
        if slot is not None and not slot.closed and slot.buf is None:
            slot.buf = dx           # first contribution of a shared input (GradSlot): the data gradients of the other consumers accumulate into it
        return dx, None


def global_avg_pool(x, grad_slot=None):
    """grad_slot: functional.GradSlot shared with the other consumers of x (ASPP: the four conv branches).  This op runs first in the backward pass
    (it is the last consumer in the forward), so its dense gradient becomes the shared buffer; published later it would stay a gradient of its own."""
    return _GlobalAvgPool.apply(x, grad_slot)


class _MaxPool3x3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = pm_dense(x)
        N, Cc, H, W = x.shape
        y = new_cl((N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), x)
        idx = torch.empty(y.numel(), device=x.device, dtype=torch.uint8)
        call('dsrl_maxpool3x3s2_fwd', x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, Cc, _stream())
        ctx.save_for_backward(idx)
        ctx.shp = (N, Cc, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        idx, = ctx.saved_tensors
        N, Cc, H, W = ctx.shp
        dy = pm_dense(dy)
        dx = new_cl((N, Cc, H, W), dy)
        call('dsrl_maxpool3x3s2_bwd', idx.data_ptr(), dy.data_ptr(), dx.data_ptr(), N, H, W, Cc, _stream())
        return dx


def max_pool3x3s2(x):
    return _MaxPool3x3s2.apply(x)


cat_one_launch = knob('DSRL_CAT_ONE_LAUNCH', True)       # 0: a strided copy per source + a magnitude pass by the consumer (until round 5)


class _Cat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        xs = [pm(x) for x in xs]
        N, _, H, W = xs[0][0].shape
        ctot = sum(x.shape[1] for x, _ in xs)
        y = new_cl((N, ctot, H, W), xs[0][0])
        off = 0
        st = _stream()
        n = len(xs)
        srcs = (ctypes.c_void_p * n)(*[x.data_ptr() for x, _ in xs])
        lds = (ctypes.c_int32 * n)(*[ld for _, ld in xs])
        cs = (ctypes.c_int32 * n)(*[x.shape[1] for x, _ in xs])
        if cat_one_launch and n <= 8 and query('dsrl_cat_channels_supported', srcs, lds, cs, n, y.data_ptr(), ctot, N * H * W):
            # one kernel for all sources, and it leaves the magnitude the consuming convs scale their operand by (no dsrl_amax pass over the buffer)
            ya = amax_slot(y.device) if f16_mode() else None
            call('dsrl_cat_channels', srcs, lds, cs, n, y.data_ptr(), ctot, N * H * W, None if ya is None else ya.data_ptr(), st)
            if ya is not None:
                set_amax(y, ya)
        else:
            for x, ld in xs:
                call('dsrl_copy2d', x.data_ptr(), ld, y.data_ptr() + 4 * off, ctot, N * H * W, x.shape[1], st)
                off += x.shape[1]
        ctx.sizes = [x.shape[1] for x, _ in xs]
        return y

    @staticmethod
    def backward(ctx, dy):
        outs, off = [], 0
        for c in ctx.sizes:
            outs.append(dy[:, off:off + c])       # channel-slice views (pixel-major with ld = total channels)
            off += c
        return tuple(outs)


def cat_channels(xs):
    return _Cat.apply(*xs)


# ------------------------------------------------------------------------------------------------ ConvTranspose k2s2 / PixelShuffle / pointwise
convt_ce_enabled = knob('DSRL_CONVT_CE', True)


class LogitsGrad:
    """Hand-over between the layer that produces the logits (the last ConvTranspose2d of the SSSR decoder, DSRL.py:64-69) and the loss that is the
    root of the backward pass (fused_losses).  When the loss finds this object on its logits and the shape qualifies, it computes only the CE VALUE,
    leaves `target`, `count` (device pointer holder) here and reports no gradient; the stride-8 feature transformer leaves its incoming gradient and
    weights; the ConvTranspose backward then forms d(CE)/d(logits) (+ the transformer's rank-one term) inside its own kernel
    (dsrl_convt2x2_bwd_ce): the 319 MB gradient of the 256x512 step is neither written nor read."""
    __slots__ = ('y', 'xshape', 'x_ptr', 'armed', 'target', 'ignore_index', 'count', 'ft', 'value', 'value_key', 'weight', 'gamma', 'eps', 'dice', 'lovasz',
                 'relax')

    def __init__(self):
        self.y = None; self.xshape = None; self.x_ptr = 0; self.armed = False; self.target = None; self.ignore_index = 255; self.count = None; self.ft = None
        self.dice = None            # the record of dsrl_dice_fwd when the loss has a Dice term (always with a table, like gamma); None: no such term
        self.lovasz = None          # (record of dsrl_lovasz_fwd, bins) when the loss has a Lovasz-Softmax term (always with a table too); None: no such term
        self.relax = None           # the class-set mask (relax_mask) of a relaxed loss (always with a table too); None: the label alone
        self.value = None           # [CE, pixel count, ...] when the producing layer already evaluated the loss (logits_target), and for which
        self.value_key = None       # (target pointer, ignore_index, NaN flag pointer, class-weight table pointer or 0, class-set mask pointer or 0, label smoothing, focal gamma)
        self.weight = None          # the 256-float class-weight table of a weighted loss (class_weight_table); `count` then holds D = sum n_c w_c
        self.gamma = 0.0            # > 0: the focal loss (always with a table: all ones when the caller gave no weights)
        self.eps = 0.0              # > 0: label smoothing (likewise always with a table; never together with gamma > 0)

    def usable(self, logits, target):
        """Can the loss leave the gradient to the producer?  logits must be exactly the producer's output buffer."""
        if not (convt_ce_enabled and self.y is not None and logits.data_ptr() == self.y.data_ptr() and tuple(logits.shape) == tuple(self.y.shape)):
            return False
        N, Ci, H, W = self.xshape
        return bool(query('dsrl_convt2x2_bwd_ce_supported', self.x_ptr, logits.data_ptr(), target.data_ptr(), N, H, W, Ci, logits.shape[1]))



def class_weight_table(weights, device, num_classes=None):
    """Per-class loss weights (nn.CrossEntropyLoss(weight=)) -> the 256-float table the weighted kernels index by the label byte: entries
    [0, len(weights)) hold the weights as fp32, the rest are zero.  Negative, NaN or infinite weights (also after rounding to fp32), an empty or
    over-long sequence, or a length other than `num_classes` when that is given, raise ValueError.  Zero weights are allowed.  Equal weights on one
    device ('cuda' means the current device) give the SAME tensor, so that the hand-over of the CE value keyed by its pointer
    (LogitsGrad.value_key) engages however the caller passes them.  A table returned by this function is recognised as that object and passed
    through without a host read; any other tensor (a clone or a copy of a table included) is validated on the host, which a graph capture does
    not allow: under capture pass the table itself, as TrainStep does."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if isinstance(weights, torch.Tensor):
        made = _weight_tables_made.get(id(weights)) if weights.device == dev else None
        if made is not None and made[0]() is weights:
            if num_classes is not None and made[1] != int(num_classes):
                raise ValueError(f'class weights: table of {made[1]} classes, the logits have {int(num_classes)}')
            return weights
        weights = weights.detach().cpu().numpy()
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f'class weights: not a sequence of numbers ({e})')
    if w.ndim != 1 or w.size == 0 or w.size > 256:
        raise ValueError(f'class weights: expected a sequence of 1..256 numbers, got shape {w.shape}')
    if num_classes is not None and w.size != int(num_classes):
        raise ValueError(f'class weights: {w.size} weights for {int(num_classes)} classes')
    with np.errstate(over='ignore'):
        w32 = w.astype(np.float32)
    if not np.isfinite(w32).all() or (w32 < 0).any():
        raise ValueError('class weights must be finite and >= 0')
    key = (w32.tobytes(), dev)
    tab = _weight_tables.get(key)
    if tab is None:
        while len(_weight_tables) >= _WEIGHT_TABLES_MAX:                # oldest first (dicts keep insertion order)
            _weight_tables.pop(next(iter(_weight_tables)))              # (a table somebody still holds stays recognised: the registry below is weak)
        full = np.zeros(256, np.float32); full[:w32.size] = w32
        tab = torch.from_numpy(full).to(dev)
        _weight_tables[key] = tab
        ident = id(tab)
        _weight_tables_made[ident] = (weakref.ref(tab, lambda _, ident=ident: _weight_tables_made.pop(ident, None)), int(w32.size))
    return tab


def focal_gamma_value(x):
    """The focal exponent as a float: any finite number >= 0 (0: the focal factor is off).  ValueError on a bool, on anything that is not a
    number, on NaN, infinity and negatives.  Touches no device."""
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f'focal_gamma = {x!r}: expected a finite number >= 0')
    g = float(x)
    if not math.isfinite(g) or g < 0.0 or g > 3.4028234663852886e38:          # (the kernels take it as fp32)
        raise ValueError(f'focal_gamma = {x!r}: expected a finite number >= 0')
    return g


def label_smoothing_value(x):
    """nn.CrossEntropyLoss's label_smoothing as a float: a finite number in [0, 1] (0: off).  ValueError on a bool, on anything that is not a
    number, on NaN, infinity and anything outside [0, 1] (-1e-30 and 1.0000001 included).  Touches no device."""
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f'label_smoothing = {x!r}: expected a number in [0, 1]')
    e = float(x)
    if not (0.0 <= e <= 1.0) or float(np.float32(e)) > 1.0:                    # (a NaN fails the comparison; the kernels take it as fp32)
        raise ValueError(f'label_smoothing = {x!r}: expected a number in [0, 1]')
    return e


OHEM_DEFAULT = (0.7, 100000)            # thresh, min_kept of `ohem=True`: the values the published Cityscapes configurations train with


def ohem_value(x):
    """Online hard example mining as (thresh, min_kept), or None when it is off.  None / False: off; True: OHEM_DEFAULT; a pair (thresh, min_kept);
    a mapping with the keys 'thresh' and / or 'min_kept' (a missing one takes its default).  thresh: a number in [0, 1]; min_kept: an integer >= 0
    (below 2^63).  ValueError on anything else - a bool where a number belongs, a NaN, a float min_kept, an unknown key.  Touches no device."""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)):
        return OHEM_DEFAULT if x else None
    if isinstance(x, dict):
        if not x or set(x) - {'thresh', 'min_kept'}:
            raise ValueError(f"ohem = {x!r}: expected a mapping with the keys 'thresh' and 'min_kept'")
        thresh, min_kept = x.get('thresh', OHEM_DEFAULT[0]), x.get('min_kept', OHEM_DEFAULT[1])
    elif isinstance(x, (tuple, list)) and len(x) == 2:
        thresh, min_kept = x
    else:
        raise ValueError(f'ohem = {x!r}: expected None, a bool, a pair (thresh, min_kept) or a mapping with these keys')
    if isinstance(thresh, (bool, np.bool_)) or not isinstance(thresh, (int, float, np.integer, np.floating)):
        raise ValueError(f'ohem: thresh = {thresh!r}: expected a number in [0, 1]')
    th = float(thresh)
    if not (0.0 <= th <= 1.0) or float(np.float32(th)) > 1.0:                   # (a NaN fails the comparison; the kernels take it as fp32)
        raise ValueError(f'ohem: thresh = {thresh!r}: expected a number in [0, 1]')
    if isinstance(min_kept, (bool, np.bool_)) or not isinstance(min_kept, (int, np.integer)) or not 0 <= int(min_kept) < 2 ** 63:
        raise ValueError(f'ohem: min_kept = {min_kept!r}: expected an integer >= 0')
    return th, int(min_kept)


def _ohem_args(ohem, gamma, eps, ignore_index):
    """ohem_value(ohem) of a CE call, after the combinations it does not go with: a focal or label-smoothed loss (scoped out: ValueError) and an
    ignore_index that is no byte value (it is written into the target: ValueError)."""
    ohem = ohem_value(ohem)
    if ohem is not None:
        if gamma > 0.0 or eps > 0.0:
            raise ValueError(f'ohem = {ohem!r} together with focal_gamma = {gamma!r} or label_smoothing = {eps!r}: the combination is not supported')
        if isinstance(ignore_index, (bool, np.bool_)) or not isinstance(ignore_index, (int, np.integer)) or not 0 <= int(ignore_index) <= 255:
            raise ValueError(f'ohem: ignore_index = {ignore_index!r} must be a byte value 0..255 (it is written into the target)')
    return ohem


def ohem_target(logits, target, ignore_index, thresh, min_kept, flag=None, stats=None):
    """The target with the label of every easy pixel set to `ignore_index`: logits (N,C,H,W) fp32, target (N,H,W) uint8/long ->
    a new uint8 tensor of target's shape.  A pixel takes part when its label is neither ignore_index nor >= C; p is the softmax probability of its
    label; with n such pixels in the call, k = min(min_kept, n - 1) and thr = max(k-th smallest p, thresh), a pixel stays iff p < thr.  The whole
    selection runs on the device (dsrl_ohem_target) without a host read, so it can be captured.  flag: the int32 NaN flag to OR into (optional);
    stats: a 4-element int32 tensor that receives {bits of thr, n, number kept, number with p < thresh} (optional).  Not differentiable: nothing is
    recorded, the logits are read as numbers."""
    th, mk = ohem_value((thresh, min_kept))
    if isinstance(ignore_index, (bool, np.bool_)) or not isinstance(ignore_index, (int, np.integer)) or not 0 <= int(ignore_index) <= 255:
        raise ValueError(f'ohem: ignore_index = {ignore_index!r} must be a byte value 0..255 (it is written into the target)')
    with torch.no_grad():
        logits, ld = pm(logits.detach())
        _need_gpu(target, flag, stats)
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        N, Cc, H, W = logits.shape
        P = N * H * W
        if target.numel() != P:
            raise DsrlHipError(f'ohem_target: target has {target.numel()} pixels, logits {P}')
        if flag is not None and flag.dtype != torch.int32:
            raise DsrlHipError(f'ohem_target: the NaN flag must be int32, got {flag.dtype}')
        if stats is None:
            stats = torch.empty(4, device=logits.device, dtype=torch.int32)
        elif stats.dtype != torch.int32 or stats.numel() < 4 or not stats.is_contiguous():
            raise DsrlHipError('ohem_target: stats must be a contiguous int32 tensor of 4 elements')
        out = torch.empty_like(target)
        ws = _ws(cquery('dsrl_ohem_workspace_bytes', P), logits)
        call('dsrl_ohem_target', logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), th, mk, out.data_ptr(), stats.data_ptr(),
             None if flag is None else flag.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out


DICE_DEFAULT = (1.0, 1.0)               # lambda, smooth of `dice=True`: an equal-weight "CE + Dice" with the usual +1 smoothing
DICE_RECORD_FLOATS = 128                # the record of dsrl_dice_fwd: {lambda L_dice, |K|, a[0..C), b[0..C), zeros}


def dice_value(x):
    """The soft Dice term as (lambda, smooth), or None when it is off.  None / False / 0: off; True: DICE_DEFAULT; a finite number > 0: lambda, with
    the default smooth; a pair (lambda, smooth); a mapping with the keys 'weight' (lambda) and / or 'smooth' (a missing one takes its default).
    smooth: a finite number >= 0.  A lambda of 0 inside a pair or a mapping is off too.  ValueError on anything else - a bool where a number belongs,
    a NaN, an infinity, a negative number, an unknown key.  Touches no device."""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)):
        return DICE_DEFAULT if x else None
    if isinstance(x, dict):
        if not x or set(x) - {'weight', 'smooth'}:
            raise ValueError(f"dice = {x!r}: expected a mapping with the keys 'weight' and 'smooth'")
        lam, smooth = x.get('weight', DICE_DEFAULT[0]), x.get('smooth', DICE_DEFAULT[1])
    elif isinstance(x, (tuple, list)) and len(x) == 2:
        lam, smooth = x
    elif isinstance(x, (int, float, np.integer, np.floating)):
        lam, smooth = x, DICE_DEFAULT[1]
    else:
        raise ValueError(f'dice = {x!r}: expected None, a bool, a number > 0, a pair (weight, smooth) or a mapping with these keys')
    for name, v in (('weight', lam), ('smooth', smooth)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f'dice: {name} = {v!r}: expected a finite number >= 0')
        with np.errstate(over='ignore'):
            v32 = float(np.float32(float(v)))                                  # (the kernels take both as fp32)
        if not (0.0 <= float(v) and math.isfinite(v32)):                       # (a NaN fails the comparison)
            raise ValueError(f'dice: {name} = {v!r}: expected a finite number >= 0')
    lam, smooth = float(lam), float(smooth)
    if lam == 0.0:
        return None
    if float(np.float32(lam)) == 0.0:
        raise ValueError(f'dice: weight = {lam!r} is zero as fp32')
    return lam, smooth


def _dice_args(dice, gamma, eps, ohem):
    """dice_value(dice) of a CE call, after the combinations it does not go with: a focal or label-smoothed loss and hard-pixel mining (scoped out:
    ValueError).  It goes with class weights."""
    dice = dice_value(dice)
    if dice is not None and (gamma > 0.0 or eps > 0.0 or ohem is not None):
        raise ValueError(f'dice = {dice!r} together with focal_gamma = {gamma!r}, label_smoothing = {eps!r} or ohem = {ohem!r}: '
                         'the combination is not supported')
    return dice


def _dice_record(logits, ld, target, P, Cc, ignore_index, dice, flag=None):
    """dsrl_dice_fwd on pixel-major logits and a contiguous uint8 target: -> the 128-float device record {lambda L_dice, |K|, a, b}.
    No host read: it can be captured."""
    rec = torch.empty(DICE_RECORD_FLOATS, device=logits.device, dtype=torch.float32)
    ws = _ws(cquery('dsrl_dice_workspace_bytes', P), logits)
    call('dsrl_dice_fwd', logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), float(dice[0]), float(dice[1]), rec.data_ptr(),
         None if flag is None else flag.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return rec


class _DiceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, dice):
        logits, ld = pm(logits)
        _need_gpu(target)
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        N, Cc, H, W = logits.shape
        P = N * H * W
        if target.numel() != P:
            raise DsrlHipError(f'dice_loss: target has {target.numel()} pixels, logits {P}')
        rec = _dice_record(logits, ld, target, P, Cc, ignore_index, dice)
        ctx.save_for_backward(logits, target, rec)
        ctx.ignore_index = int(ignore_index)
        return rec[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, target, rec = ctx.saved_tensors
        _, ld = pm(logits)
        N, Cc, H, W = logits.shape
        dl = new_cl((N, Cc, H, W), logits)
        call('dsrl_dice_bwd', logits.data_ptr(), ld, target.data_ptr(), N * H * W, Cc, ctx.ignore_index, rec.data_ptr(), 0, dl.data_ptr(), Cc, _stream())
        dl.mul_(g.reshape(1, 1, 1, 1).float())          # the incoming gradient as a device scalar: no host read (1 leaves every element as it is)
        return dl, None, None, None


def dice_loss(logits, target, ignore_index=255, weight=1.0, smooth=1.0):
    """weight * L_dice, the soft Dice loss of the softmax of logits (N,C,H,W) against target (N,H,W) uint8/long: L_dice = 1 - the
    mean over the classes PRESENT among the live pixels of the call of (2 I_c + smooth) / (P_c + G_c + smooth); a pixel is live when its label is
    neither ignore_index nor >= C.  A class that no live pixel carries adds nothing (it is not counted as a perfect score).  weight: a finite number
    > 0; smooth: a finite number >= 0.  Differentiable (dsrl_dice_fwd / dsrl_dice_bwd); the class sums are those of this call."""
    dice = dice_value((weight, smooth))
    if dice is None:
        raise ValueError(f'dice_loss: weight = {weight!r}: expected a finite number > 0')
    return _DiceLoss.apply(logits, target, int(ignore_index), dice)


LOVASZ_DEFAULT = (1.0, 1024)            # lambda, bins of `lovasz=True`: an equal-weight "CE + Lovasz-Softmax" within 1 / 2048 of the unquantised loss
LOVASZ_BINS = (16, 4096)                # bins: a power of two in this range


def lovasz_value(x):
    """The Lovasz-Softmax term as (lambda, bins), or None when it is off.  None / False / 0: off; True: LOVASZ_DEFAULT; a finite number > 0: lambda,
    with the default bins; a pair (lambda, bins); a mapping with the keys 'weight' (lambda) and / or 'bins' (a missing one takes its default).
    bins: an integer power of two in [16, 4096].  A lambda of 0 inside a pair or a mapping is off too.  ValueError on anything else - a bool where a
    number belongs, a NaN, an infinity, a negative number, an unknown key, bins that are not such a power of two.  Touches no device."""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)):
        return LOVASZ_DEFAULT if x else None
    if isinstance(x, dict):
        if not x or set(x) - {'weight', 'bins'}:
            raise ValueError(f"lovasz = {x!r}: expected a mapping with the keys 'weight' and 'bins'")
        lam, bins = x.get('weight', LOVASZ_DEFAULT[0]), x.get('bins', LOVASZ_DEFAULT[1])
    elif isinstance(x, (tuple, list)) and len(x) == 2:
        lam, bins = x
    elif isinstance(x, (int, float, np.integer, np.floating)):
        lam, bins = x, LOVASZ_DEFAULT[1]
    else:
        raise ValueError(f'lovasz = {x!r}: expected None, a bool, a number > 0, a pair (weight, bins) or a mapping with these keys')
    if isinstance(lam, (bool, np.bool_)) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise ValueError(f'lovasz: weight = {lam!r}: expected a finite number >= 0')
    with np.errstate(over='ignore'):
        lam32 = float(np.float32(float(lam)))                                  # (the kernels take it as fp32)
    if not (0.0 <= float(lam) and math.isfinite(lam32)):                       # (a NaN fails the comparison)
        raise ValueError(f'lovasz: weight = {lam!r}: expected a finite number >= 0')
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)):
        raise ValueError(f'lovasz: bins = {bins!r}: expected an integer power of two in [{LOVASZ_BINS[0]}, {LOVASZ_BINS[1]}]')
    bins = int(bins)
    if not (LOVASZ_BINS[0] <= bins <= LOVASZ_BINS[1]) or bins & (bins - 1):
        raise ValueError(f'lovasz: bins = {bins!r}: expected an integer power of two in [{LOVASZ_BINS[0]}, {LOVASZ_BINS[1]}]')
    lam = float(lam)
    if lam == 0.0:
        return None
    if lam32 == 0.0:
        raise ValueError(f'lovasz: weight = {lam!r} is zero as fp32')
    return lam, bins


def _lovasz_args(lovasz, gamma, eps, ohem, dice):
    """lovasz_value(lovasz) of a CE call, after the combinations it does not go with: a focal or label-smoothed loss, hard-pixel mining and the Dice
    term (scoped out - each would be one more build of the backward kernel: ValueError).  It goes with class weights."""
    lovasz = lovasz_value(lovasz)
    if lovasz is not None and (gamma > 0.0 or eps > 0.0 or ohem is not None or dice is not None):
        raise ValueError(f'lovasz = {lovasz!r} together with focal_gamma = {gamma!r}, label_smoothing = {eps!r}, ohem = {ohem!r} or dice = {dice!r}: '
                         'the combination is not supported')
    return lovasz


def _lovasz_record(logits, ld, target, P, Cc, ignore_index, lovasz, flag=None):
    """dsrl_lovasz_fwd on pixel-major logits and a contiguous uint8 target: -> the device record {lambda L, |Present|, 0, 0, gf[C][bins], gb[C][bins]}
    (DESIGN.md 6.1.14).  No host read: it can be captured."""
    lam, bins = lovasz
    rec = torch.empty(cquery('dsrl_lovasz_record_floats', Cc, bins), device=logits.device, dtype=torch.float32)
    ws = _ws(cquery('dsrl_lovasz_workspace_bytes', P, Cc, bins), logits)
    call('dsrl_lovasz_fwd', logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), float(lam), int(bins), rec.data_ptr(),
         None if flag is None else flag.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return rec


class _LovaszLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, lovasz):
        logits, ld = pm(logits)
        _need_gpu(target)
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        N, Cc, H, W = logits.shape
        P = N * H * W
        if target.numel() != P:
            raise DsrlHipError(f'lovasz_softmax_loss: target has {target.numel()} pixels, logits {P}')
        rec = _lovasz_record(logits, ld, target, P, Cc, ignore_index, lovasz)
        ctx.save_for_backward(logits, target, rec)
        ctx.ignore_index = int(ignore_index)
        ctx.bins = int(lovasz[1])
        return rec[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, target, rec = ctx.saved_tensors
        _, ld = pm(logits)
        N, Cc, H, W = logits.shape
        dl = new_cl((N, Cc, H, W), logits)
        call('dsrl_lovasz_bwd', logits.data_ptr(), ld, target.data_ptr(), N * H * W, Cc, ctx.ignore_index, rec.data_ptr(), ctx.bins, 0, dl.data_ptr(), Cc,
             _stream())
        dl.mul_(g.reshape(1, 1, 1, 1).float())          # the incoming gradient as a device scalar: no host read (1 leaves every element as it is)
        return dl, None, None, None


def lovasz_softmax_loss(logits, target, ignore_index=255, weight=1.0, bins=1024):
    """weight * L, the Lovasz-Softmax loss (Berman et al., CVPR 2018) of the softmax of logits (N,C,H,W) against target (N,H,W) uint8/long in its
    QUANTISED form: the errors |[t == c] - p_c| of the live pixels are put into `bins` levels and the Lovasz extension of the
    Jaccard loss is evaluated at the level centres, exactly, from integer histograms - within 1 / (2 bins) of the sorted, unquantised loss, with no
    sort.  classes = 'present' over the whole call (per_image = False): the mean runs over the classes some live pixel carries; a pixel is live when
    its label is neither ignore_index nor >= C.  The gradient keeps the ranking constant, as autograd does in the sorted form.  weight: a finite
    number > 0; bins: a power of two in [16, 4096].  Differentiable (dsrl_lovasz_fwd / dsrl_lovasz_bwd); the histograms are those of this call."""
    lovasz = lovasz_value((weight, bins))
    if lovasz is None:
        raise ValueError(f'lovasz_softmax_loss: weight = {weight!r}: expected a finite number > 0')
    return _LovaszLoss.apply(logits, target, int(ignore_index), lovasz)


LABEL_RELAX_RADIUS = (1, 4)             # the window radii dsrl_relax_mask has


def label_relax_value(x):
    """Boundary label relaxation as a setting -> the window radius, or None for none.  None, False and 0 turn it off; True is radius 1; an integer
    in [1, 4] (also as an integral float) is that radius; a mapping {'radius': r} likewise.  Anything else (a bool is not a radius, a float that is
    not integral, an unknown key, a radius outside the range) is a ValueError."""
    lo, hi = LABEL_RELAX_RADIUS
    if isinstance(x, np.bool_):
        x = bool(x)
    if x is None or x is False:
        return None
    if x is True:
        return 1
    keyed = isinstance(x, dict)
    if keyed:
        if set(x) != {'radius'}:
            raise ValueError(f"label_relax = {x!r}: expected a mapping with the key 'radius'")
        x = x['radius']
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"label_relax = {x!r}: expected None, a bool, an integer radius in [{lo}, {hi}] or a mapping {{'radius': r}}")
    if not np.isfinite(x) or x != int(x):
        raise ValueError(f'label_relax = {x!r}: the radius is not an integer')
    r = int(x)
    if r == 0 and not keyed:
        return None
    if not lo <= r <= hi:
        raise ValueError(f'label_relax = {x!r}: expected a radius in [{lo}, {hi}]')
    return r


def _label_relax_args(label_relax, gamma, eps, ohem, dice, lovasz):
    """label_relax of a CE call - label_relax_value(label_relax), or a ready class-set mask (an int32 tensor from relax_mask) as it is - after the
    combinations it does not go with: everything but class weights."""
    if not isinstance(label_relax, torch.Tensor):
        label_relax = label_relax_value(label_relax)
    elif label_relax.dtype != torch.int32:
        raise ValueError(f'label_relax: a mask of dtype {label_relax.dtype}, expected the int32 tensor of relax_mask')
    if label_relax is not None and (gamma > 0.0 or eps > 0.0 or ohem is not None or dice is not None or lovasz is not None):
        shown = 'a mask' if isinstance(label_relax, torch.Tensor) else repr(label_relax)
        raise ValueError(f'label_relax = {shown} together with focal_gamma = {gamma!r}, label_smoothing = {eps!r}, ohem = {ohem!r}, dice = {dice!r} '
                         f'or lovasz = {lovasz!r}: the combination is not built')
    return label_relax


def relax_mask(target, num_classes, ignore_index=255, radius=1, stats=None):
    """The class-set mask of boundary label relaxation (dsrl_relax_mask): target (N, H, W) uint8 on the GPU -> (N, H, W) int32 whose
    bit c says that class c occurs among the live labels < num_classes in the (2 radius + 1)^2 window around the pixel, clipped at the borders of
    its own image; 0 for a pixel that is ignored or whose label is >= num_classes.  stats: an int64 tensor of 2 on the same device that receives
    ADDED counts {live pixels, pixels with more than one class in their set}, or None.  One launch, no host read (graph-capturable)."""
    _need_gpu(target)
    if target.dtype != torch.uint8 or target.dim() != 3:
        raise DsrlHipError(f'relax_mask: target must be a (N, H, W) uint8 tensor, got {tuple(target.shape)} {target.dtype}')
    target = target.contiguous()
    N, H, W = target.shape
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < 2 or stats.device != target.device or not stats.is_contiguous()):
        raise DsrlHipError('relax_mask: stats must be a contiguous int64 tensor of 2 on the device of the target')
    mask = torch.empty((N, H, W), device=target.device, dtype=torch.int32)
    call('dsrl_relax_mask', target.data_ptr(), N, H, W, int(num_classes), int(ignore_index), int(radius), mask.data_ptr(),
         None if stats is None else stats.data_ptr(), _stream())
    return mask


def _relax_mask_of(label_relax, target, num_classes, ignore_index):
    """the mask a CE call uses: the given one, or dsrl_relax_mask of its own target at the given radius (label_relax went through _label_relax_args)"""
    if label_relax is None:
        return None
    if target.dtype != torch.uint8:
        target = target.to(torch.uint8)
    target = target.contiguous()
    if isinstance(label_relax, torch.Tensor):
        _need_gpu(label_relax)
        if label_relax.numel() != target.numel() or not label_relax.is_contiguous() or label_relax.device != target.device:
            raise DsrlHipError(f'label_relax: a mask of {label_relax.numel()} words for a target of {target.numel()} pixels (contiguous, on its device)')
        return label_relax
    if num_classes > 32:
        raise ValueError(f'label_relax: {num_classes} classes, a class set is one 32-bit word')
    return relax_mask(target if target.dim() == 3 else target.reshape(-1, 1, target.shape[-1]), num_classes, ignore_index, label_relax)


def _focal_args(weight, gamma, device, num_classes, eps=0.0, dice=None, lovasz=None, relax=None):
    """(class-weight table or None, gamma, eps) of a CE call: the focal and the label-smoothed loss run on the weighted kernels, so gamma > 0 or
    eps > 0 without weights takes the all-ones table of `num_classes` classes; so do a Dice term (`dice` not None) and a Lovasz-Softmax term
    (`lovasz` not None), whose fused backwards are builds of the weighted kernel, and the relaxed loss (`relax` not None).  gamma and eps both at once: ValueError (the combination has no
    agreed definition and no kernel)."""
    gamma = focal_gamma_value(gamma)
    eps = label_smoothing_value(eps)
    if gamma > 0.0 and eps > 0.0:
        raise ValueError(f'label_smoothing = {eps!r} together with focal_gamma = {gamma!r}: the combination is not defined')
    if weight is not None:
        weight = class_weight_table(weight, device, num_classes)
    elif gamma > 0.0 or eps > 0.0 or dice is not None or lovasz is not None or relax is not None:
        weight = class_weight_table(np.ones(int(num_classes), np.float32), device, num_classes)
    return weight, gamma, eps


def _ce_variant(weight, gamma, eps, relax=None):
    """(suffix of the entry point, the arguments that follow ignore_index in its call) of a CE call whose (class-weight table, gamma, eps) went
    through _focal_args: '' plain, '_w' class-weighted, '_f' focal, '_s' label-smoothed.  Every family (dsrl_ce_fwd, dsrl_ce_bwd, dsrl_ce_fused,
    dsrl_convt2x2_fwd_ce, dsrl_convt2x2_bwd_ce) and every workspace query names its four forms with these suffixes.  relax: the class-set mask of
    a relaxed loss (relax_mask; never with gamma or eps: _label_relax_args), the fifth form '_r'."""
    if relax is not None:
        return '_r', (weight.data_ptr(), relax.data_ptr())
    if eps > 0.0:
        return '_s', (weight.data_ptr(), eps)
    if gamma > 0.0:
        return '_f', (weight.data_ptr(), gamma)
    if weight is None:
        return '', ()
    return '_w', (weight.data_ptr(),)


_WEIGHT_TABLES_MAX = 32
_weight_tables = {}             # (fp32 weight bytes, device) -> table
_weight_tables_made = {}        # id(table) -> (weak reference, number of classes): how a table made here is recognised for as long as it lives
_logits_target = None


class logits_target:
    """with logits_target(target, ignore_index, flag): ... model(x) ... - tells the layer that produces the logits (HipConvTranspose2d.logits_layer) what
    they will be compared with, so that its forward kernel evaluates nn.CrossEntropyLoss while the output tile is on chip (dsrl_convt2x2_fwd_ce) and
    fused_losses finds the value ready (LogitsGrad.value) instead of reading the logits again.  target: (N,H,W) uint8, contiguous; flag: the int32 NaN
    flag fused_losses will be given; weight: the class weights fused_losses will be given (None: unweighted); focal_gamma: its focal exponent
    (0: none); label_smoothing: its label smoothing (0: none; not together with focal_gamma > 0); ohem: its hard-pixel mining (ohem_value; not
    together with either of the two).  Outside the block, or when the shape does not qualify, nothing changes.  With ohem nothing is engaged either:
    the target the loss will use does not exist before the logits do, so the plain forward runs and fused_losses evaluates the value itself.
    label_relax: its boundary label relaxation (a radius, or the ready mask of relax_mask; with class weights only).  Unlike OHEM's target the mask
    exists before the logits do, so the forward kernel IS engaged (dsrl_convt2x2_fwd_ce_r); fused_losses finds the value ready when it is given
    the SAME mask tensor - a step computes the mask once and passes it to both (a radius here makes a mask of the layer's own)."""

    def __init__(self, target, ignore_index, flag, weight=None, focal_gamma=0.0, label_smoothing=0.0, ohem=None, dice=None, lovasz=None, label_relax=None):
        focal_gamma = focal_gamma_value(focal_gamma)
        label_smoothing = label_smoothing_value(label_smoothing)
        if focal_gamma > 0.0 and label_smoothing > 0.0:
            raise ValueError(f'label_smoothing = {label_smoothing!r} together with focal_gamma = {focal_gamma!r}: the combination is not defined')
        ohem = _ohem_args(ohem, focal_gamma, label_smoothing, ignore_index)
        # a Dice term leaves the forward as it is: the kernel evaluates the CE value (on the weighted machinery: the all-ones table without weights,
        # as fused_losses will use) and dsrl_dice_fwd reads the logits once more
        dice = _dice_args(dice, focal_gamma, label_smoothing, ohem)
        lovasz = _lovasz_args(lovasz, focal_gamma, label_smoothing, ohem, dice)        # the same holds for a Lovasz-Softmax term (dsrl_lovasz_fwd)
        relax = _label_relax_args(label_relax, focal_gamma, label_smoothing, ohem, dice, lovasz)
        ok = (convt_ce_enabled and target is not None and target.is_cuda and target.dtype == torch.uint8 and target.is_contiguous() and target.dim() == 3
              and flag is not None and flag.dtype == torch.int32 and ohem is None)
        if weight is not None and target is not None:
            weight = class_weight_table(weight, target.device)
        if ok and isinstance(relax, torch.Tensor):
            relax = _relax_mask_of(relax, target, 0, ignore_index)         # (a ready mask: checked against the target; a radius waits for the class count)
        self.new = (target, int(ignore_index), flag, weight, focal_gamma, label_smoothing, dice is not None or lovasz is not None, relax) if ok else None

    def __enter__(self):
        global _logits_target
        self.old, _logits_target = _logits_target, self.new
        return self

    def __exit__(self, *exc):
        global _logits_target
        _logits_target = self.old
        return False


class _ConvT2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, holder=None):
        ctx.set_materialize_grads(False)        # dy is None when the loss left its gradient to this layer (LogitsGrad)
        ctx.holder = holder
        x = pm_dense(x)
        _need_gpu(w, bias)
        w_param = w
        w = w.contiguous()
        N, Ci, H, W = x.shape
        Co = w.shape[1]
        if w.shape[0] != Ci or tuple(w.shape[2:]) != (2, 2):
            raise DsrlHipError(f'conv_transpose2d_k2s2: weight {tuple(w.shape)} does not match input channels {Ci}')
        y = new_cl((N, Co, 2 * H, 2 * W), x)
        lt = _logits_target if holder is not None else None
        if (lt is not None and tuple(lt[0].shape) == (N, 2 * H, 2 * W) and lt[0].device == x.device
                and query('dsrl_convt2x2_fwd_ce_supported', x.data_ptr(), y.data_ptr(), N, H, W, Ci, Co)):       # (pointer arguments: not memoised)
            tgt, ign, flag, wt, gamma, eps, diced, rmask = lt
            if rmask is not None:
                rmask = _relax_mask_of(rmask, tgt, Co, ign)
            if wt is not None or gamma > 0.0 or eps > 0.0 or diced or rmask is not None:
                wt = _focal_args(wt, gamma, x.device, Co, eps, True if diced else None, None, rmask)[0]           # (a table of another class count: ValueError)
            sfx, extra = _ce_variant(wt, gamma, eps, rmask)
            holder.value = torch.empty(8, device=x.device, dtype=torch.float32)
            holder.value_key = (tgt.data_ptr(), ign, flag.data_ptr(), 0 if wt is None else wt.data_ptr(), 0 if rmask is None else rmask.data_ptr(), eps, gamma)
            ws = _ws(cquery(f'dsrl_convt2x2_fwd_ce{sfx}_workspace_bytes', N, H, W), x)
            call('dsrl_convt2x2_fwd_ce' + sfx, x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(), N, H, W, Ci, Co,
                 tgt.data_ptr(), ign, *extra, holder.value.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        else:
            call('dsrl_convt2x2_fwd', x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(), N, H, W, Ci, Co, _stream())
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.params = (w_param if isinstance(w_param, torch.nn.Parameter) else None, bias if isinstance(bias, torch.nn.Parameter) else None)
        if holder is not None:
            holder.y = y; holder.xshape = (N, Ci, H, W); holder.x_ptr = x.data_ptr()
            y._dsrl_logits_grad = holder
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, Ci, H, W = x.shape
        Co = w.shape[1]
        h = ctx.holder
        hand = None
        if h is not None and h.armed:           # the loss left d(CE)/d(logits) to this layer: take it over, and disarm the holder whatever happens next
            hand = (h.y, h.target, int(h.ignore_index), h.count, h.ft, h.weight, h.gamma, h.eps, h.dice, h.lovasz, h.relax)
            h.armed = False; h.ft = None; h.target = None; h.count = None; h.y = None; h.value = None; h.weight = None; h.gamma = 0.0; h.eps = 0.0
            h.dice = None; h.lovasz = None; h.relax = None
        fused = dy is None and hand is not None
        if dy is None and not fused:
            raise DsrlHipError('conv_transpose2d_k2s2: backward reached without a gradient for the output')
        if not fused:
            dy = pm_dense(dy)
        if hand is not None and not fused:
            # another consumer of the logits sent a gradient too (it is not the loss's: fused_losses returned none): d(CE)/d(logits) and the
            # transformer's term are written as the unfused step writes them (dsrl_ce_fused, dsrl_dice_bwd(accumulate = 1) when the loss has a Dice
            # term, dsrl_pointwise_strided_bwd(accumulate = 1)), dy is added as autograd would add it, and the plain backward below takes the sum
            y, target, ign, _, ft, wt, gamma, eps, dice_rec, lov, rmask = hand
            P = N * 4 * H * W
            dl = new_cl((N, Co, 2 * H, 2 * W), x)
            scal = torch.empty(8, device=x.device, dtype=torch.float32)
            sfx, extra = _ce_variant(wt, gamma, eps, rmask)          # (dsrl_ce_fused_r writes the relaxed row)
            wsc = _ws(cquery(f'dsrl_ce_fused{sfx}_workspace_bytes', P), x)
            call('dsrl_ce_fused' + sfx, y.data_ptr(), Co, target.data_ptr(), P, Co, ign, *extra, dl.data_ptr(), Co, scal.data_ptr(), None,
                 wsc.data_ptr(), wsc.numel(), _stream())
            if dice_rec is not None:
                call('dsrl_dice_bwd', y.data_ptr(), Co, target.data_ptr(), P, Co, ign, dice_rec.data_ptr(), 1, dl.data_ptr(), Co, _stream())
            if lov is not None:             # (or dsrl_lovasz_bwd(accumulate = 1) when it has a Lovasz-Softmax term)
                call('dsrl_lovasz_bwd', y.data_ptr(), Co, target.data_ptr(), P, Co, ign, lov[0].data_ptr(), lov[1], 1, dl.data_ptr(), Co, _stream())
            if ft is not None:
                ft_g, ft_w, ft_s = ft
                dwf = torch.empty(Co, device=x.device, dtype=torch.float32)          # the transformer's weight gradient was delivered by its own backward
                wsf = _ws(cquery('dsrl_pointwise_strided_bwd_workspace_bytes', N, 2 * H, 2 * W, Co, ft_s), x)
                call('dsrl_pointwise_strided_bwd', y.data_ptr(), ft_w.data_ptr(), ft_g.data_ptr(), dl.data_ptr(), dwf.data_ptr(), 1,
                     N, 2 * H, 2 * W, Co, ft_s, wsf.data_ptr(), wsf.numel(), _stream())
            dy = dl.add_(dy)
        dx = new_cl((N, Ci, H, W), x)
        wsink = _sink_flat(ctx.params[0], w.numel())
        bsink = _sink_flat(ctx.params[1], Co) if ctx.has_bias else None
        dw = wsink if wsink is not None else torch.empty_like(w)
        db = (bsink if bsink is not None else torch.empty(Co, device=x.device, dtype=torch.float32)) if ctx.has_bias else None
        ws = _ws(cquery('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, Ci, Co), x)
        if fused:
            y, target, ign, count, ft, wt, gamma, eps, dice_rec, lov, rmask = hand
            ft_g, ft_w, ft_s = ft if ft is not None else (None, None, 0)
            sfx, extra = _ce_variant(wt, gamma, eps, rmask)          # (dsrl_convt2x2_bwd_ce_r with a mask: never with gamma, eps, Dice or Lovasz)
            if dice_rec is not None:            # the weighted row plus the Dice row (never with gamma or eps: _dice_args)
                sfx, extra = '_d', (wt.data_ptr(), dice_rec.data_ptr())
            if lov is not None:                 # the weighted row plus the Lovasz row (never with gamma, eps or Dice: _lovasz_args)
                sfx, extra = '_l', (wt.data_ptr(), lov[0].data_ptr(), lov[1])
            call('dsrl_convt2x2_bwd_ce' + sfx, x.data_ptr(), w.data_ptr(), y.data_ptr(), target.data_ptr(), ign, *extra, count.data_ptr() + 4,
                 None if ft_g is None else ft_g.data_ptr(), None if ft_w is None else ft_w.data_ptr(), int(ft_s),
                 dx.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), N, H, W, Ci, Co, ws.data_ptr(), ws.numel(), _stream())
        else:
            call('dsrl_convt2x2_bwd', x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(),
                 N, H, W, Ci, Co, ws.data_ptr(), ws.numel(), _stream())
        if wsink is not None:
            _sunk(ctx.params[0]); dw = None
        if bsink is not None:
            _sunk(ctx.params[1]); db = None
        return dx, _deliver(ctx.params[0], dw), _deliver(ctx.params[1], db), None


def conv_transpose2d_k2s2(x, weight, bias=None, logits_grad=None):
    """logits_grad: a LogitsGrad when this output may be the logits of fused_losses (see there); None otherwise."""
    return _ConvT2x2.apply(x, weight, bias, logits_grad)


class _PixelShuffle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r):
        x = pm_dense(x)
        N, Cc, H, W = x.shape
        c = Cc // (r * r)
        y = new_cl((N, c, H * r, W * r), x)
        call('dsrl_pixel_shuffle_fwd', x.data_ptr(), y.data_ptr(), N, H, W, c, r, _stream())
        ctx.shp = (N, Cc, H, W, c, r)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, Cc, H, W, c, r = ctx.shp
        dy = pm_dense(dy)
        dx = new_cl((N, Cc, H, W), dy)
        call('dsrl_pixel_shuffle_bwd', dy.data_ptr(), dx.data_ptr(), N, H, W, c, r, _stream())
        return dx, None


def pixel_shuffle(x, r):
    return _PixelShuffle.apply(x, int(r))


class _PointwiseStrided(torch.autograd.Function):
    """1x1 conv, stride s, one output channel, no bias (DSRL.py:88-93)."""

    @staticmethod
    def forward(ctx, x, w, stride, out_slot=None):
        ctx.out_slot = out_slot
        ctx.logits_grad = getattr(x, '_dsrl_logits_grad', None)
        x = pm_dense(x)
        _need_gpu(w)
        N, Cc, H, W = x.shape
        wf = w.contiguous().view(-1)
        if wf.numel() != Cc:
            raise DsrlHipError('pointwise_strided: weight must be (1,C,1,1)')
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = new_cl((N, 1, Ho, Wo), x)
        call('dsrl_pointwise_strided_fwd', x.data_ptr(), wf.data_ptr(), y.data_ptr(), N, H, W, Cc, stride, _stream())
        ctx.save_for_backward(x, wf)
        ctx.stride = stride
        ctx.wshape = tuple(w.shape)
        ctx.wparam = w if isinstance(w, torch.nn.Parameter) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wf = ctx.saved_tensors
        N, Cc, H, W = x.shape
        dy = dy.contiguous()
        # x also feeds the fused loss (fused_losses): that node ran first (it is the root of the backward pass) and published the dense
        # gradient it computed for x; our contribution lives on the stride grid only (1/64 of the pixels) and is added into that buffer
        # instead of being materialised as a mostly-zero tensor that autograd would then add with a full pass.  The loss
        # left the buffer to us: it goes on to autograd as our gradient of x
        slot = ctx.out_slot
        lg = ctx.logits_grad
        if lg is not None and lg.armed and lg.y is not None and lg.y.data_ptr() == x.data_ptr() and lg.ft is None:
            # the loss left d(loss)/d(x) to the layer that produced x (LogitsGrad): that kernel adds g * w on the stride grid itself
            wsink = _sink_flat(ctx.wparam, Cc)
            dw = wsink if wsink is not None else torch.empty(Cc, device=x.device, dtype=torch.float32)
            ws = _ws(cquery('dsrl_pointwise_strided_bwd_workspace_bytes', N, H, W, Cc, ctx.stride), x)
            call('dsrl_pointwise_strided_bwd', x.data_ptr(), wf.data_ptr(), dy.data_ptr(), None, dw.data_ptr(), 2,
                 N, H, W, Cc, ctx.stride, ws.data_ptr(), ws.numel(), _stream())
            lg.ft = (dy, wf, ctx.stride)
            if wsink is not None:
                _sunk(ctx.wparam)
                return None, None, None, None
            return None, _deliver(ctx.wparam, dw.view(ctx.wshape)), None, None
        acc = (slot is not None and not slot.closed and slot.buf is not None and tuple(slot.buf.shape) == (N, Cc, H, W)
               and _ld_of(slot.buf) == Cc)
        dx = slot.buf if acc else new_cl((N, Cc, H, W), x)
        wsink = _sink_flat(ctx.wparam, Cc)
        dw = wsink if wsink is not None else torch.empty(Cc, device=x.device, dtype=torch.float32)
        ws = _ws(cquery('dsrl_pointwise_strided_bwd_workspace_bytes', N, H, W, Cc, ctx.stride), x)
        call('dsrl_pointwise_strided_bwd', x.data_ptr(), wf.data_ptr(), dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), int(acc),
             N, H, W, Cc, ctx.stride, ws.data_ptr(), ws.numel(), _stream())
        if slot is not None and not acc:
            slot.closed = True
        if wsink is not None:
            _sunk(ctx.wparam)
            return dx, None, None, None
        return dx, _deliver(ctx.wparam, dw.view(ctx.wshape)), None, None


def pointwise_strided(x, weight, stride, out_slot=None):
    return _PointwiseStrided.apply(x, weight, int(stride), out_slot)


# ------------------------------------------------------------------------------------------------ losses
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, weight=None, gamma=0.0, eps=0.0, relax=None):
        logits, ld = pm(logits)
        _need_gpu(target)
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        N, Cc, H, W = logits.shape
        P = N * H * W
        if target.numel() != P:
            raise DsrlHipError(f'cross_entropy: target has {target.numel()} pixels, logits {P}')
        out = torch.empty(2, device=logits.device, dtype=torch.float32)
        relax = _relax_mask_of(relax, target.view(N, H, W), Cc, ignore_index)
        sfx, extra = _ce_variant(weight, gamma, eps, relax)
        ws = _ws(cquery(f'dsrl_ce{sfx}_workspace_bytes', P), logits)
        call('dsrl_ce_fwd' + sfx, logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), *extra, out.data_ptr(),
             ws.data_ptr(), ws.numel(), _stream())
        ctx.save_for_backward(logits, target, out)
        ctx.ignore_index = int(ignore_index)
        ctx.weight = weight
        ctx.gamma = gamma
        ctx.eps = eps
        ctx.relax = relax
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits, target, out = ctx.saved_tensors
        _, ld = pm(logits)
        N, Cc, H, W = logits.shape
        g = g.reshape(1).contiguous().float()
        dl = new_cl((N, Cc, H, W), logits)
        sfx, extra = _ce_variant(ctx.weight, ctx.gamma, ctx.eps, ctx.relax)
        call('dsrl_ce_bwd' + sfx, logits.data_ptr(), ld, target.data_ptr(), N * H * W, Cc, ctx.ignore_index, *extra, out.data_ptr(), g.data_ptr(),
             dl.data_ptr(), Cc, _stream())
        return dl, None, None, None, None, None, None


def cross_entropy(logits, target, ignore_index=255, weight=None, focal_gamma=0.0, label_smoothing=0.0, ohem=None, dice=None, lovasz=None, label_relax=None):
    """nn.CrossEntropyLoss(weight, ignore_index, label_smoothing=) with mean reduction; target (N,H,W) uint8/long; weight: None, one number per
    class, or a class_weight_table.  focal_gamma > 0: the focal loss sum w[t] (1 - p_t)^gamma (-log p_t) / sum w[t]; 0 changes
    nothing.  label_smoothing in (0, 1]: torch's smoothed loss, with one deviation: a class of weight 0 adds nothing to the
    smoothing sum even where its -log p is +inf (torch forms 0 * inf = NaN there); 0 changes nothing; together with focal_gamma > 0: ValueError.
    ohem (ohem_value: None, True, (thresh, min_kept) or a mapping): online hard example mining - the loss of ohem_target's rewritten target, with or
    without weights (the selection is on the unweighted probability); together with focal_gamma > 0 or label_smoothing > 0: ValueError.
    dice (dice_value: None, True, a weight, (weight, smooth) or a mapping): adds weight * L_dice (dice_loss) to the CE, with or
    without class weights; together with focal_gamma > 0, label_smoothing > 0 or ohem: ValueError.
    lovasz (lovasz_value: None, True, a weight, (weight, bins) or a mapping): adds weight * L_lovasz, the quantised Lovasz-Softmax loss
    (lovasz_softmax_loss), with or without class weights; together with focal_gamma > 0, label_smoothing > 0, ohem or dice:
    ValueError.
    label_relax (label_relax_value: None, True, a radius in [1, 4] or {'radius': r}; or a ready mask from relax_mask): boundary label relaxation
     - a pixel's term is -w[t] log of the summed probability of the classes in the window around it, at most 32 classes, with
    or without class weights; together with any of the other options: ValueError."""
    dice = _dice_args(dice, focal_gamma_value(focal_gamma), label_smoothing_value(label_smoothing), ohem_value(ohem))
    lovasz = _lovasz_args(lovasz, focal_gamma_value(focal_gamma), label_smoothing_value(label_smoothing), ohem_value(ohem), dice)
    label_relax = _label_relax_args(label_relax, focal_gamma_value(focal_gamma), label_smoothing_value(label_smoothing), ohem_value(ohem), dice, lovasz)
    weight, focal_gamma, label_smoothing = _focal_args(weight, focal_gamma, logits.device, logits.shape[1], label_smoothing, relax=label_relax)
    ohem = _ohem_args(ohem, focal_gamma, label_smoothing, ignore_index)
    if ohem is not None:
        target = ohem_target(logits, target, ignore_index, *ohem)
    if label_relax is not None:
        return _CrossEntropy.apply(logits, target, ignore_index, weight, focal_gamma, label_smoothing, label_relax)
    ce =_CrossEntropy.apply(logits, target, ignore_index, weight, focal_gamma, label_smoothing)
    if lovasz is not None:
        return ce + _LovaszLoss.apply(logits, target, int(ignore_index), lovasz)
    return ce if dice is None else ce + _DiceLoss.apply(logits, target, int(ignore_index), dice)


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = pm_dense(a)
        b = pm_dense(b)
        if a.shape != b.shape:
            raise DsrlHipError(f'mse: shapes differ {tuple(a.shape)} vs {tuple(b.shape)}')
        n = a.numel()
        out = torch.empty(1, device=a.device, dtype=torch.float32)
        ws = _ws(cquery('dsrl_mse_workspace_bytes', n), a)
        call('dsrl_mse_fwd', a.data_ptr(), b.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        ctx.save_for_backward(a, b)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.reshape(1).contiguous().float()
        da = new_cl(tuple(a.shape), a)
        call('dsrl_mse_bwd', a.data_ptr(), b.data_ptr(), a.numel(), g.data_ptr(), da.data_ptr(), _stream())
        return da, None


def mse_loss(a, b):
    return _MSE.apply(a, b)


class _FusedLosses(torch.autograd.Function):
    """vals = [CE, w1 * MSE, w2 * FA, total, NaN flag] of train_or_resume.py:435-438 with the big gradients produced in the FORWARD pass:
    one pass over the logits gives the CE value and d(CE)/d(logits), one over the SISR output the MSE value and its gradient
    (dsrl_ce_fused / dsrl_mse_fused), both also check their input for NaN.  Contract: `vals[3]` is the root of the backward pass, i.e.
    its incoming gradient is 1 (TrainStep calls vals[3].backward()); the stored gradients are returned as they are."""

    @staticmethod
    def forward(ctx, sssr, sisr, ft1, ft2, target, org, ignore_index, w1, w2, stage, flag, k, weight=None, gamma=0.0, eps=0.0, dice=None, lovasz=None,
                relax=None):
        want = bool(ctx.needs_input_grad[0])          # forward-only (validation, no_grad): no gradient buffers are written
        logits, ld = pm(sssr)
        _need_gpu(target)
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        target = target.contiguous()
        N, Cc, H, W = logits.shape
        P = N * H * W
        if target.numel() != P:
            raise DsrlHipError(f'fused_losses: target has {target.numel()} pixels, logits {P}')
        st = _stream()
        dev = logits.device
        scal = torch.empty(8, device=dev, dtype=torch.float32)          # [0:2] CE + pixel count, [2] MSE
        vals = torch.empty(5, device=dev, dtype=torch.float32)
        lg = getattr(sssr, '_dsrl_logits_grad', None) if want else None
        if lg is not None and not (ld == Cc and lg.usable(logits, target)):
            lg = None
        dl = new_cl((N, Cc, H, W), logits) if (want and lg is None) else None      # lg: the producer of the logits forms this gradient in its own backward
        if lg is not None and lg.value is not None and lg.value_key == (target.data_ptr(), int(ignore_index), flag.data_ptr(),
                                                                        0 if weight is None else weight.data_ptr(),
                                                                        0 if relax is None else relax.data_ptr(), eps, gamma):
            scal = lg.value                                             # the producer's forward kernel evaluated the loss (logits_target)
        else:
            sfx, extra = _ce_variant(weight, gamma, eps, relax)
            ws = _ws(cquery(f'dsrl_ce_fused{sfx}_workspace_bytes', P), logits)
            call('dsrl_ce_fused' + sfx, logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), *extra,
                 None if dl is None else dl.data_ptr(), Cc, scal.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), st)
        ce_ptr = scal.data_ptr()
        rec = None
        if dice is not None:
            # the Dice term: one more pass over the logits leaves the record, its value joins the CE in the slot the mix reads, and
            # without a hand-over its row is added to d(CE)/d(logits) here - before any transformer contribution, as the fused backward orders them
            rec = _dice_record(logits, ld, target, P, Cc, ignore_index, dice, flag)
            ce_dice = scal[0:1] + rec[0:1]
            ce_ptr = ce_dice.data_ptr()
            if dl is not None:
                call('dsrl_dice_bwd', logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), rec.data_ptr(), 1, dl.data_ptr(), Cc, st)
        lrec = None
        if lovasz is not None:
            # the Lovasz-Softmax term, wired as the Dice term is: one more pass leaves the record, record[0] joins the CE value,
            # and without a hand-over the row is added to d(CE)/d(logits) here
            lrec = _lovasz_record(logits, ld, target, P, Cc, ignore_index, lovasz, flag)
            ce_lov = scal[0:1] + lrec[0:1]
            ce_ptr = ce_lov.data_ptr()
            if dl is not None:
                call('dsrl_lovasz_bwd', logits.data_ptr(), ld, target.data_ptr(), P, Cc, int(ignore_index), lrec.data_ptr(), lovasz[1], 1, dl.data_ptr(), Cc, st)
        da = None
        mse_ptr = fa_ptr = None
        ctx.fa = None
        if stage > 1:
            a = pm_dense(sisr); b = pm_dense(org)
            if a.shape != b.shape:
                raise DsrlHipError(f'fused_losses: SISR output {tuple(a.shape)} vs input_org {tuple(b.shape)}')
            da = new_cl(tuple(a.shape), a) if want else None
            ws2 = _ws(cquery('dsrl_mse_workspace_bytes', a.numel()), a)
            mse_ptr = scal.data_ptr() + 8
            call('dsrl_mse_fused', a.data_ptr(), b.data_ptr(), a.numel(), float(w1), None if da is None else da.data_ptr(), mse_ptr, flag.data_ptr(),
                 ws2.data_ptr(), ws2.numel(), st)
        if stage > 2:
            _need_gpu(ft1, ft2); _f32(ft1); _f32(ft2)
            if ft1.stride() != ft2.stride() or ft1.data_ptr() % 4 or ft2.data_ptr() % 4:
                ft1, ft2 = ft1.contiguous(), ft2.contiguous()
            nan_check_(flag, ft1, ft2)
            B, Cf, Hf, Wf = ft1.shape
            fa_out = torch.empty(1, device=dev, dtype=torch.float32)
            saved = torch.empty(cquery('dsrl_fa_saved_floats', B, Cf, Hf, Wf, k), device=dev, dtype=torch.float32)
            ws3 = _ws(cquery('dsrl_fa_workspace_bytes', B, Cf, Hf, Wf, k), ft1)
            sb, sc, sh, sw = ft1.stride()
            call('dsrl_fa_fwd', ft1.data_ptr(), ft2.data_ptr(), B, Cf, Hf, Wf, sb, sc, sh, sw, k, 0, fa_out.data_ptr(), saved.data_ptr(),
                 ws3.data_ptr(), ws3.numel(), st)
            fa_ptr = fa_out.data_ptr()
            ctx.fa = (ft1, ft2, saved, k, fa_out)
        call('dsrl_loss_mix', ce_ptr, mse_ptr, fa_ptr, float(w1), float(w2), flag.data_ptr(), vals.data_ptr(), st)
        if lg is not None:
            lg.target = target; lg.ignore_index = int(ignore_index); lg.count = scal; lg.ft = None; lg.weight = weight; lg.gamma = gamma; lg.eps = eps; lg.armed = True
            lg.dice = rec
            lg.lovasz = None if lrec is None else (lrec, lovasz[1])
            lg.relax = relax
        ctx.lg = lg
        ctx.grads = (dl, da)
        ctx.w2 = float(w2)
        ctx.slots = (getattr(sssr, '_dsrl_out_slot', None), getattr(sisr, '_dsrl_out_slot', None) if stage > 1 else None)
        ctx.keep = scal
        return vals

    @staticmethod
    def backward(ctx, g):
        dl, da = ctx.grads
        if dl is None and ctx.lg is None:
            raise DsrlHipError('fused_losses: backward without a gradient-enabled forward')
        # the gradients were written by the forward pass for d(total) = 1: a caller that scales the loss or differentiates another element would get
        # them unscaled.  Checked once per process (one host read), outside graph capture - the training step's own call pattern never changes.
        global _fused_losses_root_checked
        if not _fused_losses_root_checked and not torch.cuda.is_current_stream_capturing():
            gv = g.detach().float().cpu()
            if gv.numel() != 5 or float(gv[3]) != 1.0 or float(gv[:3].abs().sum()) != 0.0 or float(gv[4]) != 0.0:
                raise DsrlHipError('fused_losses: only vals[3].backward() with unit gradient is supported (the loss gradients are formed in the forward '
                                   f'pass); got an incoming gradient of {gv.tolist()} - use functional.cross_entropy / mse_loss / FALoss for a scaled loss')
            _fused_losses_root_checked = True
        d1 = d2 = None
        if ctx.fa is not None:
            ft1, ft2, saved, k, _ = ctx.fa
            B, Cf, Hf, Wf = ft1.shape
            gw = _const1(ctx.w2, ft1.device)
            d1 = torch.empty((B, Cf, Hf, Wf), device=ft1.device, dtype=torch.float32)
            d2 = torch.empty_like(d1)
            sb, sc, sh, sw = ft1.stride()
            call('dsrl_fa_bwd', ft1.data_ptr(), ft2.data_ptr(), B, Cf, Hf, Wf, sb, sc, sh, sw, k, 0, gw.data_ptr(), saved.data_ptr(),
                 d1.data_ptr(), d2.data_ptr(), None, 0, _stream())
        # publish the two dense gradients: the stride-8 feature transformers add their sparse contributions into them (GradSlot protocol) and hand
        # them on as their own input gradient.  Returned from here, a buffer would be summed with the gradient of any other consumer of the output
        # that reached autograd first - before the transformer's part is in it, which would then be lost.
        out = [dl, da]
        for i, (slot, buf) in enumerate(zip(ctx.slots, (dl, da))):
            if slot is not None and buf is not None and not slot.closed and slot.buf is None:
                slot.buf = buf
                out[i] = None
        return out[0], out[1], d1, d2, None, None, None, None, None, None, None, None, None, None, None, None, None, None


_fused_losses_root_checked = False
_const_cache = {}


def _const1(value, device):
    """One-element fp32 device constant, created once per (value, device): a torch.full per step is a 5 us launch."""
    key = (float(value), device)
    c = _const_cache.get(key)
    if c is None:
        if torch.cuda.is_current_stream_capturing():
            return torch.full((1,), float(value), device=device, dtype=torch.float32)
        c = _const_cache[key] = torch.full((1,), float(value), device=device, dtype=torch.float32)
    return c


def fused_losses_backward(vals):
    """vals[3].backward() without autograd's select / ones / zeros launches at the root of the pass: the unit gradient of element 3 is a
    cached constant."""
    drop_planes()               # every forward consumer of this step's plane operands has been enqueued
    key = ('e3', vals.device)
    e3 = _const_cache.get(key)
    if e3 is None:
        if torch.cuda.is_current_stream_capturing():
            vals[3].backward()
            return
        e3 = _const_cache[key] = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=vals.device, dtype=torch.float32)
    torch.autograd.backward([vals], [e3])


def fused_losses(outs, target, input_org, ignore_index, w1, w2, stage, flag, subsample_factor=8, weight=None, focal_gamma=0.0, label_smoothing=0.0,
                 ohem=None, dice=None, lovasz=None, label_relax=None):
    """-> 5-float device tensor [CE, w1*MSE, w2*FA, total, NaN flag]; `outs` = DSRL.forward's 4-tuple.  vals[3].backward() is the only
    supported backward (the function is the root of the pass); `flag` is the int32 NaN flag the fused kernels OR into.  weight: per-class CE
    weights (None, one number per class, or a class_weight_table): nn.CrossEntropyLoss(weight=).  focal_gamma > 0 makes the CE term the focal loss
    (as cross_entropy); 0 changes nothing.  label_smoothing in (0, 1] makes it torch's label-smoothed loss (as cross_entropy); 0 changes nothing.
    ohem (as cross_entropy) mines the hard pixels first: the target is rewritten on the device (ohem_target, which ORs into `flag` too) and
    everything after it - the loss pass, the hand-over to the layer that produced the logits - runs on the rewritten target as it stands.
    dice (as cross_entropy) adds the soft Dice term lambda L_dice of this call's pixels: vals[0] = CE + lambda L_dice and vals[3] includes it; the
    gradient of the term is added to d(CE)/d(logits), inside the ConvTranspose backward when the hand-over engages (dsrl_convt2x2_bwd_ce_d).  The CE
    then runs on the weighted kernels (all-ones weights when `weight` is None); not together with focal_gamma > 0, label_smoothing > 0 or ohem.
    lovasz (as cross_entropy) adds the quantised Lovasz-Softmax term in the same way (dsrl_convt2x2_bwd_ce_l when the hand-over engages); not
    together with any of the others but `weight`.
    label_relax (as cross_entropy: a radius, or the ready mask of relax_mask) makes the CE term the relaxed loss: dsrl_ce_fused_r, or the value of
    the logits layer's forward (logits_target given the same mask) and dsrl_convt2x2_bwd_ce_r when the hand-over engages; likewise with `weight`
    only."""
    sssr, sisr, ft1, ft2 = outs
    dice = _dice_args(dice, focal_gamma_value(focal_gamma), label_smoothing_value(label_smoothing), ohem_value(ohem))
    lovasz = _lovasz_args(lovasz, focal_gamma_value(focal_gamma), label_smoothing_value(label_smoothing), ohem_value(ohem), dice)
    label_relax = _label_relax_args(label_relax, focal_gamma_value(focal_gamma), label_smoothing_value(label_smoothing), ohem_value(ohem), dice, lovasz)
    weight, focal_gamma, label_smoothing = _focal_args(weight, focal_gamma, sssr.device, sssr.shape[1], label_smoothing, dice, lovasz, label_relax)
    ohem = _ohem_args(ohem, focal_gamma, label_smoothing, ignore_index)
    if ohem is not None:
        target = ohem_target(sssr, target, ignore_index, *ohem, flag=flag)
    relax_arg = () if label_relax is None else (_relax_mask_of(label_relax, target.reshape(-1, *target.shape[-2:]), sssr.shape[1], ignore_index),)
    dummy = _const1(0.0, sssr.device)            # stands in for the outputs a lower stage does not have (a cached constant: no fill launch per step)
    return _FusedLosses.apply(sssr, sisr if stage > 1 else dummy, ft1 if stage > 2 else dummy, ft2 if stage > 2 else dummy, target,
                              input_org if stage > 1 else dummy, int(ignore_index), float(w1), float(w2), int(stage), flag, int(subsample_factor), weight,
                              focal_gamma, label_smoothing, dice, lovasz, *relax_arg)


_RED = {'mean': 0, 'sum': 1, 'none': 2}


class _FALoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fm1, fm2, k, reduction):
        _need_gpu(fm1, fm2); _f32(fm1); _f32(fm2)
        if fm1.stride() != fm2.stride() or fm1.data_ptr() % 4 or fm2.data_ptr() % 4:
            fm1, fm2 = fm1.contiguous(), fm2.contiguous()
        B, Cc, H, W = fm1.shape
        red = _RED[reduction]
        if k <= 0:                  # the library refuses it too, but the size of 'none' below divides by k first
            raise DsrlHipError(f'fa_loss: subsample factor {k} must be positive')
        n = (W // k) ** 2
        out = torch.empty((B, Cc, n * n) if red == 2 else (1,), device=fm1.device, dtype=torch.float32)
        saved = torch.empty(cquery('dsrl_fa_saved_floats', B, Cc, H, W, k), device=fm1.device, dtype=torch.float32)
        ws = _ws(cquery('dsrl_fa_workspace_bytes', B, Cc, H, W, k), fm1)
        sb, sc, sh, sw = fm1.stride()
        call('dsrl_fa_fwd', fm1.data_ptr(), fm2.data_ptr(), B, Cc, H, W, sb, sc, sh, sw, k, red, out.data_ptr(), saved.data_ptr(),
             ws.data_ptr(), ws.numel(), _stream())
        ctx.save_for_backward(fm1, fm2, saved)
        ctx.cfg = (k, red)
        return out if red == 2 else out[0].clone()

    @staticmethod
    def backward(ctx, g):
        fm1, fm2, saved = ctx.saved_tensors
        k, red = ctx.cfg
        if red == 2:
            raise DsrlHipError("FALoss(reduction='none') has no backward kernel; use 'mean' or 'sum'")
        B, Cc, H, W = fm1.shape
        g = g.reshape(1).contiguous().float()
        d1 = torch.empty((B, Cc, H, W), device=fm1.device, dtype=torch.float32)
        d2 = torch.empty_like(d1)
        sb, sc, sh, sw = fm1.stride()
        call('dsrl_fa_bwd', fm1.data_ptr(), fm2.data_ptr(), B, Cc, H, W, sb, sc, sh, sw, k, red, g.data_ptr(), saved.data_ptr(),
             d1.data_ptr(), d2.data_ptr(), None, 0, _stream())
        return d1, d2, None, None


def fa_loss(fm1, fm2, subsample_factor=8, reduction='mean'):
    return _FALoss.apply(fm1, fm2, int(subsample_factor), reduction)


# ------------------------------------------------------------------------------------------------ optimiser / checks
def sgd_step_(p, g, buf, lr, momentum, weight_decay, grad_scale=1.0):
    """In-place SGD(momentum, weight_decay) on flat fp32 arenas."""
    _need_gpu(p, g, buf)
    call('dsrl_sgd_step', p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), float(lr), float(momentum), float(weight_decay),
         float(grad_scale), _stream())


def sgd_step_dev_(p, g, buf, hyper):
    """The same update with (lr, momentum, weight_decay, grad_scale) read from the 4-float device tensor `hyper` at run time."""
    _need_gpu(p, g, buf, hyper)
    call('dsrl_sgd_step_dev', p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), hyper.data_ptr(), _stream())


def sgd_step_ema_(p, g, buf, lr, momentum, weight_decay, grad_scale, ema, record):
    """sgd_step_ with the weight average `ema` updated from the new p in the same launch (`record`: the 16-byte EMA record, ema_record())."""
    _need_gpu(p, g, buf, ema, record)
    call('dsrl_sgd_step_ema', p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), float(lr), float(momentum), float(weight_decay),
         float(grad_scale), ema.data_ptr(), record.data_ptr(), _stream())


def sgd_step_dev_ema_(p, g, buf, hyper, ema, record):
    """sgd_step_dev_ with the weight average updated in the same launch."""
    _need_gpu(p, g, buf, hyper, ema, record)
    call('dsrl_sgd_step_dev_ema', p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), hyper.data_ptr(), ema.data_ptr(), record.data_ptr(), _stream())


# ------------------------------------------------------------------------------------------------ weight EMA
EMA_DEFAULT = (0.999, True)             # decay, warmup of `ema=True`


def ema_value(x):
    """The weight average as (decay, warmup), or None when it is off.  None / False: off; True: EMA_DEFAULT; a number d in (0, 1): (d, True); a pair
    (decay, warmup); a mapping with the keys 'decay' and / or 'warmup' (a missing one takes its default).  decay: a number in (0, 1), also as fp32;
    warmup: a bool.  ValueError on anything else - a bool where the decay belongs, a NaN, an unknown key.  Touches no device."""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)):
        return EMA_DEFAULT if x else None
    if isinstance(x, dict):
        if not x or set(x) - {'decay', 'warmup'}:
            raise ValueError(f"ema = {x!r}: expected a mapping with the keys 'decay' and 'warmup'")
        decay, warmup = x.get('decay', EMA_DEFAULT[0]), x.get('warmup', EMA_DEFAULT[1])
    elif isinstance(x, (tuple, list)) and len(x) == 2:
        decay, warmup = x
    elif isinstance(x, (int, float, np.integer, np.floating)):
        decay, warmup = x, True
    else:
        raise ValueError(f'ema = {x!r}: expected None, a bool, a decay in (0, 1), a pair (decay, warmup) or a mapping with these keys')
    if isinstance(decay, (bool, np.bool_)) or not isinstance(decay, (int, float, np.integer, np.floating)):
        raise ValueError(f'ema: decay = {decay!r}: expected a number in (0, 1)')
    d = float(decay)
    if not (0.0 < d < 1.0) or not (0.0 < float(np.float32(d)) < 1.0):            # (a NaN fails the comparison; the kernels take it as fp32)
        raise ValueError(f'ema: decay = {decay!r}: expected a number in (0, 1)')
    if not isinstance(warmup, (bool, np.bool_)):
        raise ValueError(f'ema: warmup = {warmup!r}: expected a bool')
    return d, bool(warmup)


def ema_decay(t, decay_max, warmup):
    """d_t, the decay of update number t (0-based), in fp32 as dsrl_ema_advance computes it: min(decay_max, (1 + t) / (10 + t)) under warm-up."""
    d = np.float32(decay_max)
    if warmup:
        tf = np.float32(t)
        d = min(d, (np.float32(1) + tf) / (np.float32(10) + tf))
    return np.float32(d)


def ema_record(decay_max, warmup, updates, device):
    """A new EMA record (include/dsrl_hip.h: {omd, decay_max, updates, warmup}) as a 4-word int32 tensor on `device`, omd = 1 - d_updates."""
    omd = np.float32(1) - ema_decay(updates, decay_max, warmup)
    words = np.zeros(4, dtype=np.int32)
    words[:2] = np.array([omd, decay_max], dtype=np.float32).view(np.int32)
    words[2:] = np.array([updates, 1 if warmup else 0], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(words).to(device)


def ema_record_read(record):
    """The record's fields on the host (one synchronising read): {'omd', 'decay_max', 'updates', 'warmup'}."""
    words = record.detach().cpu().numpy()
    f = words[:2].view(np.float32)
    u = words[2:].view(np.uint32)
    return {'omd': float(f[0]), 'decay_max': float(f[1]), 'updates': int(u[0]), 'warmup': bool(u[1])}


def ema_update_(ema, p, record):
    """ema <- ema + omd (p - ema) on flat fp32 arenas, omd read from the record when the kernel runs."""
    _need_gpu(ema, p, record)
    if ema.numel() != p.numel():
        raise DsrlHipError(f'ema_update: {ema.numel()} and {p.numel()} elements')
    call('dsrl_ema_update', ema.data_ptr(), p.data_ptr(), p.numel(), record.data_ptr(), _stream())


def ema_advance_(record):
    """Once per step behind its last EMA launch: updates += 1 and the next omd, on the device."""
    _need_gpu(record)
    call('dsrl_ema_advance', record.data_ptr(), _stream())


def arena_swap_(a, b):
    """Exchanges the contents of two flat fp32 arenas in place (bit patterns)."""
    _need_gpu(a, b)
    if a.numel() != b.numel() or a.dtype != torch.float32 or b.dtype != torch.float32 or not (a.is_contiguous() and b.is_contiguous()):
        raise DsrlHipError('arena_swap: two contiguous fp32 arenas of one size expected')
    call('dsrl_arena_swap', a.data_ptr(), b.data_ptr(), a.numel(), _stream())


# ------------------------------------------------------------------------------------------------ gradient-norm clipping
GRAD_CLIP_TILE = 1024                   # floats per tile of dsrl_grad_sumsq, anchored at the arena's first float
GRAD_CLIP_RECORD_WORDS = 16             # include/dsrl_hip.h: the 64-byte clip record


def grad_clip_value(x):
    """The clipping threshold as a float, or None when clipping is off.  None / False: off; a number > 0 (inf: monitor only) or a mapping
    {'max_norm': such a number}: that float.  ValueError on anything else - True, 0, a negative number, a NaN, an unknown key.  Touches no device."""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)):
        if x:
            raise ValueError('grad_clip = True: expected the threshold itself, a number > 0')
        return None
    if isinstance(x, dict):
        if set(x) != {'max_norm'}:
            raise ValueError(f"grad_clip = {x!r}: expected a mapping with the key 'max_norm'")
        x = x['max_norm']
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f'grad_clip: max_norm = {x!r}: expected a number > 0')
    v = float(x)
    if not (v > 0.0) or not (float(np.float32(v)) > 0.0):          # (a NaN fails the comparison; the kernel takes it as fp32)
        raise ValueError(f'grad_clip: max_norm = {x!r}: expected a number > 0')
    return v


def grad_clip_record(max_norm, device):
    """A new clip record (include/dsrl_hip.h) as a 16-word int32 tensor on `device`: max_norm set, everything else zero."""
    words = np.zeros(GRAD_CLIP_RECORD_WORDS, dtype=np.int32)
    words[6:7] = np.array([max_norm], dtype=np.float32).view(np.int32)
    return torch.from_numpy(words).to(device)


def grad_clip_record_read(rec):
    """The record's fields on the host (one synchronising read)."""
    words = rec.detach().cpu().numpy()
    d = words[:4].view(np.float64)
    f = words[4:8].view(np.float32)
    u = words[8:11].view(np.uint32)
    return {'sumsq': float(d[0]), 'norm_sum': float(d[1]), 'norm': float(f[0]), 'coef': float(f[1]), 'max_norm': float(f[2]), 'norm_max': float(f[3]),
            'steps': int(u[0]), 'clipped': int(u[1]), 'nonfinite': int(u[2])}


def grad_clip_workspace(n, device):
    """The float64 workspace of an n-float arena: its ceil(n / 1024) tile sums first, the scratch of the finish behind them."""
    return torch.empty(int(query('dsrl_grad_clip_workspace_bytes', int(n))) // 8, dtype=torch.float64, device=device)


def _room_behind(t):
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def grad_sumsq_(g, first, tiles):
    """Sums of squares of the 1024-float tiles of `g`, a range of a flat fp32 arena that starts at the arena's float `first` (a multiple of 1024),
    into tiles[first / 1024 ...] (float64, indexed from the arena's first tile).  Only the tiles of the range are written."""
    _need_gpu(g, tiles)
    first = int(first)
    if g.dtype != torch.float32 or tiles.dtype != torch.float64 or not (g.is_contiguous() and tiles.is_contiguous()):
        raise DsrlHipError('grad_sumsq: a contiguous fp32 range and a contiguous float64 tile array expected')
    if first >= 0 and first // GRAD_CLIP_TILE + -(-g.numel() // GRAD_CLIP_TILE) > tiles.numel():
        raise DsrlHipError(f'grad_sumsq: {g.numel()} floats from {first} need more than the {tiles.numel()} tiles given')
    call('dsrl_grad_sumsq', g.data_ptr() - 4 * first, first, g.numel(), tiles.data_ptr(), _stream())


def grad_clip_finish_(tiles, record, hyper_out, hyper=None, hp=None):
    """Behind the grad_sumsq_ launches of a step: S = the sum of `tiles` (the first tiles.numel() doubles of a grad_clip_workspace), the clip
    coefficient from it and record['max_norm'], hyper_out = {lr, momentum, weight_decay, grad_scale * coef} and the record's figures.  The four
    hyper-parameters come from the device tensor `hyper`, or from the host values `hp` = (lr, momentum, weight_decay, grad_scale)."""
    _need_gpu(tiles, record, hyper_out, hyper)
    if (hyper is None) == (hp is None):
        raise DsrlHipError('grad_clip_finish: exactly one of hyper (device) and hp (host values) expected')
    if tiles.dtype != torch.float64 or not tiles.is_contiguous() or _room_behind(tiles) < int(cquery('dsrl_grad_clip_workspace_bytes', tiles.numel() * GRAD_CLIP_TILE)):
        raise DsrlHipError('grad_clip_finish: `tiles` must be the tile sums at the start of a grad_clip_workspace')
    if record.numel() * record.element_size() != 4 * GRAD_CLIP_RECORD_WORDS or hyper_out.dtype != torch.float32 or hyper_out.numel() != 4 or \
            (hyper is not None and (hyper.dtype != torch.float32 or hyper.numel() != 4 or hyper.data_ptr() == hyper_out.data_ptr())):
        raise DsrlHipError('grad_clip_finish: a 64-byte record and 4-float hyper-parameter tensors (two different ones) expected')
    h = (0.0, 0.0, 0.0, 0.0) if hp is None else tuple(float(v) for v in hp)
    call('dsrl_grad_clip_finish', tiles.data_ptr(), tiles.numel(), None if hyper is None else hyper.data_ptr(), h[0], h[1], h[2], h[3], record.data_ptr(),
         hyper_out.data_ptr(), _stream())


# ------------------------------------------------------------------------------------------------ AdamW
ADAMW_DEFAULT = (0.9, 0.999, 1e-8)      # beta1, beta2, eps of `optimizer='adamw'`: torch.optim.AdamW's
ADAMW_RECORD_WORDS = 16                 # include/dsrl_hip.h: the 64-byte AdamW record


def adamw_value(x):
    """dataset['optimizer'] as (beta1, beta2, eps) for AdamW, or None for SGD.  None / 'sgd' / {'name': 'sgd'}: None; 'adamw': ADAMW_DEFAULT; a mapping
    {'name': 'adamw', 'betas': (b1, b2), 'eps': e} ('betas' and 'eps' optional) with 0 <= b < 1 (also as fp32) and a finite e >= 0: those values.
    ValueError on anything else - an unknown name or key, a bool or NaN where a number belongs, a beta of 1.  Touches no device."""
    def number(v, what):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f'optimizer: {what} = {v!r}: expected a number')
        return float(v)

    if x is None:
        return None
    if isinstance(x, str):
        x = {'name': x}
    if not isinstance(x, dict) or 'name' not in x or set(x) - {'name', 'betas', 'eps'}:
        raise ValueError(f"optimizer = {x!r}: expected None, 'sgd', 'adamw' or a mapping with the keys 'name', 'betas' and 'eps'")
    name = x['name']
    if name == 'sgd' and set(x) == {'name'}:
        return None
    if name != 'adamw':
        raise ValueError(f"optimizer = {x!r}: expected the name 'sgd' (without options) or 'adamw'")
    betas, eps = x.get('betas', ADAMW_DEFAULT[:2]), number(x.get('eps', ADAMW_DEFAULT[2]), 'eps')
    if not isinstance(betas, (tuple, list)) or len(betas) != 2:
        raise ValueError(f'optimizer: betas = {betas!r}: expected a pair (beta1, beta2)')
    b1, b2 = (number(b, 'beta') for b in betas)
    for b in (b1, b2):
        if not (0.0 <= b < 1.0) or not (float(np.float32(b)) < 1.0):           # (a NaN fails the comparison; the kernels multiply v by beta2 as fp32)
            raise ValueError(f'optimizer: betas = {betas!r}: expected 0 <= beta < 1')
    if not (0.0 <= eps < float('inf')):
        raise ValueError(f'optimizer: eps = {eps!r}: expected a finite number >= 0')
    return b1, b2, eps


def adamw_record(beta1, beta2, eps, device):
    """A fresh AdamW record (include/dsrl_hip.h) as a 16-word int32 tensor on `device`: the betas as float and as double, 1 - beta rounded from the
    double difference, eps, t = 0.  The two bias-correction factors are the device's to write (adamw_advance_, adamw_set_step_); no launch may read
    the record before one of them ran."""
    words = np.zeros(ADAMW_RECORD_WORDS, dtype=np.int32)
    words[:3] = np.array([beta1, beta2, eps], dtype=np.float32).view(np.int32)
    words[5:7] = np.array([1.0 - float(beta1), 1.0 - float(beta2)], dtype=np.float32).view(np.int32)
    words[10:14] = np.array([beta1, beta2], dtype=np.float64).view(np.int32)
    return torch.from_numpy(words).to(device)


def adamw_record_read(record):
    """The record's fields on the host (one synchronising read)."""
    words = record.detach().cpu().numpy()
    f = words[:7].view(np.float32)
    return {'beta1': float(words[10:12].view(np.float64)[0]), 'beta2': float(words[12:14].view(np.float64)[0]), 'eps': float(f[2]),
            'ss_factor': float(f[3]), 'isq': float(f[4]), 't': int(words[8:10].view(np.int64)[0])}


def _adamw_check(record, *arenas):
    _need_gpu(record, *arenas)
    if record.numel() * record.element_size() != 4 * ADAMW_RECORD_WORDS:
        raise DsrlHipError('adamw: a 64-byte AdamW record (adamw_record) expected')
    if any(a.numel() != arenas[0].numel() or a.dtype != torch.float32 or not a.is_contiguous() for a in arenas):
        raise DsrlHipError('adamw: contiguous fp32 arenas of one size expected')


def adamw_advance_(record):
    """Once per optimiser pass, in front of its launches: t += 1 and the factors of the new t, on the device."""
    _adamw_check(record)
    call('dsrl_adamw_advance', record.data_ptr(), _stream())


def adamw_set_step_(record, t):
    """t (optimiser passes done so far) and its factors into the record, through the device code of adamw_advance_."""
    _adamw_check(record)
    call('dsrl_adamw_set_step', record.data_ptr(), int(t), _stream())


def adamw_step_(p, g, m, v, lr, weight_decay, grad_scale, record):
    """In-place torch.optim.AdamW step on flat fp32 arenas (m: exp_avg, v: exp_avg_sq) at the t the record holds."""
    _adamw_check(record, p, g, m, v)
    call('dsrl_adamw_step', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(weight_decay), float(grad_scale),
         record.data_ptr(), _stream())


def adamw_step_dev_(p, g, m, v, hyper, record):
    """The same update with {lr, -, weight_decay, grad_scale} read from the 4-float device tensor `hyper` (the SGD launches' record) at run time."""
    _adamw_check(record, p, g, m, v)
    _need_gpu(hyper)
    call('dsrl_adamw_step_dev', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper.data_ptr(), record.data_ptr(), _stream())


def adamw_step_ema_(p, g, m, v, lr, weight_decay, grad_scale, record, ema, ema_record):
    """adamw_step_ with the weight average `ema` updated from the new p in the same launch."""
    _adamw_check(record, p, g, m, v, ema)
    _need_gpu(ema_record)
    call('dsrl_adamw_step_ema', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(weight_decay), float(grad_scale),
         record.data_ptr(), ema.data_ptr(), ema_record.data_ptr(), _stream())


def adamw_step_dev_ema_(p, g, m, v, hyper, record, ema, ema_record):
    """adamw_step_dev_ with the weight average updated in the same launch."""
    _adamw_check(record, p, g, m, v, ema)
    _need_gpu(hyper, ema_record)
    call('dsrl_adamw_step_dev_ema', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper.data_ptr(), record.data_ptr(), ema.data_ptr(),
         ema_record.data_ptr(), _stream())


class DeviceRng:
    """Device-resident twin of the host dropout key (begin_forward): three 64-bit words {key, step, base}.  While bound, every
    dropout-bearing kernel of the device reads `key` when it runs and advance() enqueues the per-step derivation, so that a step
    captured in a hipGraph draws fresh masks on every replay (include/dsrl_hip.h: dsrl_rng_bind_device_key).  The binding is one address
    per device: advance() re-binds its own state if another DeviceRng took the device in between (a captured launch keeps the address it
    was captured with)."""
    _active = {}            # device index -> the DeviceRng whose state address is currently bound

    def __init__(self, device):
        self.state = torch.zeros(3, dtype=torch.int64, device=device)
        self.sync_from_host()
        self._bind()

    def _bind(self):
        with torch.cuda.device(self.state.device):
            call('dsrl_rng_bind_device_key', self.state.data_ptr())
        DeviceRng._active[self.state.device.index] = self

    def sync_from_host(self):
        def s64(v):
            v &= 0xFFFFFFFFFFFFFFFF
            return v - (1 << 64) if v >= (1 << 63) else v
        self.state.copy_(torch.tensor([s64(_derive(_rng_state['step'])), s64(_rng_state['step']), s64(_rng_state['seed'])], dtype=torch.int64))

    def advance(self):
        if DeviceRng._active.get(self.state.device.index) is not self:
            self._bind()
        call('dsrl_rng_advance_key', self.state.data_ptr(), _stream())

    def release(self):
        if DeviceRng._active.get(self.state.device.index) is self:
            with torch.cuda.device(self.state.device):
                call('dsrl_rng_bind_device_key', None)
            del DeviceRng._active[self.state.device.index]


def nan_check_(flag, *tensors):
    """ORs 1 into the int32 device scalar `flag` if any tensor holds a NaN (one readback for all of them)."""
    st = _stream()
    for t in tensors:
        if t is None or not t.is_cuda:
            continue
        td = t if t.is_contiguous() or t.is_contiguous(memory_format=CL) else t.contiguous()
        call('dsrl_nan_check', td.data_ptr(), td.numel(), flag.data_ptr(), st)


# ------------------------------------------------------------------------------------------------ quality of the super-resolved image
SR_QUALITY_WINDOW = 11          # the SSIM window of dsrl_sr_quality: 11 x 11 Gaussian, sigma 1.5


def _sr_quality_args(pred, ref, mean, std):
    """The argument checks of sr_quality, all of them host-side: -> (C, mean, std) as ctypes float arrays.  ValueError on anything the kernel cannot take."""
    if pred.dim() != 4 or ref.dim() != 4:
        raise ValueError(f'sr_quality: 4-D (N,C,H,W) tensors expected, got shapes {tuple(pred.shape)} and {tuple(ref.shape)}')
    if tuple(pred.shape) != tuple(ref.shape):
        raise ValueError(f'sr_quality: pred {tuple(pred.shape)} and ref {tuple(ref.shape)} differ in shape')
    N, Cc, H, W = pred.shape
    if N < 1 or Cc < 1 or Cc > 4:
        raise ValueError(f'sr_quality: at least one image of 1 to 4 channels expected, got shape {tuple(pred.shape)}')
    if H < SR_QUALITY_WINDOW or W < SR_QUALITY_WINDOW:
        raise ValueError(f'sr_quality: images of {H} x {W} are smaller than the {SR_QUALITY_WINDOW}x{SR_QUALITY_WINDOW} window of the SSIM')
    mean = [0.0] * Cc if mean is None else [float(v) for v in mean]
    std = [1.0] * Cc if std is None else [float(v) for v in std]
    if len(mean) != Cc or len(std) != Cc:
        raise ValueError(f'sr_quality: mean and std of {Cc} values expected, got {len(mean)} and {len(std)}')
    mean32, std32 = (ctypes.c_float * Cc)(*mean), (ctypes.c_float * Cc)(*std)
    if not all(math.isfinite(v) for v in mean32):
        raise ValueError(f'sr_quality: mean {mean} is not finite')
    if not all(math.isfinite(v) and v != 0.0 for v in std32):
        raise ValueError(f'sr_quality: std {std} must be finite and non-zero (as fp32)')
    return Cc, mean32, std32


def sr_quality(pred, ref, mean=None, std=None, ssim_map=False):
    """Squared error and SSIM sum of `pred` against `ref`, per image (dsrl_sr_quality, include/dsrl_hip.h): both (N,C,H,W) fp32, C <= 4, H and W >= 11;
    every value is de-normalised as x * std[c] + mean[c] and clamped to [0, 1] first (`mean`, `std`: C numbers each; None: the tensors are in [0, 1]
    already).  -> records (N, 2) float64 on the device, row n = {sse, ssim_sum} of image n (sr_quality_figures turns them into PSNR and SSIM); with
    `ssim_map` also the fp32 map (N, C, H-10, W-10).  Two launches, nothing read back; bit-identical run to run and for an image alone or in a batch.
    A bad argument is a ValueError before any device work."""
    Cc, mean32, std32 = _sr_quality_args(pred, ref, mean, std)
    with torch.no_grad():
        pred, ldp = pm(pred)
        ref, ldr = pm(ref)
        if ref.device != pred.device:
            raise DsrlHipError(f'sr_quality: pred is on {pred.device}, ref on {ref.device}')
        N, _, H, W = pred.shape
        records = torch.empty((N, 2), dtype=torch.float64, device=pred.device)
        smap = torch.empty((N, Cc, H - SR_QUALITY_WINDOW + 1, W - SR_QUALITY_WINDOW + 1), dtype=torch.float32, device=pred.device) if ssim_map else None
        nbytes = cquery('dsrl_sr_quality_workspace_bytes', N, Cc, H, W)
        ws = _ws(nbytes, pred)
        call('dsrl_sr_quality', pred.data_ptr(), ldp, ref.data_ptr(), ldr, N, Cc, H, W, mean32, std32, records.data_ptr(),
             None if smap is None else smap.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return (records, smap) if ssim_map else records


def sr_quality_figures(records, C, H, W):
    """Host side: records (N, 2) {sse, ssim_sum} of (C, H, W) images (a tensor anywhere, or an array) -> (psnr, ssim), float64 arrays of N:
    psnr = 10 log10(C H W / sse) in dB at data range 1, +inf where sse == 0; ssim = ssim_sum / (C (H-10) (W-10)).  NaN records stay NaN."""
    r = records.detach().cpu().numpy() if isinstance(records, torch.Tensor) else np.asarray(records)
    r = r.astype(np.float64).reshape(-1, 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        psnr = 10.0 * np.log10(float(C * H * W) / r[:, 0])
    ssim = r[:, 1] / float(C * (H - SR_QUALITY_WINDOW + 1) * (W - SR_QUALITY_WINDOW + 1))
    return psnr, ssim


# ------------------------------------------------------------------------------------------------ inference
def _bad_label_bit(nan_flag, target, ignore_index, num_classes):
    """bit 1 of `nan_flag`: a label outside [0, num_classes) that is not the ignore label"""
    bad = ((target != ignore_index) & (target >= num_classes)).any()
    nan_flag.bitwise_or_((bad.to(torch.int32) * 2).reshape(nan_flag.shape))


def _flip_ensemble(logits):
    """logits (2N,C,H,W), the second half computed from the mirrored images -> E (N,C,H,W) = logaddexp of the two views' log-softmax - ln 2 with the
    second view mirrored back: the log of the averaged class probabilities (include/dsrl_hip.h: dsrl_sssr_tail_predict_flip)"""
    N = logits.shape[0] // 2
    la = torch.log_softmax(logits[:N], dim=1)
    lb = torch.log_softmax(logits[N:], dim=1).flip(3)
    return torch.logaddexp(la, lb) - math.log(2.0)


def check_confusion(confusion, num_classes, device, what='sssr_tail_predict'):
    """`confusion` as every producer wants it: a contiguous int64 tensor of num_classes^2 elements on `device`"""
    if confusion.dtype != torch.int64 or confusion.numel() != num_classes * num_classes or not confusion.is_contiguous():
        raise DsrlHipError(f'{what}: confusion must be a contiguous int64 tensor of {num_classes * num_classes} elements '
                           f'(got {confusion.dtype}, {confusion.numel()} elements)')
    _need_gpu(confusion)
    if confusion.device != device:
        raise DsrlHipError(f'{what}: confusion is on {confusion.device}, the batch on {device}')


CALIBRATION_DEFAULT_BINS = 15


def calibration_max_bins():
    """the largest bin count of a calibration record (dsrl_calibration_max_bins); pure host code"""
    return int(query('dsrl_calibration_max_bins'))


def calibration_bins_value(bins, what='calibration'):
    """`bins` as an int in [1, calibration_max_bins()]; ValueError on anything else (bools, floats, strings included).  Touches no device."""
    maxb = calibration_max_bins()
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= maxb:
        raise ValueError(f'{what}: bins = {bins!r}, an integer from 1 to {maxb} expected')
    return int(bins)


def check_calibration(record, bins, device, what='sssr_tail_predict'):
    """`record` as every producer wants it: a contiguous int64 tensor of 3 * bins elements [n_b | hit_b | q_b] on `device`; `bins` from 1 to
    calibration_max_bins().  -> bins as an int.  Raises before any device work."""
    bins = calibration_bins_value(bins, what)
    if not isinstance(record, torch.Tensor) or record.dtype != torch.int64 or record.numel() != 3 * bins or not record.is_contiguous():
        got = f'{record.dtype}, {record.numel()} elements' if isinstance(record, torch.Tensor) else type(record).__name__
        raise DsrlHipError(f'{what}: calibration must be a contiguous int64 tensor of {3 * bins} elements (got {got})')
    _need_gpu(record)
    if record.device != torch.device(device):
        raise DsrlHipError(f'{what}: calibration is on {record.device}, the batch on {device}')
    return bins


def _calibration_bins_of(record, what):
    """the bin count a record tensor implies (its length over 3), checked"""
    if not isinstance(record, torch.Tensor) or record.numel() % 3 or record.numel() == 0:
        got = f'{record.numel()} elements' if isinstance(record, torch.Tensor) else type(record).__name__
        raise DsrlHipError(f'{what}: calibration must be an int64 tensor of 3 * bins elements (got {got})')
    return record.numel() // 3


def calibration_counts_(record, logits, target, ignore_index=255, bins=CALIBRATION_DEFAULT_BINS, confidence=None, nan_flag=None, temperature=None):
    """record[n_b | hit_b | q_b] += the reliability histogram of logits (N,C,H,W) against target (N,H,W) over `bins` equal-width confidence bins
    (dsrl_calibration_from_logits, include/dsrl_hip.h "calibration"): the confidence of a pixel is its maximum softmax probability, counted are the
    pixels the confusion matrix counts (target != ignore_index and < C), q is the sum of rintf(conf * 2^24).  `confidence` (float32, (N,H,W),
    contiguous, optional) receives the confidence map; `nan_flag` (int32 device scalar, optional): bit 0 a NaN logit, bit 1 a label outside the
    classes.  One streaming launch, nothing read back.  A bad argument raises before any device work.
    `temperature` (temperature_value: None and 1 are "off" and the launch is today's): the record and the map of softmax(logits / T)
    (dsrl_calibration_from_logits_t: the class is that of the logits as they are, the confidence that of the scaled ones)."""
    temperature = temperature_value(temperature, 'calibration_counts_')
    with torch.no_grad():
        if logits.dim() != 4:
            raise DsrlHipError(f'calibration_counts_: 4-D (N,C,H,W) logits expected, got shape {tuple(logits.shape)}')
        bins = check_calibration(record, bins, logits.device, 'calibration_counts_')
        _need_gpu(logits, target, nan_flag, confidence)
        N, C, H, W = logits.shape
        if tuple(target.shape) != (N, H, W):
            raise DsrlHipError(f'calibration_counts_: target {tuple(target.shape)} is not {(N, H, W)}')
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1):
            raise DsrlHipError('calibration_counts_: nan_flag must be an int32 scalar')
        if confidence is not None and (confidence.dtype != torch.float32 or tuple(confidence.shape) != (N, H, W) or not confidence.is_contiguous()
                                       or confidence.device != logits.device):
            raise DsrlHipError(f'calibration_counts_: confidence must be a contiguous float32 tensor of shape {(N, H, W)} on the logits\' device')
        logits, ld = pm(logits)
        target = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).contiguous()
        if N * H * W and temperature is None:
            call('dsrl_calibration_from_logits', logits.data_ptr(), ld, target.data_ptr(), N * H * W, C, int(ignore_index), bins, record.data_ptr(),
                 None if confidence is None else confidence.data_ptr(), None if nan_flag is None else nan_flag.data_ptr(), _stream())
        elif N * H * W:
            call('dsrl_calibration_from_logits_t', logits.data_ptr(), ld, target.data_ptr(), N * H * W, C, int(ignore_index), bins, record.data_ptr(),
                 None if confidence is None else confidence.data_ptr(), None if nan_flag is None else nan_flag.data_ptr(),
                 temperature_beta(temperature), _stream())
    return record


def _calibration_of_scores(record, scores, pred, target, ignore_index, num_classes, want_conf):
    """The fall-back of heads the fused kernels do not implement, from class probabilities `scores` (N,C,H,W) that are NOT a single softmax (the flip
    and multi-scale ensembles composed from torch ops): the confidence is the winning probability; the record is binned by the definition of
    include/dsrl_hip.h in integer torch ops (exact, order independent)."""
    conf = scores.gather(1, pred.long().unsqueeze(1))[:, 0].float().clamp(max=1.0)
    if record is not None:
        B = record.numel() // 3
        counted = (target != ignore_index) & (target < num_classes) & ~torch.isnan(conf)
        c = conf[counted]
        b = torch.clamp((c * float(B)).to(torch.int64), max=B - 1)
        hit = (pred[counted] == target[counted]).to(torch.int64)
        q = torch.round(c * 16777216.0).to(torch.int64)         # round half to even, as rintf
        rec = record.view(3, B)
        rec[0].scatter_add_(0, b, torch.ones_like(b))
        rec[1].scatter_add_(0, b, hit)
        rec[2].scatter_add_(0, b, q)
    return conf.contiguous() if want_conf else None


# ------------------------------------------------------------------------------------------------ temperature scaling
def temperature_max_points():
    """the largest number of temperatures of one dsrl_temperature_stats call; pure host code"""
    return int(query('dsrl_temperature_max_points'))


def temperature_value(x, what='temperature'):
    """`x` as a temperature T: None (absent) and 1 are "off" -> None, and every launch is then the one of a call that does not know the argument;
    a finite number > 0 -> float(T).  ValueError on anything else (bools, strings, NaN, inf, 0, negatives).  Touches no device."""
    if x is None:
        return None
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f'{what}: temperature = {x!r}, None or a finite number > 0 expected')
    T = float(x)
    with np.errstate(over='ignore', under='ignore'):
        b32 = float(np.float32(1.0 / T)) if math.isfinite(T) and T > 0.0 else 0.0
    if not math.isfinite(b32) or b32 <= 0.0:
        raise ValueError(f'{what}: temperature = {x!r}, None or a finite number > 0 (with a finite fp32 inverse) expected')
    return None if T == 1.0 else T


def temperature_beta(T):
    """beta = 1 / T as the kernels receive it: rounded to fp32 once, here (a Python float that is exactly an fp32 value)"""
    return float(np.float32(1.0 / float(T)))


def temperature_betas_value(betas, what='temperature'):
    """`betas` (a sequence of numbers or a host tensor) as a float64 array of fp32 values - what the device receives, so that a solve on the host
    uses the very numbers the kernel used: 1 to temperature_max_points() of them, each a finite number > 0.  ValueError on anything else."""
    if isinstance(betas, torch.Tensor):
        betas = betas.detach().cpu().numpy()
    try:
        b = np.asarray(betas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: betas = {betas!r}, a sequence of numbers expected') from None
    maxk = temperature_max_points()
    if not 1 <= b.size <= maxk:
        raise ValueError(f'{what}: {b.size} betas, 1 to {maxk} are possible')
    with np.errstate(over='ignore'):
        b = b.astype(np.float32).astype(np.float64)
    if not np.all(np.isfinite(b) & (b > 0.0)):
        raise ValueError(f'{what}: betas = {b.tolist()}, every one must be a finite number > 0 (in fp32)')
    return b


def temperature_grid(lo, hi, K, log=True):
    """The K values of beta = 1 / T of one pass over [lo, hi], ends included, log-spaced (the first pass: a ratio is what matters) or linearly
    spaced (the second pass, across one bracket); fp32 values as a float64 array (temperature_betas_value).  K = 1 needs lo == hi.  ValueError on
    a K outside 1..temperature_max_points(), on bounds that are not finite numbers > 0 and on lo > hi (or lo == hi with K > 1)."""
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= temperature_max_points():
        raise ValueError(f'temperature_grid: K = {K!r}, an integer from 1 to {temperature_max_points()} expected')
    K = int(K)
    for v in (lo, hi):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or float(v) <= 0.0:
            raise ValueError(f'temperature_grid: bounds ({lo!r}, {hi!r}) must be finite numbers > 0')
    lo, hi = float(lo), float(hi)
    if lo > hi or (lo == hi) != (K == 1):
        raise ValueError(f'temperature_grid: {K} points over [{lo}, {hi}] (lo < hi for K > 1, lo == hi for K == 1)')
    if K == 1:
        g = np.array([lo])
    elif log:
        g = np.exp(np.linspace(math.log(lo), math.log(hi), K))
    else:
        g = np.linspace(lo, hi, K)
    g[0], g[-1] = lo, hi
    g = temperature_betas_value(g, 'temperature_grid')
    if np.any(np.diff(g) <= 0.0):
        raise ValueError(f'temperature_grid: [{lo}, {hi}] is too narrow for {K} distinct fp32 values')
    return g


def _temperature_record_value(betas, record, what):
    """-> (betas float64 [K], record float64 [1 + 3 K]) on the host, checked against each other"""
    if isinstance(record, torch.Tensor):
        record = record.detach().cpu().numpy()
    b = np.asarray(betas.detach().cpu().numpy() if isinstance(betas, torch.Tensor) else betas, dtype=np.float64).reshape(-1)
    r = np.asarray(record, dtype=np.float64).reshape(-1)
    if b.size < 1 or r.size != 1 + 3 * b.size:
        raise ValueError(f'{what}: a record of 1 + 3 K = {1 + 3 * b.size} numbers expected for {b.size} betas, got {r.size}')
    if b.size > 1 and np.any(np.diff(b) <= 0.0):
        raise ValueError(f'{what}: the betas must ascend')
    return b, r


def _hermite(x0, x1, f0, f1, g0, g1, x):
    """the cubic through (x0, f0), (x1, f1) with slopes g0, g1, at x"""
    h = x1 - x0
    t = (x - x0) / h
    t2, t3 = t * t, t * t * t
    return (2 * t3 - 3 * t2 + 1) * f0 + (t3 - 2 * t2 + t) * h * g0 + (-2 * t3 + 3 * t2) * f1 + (t3 - t2) * h * g1


def temperature_bracket(betas, record):
    """-> (i, at_bound): the grid interval [betas[i], betas[i + 1]] that holds the root of sum G (G is monotone in beta: L is convex), or the end
    the minimum lies beyond: (0, True) when G[0] >= 0, (K - 1, True) when G[-1] <= 0.  Pure host code on a float64 record."""
    b, r = _temperature_record_value(betas, record, 'temperature_bracket')
    G = r[2::3]
    if not np.all(np.isfinite(G)):
        raise ValueError('temperature_bracket: the record holds a NaN or an infinite sum (a NaN logit, or a bad beta)')
    if G[0] >= 0.0:
        return 0, True
    if G[-1] <= 0.0:
        return b.size - 1, True
    i = int(np.nonzero(G > 0.0)[0][0]) - 1          # G[i] <= 0 < G[i + 1]
    return i, False


def temperature_solve(betas, record):
    """The fitted beta = 1 / T from one record of dsrl_temperature_stats (float64 [1 + 3 K], the sums of L, G = dL/dbeta and H = d2L/dbeta2 at the
    ascending `betas`) -> (beta, at_bound).  G is monotone in beta.  If G[0] >= 0 or G[-1] <= 0 the minimum is at or beyond that end of the grid:
    that end, at_bound=True.  Otherwise the root of the cubic Hermite interpolant of G between the two bracketing grid points (G the values, H the
    slopes), found by bisection.  Pure host code."""
    b, r = _temperature_record_value(betas, record, 'temperature_solve')
    i, at_bound = temperature_bracket(b, r)
    if at_bound:
        return float(b[i]), True
    G, H = r[2::3], r[3::3]
    lo, hi = float(b[i]), float(b[i + 1])
    if G[i] == 0.0:
        return lo, False
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if _hermite(b[i], b[i + 1], G[i], G[i + 1], H[i], H[i + 1], mid) > 0.0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi), False


def temperature_nll_at(betas, record, beta):
    """The mean NLL over the live pixels at `beta` from a record: a grid point's own value, otherwise the cubic Hermite interpolant between the two
    grid points around it (L the values, G the slopes); NaN outside the grid or for an empty record.  Pure host code."""
    b, r = _temperature_record_value(betas, record, 'temperature_nll_at')
    n, L, G = r[0], r[1::3], r[2::3]
    beta = float(beta)
    if n <= 0 or not b[0] <= beta <= b[-1]:
        return float('nan')
    j = int(np.searchsorted(b, beta))
    if b[j] == beta:
        return float(L[j] / n)
    return float(_hermite(b[j - 1], b[j], L[j - 1], L[j], G[j - 1], G[j], beta) / n)


def temperature_stats_(record, logits, target, betas, ignore_index=255, nan_flag=None):
    """record[0] += live pixels, record[1 + 3 k ..] += the sums of L, G, H at betas[k] (dsrl_temperature_stats, include/dsrl_hip.h "temperature"):
    the NLL of softmax(beta v) of logits (N,C,H,W) against target (N,H,W) with its first and second derivative in beta = 1 / T, at up to 16 values of
    beta in one streaming pass.  `record`: float64, 1 + 3 K elements, contiguous, accumulated.  `betas`: a sequence of numbers or a host tensor -
    each checked here as a finite number > 0, at most temperature_max_points() of them - or a float32 tensor on the logits' device, which is taken as
    it is (its length is checked; a bad value makes its own three entries NaN): a caller that feeds many batches uploads it once
    (metrices.TemperatureFit).  `nan_flag` (int32 device scalar, optional): bit 0 a NaN logit of a live pixel, bit 1 a label outside the classes.
    Two launches, nothing read back.  A bad argument raises before any device work."""
    with torch.no_grad():
        if logits.dim() != 4:
            raise DsrlHipError(f'temperature_stats_: 4-D (N,C,H,W) logits expected, got shape {tuple(logits.shape)}')
        on_device = isinstance(betas, torch.Tensor) and betas.device.type != 'cpu'
        if on_device:
            if betas.dtype != torch.float32 or betas.dim() != 1 or not betas.is_contiguous() or not 1 <= betas.numel() <= temperature_max_points():
                raise ValueError(f'temperature_stats_: device betas must be a contiguous float32 vector of 1 to {temperature_max_points()} elements')
            if betas.device != logits.device:
                raise DsrlHipError(f'temperature_stats_: betas are on {betas.device}, the logits on {logits.device}')
            K = betas.numel()
        else:
            host = temperature_betas_value(betas, 'temperature_stats_')
            K = host.size
        if not isinstance(record, torch.Tensor) or record.dtype != torch.float64 or record.numel() != 1 + 3 * K or not record.is_contiguous():
            got = f'{record.dtype}, {record.numel()} elements' if isinstance(record, torch.Tensor) else type(record).__name__
            raise DsrlHipError(f'temperature_stats_: record must be a contiguous float64 tensor of {1 + 3 * K} elements (got {got})')
        _need_gpu(logits, target, record, nan_flag)
        if record.device != logits.device:
            raise DsrlHipError(f'temperature_stats_: record is on {record.device}, the logits on {logits.device}')
        N, C, H, W = logits.shape
        if tuple(target.shape) != (N, H, W):
            raise DsrlHipError(f'temperature_stats_: target {tuple(target.shape)} is not {(N, H, W)}')
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1):
            raise DsrlHipError('temperature_stats_: nan_flag must be an int32 scalar')
        if not on_device:
            betas = torch.tensor(host, dtype=torch.float32).to(logits.device)
        logits, ld = pm(logits)
        target = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).contiguous()
        P = N * H * W
        if P:
            nbytes = cquery('dsrl_temperature_workspace_bytes', P, K)
            ws = _ws(nbytes, logits)
            call('dsrl_temperature_stats', logits.data_ptr(), ld, target.data_ptr(), P, C, int(ignore_index), betas.data_ptr(), K, record.data_ptr(),
                 None if nan_flag is None else nan_flag.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return record


def confusion_matrix_(confusion, pred, target, num_classes, ignore_index=255, nan_flag=None):
    """confusion[t * num_classes + p] += pixels with target t and predicted class p, from two class maps of the same shape (dsrl_confusion_matrix):
    targets equal to `ignore_index` or >= num_classes are not counted; a predicted class >= num_classes on a counted pixel raises bit 1 of `nan_flag`
    (int32 device scalar, optional) and is not counted.  `confusion`: int64, num_classes^2 elements, accumulated."""
    with torch.no_grad():
        _need_gpu(pred, target, nan_flag)
        check_confusion(confusion, int(num_classes), pred.device, 'confusion_matrix_')
        if tuple(pred.shape) != tuple(target.shape):
            raise DsrlHipError(f'confusion_matrix_: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape')
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1):
            raise DsrlHipError('confusion_matrix_: nan_flag must be an int32 scalar')
        pred = (pred if pred.dtype == torch.uint8 else pred.to(torch.uint8)).contiguous()
        target = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).contiguous()
        if pred.numel():
            call('dsrl_confusion_matrix', pred.data_ptr(), target.data_ptr(), pred.numel(), int(num_classes), int(ignore_index), confusion.data_ptr(),
                 None if nan_flag is None else nan_flag.data_ptr(), _stream())
    return confusion


def boundary_distance(H, W, ratio=0.02):
    """The band distance of Boundary IoU for H x W maps: `ratio` of the image diagonal, rounded, at least 1 (46 at 1024 x 2048 for the paper's 0.02)."""
    ratio = float(ratio)
    if not math.isfinite(ratio) or ratio <= 0.0:
        raise ValueError(f'boundary_distance: ratio = {ratio} is not a finite number > 0')
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f'boundary_distance: H = {H}, W = {W} (both >= 1)')
    return max(1, int(round(ratio * math.hypot(int(H), int(W)))))


def boundary_counts_(counts, pred, target, num_classes, ignore_index=255, distance=None, ratio=0.02, nan_flag=None, band=None):
    """counts[I | G | P] += the Boundary IoU counters of two class maps of the same shape, (N, H, W) or (H, W) (dsrl_boundary_counts,
    include/dsrl_hip.h): per class the pixels of the target's band (G), of the prediction's band (P) and of both (I), a band being the pixels whose
    (2d+1) x (2d+1) window leaves the image or holds another label.  `distance` d, or `ratio` of the diagonal (boundary_distance) when None.  Targets
    equal to `ignore_index` or >= num_classes are void, and so is the prediction under them; a predicted class >= num_classes elsewhere raises bit 1 of
    `nan_flag` (int32 device scalar, optional) and is in no class's P.  `band` (uint8, the maps' shape, contiguous, optional) receives bit 0 = target
    band, bit 1 = prediction band, 0 on void pixels.  `counts`: int64, 3 * num_classes elements, accumulated.  Two launches, nothing read back.
    A bad argument is a ValueError or DsrlHipError before any device work."""
    C = int(num_classes)
    maxc = int(query('dsrl_boundary_counts_max_classes'))
    if C < 1 or C > maxc:
        raise ValueError(f'boundary_counts_: {C} classes, 1 to {maxc} are possible')
    if tuple(pred.shape) != tuple(target.shape):
        raise DsrlHipError(f'boundary_counts_: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape')
    if pred.dim() not in (2, 3):
        raise ValueError(f'boundary_counts_: class maps of shape (N, H, W) or (H, W) expected, got {tuple(pred.shape)}')
    N = int(pred.shape[0]) if pred.dim() == 3 else 1
    H, W = int(pred.shape[-2]), int(pred.shape[-1])
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f'boundary_counts_: empty class maps of shape {tuple(pred.shape)}')
    if N * H * W >= 2 ** 31:
        raise ValueError(f'boundary_counts_: maps of {N * H * W} pixels do not fit 32-bit pixel indices')
    d = boundary_distance(H, W, ratio) if distance is None else int(distance)
    maxd = int(query('dsrl_boundary_counts_max_distance'))
    if d < 1 or d > maxd:
        raise ValueError(f'boundary_counts_: distance {d}, 1 to {maxd} are possible')
    with torch.no_grad():
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1 or nan_flag.device != pred.device):
            raise DsrlHipError('boundary_counts_: nan_flag must be an int32 scalar on the maps\' device')
        if band is not None and (band.dtype != torch.uint8 or tuple(band.shape) != tuple(pred.shape) or not band.is_contiguous() or band.device != pred.device):
            raise DsrlHipError(f'boundary_counts_: band must be a contiguous uint8 tensor of shape {tuple(pred.shape)} on the maps\' device')
        if counts.dtype != torch.int64 or counts.numel() != 3 * C or not counts.is_contiguous():
            raise DsrlHipError(f'boundary_counts_: counts must be a contiguous int64 tensor of {3 * C} elements (got {counts.dtype}, {counts.numel()} elements)')
        if target.device != pred.device or counts.device != pred.device:
            raise DsrlHipError(f'boundary_counts_: pred is on {pred.device}, target on {target.device}, counts on {counts.device}')
        _need_gpu(pred, target, counts, nan_flag, band)
        pred = (pred if pred.dtype == torch.uint8 else pred.to(torch.uint8)).contiguous()
        target = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).contiguous()
        nbytes = cquery('dsrl_boundary_counts_workspace_bytes', N, H, W, d)
        ws = _ws(nbytes, pred)
        call('dsrl_boundary_counts', pred.data_ptr(), target.data_ptr(), N, H, W, C, int(ignore_index), d, counts.data_ptr(),
             None if band is None else band.data_ptr(), None if nan_flag is None else nan_flag.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return counts


def sssr_tail_predict(x, convt1, bn, convt2, target=None, ignore_index=255, counts=None, nan_flag=None, flip=False, confusion=None, calibration=None,
                      confidence=False, temperature=None):
    """Eval-mode tail of the SSSR decoder after its bilinear x2 (DSRL.py:55-69): ConvTranspose2d k2 s2 `convt1` -> BatchNorm2d `bn` (running statistics)
    -> ReLU -> ConvTranspose2d k2 s2 `convt2` -> arg-max, as one launch that writes class indices and never the logits (dsrl_sssr_tail_predict).
    -> (pred uint8 (N,4H,4W), ce): with `target` (N,4H,4W) `ce` is the 0-d device tensor of nn.CrossEntropyLoss(ignore_index) of the logits and
    `counts` (int64 [3*classes+2], optional) gets the table of dsrl_seg_metrics ADDED; `nan_flag` (int32 scalar, optional): bit 0 NaN logit, bit 1 a
    label outside the classes.  Heads the kernel does not implement run the modules one by one and reduce their logits.
    `flip=True`: the horizontal-flip ensemble.  `x` is (2N,...): image N + n is the tail input computed from the MIRRORED image n, still in the mirrored
    frame.  -> N class maps: the arg-max of the two views' averaged class probabilities (the second view mirrored back), `ce` the loss of their
    logarithm, `target` (N,4H,4W); the same single launch (dsrl_sssr_tail_predict_flip), still no logits in memory.
    `confusion` (int64 [classes^2], optional, needs a target) gets the confusion matrix of the returned class map ADDED: confusion[t * classes + p] =
    pixels with target t and predicted class p, by the same launch (dsrl_sssr_tail_predict_cm / _flip_cm); heads the kernel does not implement
    count it from `pred` (dsrl_confusion_matrix).  Without it the launches are those of a call that does not know the argument.
    `calibration` (int64 [3*bins], optional, needs a target) gets the reliability record [n_b | hit_b | q_b] of the returned class map ADDED (the bin
    count is its length over 3; include/dsrl_hip.h "calibration"), `confidence=True` appends the confidence map (float32 (N,4H,4W): the probability of
    the reported class) to the returned tuple; both come from the same single launch (dsrl_sssr_tail_predict_ex / _flip_ex).  Heads the kernel does
    not implement go modules -> logits -> dsrl_calibration_from_logits.  Without them the launches are those of a call that does not know them.
    `temperature` (temperature_value: None and 1 are "off" and every launch is then today's; a finite number T > 0): the model reports
    softmax(logits / T).  Behind the arg-max the kernel multiplies the logits by beta = 1 / T (dsrl_sssr_tail_predict_t / _flip_t), so `ce`, the
    calibration record and the confidence map are those of the scaled model while `pred`, `counts` and `confusion` of a single view keep their bits;
    with `flip` each view is scaled in front of its softmax and the ensemble is that of the scaled model.  Heads the kernel does not implement
    multiply their logits by beta and run the reductions they run today."""
    temperature = temperature_value(temperature, 'sssr_tail_predict')
    tbeta = None if temperature is None else temperature_beta(temperature)          # (`beta` is the BatchNorm's below)
    if confusion is not None and target is None:
        raise DsrlHipError('sssr_tail_predict: confusion needs a target')
    if calibration is not None and target is None:
        raise DsrlHipError('sssr_tail_predict: calibration needs a target')
    confidence = bool(confidence)
    with torch.no_grad():
        x, ldx = pm(x)
        w1, w2, b2 = convt1.weight, convt2.weight, convt2.bias
        _need_gpu(w1, w2, b2, bn.weight, bn.bias, bn.running_mean, bn.running_var, target, counts, nan_flag, confusion)
        if bn.training or bn.running_mean is None or bn.running_var is None:
            raise DsrlHipError('sssr_tail_predict: the BatchNorm must be in eval mode and track running statistics')
        N, Ci, H, W = x.shape
        if flip:
            if N % 2:
                raise DsrlHipError(f'sssr_tail_predict: flip=True takes the two views of every image, got an odd batch of {N}')
            N //= 2
        if w1.dim() != 4 or w2.dim() != 4 or w1.shape[0] != Ci or w2.shape[0] != w1.shape[1] or bn.num_features != w1.shape[1]:
            raise DsrlHipError(f'sssr_tail_predict: {Ci} input channels do not chain through filters {tuple(w1.shape)}, {tuple(w2.shape)}')
        Cm, Co = w1.shape[1], w2.shape[1]
        if target is not None:
            if tuple(target.shape) != (N, 4 * H, 4 * W):
                raise DsrlHipError(f'sssr_tail_predict: target {tuple(target.shape)} is not {(N, 4 * H, 4 * W)}')
            if target.dtype != torch.uint8:
                target = target.to(torch.uint8)
            target = target.contiguous()
            if target.data_ptr() % 4:
                target = target.clone()
        elif counts is not None or confusion is not None:
            raise DsrlHipError('sssr_tail_predict: counts and confusion need a target')
        if confusion is not None:
            check_confusion(confusion, Co, x.device)
        bins = 0
        if calibration is not None:
            bins = check_calibration(calibration, _calibration_bins_of(calibration, 'sssr_tail_predict'), x.device)
        ex = calibration is not None or confidence
        if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 3 * Co + 2 or not counts.is_contiguous()):
            raise DsrlHipError(f'sssr_tail_predict: counts must be a contiguous int64 tensor of {3 * Co + 2} elements')
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1):
            raise DsrlHipError('sssr_tail_predict: nan_flag must be an int32 scalar')
        k2s2 = all(m.kernel_size == (2, 2) and m.stride == (2, 2) and m.padding == (0, 0) and m.output_padding == (0, 0) and m.groups == 1
                   for m in (convt1, convt2))
        if k2s2 and convt1.bias is None and cquery('dsrl_sssr_tail_predict_supported', N, H, W, Ci, Cm, Co):
            st = _stream()
            invstd = frozen_invstd(bn.running_var, bn.eps)
            if invstd is None:
                invstd = torch.empty(Cm, device=x.device, dtype=torch.float32)
                call('dsrl_bn_invstd_from_var', bn.running_var.data_ptr(), Cm, float(bn.eps), invstd.data_ptr(), st)
            pred = torch.empty((N, 4 * H, 4 * W), device=x.device, dtype=torch.uint8)
            ce = torch.empty(2, device=x.device, dtype=torch.float32) if target is not None else None
            ws = _ws(cquery('dsrl_sssr_tail_predict_workspace_bytes', N, H, W) if ce is not None else 0, x)
            gamma = bn.weight if bn.weight is not None else torch.ones_like(invstd)
            beta = bn.bias if bn.bias is not None else torch.zeros_like(invstd)
            name = ('dsrl_sssr_tail_predict_flip' if flip else 'dsrl_sssr_tail_predict') + ('_ex' if ex else '' if confusion is None else '_cm')
            conf = torch.empty((N, 4 * H, 4 * W), device=x.device, dtype=torch.float32) if confidence else None
            extra = () if confusion is None else (confusion.data_ptr(),)
            if ex or tbeta is not None:
                extra = (None if confusion is None else confusion.data_ptr(), None if calibration is None else calibration.data_ptr(), bins,
                         None if conf is None else conf.data_ptr())
            if tbeta is not None:
                name = 'dsrl_sssr_tail_predict_flip_t' if flip else 'dsrl_sssr_tail_predict_t'
                extra = extra + (tbeta,)
            call(name, x.data_ptr(), ldx, N, H, W, Ci, Cm, Co, w1.contiguous().data_ptr(), bn.running_mean.data_ptr(),
                 invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w2.contiguous().data_ptr(), None if b2 is None else b2.data_ptr(),
                 pred.data_ptr(), None if target is None else target.data_ptr(), int(ignore_index), None if counts is None else counts.data_ptr(),
                 None if ce is None else ce.data_ptr(), None if nan_flag is None else nan_flag.data_ptr(), ws.data_ptr(), ws.numel(),
                 *extra, st)
            return (pred, (None if ce is None else ce[0])) + ((conf,) if confidence else ())
        # any other head: the modules as the training forward runs them in eval mode, then the reductions over their logits
        y = batch_norm_act(convt1(x), bn, relu=True)
        logits = convt2(y)
        if nan_flag is not None:
            nan_check_(nan_flag, logits)
        if flip:
            if tbeta is not None:
                logits = logits * tbeta             # each view's softmax is that of the scaled model (beta is an fp32 value: one fp32 multiply)
            logits = _flip_ensemble(logits)         # the scores of the ensemble stand in for the logits: log_softmax(E) = E
        pred = torch.argmax(logits, dim=1).to(torch.uint8)
        # a single view's temperature: the class map and the counters come from the logits as they are, the confidence from dsrl_calibration_from_logits_t
        # (which scales behind its own first-maximum search), the loss from the scaled logits
        cal_t = temperature if not flip else None
        conf = ()
        if ex:
            # softmax(E) = exp(E), so the maximum softmax probability of the scores IS the ensemble's confidence: one producer for both forms
            cmap = torch.empty((N, 4 * H, 4 * W), device=x.device, dtype=torch.float32) if confidence else None
            if calibration is not None and cal_t is None:
                calibration_counts_(calibration, logits, target, int(ignore_index), bins, cmap)
            elif calibration is not None:
                calibration_counts_(calibration, logits, target, int(ignore_index), bins, cmap, temperature=cal_t)
            elif cal_t is None:
                lg, ld = pm(logits)
                call('dsrl_calibration_from_logits', lg.data_ptr(), ld, None, N * 16 * H * W, Co, int(ignore_index), 1, None, cmap.data_ptr(), None,
                     _stream())
            else:
                lg, ld = pm(logits)
                call('dsrl_calibration_from_logits_t', lg.data_ptr(), ld, None, N * 16 * H * W, Co, int(ignore_index), 1, None, cmap.data_ptr(), None,
                     tbeta, _stream())
            conf = (cmap,) if confidence else ()
        if target is None:
            return (pred, None) + conf
        if nan_flag is not None:
            _bad_label_bit(nan_flag, target, int(ignore_index), Co)
        if counts is not None:
            lg, ld = pm(logits)
            call('dsrl_seg_metrics', lg.data_ptr(), ld, target.data_ptr(), N * 16 * H * W, Co, int(ignore_index), counts.data_ptr(), _stream())
        if confusion is not None:
            confusion_matrix_(confusion, pred, target, Co, int(ignore_index))
        if cal_t is not None:
            logits = logits * tbeta
        return (pred, cross_entropy(logits, target, int(ignore_index))) + conf


# ------------------------------------------------------------------------------------------------ multi-scale inference
MULTISCALE_MAX_SCALES = 16


def multiscale_scales_value(scales):
    """The scales of the multi-scale ensemble as a tuple of floats, or None for "off": None, () and (1.0,) are the single-scale path.  ValueError on
    anything that is not a sequence of numbers, on bools, NaN, infinity, values <= 0 and more than 16 entries.  Touches no device."""
    if scales is None:
        return None
    what = f'scales = {scales!r}: expected at most {MULTISCALE_MAX_SCALES} finite numbers > 0'
    if isinstance(scales, (str, bytes, torch.Tensor)):
        raise ValueError(what)
    try:
        seq = tuple(scales)
    except TypeError:
        raise ValueError(what) from None
    if len(seq) > MULTISCALE_MAX_SCALES:
        raise ValueError(what)
    out = []
    for s in seq:
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, float, np.integer, np.floating)):
            raise ValueError(what)
        v = float(s)
        if not math.isfinite(v) or v <= 0.0:
            raise ValueError(what)
        out.append(v)
    out = tuple(out)
    return None if out in ((), (1.0,)) else out


def multiscale_sizes(H, W, scales):
    """[(H_k, W_k)] of the views of an (H, W) input: every side is the multiple of 16 nearest to scale * side, at least 16 (the head concatenates the
    4x upsampled OS16 features with the OS4 features).  ValueError when two scales round to the same size.  Pure host code."""
    sizes = []
    for s in scales:
        size = tuple(16 * max(1, int(math.floor(float(s) * v / 16.0 + 0.5))) for v in (int(H), int(W)))
        if size in sizes:
            raise ValueError(f'scales = {tuple(scales)!r}: two of them give the same {size[0]} x {size[1]} view of a {H} x {W} input')
        sizes.append(size)
    return sizes


def resize_image_ac(x, size):
    """The input of a view: the align-corners bilinear resize of the images `x` (N,3,H,W) to `size` (dsrl_bilinear_ac_fwd, the convention of every
    interpolation of the model and its input pipeline); `x` itself when the size is its own."""
    _need_gpu(x)
    size = (int(size[0]), int(size[1]))
    if tuple(x.shape[2:]) == size:
        return x
    with torch.no_grad():
        return upsample_bilinear_ac(x, size)


def _resample_exact(logits, mirrored, Ho, Wo):
    """the resampling rule of dsrl_prob_merge in torch ops (class counts the kernel refuses)"""
    if mirrored:
        logits = logits.flip(3)

    def axis(S, O):
        o = torch.arange(O, device=logits.device, dtype=torch.int64)
        n = o * (S - 1)
        i0 = n // max(O - 1, 1)
        frac = (n - i0 * max(O - 1, 1)).to(torch.float32) / float(max(O - 1, 1))
        return i0, torch.clamp(i0 + 1, max=S - 1), frac

    y0, y1, fy = axis(logits.shape[2], Ho)
    x0, x1, fx = axis(logits.shape[3], Wo)
    fy, fx = fy.view(1, 1, Ho, 1), fx.view(1, 1, 1, Wo)
    r0, r1 = logits.index_select(2, y0), logits.index_select(2, y1)
    top = (1.0 - fx) * r0.index_select(3, x0) + fx * r0.index_select(3, x1)
    bot = (1.0 - fx) * r1.index_select(3, x0) + fx * r1.index_select(3, x1)
    return (1.0 - fy) * top + fy * bot


class ProbMerge:
    """The multi-scale ensemble one view at a time (include/dsrl_hip.h, "multi-scale ensemble"): `add(logits, mirrored)` for each of `views` views in
    turn; the call with the last view returns (pred, ce), every earlier one None.  All but the last view go through dsrl_prob_merge into one
    accumulator, the last through dsrl_prob_merge_finish.  A view's logits may be freed as soon as its `add` returns: the launch is enqueued on the
    current stream and nothing else refers to them.  Shapes dsrl_prob_merge_supported refuses for the whole batch are launched image by image; class
    counts it refuses are composed from torch ops under the same definition."""

    def __init__(self, views, N, C, out_size, device, target=None, ignore_index=255, counts=None, nan_flag=None, confusion=None, calibration=None,
                 confidence=False):
        """`calibration` (int64 [3*bins], needs a target) gets the reliability record of the ensemble's class map ADDED and `confidence=True` appends
        the confidence map (float32 (N,Ho,Wo): min(1, winning probability sum / views)) to what the last `add` returns (dsrl_prob_merge_finish_ex)."""
        self.V, self.N, self.C = int(views), int(N), int(C)
        self.Ho, self.Wo = int(out_size[0]), int(out_size[1])
        self.device, self.ignore_index = device, int(ignore_index)
        if self.V < 1 or self.N < 1 or self.C < 1 or self.Ho < 1 or self.Wo < 1:
            raise DsrlHipError(f'multiscale_merge: {self.V} views of {self.N} x {self.C} x {self.Ho} x {self.Wo}: every count must be at least 1')
        _need_gpu(target, counts, nan_flag, confusion)
        if target is not None:
            if tuple(target.shape) != (self.N, self.Ho, self.Wo):
                raise DsrlHipError(f'multiscale_merge: target {tuple(target.shape)} is not {(self.N, self.Ho, self.Wo)}')
            if target.dtype != torch.uint8:
                target = target.to(torch.uint8)
            target = target.contiguous()
        elif counts is not None or confusion is not None or calibration is not None:
            raise DsrlHipError('multiscale_merge: counts, confusion and calibration need a target')
        if confusion is not None:
            check_confusion(confusion, self.C, device, 'multiscale_merge')
        self.bins = 0
        if calibration is not None:
            self.bins = check_calibration(calibration, _calibration_bins_of(calibration, 'multiscale_merge'), device, 'multiscale_merge')
        self.calibration, self.confidence = calibration, bool(confidence)
        if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 3 * self.C + 2 or not counts.is_contiguous()):
            raise DsrlHipError(f'multiscale_merge: counts must be a contiguous int64 tensor of {3 * self.C + 2} elements')
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1):
            raise DsrlHipError('multiscale_merge: nan_flag must be an int32 scalar')
        self.target, self.counts, self.nan_flag, self.confusion = target, counts, nan_flag, confusion
        self.kernel = bool(cquery('dsrl_prob_merge_supported', 1, 1, 1, 1, 1, self.C))
        self.acc = None             # the kernels' accumulator (or, without the kernels, the sum of the views' probabilities)
        self.done = 0

    def _chunk(self, h, w, ld):
        """images per launch: the batch, or one where the batch's indices leave 32 bits"""
        for n in (self.N, 1):
            if cquery('dsrl_prob_merge_supported', n, h, w, self.Ho, self.Wo, self.C) and n * h * w * ld < 2 ** 31:
                return n
        raise DsrlHipError(f'multiscale_merge: a single {self.C} x {h} x {w} image on a {self.Ho} x {self.Wo} grid is beyond the 32-bit indices of '
                           'dsrl_prob_merge')

    def add(self, logits, mirrored=False):
        if self.done >= self.V:
            raise DsrlHipError(f'multiscale_merge: all {self.V} views were merged already')
        with torch.no_grad():
            logits, ld = pm(logits)
            if logits.shape[0] != self.N or logits.shape[1] != self.C or logits.device != self.device:
                raise DsrlHipError(f'multiscale_merge: view {self.done} is {tuple(logits.shape)} on {logits.device}, expected ({self.N}, {self.C}, h, w) '
                                   f'on {self.device}')
            self.done += 1
            last = self.done == self.V
            if not self.kernel:
                return self._add_torch(logits, mirrored, last)
            h, w = int(logits.shape[2]), int(logits.shape[3])
            n, st = self._chunk(h, w, ld), _stream()
            C, Ho, Wo = self.C, self.Ho, self.Wo
            if self.acc is None and not last:
                self.acc = torch.empty(self.N * (cquery('dsrl_prob_merge_acc_bytes', 1, Ho, Wo, C) // 4), device=self.device, dtype=torch.float32)
            acc_step = C * Ho * Wo * 4          # bytes per image (dsrl_prob_merge_acc_bytes is linear in N)
            if not last:
                for i in range(0, self.N, n):
                    call('dsrl_prob_merge', logits.data_ptr() + i * h * w * ld * 4, ld, n, h, w, C, int(bool(mirrored)), self.acc.data_ptr() + i * acc_step,
                         Ho, Wo, int(self.done == 1), st)
                return None
            tgt = self.target
            pred = torch.empty((self.N, Ho, Wo), device=self.device, dtype=torch.uint8)
            ce = torch.empty((self.N // n, 2), device=self.device, dtype=torch.float32) if tgt is not None else None
            ws = _ws(cquery('dsrl_prob_merge_workspace_bytes', n, Ho, Wo) if ce is not None else 0, logits)
            ex = self.calibration is not None or self.confidence
            conf = torch.empty((self.N, Ho, Wo), device=self.device, dtype=torch.float32) if self.confidence else None
            more = (conf,) if self.confidence else ()
            for k, i in enumerate(range(0, self.N, n)):
                extra = () if not ex else (None if self.calibration is None else self.calibration.data_ptr(), self.bins,
                                           None if conf is None else conf.data_ptr() + 4 * i * Ho * Wo)
                call('dsrl_prob_merge_finish_ex' if ex else 'dsrl_prob_merge_finish', logits.data_ptr() + i * h * w * ld * 4, ld, n, h, w, C, int(bool(mirrored)),
                     None if self.acc is None else self.acc.data_ptr() + i * acc_step, Ho, Wo, self.V, pred.data_ptr() + i * Ho * Wo,
                     None if tgt is None else tgt.data_ptr() + i * Ho * Wo, self.ignore_index, None if self.counts is None else self.counts.data_ptr(),
                     None if ce is None else ce.data_ptr() + 8 * k, None if self.nan_flag is None else self.nan_flag.data_ptr(), ws.data_ptr(), ws.numel(),
                     None if self.confusion is None else self.confusion.data_ptr(), *extra, st)
            self.acc = None
            if ce is None:
                return (pred, None) + more
            if ce.shape[0] == 1:
                return (pred, ce[0, 0]) + more
            mean, cnt = ce[:, 0].double(), ce[:, 1].double()            # per image: a mean over no pixel (NaN) carries no weight
            return (pred, (torch.where(cnt > 0, mean * cnt, torch.zeros_like(mean)).sum() / cnt.sum()).float()) + more

    def _add_torch(self, logits, mirrored, last):
        p = torch.softmax(_resample_exact(logits, mirrored, self.Ho, self.Wo), dim=1)
        self.acc = p if self.acc is None else self.acc.add_(p)
        if not last:
            return None
        tot, self.acc = self.acc, None
        if self.nan_flag is not None:
            nan_check_(self.nan_flag, tot)
        pred = torch.argmax(tot, dim=1).to(torch.uint8)
        tgt = self.target
        more = ()
        if self.calibration is not None or self.confidence:
            conf = _calibration_of_scores(self.calibration, tot / float(self.V), pred, tgt, self.ignore_index, self.C, self.confidence)
            more = (conf,) if self.confidence else ()
        if tgt is None:
            return (pred, None) + more
        if self.nan_flag is not None:
            _bad_label_bit(self.nan_flag, tgt, self.ignore_index, self.C)
        if self.counts is not None:
            lg, ld = pm(tot)
            call('dsrl_seg_metrics', lg.data_ptr(), ld, tgt.data_ptr(), tgt.numel(), self.C, self.ignore_index, self.counts.data_ptr(), _stream())
        if self.confusion is not None:
            confusion_matrix_(self.confusion, pred, tgt, self.C, self.ignore_index)
        counted = tgt != self.ignore_index
        picked = (tot / float(self.V)).gather(1, tgt.long().clamp(max=self.C - 1).unsqueeze(1))[:, 0]
        ce = (-torch.log(picked))[counted].mean()
        bad = (counted & (tgt >= self.C)).any()
        return (pred, torch.where(bad, torch.full_like(ce, float('nan')), ce)) + more


def multiscale_merge(views, out_size, target=None, ignore_index=255, counts=None, nan_flag=None, confusion=None, calibration=None, confidence=False):
    """The multi-scale (and flip) ensemble of given logits: `views` is a list of (logits (N,C,h,w), mirrored) - the logits of one scale each, in the
    horizontally mirrored frame where `mirrored` is true; sizes may differ from view to view.  Every view is resampled onto the `out_size` = (Ho, Wo)
    grid by align-corners bilinear interpolation of the logits (a mirrored one mirrored back first), its softmax taken and the class probabilities
    averaged (dsrl_prob_merge, and dsrl_prob_merge_finish for the last view).  -> (pred uint8 (N,Ho,Wo), ce): pred is the first maximum of the
    summed probabilities; with `target` (N,Ho,Wo) `ce` is the 0-d mean of -log P[target] over target != ignore_index, `counts` (int64
    [3*classes+2], optional) gets the dsrl_seg_metrics table of pred ADDED and `confusion` (int64 [classes^2], optional) its confusion matrix;
    `nan_flag` (int32 scalar, optional): bit 0 a NaN logit in any view, bit 1 a label outside the classes.  Beyond pred the call allocates one
    accumulator of N * classes * Ho * Wo floats (none for a single view) and the loss workspace.
    `calibration` (int64 [3*bins], optional, needs a target) gets the reliability record of pred ADDED, `confidence=True` appends the confidence map
    (float32 (N,Ho,Wo)) to the returned tuple: both by the last view's launch (dsrl_prob_merge_finish_ex)."""
    views = list(views)
    if not views:
        raise DsrlHipError('multiscale_merge: no views')
    first = views[0][0]
    _need_gpu(*(v[0] for v in views))
    if first.dim() != 4:
        raise DsrlHipError(f'4-D (N,C,H,W) tensor expected, got shape {tuple(first.shape)}')
    merge = ProbMerge(len(views), first.shape[0], first.shape[1], out_size, first.device, target, ignore_index, counts, nan_flag, confusion, calibration,
                      confidence)
    out = None
    for logits, mirrored in views:
        out = merge.add(logits, mirrored)
    return out


# ------------------------------------------------------------------------------------------------ sliding-window inference
WINDOW_MAX_POSITIONS = 32           # per axis: the positions travel in the finish launch's argument struct (csrc/window.hip)


def _window_pair(value, what):
    """an integer >= 1 or a pair of them -> (int, int); ValueError on bools, strings, tensors, non-integers and values < 1"""
    msg = f'{what} = {value!r}: expected an integer >= 1 or a pair (rows, columns) of them'
    if isinstance(value, (str, bytes, torch.Tensor, bool, np.bool_)):
        raise ValueError(msg)
    if isinstance(value, (int, np.integer)):
        value = (value, value)
    try:
        seq = tuple(value)
    except TypeError:
        raise ValueError(msg) from None
    if len(seq) != 2:
        raise ValueError(msg)
    for v in seq:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError(msg)
    return int(seq[0]), int(seq[1])


def window_value(window, stride=None):
    """The window of sliding-window inference as ((h, w), (sy, sx)) in input pixels, or None for "off" (window None).  `window` and `stride`: an
    integer or a pair (rows, columns) of integers >= 1; a missing stride is ceil(2 side / 3) per axis (mmseg's stride of 2/3 of the crop).
    ValueError on bools, strings, tensors, non-integers, values < 1 and a stride without a window.  Touches no device."""
    if window is None:
        if stride is not None:
            raise ValueError(f'stride = {stride!r} without a window: expected window = an integer >= 1 or a pair of them')
        return None
    size = _window_pair(window, 'window')
    step = tuple(-(-2 * v // 3) for v in size) if stride is None else _window_pair(stride, 'stride')
    return size, step


def window_positions(S, w, s):
    """The window positions along an axis of S pixels, window side w, stride s (mmseg's slide rule): n = max(S - w + s - 1, 0) // s + 1 of them,
    a_i = max(min(i s + w, S) - w, 0) - the last window is pulled back to end at S.  Strictly increasing for 1 <= s and w <= S.  Pure host code."""
    S, w, s = int(S), int(w), int(s)
    n = max(S - w + s - 1, 0) // s + 1
    return tuple(max(min(i * s + w, S) - w, 0) for i in range(n))


def window_plan(H, W, window, stride=None):
    """(ys, xs): the window positions of an (H, W) input in input pixels, their product visited row-major; None when the window is "off" (None, or
    the whole image).  `window` / `stride` as window_value takes them.  ValueError on a window larger than the image, a stride larger
    than the window (it would leave pixels uncovered), an image or window side that is not a multiple of 16 (the head concatenates the 4x upsampled
    OS16 features with the OS4 features) and more than 32 positions on an axis.  Pure host code."""
    value = window_value(window, stride)
    if value is None:
        return None
    (h, w), (sy, sx) = value
    H, W = int(H), int(W)
    what = f'window = {h} x {w}, stride = {sy} x {sx} on a {H} x {W} input'
    if h > H or w > W:
        raise ValueError(f'{what}: the window is larger than the image')
    if sy > h or sx > w:
        raise ValueError(f'{what}: a stride larger than the window leaves pixels uncovered')
    if H % 16 or W % 16 or h % 16 or w % 16:
        raise ValueError(f'{what}: every side of the image and of the window must be a multiple of 16')
    if (h, w) == (H, W):
        return None
    ys, xs = window_positions(H, h, sy), window_positions(W, w, sx)
    if len(ys) > WINDOW_MAX_POSITIONS or len(xs) > WINDOW_MAX_POSITIONS:
        raise ValueError(f'{what}: {len(ys)} x {len(xs)} positions, at most {WINDOW_MAX_POSITIONS} per axis are possible')
    return ys, xs


def window_fresh(positions, side, i):
    """fresh_y (or fresh_x) of the first view of position i along an axis (include/dsrl_hip.h, dsrl_window_merge): the window's rows from this one on
    were not covered by position i - 1"""
    return 0 if i == 0 else positions[i - 1] + side - positions[i]


def _window_axis(positions, side, size, what):
    """positions along one axis of the output grid as a tuple of ints: 1 to 32, from 0, strictly increasing, no gap, the last one ending at `size`"""
    msg = f'{what} = {positions!r}: expected 1 to {WINDOW_MAX_POSITIONS} integers that start at 0, increase, leave no gap between windows of side {side} and end at {size - side}'
    if isinstance(positions, (str, bytes, torch.Tensor)):
        raise ValueError(msg)
    try:
        seq = tuple(positions)
    except TypeError:
        raise ValueError(msg) from None
    if not 1 <= len(seq) <= WINDOW_MAX_POSITIONS or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in seq):
        raise ValueError(msg)
    seq = tuple(int(v) for v in seq)
    if seq[0] != 0 or seq[-1] + side != size or any(b <= a or b > a + side for a, b in zip(seq, seq[1:])):
        raise ValueError(msg)
    return seq


class WindowMerge:
    """The sliding-window ensemble one view at a time (include/dsrl_hip.h, "sliding-window ensemble"): `add(logits)` once per view in plan order -
    positions `ys` x `xs` (offsets on the OUTPUT grid) row-major, with `flip` the plain and then the mirrored-frame view of each position; the call
    with the last view returns (pred, ce[, conf]), every earlier one None.  Every view goes through dsrl_window_merge into one accumulator, which the
    launches fill without a zero fill (this class owns the order and the store-or-add offsets: callers hand it logits only), and the last call ends
    in dsrl_window_merge_finish(_ex).  A view's logits may be freed as soon as its `add` returns.  Shapes dsrl_window_merge_supported refuses for
    the whole batch are launched image by image; class counts it refuses are composed from torch ops under the same definition.  Bad positions are
    a ValueError before any device work."""

    def __init__(self, ys, xs, window_out, N, C, out_size, device, target=None, ignore_index=255, counts=None, nan_flag=None, confusion=None,
                 calibration=None, confidence=False, flip=False):
        self.N, self.C = int(N), int(C)
        self.Ho, self.Wo = int(out_size[0]), int(out_size[1])
        self.hw, self.ww = int(window_out[0]), int(window_out[1])
        self.device, self.ignore_index = device, int(ignore_index)
        if self.N < 1 or self.C < 1 or self.hw < 1 or self.ww < 1 or self.hw > self.Ho or self.ww > self.Wo:
            raise ValueError(f'window_merge: {self.N} x {self.C} x {self.hw} x {self.ww} windows on a {self.Ho} x {self.Wo} grid: every count must be at '
                             'least 1 and the window inside the grid')
        self.ys, self.xs = _window_axis(ys, self.hw, self.Ho, 'ys'), _window_axis(xs, self.ww, self.Wo, 'xs')
        self.vpp = 2 if flip else 1
        self.V = len(self.ys) * len(self.xs) * self.vpp
        _need_gpu(target, counts, nan_flag, confusion)
        if target is not None:
            if tuple(target.shape) != (self.N, self.Ho, self.Wo):
                raise DsrlHipError(f'window_merge: target {tuple(target.shape)} is not {(self.N, self.Ho, self.Wo)}')
            if target.dtype != torch.uint8:
                target = target.to(torch.uint8)
            target = target.contiguous()
        elif counts is not None or confusion is not None or calibration is not None:
            raise DsrlHipError('window_merge: counts, confusion and calibration need a target')
        if confusion is not None:
            check_confusion(confusion, self.C, device, 'window_merge')
        self.bins = 0
        if calibration is not None:
            self.bins = check_calibration(calibration, _calibration_bins_of(calibration, 'window_merge'), device, 'window_merge')
        self.calibration, self.confidence = calibration, bool(confidence)
        if counts is not None and (counts.dtype != torch.int64 or counts.numel() != 3 * self.C + 2 or not counts.is_contiguous()):
            raise DsrlHipError(f'window_merge: counts must be a contiguous int64 tensor of {3 * self.C + 2} elements')
        if nan_flag is not None and (nan_flag.dtype != torch.int32 or nan_flag.numel() != 1):
            raise DsrlHipError('window_merge: nan_flag must be an int32 scalar')
        self.target, self.counts, self.nan_flag, self.confusion = target, counts, nan_flag, confusion
        self.kernel = bool(cquery('dsrl_window_merge_supported', 1, 1, 1, 1, 1, self.C))
        self.acc = None             # the kernels' accumulator (or, without the kernels, the canvas of summed probabilities)
        self.done = 0

    def _chunk(self, ld):
        """images per launch: the batch, or one where the batch's indices leave 32 bits"""
        for n in (self.N, 1):
            if cquery('dsrl_window_merge_supported', n, self.hw, self.ww, self.Ho, self.Wo, self.C) and n * self.hw * self.ww * ld < 2 ** 31:
                return n
        raise DsrlHipError(f'window_merge: a single {self.C} x {self.hw} x {self.ww} window on a {self.Ho} x {self.Wo} grid is beyond the 32-bit '
                           'indices of dsrl_window_merge')

    def add(self, logits):
        if self.done >= self.V:
            raise DsrlHipError(f'window_merge: all {self.V} views were merged already')
        with torch.no_grad():
            logits, ld = pm(logits)
            if tuple(logits.shape) != (self.N, self.C, self.hw, self.ww) or logits.device != self.device:
                raise DsrlHipError(f'window_merge: view {self.done} is {tuple(logits.shape)} on {logits.device}, expected '
                                   f'{(self.N, self.C, self.hw, self.ww)} on {self.device}')
            position, view = divmod(self.done, self.vpp)
            i, j = divmod(position, len(self.xs))
            mirrored = view == 1
            self.done += 1
            last = self.done == self.V
            if not self.kernel:
                return self._add_torch(logits, i, j, mirrored, last)
            C, Ho, Wo, hw, ww = self.C, self.Ho, self.Wo, self.hw, self.ww
            n, st = self._chunk(ld), _stream()
            if self.acc is None:
                self.acc = torch.empty(self.N * (cquery('dsrl_prob_merge_acc_bytes', 1, Ho, Wo, C) // 4), device=self.device, dtype=torch.float32)
            acc_step = C * Ho * Wo * 4          # bytes per image (dsrl_prob_merge_acc_bytes is linear in N)
            # a mirrored view is never the first one of its pixels: nothing of it is stored
            fresh = (hw, 0) if mirrored else (window_fresh(self.ys, hw, i), window_fresh(self.xs, ww, j))
            for k in range(0, self.N, n):
                call('dsrl_window_merge', logits.data_ptr() + k * hw * ww * ld * 4, ld, n, hw, ww, C, int(mirrored), self.acc.data_ptr() + k * acc_step,
                     Ho, Wo, self.ys[i], self.xs[j], fresh[0], fresh[1], st)
            if not last:
                return None
            tgt = self.target
            pred = torch.empty((self.N, Ho, Wo), device=self.device, dtype=torch.uint8)
            ce = torch.empty((self.N // n, 2), device=self.device, dtype=torch.float32) if tgt is not None else None
            ws = _ws(cquery('dsrl_window_merge_workspace_bytes', n, Ho, Wo) if ce is not None else 0, logits)
            ex = self.calibration is not None or self.confidence
            conf = torch.empty((self.N, Ho, Wo), device=self.device, dtype=torch.float32) if self.confidence else None
            more = (conf,) if self.confidence else ()
            ys, xs = (ctypes.c_int * len(self.ys))(*self.ys), (ctypes.c_int * len(self.xs))(*self.xs)
            for q, k in enumerate(range(0, self.N, n)):
                extra = () if not ex else (None if self.calibration is None else self.calibration.data_ptr(), self.bins,
                                           None if conf is None else conf.data_ptr() + 4 * k * Ho * Wo)
                call('dsrl_window_merge_finish_ex' if ex else 'dsrl_window_merge_finish', self.acc.data_ptr() + k * acc_step, n, C, Ho, Wo, ys, len(self.ys),
                     xs, len(self.xs), hw, ww, self.vpp, pred.data_ptr() + k * Ho * Wo, None if tgt is None else tgt.data_ptr() + k * Ho * Wo,
                     self.ignore_index, None if self.counts is None else self.counts.data_ptr(), None if ce is None else ce.data_ptr() + 8 * q,
                     None if self.nan_flag is None else self.nan_flag.data_ptr(), ws.data_ptr(), ws.numel(),
                     None if self.confusion is None else self.confusion.data_ptr(), *extra, st)
            self.acc = None
            if ce is None:
                return (pred, None) + more
            if ce.shape[0] == 1:
                return (pred, ce[0, 0]) + more
            mean, cnt = ce[:, 0].double(), ce[:, 1].double()            # per image: a mean over no pixel (NaN) carries no weight
            return (pred, (torch.where(cnt > 0, mean * cnt, torch.zeros_like(mean)).sum() / cnt.sum()).float()) + more

    def _add_torch(self, logits, i, j, mirrored, last):
        if self.acc is None:
            self.acc = torch.zeros((self.N, self.C, self.Ho, self.Wo), device=self.device, dtype=torch.float32)
        p = torch.softmax(logits.flip(3) if mirrored else logits, dim=1)
        self.acc[:, :, self.ys[i]:self.ys[i] + self.hw, self.xs[j]:self.xs[j] + self.ww] += p
        if not last:
            return None
        tot, self.acc = self.acc, None
        cover = []
        for positions, side, size in ((self.ys, self.hw, self.Ho), (self.xs, self.ww, self.Wo)):
            o = torch.arange(size, device=self.device).unsqueeze(0)
            a = torch.tensor(positions, device=self.device).unsqueeze(1)
            cover.append(((o >= a) & (o < a + side)).sum(0))
        cnt = (cover[0].unsqueeze(1) * cover[1].unsqueeze(0) * self.vpp).to(torch.float32)
        if self.nan_flag is not None:
            nan_check_(self.nan_flag, tot)
        pred = torch.argmax(tot, dim=1).to(torch.uint8)
        tgt = self.target
        prob = tot / cnt
        more = ()
        if self.calibration is not None or self.confidence:
            conf = _calibration_of_scores(self.calibration, prob, pred, tgt, self.ignore_index, self.C, self.confidence)
            more = (conf,) if self.confidence else ()
        if tgt is None:
            return (pred, None) + more
        if self.nan_flag is not None:
            _bad_label_bit(self.nan_flag, tgt, self.ignore_index, self.C)
        if self.counts is not None:
            lg, ld = pm(tot)
            call('dsrl_seg_metrics', lg.data_ptr(), ld, tgt.data_ptr(), tgt.numel(), self.C, self.ignore_index, self.counts.data_ptr(), _stream())
        if self.confusion is not None:
            confusion_matrix_(self.confusion, pred, tgt, self.C, self.ignore_index)
        counted = tgt != self.ignore_index
        picked = prob.gather(1, tgt.long().clamp(max=self.C - 1).unsqueeze(1))[:, 0]
        ce = (-torch.log(picked))[counted].mean()
        bad = (counted & (tgt >= self.C)).any()
        return (pred, torch.where(bad, torch.full_like(ce, float('nan')), ce)) + more


def window_merge(views, ys, xs, out_size, target=None, ignore_index=255, counts=None, nan_flag=None, confusion=None, calibration=None, confidence=False,
                 flip=False):
    """The sliding-window (and flip) ensemble of given logits: `views` is the list of the windows' logits (N,C,hw,ww), all of one size, in plan
    order - positions `ys` x `xs` (offsets on the `out_size` = (Ho, Wo) grid: any integers that start at 0, increase, leave no gap and end at the
    grid's end) row-major, with `flip` two per position, the second in the horizontally mirrored frame.  Every view's softmax is added where the
    window lies (a mirrored one mirrored back first) and the sum divided by the number of views covering the pixel (dsrl_window_merge,
    dsrl_window_merge_finish).  -> (pred uint8 (N,Ho,Wo), ce): pred is the first maximum of the summed probabilities; with `target` (N,Ho,Wo)
    `ce` is the 0-d mean of -log P[target] over target != ignore_index, `counts` (int64 [3*classes+2], optional) gets the dsrl_seg_metrics table of
    pred ADDED and `confusion` (int64 [classes^2], optional) its confusion matrix; `nan_flag` (int32 scalar, optional): bit 0 a NaN logit in any
    view, bit 1 a label outside the classes; `calibration` (int64 [3*bins], optional, needs a target) gets the reliability record of pred ADDED,
    `confidence=True` appends the confidence map (float32 (N,Ho,Wo): min(1, winning sum / views covering the pixel)).  Beyond pred the call
    allocates one accumulator of N * classes * Ho * Wo floats, which is never filled, and the loss workspace."""
    views = list(views)
    if not views:
        raise DsrlHipError('window_merge: no views')
    first = views[0]
    _need_gpu(*views)
    if first.dim() != 4:
        raise DsrlHipError(f'4-D (N,C,H,W) tensor expected, got shape {tuple(first.shape)}')
    merge = WindowMerge(ys, xs, first.shape[2:], first.shape[0], first.shape[1], out_size, first.device, target, ignore_index, counts, nan_flag, confusion,
                        calibration, confidence, flip)
    if len(views) != merge.V:
        raise DsrlHipError(f'window_merge: {len(views)} views for {len(merge.ys)} x {len(merge.xs)} positions of {merge.vpp}: {merge.V} expected')
    out = None
    for logits in views:
        out = merge.add(logits)
    return out


_palettes = {}


def palette_tensor(class_rgb_color, device):
    """uint8 [256][3] device table label -> colour of a {label: (r, g, b)} dict, labels it does not name black (as utils.make_input_output_visualization
    builds it on the host); one per (palette, device)."""
    key = (tuple(sorted((int(k) & 0xff, tuple(int(c) for c in v)) for k, v in class_rgb_color.items())), str(device))
    tab = _palettes.get(key)
    if tab is None:
        host = torch.zeros((256, 3), dtype=torch.uint8)
        for label, rgb in class_rgb_color.items():
            host[int(label) & 0xff] = torch.tensor([int(c) for c in rgb], dtype=torch.uint8)
        tab = _palettes[key] = host.to(device)
    return tab


def class_map_visualize(rgb, classes, palette, mask=None, ignore_index=255, blend_factor=0.4, out=None):
    """The test command's panel on the device (include/dsrl_hip.h: dsrl_class_map_visualize): rgb uint8 (N,H,W,3), classes uint8 (N,H,W), palette uint8
    [256][3] (palette_tensor), mask uint8 (N,H,W) or None (where mask == ignore_index the class becomes ignore_index) -> uint8 (N,H,3W,3):
    input | class colours | overlay, byte for byte utils.make_input_output_visualization."""
    _need_gpu(rgb, classes, palette, mask)
    for t_, name in ((rgb, 'rgb'), (classes, 'classes'), (palette, 'palette'), (mask, 'mask')):
        if t_ is not None and t_.dtype != torch.uint8:
            raise DsrlHipError(f'class_map_visualize: {name} must be uint8, got {t_.dtype}')
    if rgb.dim() != 4 or rgb.shape[3] != 3 or classes.dim() != 3 or tuple(classes.shape) != tuple(rgb.shape[:3]):
        raise DsrlHipError(f'class_map_visualize: rgb {tuple(rgb.shape)} must be (N,H,W,3) and classes {tuple(classes.shape)} (N,H,W)')
    if mask is not None and tuple(mask.shape) != tuple(classes.shape):
        raise DsrlHipError(f'class_map_visualize: mask {tuple(mask.shape)} does not match classes {tuple(classes.shape)}')
    if tuple(palette.shape) != (256, 3):
        raise DsrlHipError(f'class_map_visualize: palette must be [256][3], got {tuple(palette.shape)}')
    if not 0.0 < float(blend_factor) < 1.0:
        raise DsrlHipError('class_map_visualize: 0 < blend_factor < 1')
    rgb, classes, palette = rgb.contiguous(), classes.contiguous(), palette.contiguous()
    mask = None if mask is None else mask.contiguous()
    N, H, W, _ = rgb.shape
    if out is None:
        out = torch.empty((N, H, 3 * W, 3), device=rgb.device, dtype=torch.uint8)
    elif tuple(out.shape) != (N, H, 3 * W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != rgb.device:
        raise DsrlHipError('class_map_visualize: out must be a contiguous uint8 (N,H,3W,3) tensor on the same device')
    call('dsrl_class_map_visualize', rgb.data_ptr(), classes.data_ptr(), None if mask is None else mask.data_ptr(), palette.data_ptr(), out.data_ptr(),
         N, H, W, int(ignore_index), float(blend_factor), _stream())
    return out


def conv2d_inbounds_macs(N, H, W, Cc, K, R, S, stride, pad, dil):
    return cquery('dsrl_conv2d_inbounds_macs', N, H, W, Cc, K, R, S, stride, pad, dil)

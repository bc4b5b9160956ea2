"""Compiled inference: what an eval-mode model can prepare once because its weights are frozen, and its forward pass as a replayed hipGraph.

  * FrozenOperands(model): for every conv filter the kernels take them for, the amax record, the pre-split form and the fp16 planes of the forward layout
    (a forward-only filter_operands.FilterOperands: the launches ddp.FlatParams runs once per training step, here once per model), and
    1 / sqrt(var + eps) of every eval BatchNorm.  functional.py finds them through the hooks it already reads (`w._dsrl_operands`;
    `running_var._dsrl_invstd`), so `model.predict` and `model.forward` launch the same conv kernels on the same values, without the per-call filter
    measurement, the in-kernel filter split and the ~105 one-block invstd launches.
  * CompiledPredictor (DSRL.compile_predict): `DSRL.predict` captured per (N, H, W, with target, conv arithmetic, flip) into a hipGraph and replayed - about a
    thousand eager launches become one hipGraphLaunch.  The contract is bit identity with eager `predict`.
  * load_compiled_model: the file the compile_model command writes (data only) -> (model, CompiledPredictor).
"""
import torch

from . import functional as HF
from ._lib import DsrlHipError, call, load as _load_lib, query
from .filter_operands import FilterOperands, align as _align, conv_filters

FORMAT, FORMAT_VERSION = 'dsrl-hip-compiled', 1
STALE_BIT = 4           # bit of the NaN flag word the device-side fingerprint check raises (bit 0: NaN, bit 1: label outside the classes)
# graph replay of DSRL.predict(scales=...) is not built: a compiled predictor, and the commands asked for one, refuse the combination
MULTISCALE_NOT_COMPILED = ('multi-scale inference (scales=...) runs through the eager DSRL.predict: a compiled predictor replays the single-scale '
                           'and flip paths only')
_private_gen = [1 << 40]


class FrozenOperands:
    """Prepared operands of an eval-mode model on the GPU; see the module docstring.  Inference only: it is the gradient sink (`_dsrl_arena`) of the
    filters it froze, and a backward pass that asks it for a slot raises."""

    def __init__(self, model):
        params = list(model.parameters())
        if not params or not params[0].is_cuda:
            raise DsrlHipError('FrozenOperands: the model must be on the HIP device')
        if model.training or any(m.training for m in model.modules()):
            raise DsrlHipError('FrozenOperands: inference only - call model.eval() first')
        for p in params:
            if getattr(p, '_dsrl_arena', None) is not None:
                raise DsrlHipError('FrozenOperands: a parameter of this model is bound to a ddp.FlatParams arena or to another FrozenOperands (release() that one first)')
        self.model, self.device = model, params[0].device
        self.released = False
        self.precision = None
        self._sets = {}             # conv arithmetic -> its FilterOperands (a captured graph keeps reading the set it was captured with)
        self._filters = conv_filters(model)          # the RGB stem and the C -> 1 transformers have no such operands
        self._bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.running_var is not None]
        # what every call compares: (dict that holds the tensor, its name, address, version counter) of every parameter and buffer
        self._watch = []
        for mod in model.modules():
            for held in (mod._parameters, mod._buffers):
                for name, t in held.items():
                    if t is not None:
                        self._watch.append((held, name, t.data_ptr(), t._version))
        self._modules = list(model.modules())
        with torch.no_grad(), torch.cuda.device(self.device):
            self._freeze_invstd()
            self._fingerprint()
            self.attach()

    # ------------------------------------------------------------------ what backward asks of a gradient sink first
    def claim(self, _p):
        raise DsrlHipError('FrozenOperands is inference-only: a backward pass reached a filter whose operands are frozen - call release() '
                           '(CompiledPredictor.release()) before training this model')

    # ------------------------------------------------------------------ BatchNorm constants
    def _freeze_invstd(self):
        total = sum(_align(m.num_features) for m in self._bns)
        self._invstd = torch.empty(max(total, 4), device=self.device, dtype=torch.float32)
        off, st = 0, HF._stream()
        self._invstd_held = []
        for m in self._bns:
            rv, C = m.running_var, m.num_features
            view = self._invstd[off:off + C]
            off += _align(C)
            call('dsrl_bn_invstd_from_var', rv.data_ptr(), C, float(m.eps), view.data_ptr(), st)      # the kernel every eval forward runs: the same bits
            held = (view, float(m.eps), rv._version)
            rv._dsrl_invstd = held
            self._invstd_held.append((m, held))

    # ------------------------------------------------------------------ device-side fingerprint of every float parameter and buffer
    def _fingerprint(self):
        seg = int(query('dsrl_fingerprint_segment_words'))
        rows = []
        for held, name, ptr, _ in self._watch:
            t = held[name]
            if t.dtype != torch.float32 or not t.is_cuda or t.numel() == 0:
                continue
            if not (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
                continue                    # dense tensors only (contiguous or channels_last): numel() words from data_ptr()
            n = t.numel()
            for a in range(0, n, seg):
                rows.append([ptr + 4 * a, min(seg, n - a)])
        self._fp_table = torch.tensor(rows, dtype=torch.int64, device=self.device)
        self._fp_rows = len(rows)
        self._fp = torch.empty(len(rows), dtype=torch.int64, device=self.device)
        call('dsrl_fingerprint_segments', self._fp_table.data_ptr(), self._fp_rows, self._fp.data_ptr(), None, None, 0, HF._stream())

    def check_values(self, flag):
        """Enqueues the comparison of every float parameter and buffer with its fingerprint at freeze time: bit 2 (value 4) of the int32 device scalar
        `flag` is raised on a difference.  A write through `.data` or a raw pointer moves neither address nor version counter; this finds it.  One
        launch that reads the whole model once, so CompiledPredictor runs it only in the form of the call that reads its flag back anyway."""
        call('dsrl_fingerprint_segments', self._fp_table.data_ptr(), self._fp_rows, None, self._fp.data_ptr(), flag.data_ptr(), STALE_BIT, HF._stream())

    # ------------------------------------------------------------------ filter operands
    def _prepare(self):
        """amax records, w_split and w_planes of every filter under the CURRENT conv arithmetic, one launch of each batched kernel."""
        ops = FilterOperands(self._filters, self.device, transposed=False)          # no transposed forms: inference has no data gradients
        if ops.rows:
            ops.measure(streaming=False)
            ops.write_split()
            # fp16 planes [K][R][S][C] (two for 'f16x3'; 'f16x1' reads the first) of every eligible filter
            if HF.planes_mode != 'off':
                ops.add_plane_set()
                ops.write_planes()
        return ops

    def attach(self, precision=None):
        """Presents the operands of conv arithmetic `precision` (default: the current one) through the hooks of functional.py, preparing them on
        first use.  Only the arithmetics that scale their operands ('f16x3', 'f16x1') have filter operands; under the others the filters stay as they
        are and only the BatchNorm constants are shared."""
        precision = HF.get_conv_precision() if precision is None else precision
        if precision != HF.get_conv_precision():
            raise DsrlHipError(f'FrozenOperands.attach({precision!r}) while the conv arithmetic is {HF.get_conv_precision()!r}')
        for ops in self._sets.values():
            ops.detach()
        for w in self._filters:
            w._dsrl_arena = self
        if precision in ('f16x3', 'f16x1'):
            if precision not in self._sets:
                with torch.no_grad(), torch.cuda.device(self.device):
                    self._sets[precision] = self._prepare()
            self._sets[precision].attach()
        self.precision = precision

    def nbytes(self):
        """Bytes of device memory the prepared operands hold (all arithmetics prepared so far, the BatchNorm constants and the fingerprints)."""
        n = self._invstd.numel() * 4 + self._fp.numel() * 8 + self._fp_table.numel() * 8
        return n + sum(ops.nbytes() for ops in self._sets.values())

    # ------------------------------------------------------------------ staleness
    def stale_reason(self):
        if self.released:
            return 'the operands were released'
        for m in self._modules:
            if m.training:
                return f'a {type(m).__name__} of the model is in train mode'
        for held, name, ptr, ver in self._watch:
            t = held.get(name)
            if t is None or t.data_ptr() != ptr:
                return f"the tensor '{name}' of a module moved (.to(), a ddp.FlatParams arena, a replaced parameter)"
            if t._version != ver:
                return f"'{name}' was written in place (an optimiser step, load_state_dict, copy_)"
        for m, held in self._invstd_held:
            if getattr(m.running_var, '_dsrl_invstd', None) is not held:
                return 'a BatchNorm ran in train mode and rewrote its running statistics'
        for w in self._filters:
            if getattr(w, '_dsrl_arena', None) is not self:
                return 'a filter was bound to another arena (ddp.FlatParams)'
        return None

    def check(self):
        """Every call: one Python loop, no device work.  Raises when anything the operands were derived from changed; re-attaches (preparing another
        set if need be) when the conv arithmetic is not the one the attached operands were prepared for."""
        why = self.stale_reason()
        if why is not None:
            raise DsrlHipError(f'the frozen operands of this model are stale: {why} - call release() and compile_predict() again')
        if HF.get_conv_precision() != self.precision:
            self.attach()

    def release(self):
        """Detaches everything: model.predict and model.forward run as they did before the model was frozen."""
        if self.released:
            return
        for ops in self._sets.values():
            ops.detach()
        for w in self._filters:
            if getattr(w, '_dsrl_arena', None) is self:
                del w._dsrl_arena
        for m, held in self._invstd_held:
            rv = m.running_var
            if rv is not None and getattr(rv, '_dsrl_invstd', None) is held:
                del rv._dsrl_invstd
        self._sets, self._invstd_held, self._invstd = {}, [], None
        self.released = True


class _CapturedPredict:
    __slots__ = ('graph', 'img', 'tgt', 'flag', 'pred', 'counts', 'ce', 'cm', 'arena', 'keep', 'ignore_index')


_FLAG_MESSAGES = ((1, 'NaN in the input or the logits'), (2, 'labels outside the classes'),
                  (STALE_BIT, 'a parameter or buffer changed since compile_predict() (written through .data or a raw pointer): call release() and compile_predict() again'))


class CompiledPredictor:
    """`pred, counts, ce = compiled(images, target=None, ignore_index=255, nan_flag=None, flip=False, confusion=None)`: DSRL.predict on frozen operands,
    replayed from a hipGraph.  `flip` is a call-time option (DSRL.predict(flip=True): the horizontal-flip ensemble), not a property of a compiled model file.
    `confusion` (DSRL.predict_head): the caller's matrix gets exactly this batch's counts added, replayed or eager.  A graph never holds the caller's
    pointer: it fills a static matrix of its own, zeroed by a node of the graph, which the call then adds to the tensor it was given - successive
    calls may pass different tensors.  `scales` (DSRL.predict: the multi-scale ensemble) other than "off" raises DsrlHipError before anything else is
    looked at - its graph replay is not built - and leaves the predictor as it was; so does `window` (DSRL.predict: sliding-window inference), with a
    ValueError.

    One graph per key (N, H, W, with target, conv arithmetic, flip, with confusion), captured at the key's first use after GRAPH_WARMUP eager calls (the frozen eager path:
    the same kernels), at most MAX_GRAPHS keys; further shapes, and every shape when `graph` is False or a capture failed, run the frozen eager path.
    The graph reads static input buffers (the call copies the batch in) and writes static outputs; the call returns copies of them (the class map is
    N*H*W bytes), or with copy=False the static tensors themselves, which the next call with the same key overwrites.
    Without a `nan_flag` the call reads its own flag back once and raises, as DSRL.predict does; that form also compares every parameter and buffer with
    its fingerprint at compile time on the device (FrozenOperands.check_values).  With a caller's flag nothing synchronises with the host.
    Activation amax records are the graph's own: a private arena whose zero fill is the graph's first node, so neither an eager predict nor a training
    step between two replays sees or disturbs them."""

    MAX_GRAPHS = 4
    GRAPH_WARMUP = HF.GRAPH_WARMUP

    def __init__(self, model, batch_size=None, input_size=None, graph=True):
        import time
        t0 = time.perf_counter()
        self.model = model
        self.frozen = FrozenOperands(model)
        self.device = self.frozen.device
        self.use_graph = bool(graph)
        self._graphs, self._warm = {}, {}
        self._restore_precision = None
        self.replays = 0
        if batch_size is not None and input_size is not None:
            x = torch.zeros((int(batch_size), 3, int(input_size[0]), int(input_size[1])), device=self.device).contiguous(memory_format=HF.CL)
            flag = torch.zeros((), dtype=torch.int32, device=self.device)
            for _ in range(self.GRAPH_WARMUP + 1):          # the warm-up calls, then the one that captures and replays
                self(x, nan_flag=flag)
        torch.cuda.synchronize(self.device)
        self.compile_seconds = time.perf_counter() - t0

    @property
    def num_graphs(self):
        return len(self._graphs)

    def _key(self, images, target, flip=False, confusion=None):
        N, _, H, W = images.shape
        return (int(N), int(H), int(W), target is not None, HF.get_conv_precision(), bool(flip), confusion is not None)

    # ------------------------------------------------------------------ capture
    def _capture(self, key, images, target, ignore_index, flip=False, confusion=None):
        """-> the captured call; after a capture that failed None, and this predictor stays on the frozen eager path."""
        c = _CapturedPredict()
        try:
            c.img = images.clone()
            c.tgt = None if target is None else target.clone()
            c.ignore_index = int(ignore_index)
            c.flag = torch.zeros((), dtype=torch.int32, device=self.device)
            c.cm = None if confusion is None else torch.zeros_like(confusion)
            c.graph = torch.cuda.CUDAGraph()
            _private_gen[0] += 1
            c.arena = [HF._new_arena(self.device), 0, _private_gen[0], True]      # pinned: it can never be replaced while the graph lives
            with HF.capture_scope(1 << 16) as c.keep, HF.amax_private(c.arena):
                with torch.cuda.graph(c.graph, capture_error_mode='thread_local'):          # linear: one stream, no side streams in an eval forward
                    c.arena[0].zero_()              # first node: every record a replay maxes into starts at zero
                    c.flag.zero_()
                    if c.cm is not None:
                        c.cm.zero_()                # a replay leaves exactly its batch's matrix
                    c.pred, c.counts, c.ce = self.model.predict(c.img, c.tgt, c.ignore_index, c.flag, flip, c.cm)
        except Exception as e:          # noqa: BLE001
            self.use_graph = False
            HF.abandon_capture(self.device, e, ' of predict', 'this CompiledPredictor continues on the frozen eager path')
            return None
        finally:
            HF.drop_planes()
        self._graphs[key] = c
        return c

    # ------------------------------------------------------------------ the call
    def __call__(self, images, target=None, ignore_index=255, nan_flag=None, copy=True, flip=False, confusion=None, scales=None, calibration=None,
                 confidence=False, temperature=None, window=None, stride=None):
        if calibration is not None or confidence:
            # graphs are keyed on their outputs: the calibration record and the confidence map are not among the keys
            raise ValueError('CompiledPredictor: calibration and confidence are outputs of DSRL.predict only, not of a compiled predictor')
        if HF.temperature_value(temperature, 'CompiledPredictor') is not None:
            # a graph bakes its kernel arguments in: a temperature would have to be one more key
            raise ValueError('CompiledPredictor: temperature is an option of DSRL.predict only, not of a compiled predictor')
        if HF.multiscale_scales_value(scales) is not None:
            raise DsrlHipError(MULTISCALE_NOT_COMPILED)
        if HF.window_value(window, stride) is not None:
            # a graph is keyed on the batch's shape: the windows of an image would be a loop of replays with a merge between them, which is not built
            raise ValueError('CompiledPredictor: window is an option of DSRL.predict only, not of a compiled predictor')
        if self.frozen.released:
            raise DsrlHipError('this CompiledPredictor was released: call compile_predict() again')
        self.frozen.check()
        HF._need_gpu(images, target, nan_flag)
        if images.dim() != 4:
            raise DsrlHipError(f'4-D (N,3,H,W) images expected, got shape {tuple(images.shape)}')
        if confusion is not None:
            if target is None:
                raise DsrlHipError('CompiledPredictor: confusion needs a target')
            HF.check_confusion(confusion, self.model.SSSR_decoder['upsample16_pred'][6].out_channels, images.device, 'CompiledPredictor')
        own = nan_flag is None
        key = self._key(images, target, flip, confusion)
        c = self._graphs.get(key)
        if c is not None and target is not None and c.ignore_index != int(ignore_index):
            c = None                                # the label to ignore is a launch argument of the captured kernels: this call runs eagerly
        elif (c is None and self.use_graph and len(self._graphs) < self.MAX_GRAPHS and self._warm.get(key, 0) >= self.GRAPH_WARMUP
              and (target is None or (target.dtype == torch.uint8 and tuple(target.shape) == (images.shape[0], 2 * images.shape[2], 2 * images.shape[3])))):
            c = self._capture(key, images, target, ignore_index, flip, confusion)
        with torch.no_grad():
            if c is None:
                self._warm[key] = self._warm.get(key, 0) + 1
                flag = torch.zeros((), dtype=torch.int32, device=images.device) if own else nan_flag
                out = self.model.predict(images, target, ignore_index, flag, flip, confusion)
                HF.drop_planes()
            else:
                if c.img.data_ptr() != images.data_ptr():
                    c.img.copy_(images, non_blocking=True)
                if c.tgt is not None and c.tgt.data_ptr() != target.data_ptr():
                    c.tgt.copy_(target, non_blocking=True)
                c.graph.replay()
                self.replays += 1
                flag = c.flag
                if not own:
                    nan_flag.bitwise_or_(flag.reshape(nan_flag.shape))
                if c.cm is not None:
                    confusion.add_(c.cm.view_as(confusion))
                out = (c.pred, c.counts, c.ce)
                if copy:
                    out = tuple(None if o is None else o.clone() for o in out)
            if own:
                self.frozen.check_values(flag)
                bits = int(flag.item())             # the one readback of this form of the call
                if bits:
                    raise DsrlHipError('CompiledPredictor: ' + ' and '.join(m for b, m in _FLAG_MESSAGES if bits & b))
        return out

    def release(self):
        """Drops the graphs and the frozen operands; the model is what it was before compile_predict()."""
        self._graphs.clear()
        self.frozen.release()
        if self._restore_precision is not None:
            HF.set_conv_precision(self._restore_precision[0])
            self._restore_precision = None


# ------------------------------------------------------------------------------------------------ compiled model files
class _Settings:
    """The dataset constants a compiled model file records, with the attribute names of datasets.*.settings."""

    def __init__(self, d):
        self.NUM_CLASSES, self.IGNORE_CLASS_LABEL = int(d['NUM_CLASSES']), int(d['IGNORE_CLASS_LABEL'])
        self.MEAN, self.STD = [float(v) for v in d['MEAN']], [float(v) for v in d['STD']]
        self.CLASS_RGB_COLOR = {int(k): tuple(int(c) for c in v) for k, v in d['CLASS_RGB_COLOR'].items()}


def read_compiled_file(filename):
    """Host-side half of load_compiled_model: reads the file (data only: torch.load(weights_only=True)) and checks format, version and ABI before any
    device work.  Raises RuntimeError naming the command that writes such files."""
    import os
    if not os.path.isfile(filename):
        raise RuntimeError(f"compiled_model: '{filename}' does not exist (the compile_model command writes compiled model files)")
    try:
        d = torch.load(filename, map_location='cpu', weights_only=True)
    except Exception as e:          # noqa: BLE001
        raise RuntimeError(f"compiled_model: '{filename}' is not a compiled model file of this project ({type(e).__name__}); write one with the compile_model command") from e
    if not isinstance(d, dict) or d.get('format') != FORMAT:
        plain = isinstance(d, dict) and 'model_state_dict' in d
        raise RuntimeError(f"compiled_model: '{filename}' is {'a plain weights / checkpoint file' if plain else 'not a compiled model file'}: run the compile_model "
                           'command on the weights first, or call the command without compiled_model')
    if d.get('format_version') != FORMAT_VERSION:
        raise RuntimeError(f"compiled_model: '{filename}' has format_version {d.get('format_version')!r}, this build reads {FORMAT_VERSION}: run compile_model again")
    abi = int(_load_lib().dsrl_version())
    if d.get('abi_version') != abi:
        raise RuntimeError(f"compiled_model: '{filename}' was written for library ABI {d.get('abi_version')!r}, libdsrl_hip.so has {abi}: run compile_model again")
    missing = [k for k in ('model_state_dict', 'model_input_size', 'batch_size', 'conv_precision', 'NUM_CLASSES', 'MEAN', 'STD', 'IGNORE_CLASS_LABEL',
                           'CLASS_RGB_COLOR') if k not in d]
    if missing:
        raise RuntimeError(f"compiled_model: '{filename}' lacks {missing}: run compile_model again")
    if d['conv_precision'] not in HF.CONV_PRECISION_MODES:
        raise RuntimeError(f"compiled_model: '{filename}' names the unknown conv arithmetic {d['conv_precision']!r}")
    return d


def load_compiled_model(filename, device_obj, data=None):
    """-> (model, CompiledPredictor) of a compiled model file: builds the stage-1 model, selects the recorded conv arithmetic for the predictor's
    lifetime (release() restores the previous one), freezes the operands and captures the recorded (batch size, input size) key."""
    from .models import DSRL
    d = read_compiled_file(filename) if data is None else data          # `data`: what read_compiled_file(filename) returned to a caller that checked first
    info = {k: v for k, v in d.items() if k != 'model_state_dict'}
    model = DSRL(stage=1, dataset_settings=_Settings(d)).eval()
    model.load_state_dict(d['model_state_dict'], strict=True)
    model = model.to(device_obj).to(memory_format=torch.channels_last)
    prev = HF.set_conv_precision(d['conv_precision'])
    try:
        with torch.cuda.device(device_obj):
            predictor = CompiledPredictor(model, batch_size=int(d['batch_size']), input_size=tuple(int(v) for v in d['model_input_size']))
    except BaseException:
        HF.set_conv_precision(None if prev < 0 else prev)
        raise
    predictor._restore_precision = (None if prev < 0 else prev,)
    predictor.info = info
    predictor.settings = _Settings(d)
    return model, predictor

"""Stage-1/2/3 training driver on the MI355X kernels - counterpart of the reference's
command_handlers/train_or_resume.py (same `train_or_resume(...)` signature, same seeding, SGD hyper-parameters, loss mix,
per-epoch polynomial LR, per-rank batch size, mean-reduced gradients and `final.weights` / `.checkpoint` dict formats).

What differs by design:
  * gradients are reduced and the SGD update applied on flat arenas (ddp.FlatParams) over RCCL instead of torch DDP buckets;
  * the reference's 8 blocking device->host reads and 3 host-side NaN scans per iteration (train_or_resume.py:406-451) are
    folded into ONE readback of [CE, MSE, FA, Total, nan_flag] per iteration with the same abort-on-NaN behaviour;
  * apex is not used. `mixed_precision` (apex opt levels 'O0'..'O3' in the reference, train_or_resume.py:68-72, 441-444) selects the
    arithmetic of the MFMA conv kernels instead: 'O0' = fp32-equivalent f16x3 (the default), 'O1' = bf16x6 forward / bf16x3 gradients, 'O2'/'O3' =
    bf16x3 everywhere (BASELINE config 5's reduced-precision MFMA path).  Storage and accumulation stay fp32 in every mode, so there
    is no loss scaling (nothing can underflow that fp32 training would keep) and `amp_state_dict` is None;
  * the input pipeline (torchvision Cityscapes + PIL transforms) reads a pre-decoded uint8 cache of the Cityscapes tree and runs the random
    augmentations as HIP kernels (datasets/Cityscapes/loader.py, models/transforms/augment.py).  `dataset` may instead carry a 'loader_factory'
    (callable(split, batch_size, device, rank, world) -> iterable of ((input_image, input_org), (target, _))), which is used as given;
    `SyntheticCityscapes` below provides device-resident batches of the Cityscapes shapes;
  * `dataset['optimizer'] = 'adamw'` (or {'name': 'adamw', 'betas': (b1, b2), 'eps': e}) replaces SGD by torch.optim.AdamW(lr, betas, eps,
    weight_decay) semantics inside the same optimiser pass (ddp.FlatParams.enable_adamw): `learning_rate`, `end_learning_rate`,
    `poly_power` and `weights_decay` keep their meaning, `momentum` is unused (stored in checkpoints as given; one warning), the checkpoint's
    `optimizer_state_dict` has torch.optim.AdamW's layout and every epoch record carries 'optimizer': 'adamw'.  Absent, None or 'sgd': SGD, as ever.
"""
import contextlib
import glob
import os
import warnings
from datetime import datetime

import torch as t
import torch.distributed as dist

from .. import functional as HF
from .. import settings
from ..ddp import FlatParams
from ..models import DSRL
from ..models.losses import FALoss


def isCUDAdevice(device):
    return device.casefold() == 'gpu'


def polynomial_lr(base_lr, end_lr, epoch, max_decay_steps, power):
    """models/schedulers/PolynomialLR.py:22-34: lr used during `epoch` (0-based); epoch 0 keeps the base lr."""
    if epoch <= 0:
        return base_lr
    return (base_lr - end_lr) * ((1. - epoch / max_decay_steps) ** power) + end_lr


class SyntheticCityscapes:
    """Device-resident synthetic batches of the shapes JointScaledImage produces (models/transforms/JointScaledImage.py:27-32):
    input_org ~ N(0,1) at the output size, input_image = align-corners bilinear resize of it to the input size,
    target uint8 in [0,19) with ~10 % of the pixels set to the ignore label."""

    def __init__(self, batch_size, input_size, device, rank=0, length=8, num_classes=19, ignore=255, distinct=1):
        g = t.Generator(device='cpu').manual_seed(1234 + rank)
        H, W = input_size
        self.batches = []
        for _ in range(distinct):
            org = t.randn((batch_size, 3, 2 * H, 2 * W), generator=g).to(device).contiguous(memory_format=t.channels_last)
            tgt = t.randint(0, num_classes, (batch_size, 2 * H, 2 * W), generator=g, dtype=t.uint8)
            tgt[t.rand(tgt.shape, generator=g) < 0.1] = ignore
            img = HF.upsample_bilinear_ac(org, (H, W))
            self.batches.append(((img, org), (tgt.to(device), None)))
        self.length = length

    def __len__(self):
        return self.length

    def __iter__(self):
        for i in range(self.length):
            yield self.batches[i % len(self.batches)]


class _CapturedStep:
    __slots__ = ('graph', 'graph_b', 'ready', 'img', 'org', 'tgt', 'outs', 'vals', 'bns', 'keep')


class TrainStep:
    """One iteration of train_or_resume.py:404-460 for a fixed model/arena.

    With `graph` (default: on, DSRL_GRAPH=0 turns it off) a training iteration is captured once per batch shape into a hipGraph -
    key advance, gradient zeroing, filter transposes, forward, losses, backward, SGD update - and replayed: ~1000 kernel launches
    become one hipGraphLaunch, so the host no longer paces the device.  What makes the capture replayable: the dropout key and the
    optimiser hyper-parameters are read from device memory (functional.DeviceRng, dsrl_sgd_step_dev), the fused BatchNorm barrier
    is self-resetting, and the batch is copied into static input buffers.  With more than one rank the collectives stay outside the
    graph: BN-buffer broadcast before the replay, chunked gradient all-reduce and the SGD kernel after it.

    `class_weights` (None, or one number per class): nn.CrossEntropyLoss(weight=) for the CE term of every path of the step - fused and unfused
    losses, eager and captured, training and `do_train=False` (the reference shares one `loss_funcs` between training and validation).  With more
    than one rank each rank normalises by the weight sum of its own batch and the gradients are averaged, as DDP with a weighted loss does.

    `focal_gamma` (a finite number >= 0; 0: off): the CE term becomes the focal loss sum w[t] (1 - p_t)^gamma (-log p_t) / sum w[t] on the same paths,
    `do_train=False` included (early stopping compares the two).  It runs on the weighted kernels: without `class_weights` the weights are all ones.

    `label_smoothing` (a number in [0, 1]; 0: off): nn.CrossEntropyLoss(label_smoothing=) for the CE term on the same paths, training and
    `do_train=False` alike, also on the weighted kernels.  Together with `focal_gamma` > 0: ValueError.  The value is fixed for the life of the
    step, as `focal_gamma` is, so every graph this step captures was captured with it.

    `ohem` (HF.ohem_value: None / False off, True = (0.7, 100000), (thresh, min_kept) or a mapping): online hard example mining for the CE term of
    the TRAINING iterations - the hard pixels of the batch are selected on the device and every other label becomes `ignore_index` before the CE paths
    run (HF.ohem_target), fused and unfused losses, eager and captured.  `do_train=False` keeps the configured CE without mining, so
    validation losses stay comparable between runs with and without it.  It goes with `class_weights` (the selection is on the unweighted
    probability) and not with `focal_gamma` > 0 or `label_smoothing` > 0 (ValueError); `ignore_index` must then be a byte value.  With more than one
    rank each rank mines its own batch.  Fixed for the life of the step, like the other two.

    `dice` (HF.dice_value: None / False / 0 off, True = (1.0, 1.0), a weight, (weight, smooth) or a mapping): the soft Dice term weight * L_dice is
    added to the CE term of the TRAINING iterations (HF.dice_loss) - the class sums are formed on the device from the batch of the
    iteration, the term's gradient joins d(CE)/d(logits) inside the ConvTranspose backward, fused and unfused losses, eager and captured.  The CE
    figure a training iteration reports is then CE + weight * L_dice.  `do_train=False` keeps the configured CE, so validation losses and checkpoint
    selection stay comparable between runs with and without it.  It goes with `class_weights` and not with `focal_gamma` > 0, `label_smoothing` > 0
    or `ohem` (ValueError).  With more than one rank each rank uses the sums of its own batch.  Fixed for the life of the step, like the others.

    `lovasz` (HF.lovasz_value: None / False / 0 off, True = (1.0, 1024), a weight, (weight, bins) or a mapping): the quantised Lovasz-Softmax term
    weight * L_lovasz is added to the CE term of the TRAINING iterations (HF.lovasz_softmax_loss) - the error histograms are
    formed on the device from the batch of the iteration (classes = 'present' over the batch), the term's gradient joins d(CE)/d(logits) inside the
    ConvTranspose backward, fused and unfused losses, eager and captured.  The CE figure a training iteration reports is then CE + weight * L_lovasz.
    `do_train=False` keeps the configured CE, so validation losses and checkpoint selection are unchanged.  It goes with `class_weights` and not
    with `focal_gamma` > 0, `label_smoothing` > 0, `ohem` or `dice` (ValueError).  With more than one rank each rank uses the histograms of its own
    batch.  Fixed for the life of the step, like the others.

    `label_relax` (HF.label_relax_value: None / False / 0 off, True = radius 1, a radius in [1, 4] or {'radius': r}): boundary label relaxation
     in the TRAINING iterations - the class-set mask of the batch's labels is formed on the device in front of the model's forward
    (HF.relax_mask, one launch, captured with the step), the logits layer evaluates the relaxed CE in its forward kernel and forms its gradient in
    its backward, fused and unfused losses, eager and captured.  `do_train=False` keeps the configured CE, so validation losses and checkpoint
    selection are unchanged.  It goes with `class_weights` and with none of the other loss options (ValueError).  With more than one rank each rank
    uses the masks of its own batch.  `relax_stats` (int64 {live pixels, pixels with more than one class in their set}) accumulates on the device;
    `relax_fraction(reset=True)` reads it - one device read.  Fixed for the life of the step, like the others.

    The weight average (`flat.enable_ema`) needs nothing here: the optimiser pass of the step updates it, eagerly and in the captured
    graph alike, and whether it is enabled is part of the graph key.  A training iteration inside `flat.ema_weights()` raises DsrlHipError.

    Gradient-norm clipping (`flat.enable_grad_clip`) needs nothing here either: the optimiser pass forms the norm and folds the
    coefficient into the device hyper-parameters, eagerly and in the captured graph alike; whether it is enabled is part of the graph key.  It does
    not go with the two-graph schedule (DSRL_GRAPH_SPLIT): a training iteration then raises DsrlHipError.

    AdamW (`flat.enable_adamw`) is the optimiser pass's business as well: the same launches in their AdamW forms, the step counter
    advanced on the device, eagerly and in the captured graph alike; whether it is enabled is part of the graph key.  The momentum a step is called
    with is then not read.  Like clipping it does not go with the two-graph schedule: a training iteration then raises DsrlHipError."""

    GRAPH_WARMUP = HF.GRAPH_WARMUP          # eager iterations per batch shape before the capture

    def __init__(self, model, flat, stage, w1, w2, ignore_index, graph=None, class_weights=None, focal_gamma=0.0, label_smoothing=0.0, ohem=None,
                 dice=None, lovasz=None, label_relax=None):
        self.model, self.flat, self.stage, self.w1, self.w2, self.ignore = model, flat, stage, w1, w2, ignore_index
        self.focal_gamma = HF.focal_gamma_value(focal_gamma)                                                          # ValueError on a bad gamma
        self.label_smoothing = HF.label_smoothing_value(label_smoothing)                                              # ValueError on a bad eps
        if self.focal_gamma > 0.0 and self.label_smoothing > 0.0:
            raise ValueError(f'label_smoothing = {label_smoothing!r} together with focal_gamma = {focal_gamma!r}: the combination is not defined')
        self.ohem = HF._ohem_args(ohem, self.focal_gamma, self.label_smoothing, ignore_index)                        # ValueError on a bad value or combination
        self.dice = HF._dice_args(dice, self.focal_gamma, self.label_smoothing, self.ohem)                           # ValueError on a bad value or combination
        self.lovasz = HF._lovasz_args(lovasz, self.focal_gamma, self.label_smoothing, self.ohem, self.dice)          # ValueError on a bad value or combination
        self.class_weight = None if class_weights is None else HF.class_weight_table(class_weights, flat.device)     # ValueError on bad weights
        if isinstance(label_relax, t.Tensor):
            raise ValueError('label_relax: a TrainStep takes the setting (a radius), not a mask: the mask is that of each batch')
        self.label_relax = HF._label_relax_args(label_relax, self.focal_gamma, self.label_smoothing, self.ohem, self.dice, self.lovasz)   # likewise
        self.relax_stats = self.relax_classes = None
        if self.label_relax is not None:
            layers = [m for m in model.modules() if getattr(m, 'logits_layer', False)]
            if not layers:
                raise ValueError('label_relax: the model has no logits layer to take the class count from')
            self.relax_classes = int(layers[0].weight.shape[1])
            if self.relax_classes > 32:
                raise ValueError(f'label_relax: {self.relax_classes} classes, a class set is one 32-bit word')
            self.relax_stats = t.zeros(2, dtype=t.int64, device=flat.device)
        self.fa = FALoss()
        dev = flat.device
        self.flag = t.zeros(1, dtype=t.int32, device=dev)
        self.zero = t.zeros((), device=dev)
        self._pending, self._free = [], []           # (pinned host buffer, event) of iterations in flight / reusable
        self.use_graph = HF.knob('DSRL_GRAPH', True) if graph is None else bool(graph)
        self.fused_losses = True
        self._graphs, self._warm = {}, {}
        self.rng = self.hyper = self._hyper_host = self._hyper_vals = None
        self.host_enqueue_s = 0.0
        self.graph_replays = 0
        if self.use_graph and flat.world > 1:
            # the collectives of a replayed step are launched between / behind its graphs (no hook-launched all-reduce).  The fused BatchNorm
            # kernels keep the 128-block budget ddp.FlatParams selected: an all-reduce of the first gradient chunks runs beside the second
            # half of backward (split capture), and RCCL blocks hold CUs while they wait for peers - a 256-block barrier launch needs every CU
            flat.defer_collectives = True
        # Two-phase backward with more than one rank (DSRL_GRAPH_SPLIT=1; off by default since round 4): backward stops at the layer3 / layer4
        # boundary, the gradient chunks complete by then (head, ASPP, layer4) are all-reduced while layers 3..1 run, the rest behind them.  That
        # schedule puts RCCL kernels beside the device-wide-barrier BatchNorm kernels of the second graph; it is bit-identical to the one-graph
        # schedule and was rehearsed on one GPU, but it has never run with two GPUs on RCCL, so it stays opt-in until a multi-GPU run has recorded
        # `bn_fused_barrier_timeouts` and the exposed all-reduce time with it.  Default: ONE graph, one all-reduce of the whole
        # 239.5 MB arena behind it (round 2's schedule).
        self.split = flat.world > 1 and flat.defer_collectives and HF.knob('DSRL_GRAPH_SPLIT', False)
        self.time_collectives = False           # bench.py: bracket the exposed part of the collectives with events
        self.comm_events = []                   # (broadcast start, end, replay end, end of exchange [+ update: one-graph schedule]) per step

    def relax_fraction(self, reset=False):
        """pixels with more than one class in their set over live pixels, of the training iterations since the record was made or last reset: one
        device read.  None without label_relax; 0.0 before the first live pixel."""
        if self.relax_stats is None:
            return None
        live, multi = (int(v) for v in self.relax_stats.cpu())
        if reset:
            self.relax_stats.zero_()
        return multi / live if live else 0.0

    def _relax_mask(self, target, do_train):
        """the class-set mask of this iteration's labels (training iterations with label_relax only), with the counts added to relax_stats"""
        if not do_train or self.label_relax is None:
            return None
        tg = target if target.dtype == t.uint8 else target.to(t.uint8)
        return HF.relax_mask(tg, self.relax_classes, self.ignore, self.label_relax, self.relax_stats)

    def losses(self, outs, input_org, target, do_train=True, relax=None):
        SSSR, SISR, SSSR_ft, SISR_ft = outs
        extra = {} if relax is None else {'label_relax': relax}
        ce = HF.cross_entropy(SSSR, target, self.ignore, self.class_weight, self.focal_gamma, self.label_smoothing,      # train_or_resume.py:435
                              self.ohem if do_train else None, self.dice if do_train else None, self.lovasz if do_train else None, **extra)
        ms = self.w1 * HF.mse_loss(SISR, input_org) if self.stage > 1 else self.zero       # :436
        fa = self.w2 * self.fa(SSSR_ft, SISR_ft) if self.stage > 2 else self.zero          # :437
        return ce, ms, fa, ce + ms + fa                                                    # :438

    # ------------------------------------------------------------------ the iteration itself (eager, or under capture)
    def _phase_a(self, input_image, input_org, target, do_train, in_graph, split):
        """Step start, forward, losses and - when training - backward: all of it, or (split) down to the layer3 / layer4 cut."""
        flat = self.flat
        bb = None
        if do_train:
            if self.rng is not None:
                self.rng.advance()                # this step's dropout key, derived on the device
            flat.zero_grad()                                                               # optimizer.zero_grad(), :418
            if not in_graph:
                flat.sync_buffers()
            flat.refresh_transposed_filters()     # one launch: the [C][R][S][K] filter copies every dgrad of this step reads
            if split:
                bb = self.model.feature_extractor['backbone']
                bb._dsrl_cut = []
        self.flag.zero_()
        ohem = self.ohem if do_train else None    # validation keeps the configured CE without mining
        dice = self.dice if do_train else None    # and without the Dice term
        lovasz = self.lovasz if do_train else None      # or the Lovasz-Softmax term
        relax = self._relax_mask(target, do_train)      # or the relaxation: the mask launch sits in front of the model's forward
        rx = {} if relax is None else {'label_relax': relax}
        cuts = None
        try:
            with t.set_grad_enabled(do_train):
                if self.fused_losses and do_train:
                    # the layer that produces the logits evaluates the CE value in its own forward kernel (HF.logits_target), :435
                    with HF.logits_target(target if target.dtype == t.uint8 and target.is_contiguous() else None, self.ignore, self.flag,
                                          self.class_weight, self.focal_gamma, self.label_smoothing, ohem, dice, lovasz, **rx):
                        outs = self.model(input_image)                                     # :420
                else:
                    outs = self.model(input_image)                                         # :420
                if self.fused_losses:
                    # CE + MSE + FA, their gradients, the NaN asserts (:426-433) and the loss mix (:435-438) in one launch set
                    vals = HF.fused_losses(outs, target, input_org, self.ignore, self.w1, self.w2, self.stage, self.flag, self.fa.subsample_factor,
                                           self.class_weight, self.focal_gamma, self.label_smoothing, ohem, dice, lovasz, **rx)
                    total = vals[3]
                else:
                    HF.nan_check_(self.flag, *[o for o in outs if o.is_cuda])              # the four NaN asserts, :426-433
                    ce, ms, fa, total = self.losses(outs, input_org, target, do_train, relax)
                    vals = t.cat([t.stack([ce, ms, fa, total]).detach().float(), self.flag.float()])
                if in_graph and HF.knob('DSRL_GRAPH_FAIL_TEST', ''):
                    raise RuntimeError('DSRL_GRAPH_FAIL_TEST: simulated failure in the middle of a capture')      # tests/test_rccl_gpu.py
                if do_train:
                    if self.fused_losses:
                        HF.fused_losses_backward(vals)                                     # :444 (total.backward(), the root gradient a cached constant)
                    else:
                        total.backward()                                                   # :444
                    if split:
                        cuts = bb._dsrl_cut
                        HF.flush_wgrad_queue(reopen=True)      # the weight gradients of head, ASPP and layer4 as one grouped launch set
                        HF.join_side_streams()
        finally:
            if bb is not None:
                bb._dsrl_cut = None
        return outs, vals.detach(), cuts

    def _phase_b(self, cuts):
        """Second backward phase: from the cut tensors through layers 3..1 and the stem, then their grouped weight gradients."""
        pairs = [(o, d.grad) for o, d in cuts if d.grad is not None]
        if pairs:
            t.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        HF.flush_wgrad_queue()
        HF.join_side_streams()

    def _finish(self, hp, in_graph):
        """Gradient exchange (when it did not run between the phases) and the optimiser step."""
        flat = self.flat
        flat.settle_grads()                       # every gradient kernel of the pass has been enqueued or recorded: the arena fill could be skipped again
        hyper = self.hyper if self.rng is not None else None
        if flat.world > 1 and flat.defer_collectives:
            HF.flush_wgrad_queue()
            HF.join_side_streams()
            if in_graph:
                return                            # the collectives and the update follow the replay (_replay)
            if self.split:
                flat.reduce_rest()
                flat.sgd_step(hp[0], hp[1], hp[2], hyper=hyper, reduce=False)
            else:
                flat.reduce_chunked_and_step(hyper=hyper, hp=hp)      # the all-reduce in a few ranges, the update of each range under the next one's exchange
        else:
            flat.sgd_step(hp[0], hp[1], hp[2], hyper=hyper)                                # :445 (eager, world > 1: hook-launched chunk all-reduces overlap)

    def _body(self, input_image, input_org, target, hp, do_train, in_graph=False):
        """One whole iteration, eagerly (graph mode: the iterations before the capture, with the same order of events)."""
        split = self.split and do_train
        try:
            outs, vals, cuts = self._phase_a(input_image, input_org, target, do_train, in_graph, split)
            if do_train:
                if split:
                    self.flat.reduce_chunks(self.flat.ready_chunks())      # runs beside the second phase
                    self._phase_b(cuts)
                self._finish(hp, in_graph)
        except BaseException:
            # a step that aborts between zero_grad() and sgd_step() (an exception in forward / backward, an allocation failure) must not leave the step
            # arena open: the validation forwards that follow would draw records from it, and an arena a graph has pinned cannot grow
            if do_train and self.flat.device.type == 'cuda':
                HF.amax_end_step(self.flat.device)
                HF.wgrad_queue = None
            raise
        return outs, vals

    def _set_hyper(self, hp):
        vals = (float(hp[0]), float(hp[1]), float(hp[2]), 1.0 / self.flat.world)
        if vals != self._hyper_vals:
            self._hyper_host.copy_(t.tensor(vals, dtype=t.float32))
            self.hyper.copy_(self._hyper_host, non_blocking=True)
            self._hyper_vals = vals

    def _graph_key(self, input_image, input_org, target):
        return (tuple(input_image.shape), tuple(input_org.shape), tuple(target.shape), HF.get_conv_precision(), HF.overlap_wgrad,
                self.flat.e_flat is not None,           # "EMA enabled": a step captured without the weight average has no launch that updates it
                self.flat.clip_rec is not None,         # "clip enabled": a step captured without it has neither the norm launches nor hyper_eff
                self.flat.v_flat is not None,           # "AdamW enabled": a step captured without it holds the SGD launches and no advance of t
                self.focal_gamma, self.label_smoothing, self.dice, self.lovasz, self.label_relax, self.ohem)

    def _capture(self, key, input_image, input_org, target, hp):
        """-> the captured step, or None: a capture that fails (a runtime that refuses something inside it) must not end the training run.  This
        TrainStep then keeps launching eagerly - the same kernels and, with more than one rank, the same collectives in the same order, so ranks that
        captured and ranks that did not stay in step.  Nothing of a capture has executed, failed or not: its host-side bookkeeping is rolled back."""
        c = _CapturedStep()
        bns = [m for m in self.model.modules() if isinstance(m, t.nn.modules.batchnorm._BatchNorm)]
        before = [getattr(m, '_dsrl_batches', 0) for m in bns]
        step_before = HF._rng_state['step']
        # A forked capture (weight gradients on a side stream) replays slower than a linear one on this runtime: the graph executor
        # pays more for its cross-queue dependencies than the overlap wins (measured 24.2 vs 23.8 ms per step), so the capture is
        # linear
        overlap_was, HF.overlap_wgrad = HF.overlap_wgrad, False
        c.graph_b, c.ready, mode = None, [], 'thread_local'
        try:
            c.img, c.org, c.tgt = input_image.clone(), input_org.clone(), target.clone()
            c.graph = t.cuda.CUDAGraph()
            with HF.capture_scope(2 << 20) as c.keep:
                if HF.f16_mode():
                    c.keep.append(HF.amax_pin(self.flat.device))      # the graph zeroes, maxes into and reads this arena on every replay: it lives as long as the graph
                if self.split:
                    # two graphs sharing one memory pool: [step start .. backward down to the cut + its weight gradients] and [the rest of backward];
                    # the chunks complete after the first are recorded - on replay their all-reduce is launched between the two graphs
                    with t.cuda.graph(c.graph, capture_error_mode=mode):
                        c.outs, c.vals, cuts = self._phase_a(c.img, c.org, c.tgt, True, True, True)
                    c.ready = self.flat.ready_chunks()
                    c.graph_b = t.cuda.CUDAGraph()
                    with t.cuda.graph(c.graph_b, pool=c.graph.pool(), capture_error_mode=mode):
                        self._phase_b(cuts)
                    del cuts
                else:
                    with t.cuda.graph(c.graph, capture_error_mode=mode):
                        c.outs, c.vals, _ = self._phase_a(c.img, c.org, c.tgt, True, True, False)
                        self._finish(hp, True)
        except Exception as e:          # noqa: BLE001
            self.use_graph = False
            HF.wgrad_queue = None
            HF.abandon_capture(self.flat.device, e, '', 'this TrainStep continues with eager launches')
            return None
        finally:
            # captured or failed, nothing ran: take back the host-side bookkeeping of that phantom iteration
            HF.overlap_wgrad, HF._rng_state['step'] = overlap_was, step_before
            c.bns = [m for m, n in zip(bns, before) if getattr(m, '_dsrl_batches', 0) != n]
            for m, n in zip(bns, before):
                if hasattr(m, '_dsrl_batches'):
                    m._dsrl_batches = n
        self._graphs[key] = c
        return c

    def _replay(self, c, input_image, input_org, target):
        flat = self.flat
        for dst, src in ((c.img, input_image), (c.org, input_org), (c.tgt, target)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        ev = [t.cuda.Event(enable_timing=True) for _ in range(4)] if (self.time_collectives and flat.world > 1) else None
        if flat.world > 1:
            if ev:
                ev[0].record()
            flat.sync_buffers()
            if ev:
                ev[1].record()
            flat._reduced, flat._works = set(), []      # no hook fires during a replay: the chunk bookkeeping of the step starts here
        flat.ensure_filter_amax()           # the graph may rely on the filter magnitudes the previous optimiser pass left (ddp.FlatParams._sgd_range)
        c.graph.replay()
        if c.graph_b is not None:
            flat.reduce_chunks(c.ready)         # head / ASPP / layer4 chunks: their all-reduce runs beside the second graph
            c.graph_b.replay()
        HF._rng_state['step'] += 1              # host mirror of the key the device just derived
        HF._rng_state['current'] = HF._derive(HF._rng_state['step'])
        for m in c.bns:
            m._dsrl_batches += 1
        if flat.world > 1:
            if ev:
                ev[2].record()
            if c.graph_b is not None:
                flat.reduce_rest()
                if ev:
                    ev[3].record()
                flat.sgd_step(0.0, 0.0, 0.0, hyper=self.hyper, reduce=False)
            else:
                flat.reduce_chunked_and_step(hyper=self.hyper)       # exchange + update: SGD of range k under the all-reduce of range k + 1
                if ev:
                    ev[3].record()
            if ev:
                self.comm_events.append(ev)
        self.graph_replays += 1
        return c.outs, c.vals

    def enqueue(self, input_image, input_org, target, lr, momentum, weight_decay, do_train=True):
        """Enqueue one whole iteration on the device and start the asynchronous device->host copy of its five scalars (CE, MSE,
        FA, total, NaN flag) into pinned memory.  Nothing is waited for: collect() returns the values of the OLDEST iteration
        still outstanding.  Calling enqueue(k+1) before collect(k) keeps the launch queue fed across the iteration boundary
        (the reference reads its losses synchronously every iteration, train_or_resume.py:457-460; here the read of
        iteration k overlaps the enqueue of k+1 and the NaN assert fires one iteration late).  Returns the network outputs
        (in graph mode: the capture's static output tensors, overwritten by the next replay)."""
        import time
        t_host0 = time.perf_counter()
        hp = (lr, momentum, weight_decay)
        if do_train and self.flat.ema_swapped:
            raise HF.DsrlHipError('a training step inside FlatParams.ema_weights(): the parameters are the averaged ones')
        if do_train and self.split and self.flat.clip_rec is not None:
            raise HF.DsrlHipError('gradient clipping (grad_clip) is not supported in the two-graph schedule: unset DSRL_GRAPH_SPLIT')
        if do_train and self.split and self.flat.v_flat is not None:
            raise HF.DsrlHipError("AdamW (optimizer='adamw') is not supported in the two-graph schedule: unset DSRL_GRAPH_SPLIT")
        if do_train and self.use_graph:
            if self.rng is None:
                self.rng = HF.DeviceRng(self.flat.device)
                self.hyper = t.zeros(4, device=self.flat.device)
                self._hyper_host = t.empty(4, dtype=t.float32, pin_memory=True)
            self._set_hyper(hp)
            key = self._graph_key(input_image, input_org, target)
            c = self._graphs.get(key)
            if c is None and self._warm.get(key, 0) >= self.GRAPH_WARMUP:
                c = self._capture(key, input_image, input_org, target, hp)
            if c is None:
                self._warm[key] = self._warm.get(key, 0) + 1
                outs, vals = self._body(input_image, input_org, target, hp, True)
            else:
                outs, vals = self._replay(c, input_image, input_org, target)
        else:
            outs, vals = self._body(input_image, input_org, target, hp, do_train)
        if len(self._free) == 0:
            self._free.append((t.empty(5, dtype=t.float32, pin_memory=True), t.cuda.Event()))
        host, ev = self._free.pop()
        host.copy_(vals, non_blocking=True)                                                # ONE device->host read per iteration
        ev.record()
        self._pending.append((host, ev))
        self.host_enqueue_s = time.perf_counter() - t_host0                   # time the host needed to enqueue the whole step
        return outs

    def pending(self):
        return len(self._pending)

    def collect(self):
        """Losses [CE, MSE, FA, total] of the oldest outstanding iteration (waits for it); raises on NaN network outputs."""
        host, ev = self._pending.pop(0)
        ev.synchronize()
        vals = [float(v) for v in host]
        self._free.append((host, ev))
        if int(vals[4]) & 2:
            raise AssertionError('a target label is outside [0, num_classes) and is not the ignore index (CrossEntropyLoss would assert).')
        if vals[4] != 0:
            stuck = HF.bn_fused_barrier_timeouts()
            if stuck:
                raise RuntimeError(f'{stuck} blocks of the fused BatchNorm kernels timed out at their device-wide barrier and poisoned their outputs: '
                                   'is another process using this GPU? (functional.set_bn_fused_max_blocks(0) selects the three-kernel path)')
            raise AssertionError("network output contains 'NaN' values and so cannot continue.")
        return vals[:4]

    def release(self):
        """Drops the captured graphs and unbinds the device-resident dropout key (launches take their `seed` argument again)."""
        self._graphs.clear()
        if self.rng is not None:
            self.rng.release()
            self.rng = None

    def __call__(self, input_image, input_org, target, lr, momentum, weight_decay, do_train=True):
        """Synchronous form: enqueue + collect of the same iteration."""
        while self._pending:
            self.collect()
        outs = self.enqueue(input_image, input_org, target, lr, momentum, weight_decay, do_train)
        return self.collect(), outs


def _get_state_dict(model):
    return model.state_dict()


def check_class_weights(dataset, num_classes):
    """dataset['class_weights']: absent / None, a sequence of `num_classes` finite numbers >= 0, or 'enet'.  -> None, a float32 numpy array, or
    'enet'; ValueError otherwise.  Touches no device: called before anything is set up.  'enet' (w_c = 1 / ln(1.02 + f_c) from the class
    frequencies of the training split) needs the pre-decoded cache of the project's own loader to count from."""
    cw = dataset.get('class_weights')
    if cw is None:
        return None
    if isinstance(cw, str):
        if cw != 'enet':
            raise ValueError(f"dataset['class_weights'] = {cw!r}: expected None, {num_classes} numbers or 'enet'")
        if dataset.get('loader_factory') is not None:
            from ..datasets.Cityscapes.loader import cache_dir_of, has_cache
            if not (dataset.get('cache_path') or dataset.get('path')) or not has_cache(cache_dir_of(dataset)):
                raise ValueError("dataset['class_weights'] = 'enet' counts the classes of the pre-decoded Cityscapes cache: with a caller's "
                                 "'loader_factory' there is none (set dataset['cache_path'] to one, or pass the weights as numbers)")
        return 'enet'
    return HF.class_weight_table(cw, 'cpu', num_classes)[:num_classes].numpy()


def check_focal_gamma(dataset):
    """dataset['focal_gamma']: absent, None or 0 -> 0.0 (off); a finite number > 0 -> that float; ValueError otherwise.  Touches no device."""
    g = dataset.get('focal_gamma')
    return 0.0 if g is None else HF.focal_gamma_value(g)


def check_label_smoothing(dataset):
    """dataset['label_smoothing']: absent, None or 0 -> 0.0 (off); a number in (0, 1] -> that float; ValueError otherwise, and on a value > 0
    together with dataset['focal_gamma'] > 0 (the combination has no definition).  Touches no device."""
    e = dataset.get('label_smoothing')
    e = 0.0 if e is None else HF.label_smoothing_value(e)
    if e > 0.0 and check_focal_gamma(dataset) > 0.0:
        raise ValueError(f"label_smoothing = {e!r} together with focal_gamma = {dataset.get('focal_gamma')!r}: the combination is not defined")
    return e


def check_ohem(dataset):
    """dataset['ohem']: absent, None or False -> None (off); True, a pair (thresh, min_kept) or a mapping with these keys -> (thresh, min_kept), as
    HF.ohem_value; ValueError otherwise, on a value together with dataset['focal_gamma'] > 0 or dataset['label_smoothing'] > 0 (scoped out), and on
    an ignore label of the dataset that is no byte value.  Touches no device."""
    return HF._ohem_args(dataset.get('ohem'), check_focal_gamma(dataset), check_label_smoothing(dataset), dataset['settings'].IGNORE_CLASS_LABEL)


def check_dice(dataset):
    """dataset['dice']: absent, None, False or 0 -> None (off); True, a weight > 0, a pair (weight, smooth) or a mapping with the keys 'weight' and
    'smooth' -> (weight, smooth), as HF.dice_value; ValueError otherwise, and on a value together with dataset['focal_gamma'] > 0,
    dataset['label_smoothing'] > 0 or dataset['ohem'] (scoped out).  Touches no device."""
    return HF._dice_args(dataset.get('dice'), check_focal_gamma(dataset), check_label_smoothing(dataset), check_ohem(dataset))


def check_lovasz(dataset):
    """dataset['lovasz']: absent, None, False or 0 -> None (off); True, a weight > 0, a pair (weight, bins) or a mapping with the keys 'weight' and
    'bins' -> (weight, bins), as HF.lovasz_value; ValueError otherwise, and on a value together with dataset['focal_gamma'] > 0,
    dataset['label_smoothing'] > 0, dataset['ohem'] or dataset['dice'] (scoped out).  Touches no device."""
    return HF._lovasz_args(dataset.get('lovasz'), check_focal_gamma(dataset), check_label_smoothing(dataset), check_ohem(dataset), check_dice(dataset))


def check_ema(dataset):
    """dataset['ema']: absent, None or False -> None (off); True, a decay in (0, 1), a pair (decay, warmup) or a mapping with these keys ->
    (decay, warmup), as HF.ema_value; ValueError otherwise.  Touches no device."""
    return HF.ema_value(dataset.get('ema'))


def check_optimizer(dataset):
    """dataset['optimizer']: absent, None or 'sgd' -> None (SGD); 'adamw' or {'name': 'adamw', 'betas': (b1, b2), 'eps': e} -> (beta1, beta2, eps),
    as HF.adamw_value; ValueError otherwise.  Touches no device."""
    return HF.adamw_value(dataset.get('optimizer'))


def check_label_relax(dataset):
    """dataset['label_relax']: absent, None, False or 0 -> None (off); True (radius 1), an integer radius in [1, 4] or {'radius': r} -> the radius, as
    HF.label_relax_value; ValueError otherwise, and on a value together with dataset['focal_gamma'] > 0, dataset['label_smoothing'] > 0,
    dataset['ohem'], dataset['dice'] or dataset['lovasz'].  Touches no device."""
    value = dataset.get('label_relax')
    if isinstance(value, t.Tensor):
        raise ValueError("dataset['label_relax']: expected a setting (a radius), not a tensor")
    return HF._label_relax_args(value, check_focal_gamma(dataset), check_label_smoothing(dataset), check_ohem(dataset), check_dice(dataset),
                                check_lovasz(dataset))


def check_grad_clip(dataset):
    """dataset['grad_clip']: absent, None or False -> None (off); a number > 0 (inf: monitor only) or {'max_norm': such a number} -> that float,
    as HF.grad_clip_value; ValueError otherwise.  Touches no device."""
    return HF.grad_clip_value(dataset.get('grad_clip'))


def checkpoint_dict(have, ema_state_dict=None):
    """What a checkpoint file holds: every key of settings.VARIABLES_IN_CHECKPOINT out of `have` and nothing else - the reference's layout -, plus
    'ema_state_dict' (FlatParams.ema_state_dict()) in a run with dataset['ema'].  'model_state_dict' stays the live weights: a resume needs them."""
    out = {k: have[k] for k in settings.VARIABLES_IN_CHECKPOINT}
    if ema_state_dict is not None:
        out['ema_state_dict'] = ema_state_dict
    return out


def train_or_resume(is_resuming_training, device, distributed, mixed_precision, disable_cudnn_benchmark, num_workers, dataset, val_interval,
                    checkpoint_interval, checkpoint_history, init_weights, batch_size, epochs, learning_rate, end_learning_rate, momentum,
                    weights_decay, poly_power, stage, w1, w2, freeze_batch_norm, experiment_id, description, early_stopping, dry_run=False, **other_args):
    if not isCUDAdevice(device):
        raise RuntimeError("this build runs on the MI355X only: use device='gpu' (the reference's --device cpu path is its own)")
    if mixed_precision not in settings.MIXED_PRECISION_TO_CONV_ARITHMETIC:
        raise RuntimeError(f"mixed_precision={mixed_precision!r}: expected one of {sorted(k for k in settings.MIXED_PRECISION_TO_CONV_ARITHMETIC if k)} "
                           '(apex itself is not used: the opt level selects the MFMA conv arithmetic)')
    conv_arith = settings.MIXED_PRECISION_TO_CONV_ARITHMETIC[mixed_precision]
    class_weights = check_class_weights(dataset, dataset['settings'].NUM_CLASSES)
    focal_gamma = check_focal_gamma(dataset)
    label_smoothing = check_label_smoothing(dataset)
    ohem = check_ohem(dataset)
    dice = check_dice(dataset)
    lovasz = check_lovasz(dataset)
    label_relax = check_label_relax(dataset)
    ema = check_ema(dataset)
    grad_clip = check_grad_clip(dataset)
    adamw = check_optimizer(dataset)
    input_size = other_args.get('model_input_size', settings.MODEL_INPUT_SIZE)
    if distributed:
        t.manual_seed(settings.RANDOM_SEED)                                                # identical init on all ranks, :31
        if not dist.is_initialized():
            dist.init_process_group(distributed['BACKEND'], distributed['INIT_METHOD'], world_size=distributed['WORLD_SIZE'], rank=distributed['RANK'])
        if not dist.is_initialized():
            raise RuntimeError("Couldn't initialize distributed process group!")
        is_master_rank = (distributed['RANK'] == 0)
        device_obj = t.device('cuda', distributed['DEVICE_ID'])
        rank, world = distributed['RANK'], distributed['WORLD_SIZE']
    else:
        is_master_rank, device_obj, rank, world = True, t.device('cuda', t.cuda.current_device()), 0, 1
    t.cuda.set_device(device_obj)
    if is_master_rank:
        process_start_timestamp = datetime.now()
        best_validation_dict = other_args['best_validation_dict'] if is_resuming_training else {'epoch': -1, 'best_miou_percent': 0., 'loss': 0.}

    ds = dataset['settings']
    model = DSRL(stage, ds)                                                                # :62
    if is_resuming_training:
        model.load_state_dict(other_args['model_state_dict'], strict=True)
        starting_epoch = other_args['epoch']
    else:
        starting_epoch = 0
        if init_weights:
            model.load_state_dict(t.load(init_weights, map_location='cpu')['model_state_dict'], strict=False)
        elif stage == 1:
            if other_args.get('pretrained_backbone', True):
                model.initialize_with_pretrained_weights(settings.WEIGHTS_ROOT_DIR)
        else:
            prev = os.path.join(experiment_id, settings.WEIGHTS_DIR.format(stage=stage - 1), settings.FINAL_WEIGHTS_FILE)
            if os.path.isfile(prev):
                model.load_state_dict(t.load(prev, map_location='cpu')['model_state_dict'], strict=False)      # :91-96
            elif other_args.get('pretrained_backbone', True):
                model.initialize_with_pretrained_weights(settings.WEIGHTS_ROOT_DIR)
    model = model.to(device_obj).to(memory_format=t.channels_last)                        # :103 (+ kernel weight layout)
    flat = FlatParams(model)                                                               # DDP wrap, :105-106
    if adamw is not None:
        # dataset['optimizer']: AdamW inside the optimiser pass, its step counter and bias corrections on the device.  In front of the
        # state load - which then expects torch.optim.AdamW's layout and refuses SGD's - and of the average and the clipping.
        flat.enable_adamw(adamw[:2], adamw[2])
        if momentum:
            warnings.warn(f"dataset['optimizer'] = 'adamw': momentum = {momentum!r} is not used (betas = {adamw[:2]!r}); it is stored in checkpoints as given")
    if is_resuming_training and 'optimizer_state_dict' in other_args:
        flat.load_state_dict(other_args['optimizer_state_dict'])
    if ema is not None:
        # dataset['ema']: an exponential moving average of the weights and BatchNorm statistics, updated inside the optimiser launches.
        # Validation - and with it the best checkpoint, early stopping and the dataset-level figures - measures the AVERAGED model, the final weights file
        # stores it, checkpoints carry it as 'ema_state_dict' beside the live weights a resume needs.  With several ranks every rank averages its own
        # arenas: the parameters are identical on all of them, the buffers are rank 0's, and only rank 0's average is ever read (validation and files).
        flat.enable_ema(*ema)             # after the broadcast and the state load: the average starts from the weights training starts from
        if is_resuming_training:
            if other_args.get('ema_state_dict') is not None:
                flat.load_ema_state_dict(other_args['ema_state_dict'])
            else:
                warnings.warn("resuming with dataset['ema'] from a checkpoint without 'ema_state_dict': the average starts from the loaded weights at 0 updates")
    if grad_clip is not None:
        # dataset['grad_clip']: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) inside the optimiser pass, on the device;
        # every epoch record carries the gradient-norm figures of its training iterations.  inf reports the figures and changes nothing else.
        flat.enable_grad_clip(grad_clip)
    factory = dataset.get('loader_factory')
    own_loader = factory is None
    if own_loader:
        os.makedirs(dataset['path'], exist_ok=True)
        if len(os.listdir(dataset['path'])) == 0:
            raise Exception("Cityscapes dataset was not found under '{:s}'.".format(dataset['path']))
        # the Cityscapes tree (or its pre-decoded cache): HIP augmentations on a side stream, datasets/Cityscapes/loader.py
        from ..datasets.Cityscapes.loader import loader_factory
        factory = loader_factory(dataset, input_size, settings.RANDOM_SEED, distributed=bool(distributed))
    if isinstance(class_weights, str):          # 'enet': from the class counts of the cached training labels (counted once, kept beside the cache)
        from ..datasets.Cityscapes.class_weights import class_counts, enet_weights
        from ..datasets.Cityscapes.loader import cache_dir_of
        from ..models.transforms import DeviceBatchPreparation
        lut = DeviceBatchPreparation(ds.LABEL_MAPPING_DICT, ds.MEAN, ds.STD, input_size, ds.IGNORE_CLASS_LABEL).lut_host
        class_weights = enet_weights(class_counts(cache_dir_of(dataset), 'train', lut, device_obj)[:ds.NUM_CLASSES])
    step = TrainStep(model, flat, stage, w1, w2, ds.IGNORE_CLASS_LABEL, class_weights=class_weights, focal_gamma=focal_gamma,
                     label_smoothing=label_smoothing, ohem=ohem, dice=dice, lovasz=lovasz, **({} if label_relax is None else {'label_relax': label_relax}))
    train_loader = factory('train', batch_size, device_obj, rank, world)
    val_loader = factory('val', batch_size, device_obj, rank, world) if is_master_rank else None

    history = []
    CE_val_avg_loss = MSE_val_avg_loss = FA_val_avg_loss = Avg_val_loss = None
    amp_state_dict = None

    def save_checkpoint(filename, epoch, train_means):
        """utils.py:273-275 with every key of settings.VARIABLES_IN_CHECKPOINT (train_or_resume.py:268-282, 318-332)."""
        ckpt_dir = os.path.join(experiment_id, settings.CHECKPOINTS_DIR.format(stage=stage))
        os.makedirs(ckpt_dir, exist_ok=True)
        have = {'device': device, 'mixed_precision': mixed_precision, 'amp_state_dict': amp_state_dict, 'disable_cudnn_benchmark': disable_cudnn_benchmark,
                'num_workers': num_workers, 'val_interval': val_interval, 'checkpoint_interval': checkpoint_interval, 'checkpoint_history': checkpoint_history,
                'init_weights': init_weights, 'batch_size': batch_size, 'epochs': epochs, 'learning_rate': learning_rate,
                'end_learning_rate': end_learning_rate, 'momentum': momentum, 'weights_decay': weights_decay, 'poly_power': poly_power, 'stage': stage,
                'w1': w1, 'w2': w2, 'freeze_batch_norm': freeze_batch_norm, 'experiment_id': experiment_id, 'description': description,
                'early_stopping': early_stopping, 'CE_train_avg_loss': train_means[0], 'MSE_train_avg_loss': train_means[1],
                'FA_train_avg_loss': train_means[2], 'Avg_train_loss': train_means[3], 'CE_val_avg_loss': CE_val_avg_loss,
                'MSE_val_avg_loss': MSE_val_avg_loss, 'FA_val_avg_loss': FA_val_avg_loss, 'Avg_val_loss': Avg_val_loss, 'epoch': epoch,
                'best_validation_dict': best_validation_dict, 'model_state_dict': _get_state_dict(model),
                'optimizer_state_dict': flat.state_dict(lr, momentum, weights_decay, initial_lr=learning_rate)}
        t.save(checkpoint_dict(have, flat.ema_state_dict() if ema is not None else None), os.path.join(ckpt_dir, filename))
        return ckpt_dir

    if conv_arith is not None:
        HF.set_conv_precision(conv_arith)
    try:
        for epoch in range(starting_epoch + 1, epochs + 1):
            lr = polynomial_lr(learning_rate, end_learning_rate, epoch - 1, epochs, poly_power)       # scheduler.step() per epoch, :349
            if own_loader:
                train_loader.set_epoch(epoch)     # the sample order and the augmentation draws of this epoch
            means = _do_train_val(True, epoch, model, step, train_loader, lr, momentum, weights_decay, freeze_batch_norm, is_master_rank)
            rec = {'epoch': epoch, 'lr': lr, 'train': means}
            if adamw is not None:
                rec['optimizer'] = 'adamw'
            if dice is not None:
                rec['train_ce_includes_dice'] = list(dice)      # (weight, smooth): means[0] is CE + weight * L_dice; the validation figures are the CE alone
            if lovasz is not None:
                rec['train_ce_includes_lovasz'] = True          # means[0] is CE + weight * L_lovasz; the validation figures are the CE alone
            if label_relax is not None:
                rec['train_ce_is_relaxed'] = True               # means[0] is the relaxed CE at this radius; the validation figures are the configured CE
                rec['relaxed_fraction'] = step.relax_fraction(reset=True)       # one device read per epoch: border pixels over live pixels
            if grad_clip is not None:
                gc = flat.grad_clip_stats(reset=True)           # one device read per epoch: the norms of this epoch's training iterations
                rec['grad_norm_mean'], rec['grad_norm_max'] = gc['norm_mean'], gc['norm_max']
                rec['grad_clipped_fraction'] = gc['clipped'] / gc['steps'] if gc['steps'] else 0.0
                rec['grad_nonfinite_steps'] = gc['nonfinite']
            stop = False
            if is_master_rank:
                if checkpoint_history > 0 and epoch % checkpoint_interval == 0 and experiment_id:                 # :264
                    CE_val_avg_loss = MSE_val_avg_loss = FA_val_avg_loss = Avg_val_loss = None                      # :270-273
                    ckpt_dir = save_checkpoint(settings.CHECKPOINT_FILE.format(epoch=epoch), epoch, means)
                    old = epoch - checkpoint_history * checkpoint_interval                                            # :285-291
                    if old > 0:
                        stale = os.path.join(ckpt_dir, settings.CHECKPOINT_FILE.format(epoch=old))
                        if os.path.isfile(stale):
                            os.remove(stale)
                if val_loader is not None and epoch % val_interval == 0:                                            # :294
                    details = {}
                    if stage > 1:           # PSNR and SSIM of the SISR output against the 2x original; reported, nothing is decided from them
                        from ..metrices import SRQuality
                        details['sr_quality'] = SRQuality(ds.MEAN, ds.STD)
                    from ..metrices import Calibration      # ECE / MCE of the validated model; reported, nothing is decided from them
                    details['calibration'] = Calibration(ignore_index=step.ignore)
                    with flat.ema_weights() if ema is not None else contextlib.nullcontext():      # the averaged model is the one that is measured
                        rec['val'] = _do_train_val(False, epoch, model, step, val_loader, lr, momentum, weights_decay, False, True, details)
                    rec['val_mIoU_dataset'], rec['val_IoU_per_class'] = rec['val'][6], details['IoU_per_class']
                    if 'sr_quality' in details:
                        rec['val_PSNR'], rec['val_SSIM'] = details['PSNR'], details['SSIM']
                    rec['val_ECE'], rec['val_MCE'] = details['ECE'], details['MCE']
                    CE_val_avg_loss, MSE_val_avg_loss, FA_val_avg_loss, Avg_val_loss, val_mIoU = rec['val'][:5]
                    if val_mIoU > best_validation_dict['best_miou_percent']:                                        # :318-337
                        best_validation_dict = {'epoch': epoch, 'best_miou_percent': val_mIoU, 'loss': Avg_val_loss}
                        if experiment_id:
                            ckpt_dir = os.path.join(experiment_id, settings.CHECKPOINTS_DIR.format(stage=stage))
                            for x in glob.glob(os.path.join(ckpt_dir, '*_bestval.checkpoint')):
                                if os.path.isfile(x):
                                    os.remove(x)
                            save_checkpoint(settings.CHECKPOINT_FILE.format(epoch='{:d}_bestval'.format(epoch)), epoch, means)
                    if means[3] < Avg_val_loss and early_stopping:                                                  # :341-347
                        rec['early_stopped'] = stop = True
            history.append(rec)
            if distributed:
                # the reference breaks on the master rank only (its other ranks would hang in the next collective); here every rank learns it
                flag = t.tensor([1 if stop else 0], device=device_obj)
                dist.broadcast(flag, 0)
                stop = bool(flag.item())
            if stop:
                break
    finally:
        step.release()
        if conv_arith is not None:
            HF.set_conv_precision(None)
    if is_master_rank and experiment_id:
        wdir = os.path.join(experiment_id, settings.WEIGHTS_DIR.format(stage=stage))
        os.makedirs(wdir, exist_ok=True)
        final = {'model_state_dict': _get_state_dict(model), 'mixed_precision': mixed_precision, 'amp_state_dict': amp_state_dict}
        if ema is not None:
            # the averaged weights: the model validation measured, and what the next stage starts from
            avg = flat.ema_state_dict()
            final['ema'] = {'decay': avg.pop('ema_decay'), 'updates': avg.pop('ema_updates')}
            final['model_state_dict'] = avg
        t.save(final, os.path.join(wdir, settings.FINAL_WEIGHTS_FILE))                        # utils.py:277-282
        history.append({'elapsed': str(datetime.now() - process_start_timestamp)})
    return history


def _do_train_val(do_train, epoch, model, step, data_loader, lr, momentum, weights_decay, freeze_batch_norm, is_master_rank, details=None):
    """train_or_resume.py:373-533 without the progress-bar / TensorBoard plumbing. Returns the running means
    (CE, MSE, FA, Total, mIoU %, accuracy %) and, as a last element, the dataset-level mIoU % (metrices.ConfusionMatrix over the whole loader);
    the last three only for validation.  Everything decided from a validation - best checkpoint, early stopping - uses the reference's per-batch
    mIoU.  `details` (a dict, optional) receives 'IoU_per_class' of the dataset-level figure; a validation that finds a metrices.SRQuality under
    details['sr_quality'] feeds it every batch's SISR output and original (two launches per batch, one read at the end) and leaves 'PSNR' and 'SSIM';
    one that finds a metrices.Calibration under details['calibration'] feeds it the logits validation already has (one launch per batch, one read at
    the end) and leaves 'ECE' and 'MCE' (fractions in [0, 1])."""
    model.train(mode=do_train)
    if do_train and freeze_batch_norm:
        for m in model.modules():
            if isinstance(m, t.nn.modules.batchnorm._BatchNorm):
                m.eval()                                                                   # :379-382
    from ..metrices import Accuracy, AverageMeter, ConfusionMatrix, mIoU
    meters = [AverageMeter() for _ in range(4)]                                            # CE, MSE, FA, Total (:385-388)
    nc = model.SSSR_decoder['cls_conv'].out_channels
    miou, mean_accuracy = mIoU(num_classes=nc, ignore_index=step.ignore), Accuracy(num_classes=nc, ignore_index=step.ignore)
    whole = ConfusionMatrix(num_classes=nc, ignore_index=step.ignore)
    whole_fits = nc <= ConfusionMatrix.max_classes_from_logits()        # beyond it the one-pass kernel has no room for the matrix: the figure is NaN
    srq = details.get('sr_quality') if (details is not None and not do_train and is_master_rank) else None
    cal = details.get('calibration') if (details is not None and not do_train and is_master_rank) else None
    sizes = []

    def drain(keep):
        while step.pending() > keep:
            vals, n = step.collect(), sizes.pop(0)
            for mtr, v in zip(meters, vals):
                mtr.update(v, n)                                                           # AverageMeter.update(value, batch), :457-460

    for (input_image, input_org), (target, _) in data_loader:
        outs = step.enqueue(input_image, input_org, target, lr, momentum, weights_decay, do_train)
        sizes.append(input_image.shape[0])
        if not do_train and is_master_rank:
            miou.update_from_logits(outs[0], target)                                       # argmax + histograms on the device (:476-480)
            mean_accuracy.update_from_logits(outs[0], target)
            if whole_fits:
                whole.update_from_logits(outs[0], target)
            if srq is not None:
                srq.update(outs[1], input_org)
            if cal is not None:
                cal.update_from_logits(outs[0], target)
        drain(1)              # the losses of iteration k are read while iteration k+1 is already queued
    drain(0)
    fig = whole.result() if not do_train else None
    if details is not None and fig is not None:
        details['IoU_per_class'] = [float(v) for v in fig['IoU']]
    if srq is not None:
        quality = srq.result()
        details['PSNR'], details['SSIM'] = quality['PSNR'], quality['SSIM']
    if cal is not None:
        cfig = cal.result()
        details['ECE'], details['MCE'] = cfig['ECE'], cfig['MCE']
    return [m() for m in meters] + [miou() if not do_train else 0.0, mean_accuracy() if not do_train else 0.0, fig['mIoU'] if fig is not None else 0.0]


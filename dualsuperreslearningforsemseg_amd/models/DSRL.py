"""Dual Super-Resolution Learning model on the MI355X kernels - the surface of the reference's models/DSRL.py:11-186:
`DSRL(stage, dataset_settings, init_weights=True, BatchNorm2d=...)`, the same sub-module attribute names and therefore the
same 702 state_dict keys, `.forward(x) -> (SSSR, SISR, SSSR_ft, SISR_ft)`.  Tensors are logical NCHW in
torch.channels_last memory; call `model.to(device).to(memory_format=torch.channels_last)` to store conv weights in
the [K][R][S][C] layout the kernels read without a per-step re-layout.
"""
import torch as t

from .. import consts
from .. import functional as HF
from ..nn_modules import (HipBatchNorm2d, HipConv2d, HipConvTranspose2d, HipDropout, HipPixelShuffle, HipReLU, HipSequential,
                          HipUpsamplingBilinear2d)
from .BaseModel import BaseModel
from .modules.ASPP import ASPP
from .modules.backbone import ResNet101

# Philox stream id of each Dropout module (shared with oracle.dsrl_oracle.DROPOUT_STREAMS)
_DROPOUT_STREAMS = {('cat_conv', 3): 1, ('cat_conv', 7): 2, ('upsample16_pred', 1): 3, ('upsample16_pred', 5): 4}


class DSRL(BaseModel):

    @staticmethod
    def _define_feature_extractor(in_channels: int, out_channels1: int, out_channels2: int):
        return t.nn.ModuleDict({
            'backbone': ResNet101(replace_stride_with_dilation=[False, False, True]),                       # DSRL.py:17
            'aspp': ASPP(in_channels=in_channels, out_channels=out_channels1, rate=1),                       # DSRL.py:18
            'shortcut_conv': HipSequential(HipConv2d(out_channels1, out_channels2, kernel_size=1, padding=0, bias=False),
                                           HipBatchNorm2d(num_features=out_channels2), HipReLU())})        # DSRL.py:19-25

    @staticmethod
    def _define_SSSR_decoder(in_channels1: int, in_channels2: int, mid_channels: int, out_channels: int):
        mods = t.nn.ModuleDict({
            'cat_conv': HipSequential(HipConv2d(in_channels1 + in_channels2, mid_channels, kernel_size=3, padding=1, bias=False),
                                      HipBatchNorm2d(num_features=mid_channels), HipReLU(), HipDropout(p=0.2),
                                      HipConv2d(mid_channels, mid_channels, kernel_size=3, padding=1, bias=False),
                                      HipBatchNorm2d(num_features=mid_channels), HipReLU(), HipDropout(p=0.2)),     # DSRL.py:34-49
            'cls_conv': HipConv2d(mid_channels, out_channels, kernel_size=1, bias=True),                             # DSRL.py:50
            'upsample16_pred': HipSequential(HipUpsamplingBilinear2d(scale_factor=2.0), HipDropout(p=0.2),
                                             HipConvTranspose2d(out_channels, out_channels, kernel_size=2, stride=2, padding=0, bias=False),
                                             HipBatchNorm2d(num_features=out_channels), HipReLU(), HipDropout(p=0.2),
                                             HipConvTranspose2d(out_channels, out_channels, kernel_size=2, stride=2, padding=0, bias=True))})  # DSRL.py:53-69
        for (name, idx), stream in _DROPOUT_STREAMS.items():
            mods[name][idx].rng_stream = stream
        mods['upsample16_pred'][6].logits_layer = True        # its output is SSSR_output: the CE gradient can be formed inside its backward (HF.LogitsGrad)
        return mods

    @staticmethod
    def _define_SISR_decoder(in_channels: int, out_channels: int, upscale_factor: int):
        assert type(upscale_factor) == int, "BUG CHECK: 'upscale_factor' must be an integer type."
        return HipSequential(HipConv2d(in_channels, out_channels * (upscale_factor ** 2), kernel_size=3, stride=1, padding=1, bias=True),
                             HipPixelShuffle(upscale_factor=upscale_factor))                                                # DSRL.py:78-84

    @staticmethod
    def _define_feature_transformer(in_channels: int, out_channels: int):
        return HipSequential(HipConv2d(in_channels, out_channels, kernel_size=1, stride=8, padding=0, bias=False),
                             HipBatchNorm2d(num_features=out_channels), HipReLU())                                          # DSRL.py:88-95

    def __init__(self, stage, dataset_settings, init_weights=True, BatchNorm2d=HipBatchNorm2d):
        assert stage in [1, 2, 3], "BUG CHECK: Unsupported stage {0} specified in DSRL.__init__().".format(stage)
        super().__init__()
        self.stage = stage
        self.feature_extractor = DSRL._define_feature_extractor(in_channels=2048, out_channels1=256, out_channels2=48)
        self.SSSR_decoder = DSRL._define_SSSR_decoder(in_channels1=256, in_channels2=48, mid_channels=256,
                                                      out_channels=dataset_settings.NUM_CLASSES)
        if init_weights:
            self._init_weights(BatchNorm2d, self.feature_extractor['shortcut_conv'], self.SSSR_decoder)
        if self.stage > 1:
            self.SISR_decoder = DSRL._define_SISR_decoder(in_channels=(256 + 48), out_channels=consts.NUM_RGB_CHANNELS, upscale_factor=8)
            if init_weights:
                self._init_weights(BatchNorm2d, self.SISR_decoder)
            if self.stage > 2:
                self.SSSR_feature_transformer = DSRL._define_feature_transformer(in_channels=dataset_settings.NUM_CLASSES, out_channels=1)
                self.SISR_feature_transformer = DSRL._define_feature_transformer(in_channels=consts.NUM_RGB_CHANNELS, out_channels=1)
                if init_weights:
                    self._init_weights(BatchNorm2d, self.SSSR_feature_transformer, self.SISR_feature_transformer)

    @t.no_grad()
    def _init_weights(self, BatchNorm2d, *modules):
        # DSRL.py:143-151 (conv biases keep torch's default init)
        for module in modules:
            for m in module.modules():
                if isinstance(m, (t.nn.Conv2d, t.nn.ConvTranspose2d)):
                    t.nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                elif isinstance(m, BatchNorm2d):
                    m.weight.fill_(1.0)
                    m.bias.zero_()

    def initialize_with_pretrained_weights(self, weights_dir, map_location=t.device('cpu')):
        self.feature_extractor['backbone'].initialize_with_pretrained_weights(weights_dir, map_location)

    def forward_head(self, backbone_features: t.Tensor, lowlevel_features: t.Tensor):
        """DSRL.py:162-184 on given backbone outputs (the part SURVEY.md section 8 scopes; used directly by the parity tests)."""
        fe = self.feature_extractor
        aspp_features = fe['aspp'](backbone_features)
        h, w = aspp_features.shape[-2:]
        aspp_features = HF.upsample_bilinear_ac(aspp_features, (4 * h, 4 * w))                 # DSRL.py:163
        oslot = getattr(lowlevel_features, '_dsrl_outer_slot', None)                          # shared with layer2's first block (ResNet101.forward)
        lowlevel_features = (fe['shortcut_conv'](lowlevel_features, grad_slot=oslot) if (oslot is not None and isinstance(fe['shortcut_conv'], HipSequential))
                             else fe['shortcut_conv'](lowlevel_features))                     # DSRL.py:164
        cat_features = HF.cat_channels([aspp_features, lowlevel_features])                    # DSRL.py:165
        # cat_features feeds cat_conv.0 and (stage > 1) the SISR conv: both data gradients accumulate in one buffer (HF.GradSlot)
        slot = None
        if (HF.grad_slots_enabled and self.stage > 1 and cat_features.requires_grad and t.is_grad_enabled()
                and isinstance(self.SSSR_decoder['cat_conv'], HipSequential) and isinstance(self.SISR_decoder, HipSequential)):
            cat_features, slot = HF.fork(cat_features), HF.GradSlot()
        # the output of cat_conv (BN -> ReLU -> Dropout, DSRL.py:44-49) feeds cls_conv only: its data gradient leaves that BatchNorm's backward sums
        link = HF.BNLink() if (HF.bn_bwd_stats_enabled and t.is_grad_enabled() and isinstance(self.SSSR_decoder['cat_conv'], HipSequential)
                               and isinstance(self.SSSR_decoder['cls_conv'], HipConv2d)) else None
        kw = {} if link is None else {'out_link': link}
        SSSR_output = (self.SSSR_decoder['cat_conv'](cat_features, grad_slot=slot, **kw) if slot is not None
                       else self.SSSR_decoder['cat_conv'](cat_features, **kw))                # DSRL.py:168
        SSSR_output = (self.SSSR_decoder['cls_conv'](SSSR_output, in_link=link) if (link is not None and link.valid)
                       else self.SSSR_decoder['cls_conv'](SSSR_output))                       # DSRL.py:169
        SSSR_output = self.SSSR_decoder['upsample16_pred'](SSSR_output)                       # DSRL.py:170
        # DSRL.py:172-174: unused outputs are CPU zeros(1) whatever the model device
        SISR_output = t.zeros(1, requires_grad=False)
        SSSR_transform_output = t.zeros(1, requires_grad=False)
        SISR_transform_output = t.zeros(1, requires_grad=False)
        if self.stage > 1:
            SISR_output = self.SISR_decoder(cat_features, grad_slot=slot) if slot is not None else self.SISR_decoder(cat_features)   # DSRL.py:177
            if self.stage > 2:
                if HF.grad_slots_enabled and t.is_grad_enabled() and SSSR_output.requires_grad:
                    # each output feeds its feature transformer and the loss: with functional.fused_losses the loss publishes the dense
                    # gradient and the stride-8 transformer adds its sparse one into it (no 320 MB mostly-zero tensor + add pass)
                    SSSR_output._dsrl_out_slot, SISR_output._dsrl_out_slot = HF.GradSlot(), HF.GradSlot()
                SSSR_transform_output = self.SSSR_feature_transformer(SSSR_output)            # DSRL.py:181
                SISR_transform_output = self.SISR_feature_transformer(SISR_output)            # DSRL.py:184
        return SSSR_output, SISR_output, SSSR_transform_output, SISR_transform_output

    def forward(self, x: t.Tensor):
        with t.autograd.profiler.record_function(DSRL.forward.__qualname__):                  # DSRL.py:159
            HF.begin_forward(self.training)
            backbone_features, lowlevel_features = self.feature_extractor['backbone'](x)      # DSRL.py:161
            return self.forward_head(backbone_features, lowlevel_features)

    def predict_head(self, backbone_features: t.Tensor, lowlevel_features: t.Tensor, target: t.Tensor = None, ignore_index: int = 255, nan_flag: t.Tensor = None,
                     flip: bool = False, confusion: t.Tensor = None, calibration: t.Tensor = None, confidence: bool = False, temperature=None):
        """Inference counterpart of forward_head: the SSSR branch in eval mode down to the bilinear x2 of `upsample16_pred`, then its ConvTranspose ->
        BatchNorm -> ReLU -> ConvTranspose tail and the arg-max as one kernel (functional.sssr_tail_predict) -> (pred uint8 (N,H,W), counts, ce).
        With `target` (N,H,W): `counts` is the int64 table of dsrl_seg_metrics of this batch (metrices.mIoU / Accuracy.update_from_counts), a fresh
        tensor per call, and `ce` the 0-d CrossEntropyLoss(ignore_index); both None otherwise.  `confusion` (int64 device tensor of classes^2 elements,
        needs a target; metrices.ConfusionMatrix.matrix) gets this batch's confusion matrix [target, predicted] ADDED by the same kernel and is never
        cleared here: one buffer collects a whole split.  `nan_flag` (int32 device scalar) collects bit 0 = NaN logit, bit 1 = label outside
        the classes; nothing is read back here.  Neither the SISR decoder nor the feature transformers run, whatever the stage.
        `flip=True`: the features are those of 2N images, the second half from the horizontally mirrored images; the tail kernel mirrors that half back
        and averages the two views' class probabilities -> N class maps (functional.sssr_tail_predict(flip=True)), `target` (N,H,W).
        `calibration` (int64 device tensor of 3 * bins elements, needs a target; metrices.Calibration.record) gets this batch's reliability record
        ADDED by the same kernel; `confidence=True` appends the confidence map (float32 (N,H,W): the probability of the reported class) to the
        returned tuple.  Without them every launch is the one of a call that does not know them.
        `temperature` (functional.temperature_value: None and 1 are "off" and leave every launch as it is; a finite number T > 0): the model reports
        softmax(logits / T) - `ce`, the calibration record and the confidence map are those of the scaled model, the class map and the counters of a
        single view do not change (functional.sssr_tail_predict(temperature=))."""
        if self.training:
            raise HF.DsrlHipError('DSRL.predict* is inference: call model.eval() first')
        temperature = HF.temperature_value(temperature, 'DSRL.predict_head')
        with t.no_grad():
            fe, dec = self.feature_extractor, self.SSSR_decoder
            aspp_features = fe['aspp'](backbone_features)
            h, w = aspp_features.shape[-2:]
            aspp_features = HF.upsample_bilinear_ac(aspp_features, (4 * h, 4 * w))            # DSRL.py:163
            cat_features = HF.cat_channels([aspp_features, fe['shortcut_conv'](lowlevel_features)])    # DSRL.py:164-165
            up = dec['upsample16_pred']
            y = up[0](dec['cls_conv'](dec['cat_conv'](cat_features)))                          # DSRL.py:168-170 up to the bilinear x2
            counts = None
            if target is not None:
                counts = t.zeros(3 * up[6].out_channels + 2, dtype=t.int64, device=y.device)
            more = {} if temperature is None else {'temperature': temperature}
            out = HF.sssr_tail_predict(y, up[2], up[3], up[6], target=target, ignore_index=ignore_index, counts=counts, nan_flag=nan_flag, flip=flip,
                                       confusion=confusion, calibration=calibration, confidence=confidence, **more)
        return (out[0], counts, out[1]) + tuple(out[2:])

    def predict(self, x: t.Tensor, target: t.Tensor = None, ignore_index: int = 255, nan_flag: t.Tensor = None, flip: bool = False,
                confusion: t.Tensor = None, scales=None, calibration: t.Tensor = None, confidence: bool = False, temperature=None, window=None,
                stride=None):
        """Class map of a batch: (pred, counts or None, ce or None), see predict_head.  Runs under no_grad and raises in train mode.  Without a
        `nan_flag` of the caller's the flag is read back here and a NaN logit or an out-of-range label raises; a caller that passes one reads it when
        it chooses to (command_handlers.benchmark: once, after the last batch).
        `flip=True`: the horizontal-flip ensemble.  The trunk runs once on cat([x, x.flip(3)]) (2N images) and the tail kernel forms the ensemble:
        N class maps, counters and the loss of the averaged class probabilities.
        `confusion`: see predict_head; with `flip` it is the matrix of the ensemble's class map.
        `scales` (a sequence of numbers, functional.multiscale_scales_value; None, () and (1.0,) are "off" and leave every launch as it is): the
        multi-scale ensemble.  For each scale in turn the images are resized to the multiple of 16 nearest to scale x size (align corners), the SSSR
        logits of the eval forward path are written (with `flip` for the image and its mirror image in one batch), merged into the ensemble and
        released before the next scale runs (functional.ProbMerge: the logits of every view resampled to the output grid, softmax, class probabilities
        averaged); pred, counts, ce, confusion and the NaN flag are those of the ensemble.
        `calibration`, `confidence`: see predict_head; with `flip` and `scales` they are the record and the confidence map of the ensemble.
        `temperature`: see predict_head (a T fitted by command_handlers.fit_temperature); combines with flip, target, confusion, calibration and
        confidence.  With `scales` it is a ValueError before any device work: the multi-scale merge takes no temperature.
        `window`, `stride` (functional.window_value: an integer or a pair (rows, columns) of input pixels; None, and a window that is the whole image,
        are "off" and leave every launch as it is; a missing stride is 2/3 of the window): sliding-window inference.  The ASPP's global-average-pool
        branch makes the network depend on the input size, so an image larger than the training crop is evaluated in overlapping windows of the
        training size: for each position of functional.window_plan in turn the crop goes through the eval forward path (with `flip` the crop and its
        mirror image in one batch), its SSSR logits are merged into the ensemble where the window lies and released before the next position runs
        (functional.WindowMerge: softmax per view, class probabilities averaged over the views covering a pixel - mmseg's slide mode averages
        logits); pred, counts, ce, confusion, calibration, confidence and the NaN flag are those of the ensemble.  With `scales` or `temperature`
        it is a ValueError before any device work."""
        if self.training:
            raise HF.DsrlHipError('DSRL.predict* is inference: call model.eval() first')
        if confusion is not None and target is None:
            raise HF.DsrlHipError('DSRL.predict: confusion needs a target')
        if calibration is not None and target is None:
            raise HF.DsrlHipError('DSRL.predict: calibration needs a target')
        temperature = HF.temperature_value(temperature, 'DSRL.predict')
        scales = HF.multiscale_scales_value(scales)
        if temperature is not None and scales is not None:
            raise ValueError('DSRL.predict: temperature does not combine with scales (the multi-scale merge takes no temperature)')
        window = HF.window_value(window, stride)
        if window is not None:
            if scales is not None or temperature is not None:
                raise ValueError('DSRL.predict: window does not combine with scales or temperature (the window merge resamples nothing and takes no temperature)')
            if x.dim() != 4:
                raise HF.DsrlHipError(f'DSRL.predict: (N,3,H,W) images expected, got shape {tuple(x.shape)}')
            plan = HF.window_plan(x.shape[2], x.shape[3], *window)           # None: the window is the whole image, "off"
            if plan is not None:
                return self._predict_windows(x, target, ignore_index, nan_flag, flip, confusion, window, plan, calibration, confidence)
        if scales is not None:
            return self._predict_multiscale(x, target, ignore_index, nan_flag, flip, confusion, scales, calibration, confidence)
        own = nan_flag is None
        with t.no_grad():
            if own:
                nan_flag = t.zeros((), dtype=t.int32, device=x.device)
            HF.nan_check_(nan_flag, x)          # a NaN pixel would not reach the logits: the first ReLU (fmaxf) maps it to 0
            if flip:
                both = t.empty((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device, memory_format=t.channels_last)
                both[:x.shape[0]].copy_(x)
                both[x.shape[0]:].copy_(x.flip(3))          # 3 channels at input size: torch ops
                x = both
            backbone_features, lowlevel_features = self.feature_extractor['backbone'](x)
            more = {} if temperature is None else {'temperature': temperature}
            out = self.predict_head(backbone_features, lowlevel_features, target, ignore_index, nan_flag, flip, confusion, calibration, confidence, **more)
        if own:
            bits = int(nan_flag.item())
            if bits:
                raise HF.DsrlHipError('DSRL.predict: ' + ' and '.join(m for b, m in ((1, 'NaN in the input or the logits'), (2, 'labels outside the classes')) if bits & b))
        return out

    def super_resolve_head(self, backbone_features: t.Tensor, lowlevel_features: t.Tensor):
        """Inference counterpart of forward_head for the other branch: ASPP, upsample, shortcut, concatenation and `SISR_decoder` in eval mode ->
        the super-resolved image (N,3,2H,2W), normalised as the input is and bit-identical to `forward(x)[1]`.  Neither the SSSR decoder nor the
        feature transformers run.  Raises in train mode and at stage 1, which has no SISR decoder."""
        if self.training:
            raise HF.DsrlHipError('DSRL.super_resolve* is inference: call model.eval() first')
        if self.stage < 2:
            raise HF.DsrlHipError('DSRL.super_resolve*: a stage-1 model has no SISR decoder')
        with t.no_grad():
            fe = self.feature_extractor
            aspp_features = fe['aspp'](backbone_features)
            h, w = aspp_features.shape[-2:]
            aspp_features = HF.upsample_bilinear_ac(aspp_features, (4 * h, 4 * w))            # DSRL.py:163
            cat_features = HF.cat_channels([aspp_features, fe['shortcut_conv'](lowlevel_features)])    # DSRL.py:164-165
            return self.SISR_decoder(cat_features)                                             # DSRL.py:177

    def super_resolve(self, x: t.Tensor):
        """The super-resolved image of a batch, see super_resolve_head.  Runs under no_grad."""
        if self.training:
            raise HF.DsrlHipError('DSRL.super_resolve* is inference: call model.eval() first')
        if self.stage < 2:
            raise HF.DsrlHipError('DSRL.super_resolve*: a stage-1 model has no SISR decoder')
        with t.no_grad():
            HF.begin_forward(False)
            backbone_features, lowlevel_features = self.feature_extractor['backbone'](x)      # DSRL.py:161
            return self.super_resolve_head(backbone_features, lowlevel_features)

    def _eval_sssr_logits(self, x: t.Tensor):
        """The SSSR logits (N,classes,2H,2W) of the eval-mode forward path on `x`: forward() without the SISR decoder and the feature transformers."""
        HF.begin_forward(False)
        fe, dec = self.feature_extractor, self.SSSR_decoder
        backbone_features, lowlevel_features = fe['backbone'](x)                              # DSRL.py:161
        aspp_features = fe['aspp'](backbone_features)
        h, w = aspp_features.shape[-2:]
        aspp_features = HF.upsample_bilinear_ac(aspp_features, (4 * h, 4 * w))                 # DSRL.py:163
        cat_features = HF.cat_channels([aspp_features, fe['shortcut_conv'](lowlevel_features)])    # DSRL.py:164-165
        return dec['upsample16_pred'](dec['cls_conv'](dec['cat_conv'](cat_features)))         # DSRL.py:168-170

    def _predict_multiscale(self, x, target, ignore_index, nan_flag, flip, confusion, scales, calibration=None, confidence=False):
        HF._need_gpu(x, target, nan_flag, confusion, calibration)
        if x.dim() != 4 or x.shape[2] % 16 or x.shape[3] % 16:
            raise HF.DsrlHipError(f'DSRL.predict: (N,3,H,W) images with H and W multiples of 16 expected, got shape {tuple(x.shape)}')
        N, _, H, W = x.shape
        sizes = HF.multiscale_sizes(H, W, scales)
        own = nan_flag is None
        with t.no_grad():
            if own:
                nan_flag = t.zeros((), dtype=t.int32, device=x.device)
            HF.nan_check_(nan_flag, x)          # once, on the images as given: every view is interpolated from them
            classes = self.SSSR_decoder['upsample16_pred'][6].out_channels
            counts = t.zeros(3 * classes + 2, dtype=t.int64, device=x.device) if target is not None else None
            merge = HF.ProbMerge(len(sizes) * (2 if flip else 1), N, classes, (2 * H, 2 * W), x.device, target, ignore_index, counts, nan_flag, confusion,
                                 calibration, confidence)
            out = None
            for size in sizes:
                xk = HF.resize_image_ac(x, size)
                if flip:
                    both = t.empty((2 * N,) + tuple(xk.shape[1:]), dtype=xk.dtype, device=xk.device, memory_format=t.channels_last)
                    both[:N].copy_(xk)
                    both[N:].copy_(xk.flip(3))
                    xk = both
                logits = self._eval_sssr_logits(xk)
                if flip:
                    merge.add(logits[:N], False)
                    out = merge.add(logits[N:], True)
                else:
                    out = merge.add(logits, False)
                del logits, xk                  # one scale's logits at a time
        if own:
            bits = int(nan_flag.item())
            if bits:
                raise HF.DsrlHipError('DSRL.predict: ' + ' and '.join(m for b, m in ((1, 'NaN in the input or the logits'), (2, 'labels outside the classes')) if bits & b))
        return (out[0], counts, out[1]) + tuple(out[2:])

    def _predict_windows(self, x, target, ignore_index, nan_flag, flip, confusion, window, plan, calibration=None, confidence=False):
        HF._need_gpu(x, target, nan_flag, confusion, calibration)
        N, _, H, W = x.shape
        (h, w), (ys, xs) = window[0], plan
        own = nan_flag is None
        with t.no_grad():
            if own:
                nan_flag = t.zeros((), dtype=t.int32, device=x.device)
            HF.nan_check_(nan_flag, x)          # once, on the images as given: every window is a crop of them
            classes = self.SSSR_decoder['upsample16_pred'][6].out_channels
            counts = t.zeros(3 * classes + 2, dtype=t.int64, device=x.device) if target is not None else None
            merge = HF.WindowMerge(tuple(2 * y for y in ys), tuple(2 * v for v in xs), (2 * h, 2 * w), N, classes, (2 * H, 2 * W), x.device, target,
                                   ignore_index, counts, nan_flag, confusion, calibration, confidence, flip)
            out = None
            for y0 in ys:
                for x0 in xs:
                    crop = x[:, :, y0:y0 + h, x0:x0 + w]
                    if flip:
                        xk = t.empty((2 * N, x.shape[1], h, w), dtype=x.dtype, device=x.device, memory_format=t.channels_last)
                        xk[:N].copy_(crop)
                        xk[N:].copy_(crop.flip(3))
                    else:
                        xk = crop.contiguous(memory_format=t.channels_last)
                    logits = self._eval_sssr_logits(xk)
                    if flip:
                        merge.add(logits[:N])
                        out = merge.add(logits[N:])
                    else:
                        out = merge.add(logits)
                    del logits, xk              # one position's logits at a time
        if own:
            bits = int(nan_flag.item())
            if bits:
                raise HF.DsrlHipError('DSRL.predict: ' + ' and '.join(m for b, m in ((1, 'NaN in the input or the logits'), (2, 'labels outside the classes')) if bits & b))
        return (out[0], counts, out[1]) + tuple(out[2:])

    def compile_predict(self, batch_size=None, input_size=None, graph=True):
        """-> inference.CompiledPredictor: `predict` on operands prepared once (inference.FrozenOperands: filter amax records, pre-split filters, fp16
        filter planes, BatchNorm 1/std) and replayed from one hipGraph per (N, H, W, with target, conv arithmetic); bit-identical to `predict`.
        `batch_size` and `input_size` (H, W) given: that key is captured right away.  While the predictor lives the model's weights are frozen: any
        change makes its calls raise until release() and a new compile_predict(); release() leaves the model exactly as it was."""
        from ..inference import CompiledPredictor
        return CompiledPredictor(self, batch_size=batch_size, input_size=input_size, graph=graph)

"""Segment an image, a folder of images or a dataset split with given weights and write visualisations - counterpart of the reference's
command_handlers/test.py (same `test(...)` signature and file names).

What differs by design: image files are normalised and resized to the model input by dsrl_prepare_batch, the align-corners transform the network
was trained with (the reference's torchvision Resize here is a different one); the class map comes from `DSRL.predict`; the command is headless
(no window, no wait for a key) and returns the files it wrote.  `compiled_model=True`: `weights` names a file written by the compile_model command
(data, not TorchScript) and the class maps come from inference.CompiledPredictor - frozen operands and a hipGraph replay, the same bytes.  Either
way the input | class colours | overlay panels are built on the device (utils.make_input_output_visualization_device): what crosses to the host
per image is the finished uint8 panel, which PIL encodes.  `flip=True` in other_args: the class maps are those of the horizontal-flip ensemble
(`DSRL.predict(flip=True)`).  `scales=(...)` in other_args: those of the multi-scale ensemble (`DSRL.predict(scales=...)`; combines with `flip`);
the value is validated before any device work, and with `compiled_model` the command raises before it reads the file.  `window=` / `stride=` in
other_args (an integer or a pair, in pixels of `model_input_size`): those of sliding-window inference (`DSRL.predict(window=...)`; combines with
`flip`); validated against `model_input_size` before any device work, a ValueError with `scales` or `compiled_model`."""
import functools
import os

import numpy as np
import torch as t

from .. import consts, settings
from .._lib import DsrlHipError
from ..functional import multiscale_scales_value, window_plan, window_value
from ..models.transforms import DeviceBatchPreparation
from ..utils import make_input_output_visualization_device
from .benchmark import NOT_GPU, load_eval_model, split_loader
from .train_or_resume import isCUDAdevice


def _save_png(hwc, filename):
    from PIL import Image
    os.makedirs(os.path.dirname(filename) or '.', exist_ok=True)
    Image.fromarray(np.ascontiguousarray(hwc), mode='RGB').save(filename, format='PNG')
    print('Output image saved as: {0:s}.'.format(filename))
    return filename


@t.no_grad()
def test(image_file, images_dir, dataset, output_dir, weights, device, compiled_model, **other_args):
    scales = multiscale_scales_value(other_args.get('scales'))          # ValueError on a bad value, before any device work
    window = window_value(other_args.get('window'), other_args.get('stride'))
    if window is not None:
        clash = [k for k, on in (('scales', scales is not None), ('compiled_model', compiled_model)) if on]
        if clash:
            raise ValueError(f"test: window does not combine with {', '.join(clash)} (the windows run through the eager single-scale DSRL.predict)")
        size = tuple(other_args.get('model_input_size', settings.MODEL_INPUT_SIZE))
        if window_plan(size[0], size[1], *window) is None:       # ValueError on a window the input cannot take; the whole input is "off"
            window = None
    if not isCUDAdevice(device):
        raise RuntimeError(NOT_GPU)
    data = None
    if compiled_model and scales is not None:
        from ..inference import MULTISCALE_NOT_COMPILED
        raise DsrlHipError(MULTISCALE_NOT_COMPILED)
    if compiled_model:
        from ..inference import load_compiled_model, read_compiled_file
        data = read_compiled_file(weights)                  # format, version and ABI are checked on the host, before any device work
    if not dataset:
        dataset = settings.DATASETS['cityscapes']          # the normalisation constants are not stored with the weights
    ds = dataset['settings']
    input_size = tuple(other_args.get('model_input_size', settings.MODEL_INPUT_SIZE))
    output_size = tuple(2 * v for v in input_size)
    device_obj = t.device('cuda', t.cuda.current_device())
    predictor = None
    if compiled_model:
        model, predictor = load_compiled_model(weights, device_obj, data=data)
        predict = predictor
    else:
        model = load_eval_model(weights, ds, device_obj)
        predict = model.predict
    try:
        if other_args.get('flip'):
            predict = functools.partial(predict, flip=True)
        if scales is not None:
            predict = functools.partial(predict, scales=scales)
        if window is not None:
            predict = functools.partial(predict, window=window[0], stride=window[1])
        return _run(predict, image_file, images_dir, dataset, ds, output_dir, device_obj, input_size, output_size)
    finally:
        if predictor is not None:
            predictor.release()


def _run(predict, image_file, images_dir, dataset, ds, output_dir, device_obj, input_size, output_size):
    written = []

    if image_file or images_dir:
        from PIL import Image, ImageOps
        names = [image_file] if image_file else sorted(os.path.join(images_dir, f) for f in os.listdir(images_dir)
                                                       if f.lower().endswith(consts.IMAGE_FILE_EXTENSIONS))
        prepare = DeviceBatchPreparation(ds.LABEL_MAPPING_DICT, ds.MEAN, ds.STD, input_size, ds.IGNORE_CLASS_LABEL)
        for name in names:
            with Image.open(name) as opened:
                rgb = np.array(ImageOps.exif_transpose(opened).convert('RGB').resize((output_size[1], output_size[0]), resample=Image.BILINEAR),
                               dtype=np.uint8)
            rgb_dev = t.from_numpy(rgb).unsqueeze(0).to(device_obj)
            (input_image, _), _ = prepare(rgb_dev)
            pred, _, _ = predict(input_image)
            vis = make_input_output_visualization_device(rgb_dev, pred, ds.CLASS_RGB_COLOR)
            written.append(_save_png(vis[0].cpu().numpy(), os.path.join(output_dir, os.path.splitext(os.path.basename(name))[0] + '.png')))
        return written

    loader = split_loader(dataset, dataset['split'], 1, device_obj, input_size)
    first, limit = int(dataset.get('starting_index', 0)), dataset.get('max_images')
    # the shown image, (std * x + mean) * 255 clipped, in float64 as three separately rounded element-wise passes: what numpy evaluated on the host
    mean = t.tensor(np.array(ds.MEAN), dtype=t.float64, device=device_obj).reshape(1, 1, consts.NUM_RGB_CHANNELS)
    std = t.tensor(np.array(ds.STD), dtype=t.float64, device=device_obj).reshape(1, 1, consts.NUM_RGB_CHANNELS)
    for i, ((input_image, input_org), (target, _)) in enumerate(loader):
        if i < first:
            continue
        if limit is not None and len(written) >= int(limit):
            break
        pred, _, _ = predict(input_image)
        scaled = std * input_org[0].permute(1, 2, 0).to(t.float64)
        scaled = (scaled + mean) * 255.
        shown = t.clamp(scaled, 0., 255.).to(t.uint8)
        # two panels, target above prediction; in the prediction the pixels the target ignores are drawn as ignored (the mask; a no-op for the target itself)
        tgt = target[0].to(t.uint8)
        vis = make_input_output_visualization_device(shown.unsqueeze(0).expand(2, -1, -1, -1), t.stack((tgt, pred[0])), ds.CLASS_RGB_COLOR,
                                                     mask=t.stack((tgt, tgt)), ignore_index=ds.IGNORE_CLASS_LABEL)
        written.append(_save_png(vis.reshape(-1, vis.shape[2], 3).cpu().numpy(), os.path.join(output_dir, str(i) + '.png')))
    return written

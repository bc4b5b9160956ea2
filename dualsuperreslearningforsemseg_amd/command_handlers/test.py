"""Segment an image, a folder of images or a dataset split with given weights and write visualisations - counterpart of the reference's
command_handlers/test.py (same `test(...)` signature and file names).

What differs by design: image files are normalised and resized to the model input by dsrl_prepare_batch, the align-corners transform the network
was trained with (the reference's torchvision Resize here is a different one); the class map comes from `DSRL.predict`; the command is headless
(no window, no wait for a key) and returns the files it wrote; there is no TorchScript, so `compiled_model` raises."""
import os

import numpy as np
import torch as t

from .. import consts, settings
from ..models.transforms import DeviceBatchPreparation
from ..utils import make_input_output_visualization
from .benchmark import NOT_GPU, load_eval_model, split_loader
from .train_or_resume import isCUDAdevice


def _save_png(chw, filename):
    from PIL import Image
    os.makedirs(os.path.dirname(filename) or '.', exist_ok=True)
    Image.fromarray(np.ascontiguousarray(chw.transpose(1, 2, 0)), mode='RGB').save(filename, format='PNG')
    print('Output image saved as: {0:s}.'.format(filename))
    return filename


@t.no_grad()
def test(image_file, images_dir, dataset, output_dir, weights, device, compiled_model, **other_args):
    if not isCUDAdevice(device):
        raise RuntimeError(NOT_GPU)
    if compiled_model:
        raise RuntimeError('compiled_model: TorchScript models are not supported by this build (the kernels are reached through ctypes)')
    if not dataset:
        dataset = settings.DATASETS['cityscapes']          # the normalisation constants are not stored with the weights
    ds = dataset['settings']
    input_size = tuple(other_args.get('model_input_size', settings.MODEL_INPUT_SIZE))
    output_size = tuple(2 * v for v in input_size)
    device_obj = t.device('cuda', t.cuda.current_device())
    model = load_eval_model(weights, ds, device_obj)
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
            (input_image, _), _ = prepare(t.from_numpy(rgb).unsqueeze(0).to(device_obj))
            pred, _, _ = model.predict(input_image)
            vis = make_input_output_visualization(rgb.transpose(2, 0, 1), pred[0].cpu().numpy(), ds.CLASS_RGB_COLOR)
            written.append(_save_png(vis, os.path.join(output_dir, os.path.splitext(os.path.basename(name))[0] + '.png')))
        return written

    loader = split_loader(dataset, dataset['split'], 1, device_obj, input_size)
    first, limit = int(dataset.get('starting_index', 0)), dataset.get('max_images')
    mean = np.array(ds.MEAN).reshape(consts.NUM_RGB_CHANNELS, 1, 1)
    std = np.array(ds.STD).reshape(consts.NUM_RGB_CHANNELS, 1, 1)
    for i, ((input_image, input_org), (target, _)) in enumerate(loader):
        if i < first:
            continue
        if limit is not None and len(written) >= int(limit):
            break
        pred, _, _ = model.predict(input_image)
        shown = np.clip((std * input_org[0].float().cpu().numpy() + mean) * 255., 0., 255.).astype(np.uint8)
        target_map, pred_map = target[0].cpu().numpy(), pred[0].cpu().numpy()
        pred_map[target_map == ds.IGNORE_CLASS_LABEL] = ds.IGNORE_CLASS_LABEL
        vis = np.concatenate((make_input_output_visualization(shown, target_map, ds.CLASS_RGB_COLOR),
                              make_input_output_visualization(shown, pred_map, ds.CLASS_RGB_COLOR)), axis=1)
        written.append(_save_png(vis, os.path.join(output_dir, str(i) + '.png')))
    return written

"""Host-side helpers of the inference commands (the reference keeps theirs in utils.py)."""
import numpy as np
import torch as t


def load_checkpoint_or_weights(filename, map_location='cpu', ema=False):
    """A `.weights` or `.checkpoint` file written by train_or_resume: a dict with at least 'model_state_dict'.  `ema=True`: the averaged weights of
    a checkpoint written with dataset['ema'] - its 'ema_state_dict' without the two bookkeeping keys - are returned as 'model_state_dict'; a file
    without one raises.  (A final weights file of such a run already holds the averaged weights as 'model_state_dict'.)"""
    d = t.load(filename, map_location=map_location)
    if not isinstance(d, dict) or 'model_state_dict' not in d:
        raise RuntimeError(f"'{filename}' holds no 'model_state_dict': not a .weights / .checkpoint file of this project")
    if ema:
        if not isinstance(d.get('ema_state_dict'), dict):
            raise RuntimeError(f"'{filename}' holds no 'ema_state_dict': it was not written by a training run with dataset['ema']")
        d = dict(d)
        d['model_state_dict'] = {k: v for k, v in d['ema_state_dict'].items() if k not in ('ema_updates', 'ema_decay')}
    return d


def make_input_output_visualization(input_image, output_map, class_rgb_color, blend_factor=0.4):
    """input_image (3,H,W) uint8, output_map (H,W) of class labels, class_rgb_color {label: (r, g, b)} -> (3,H,3W) uint8:
    input | class colours | overlay, overlay = uint8(min((1 - blend_factor) * input + blend_factor * colour, 255)) evaluated in float64.
    Labels the palette does not name are drawn black.  numpy on the host: 6 MB per 1024x2048 image, not a hot path."""
    input_image = np.asarray(input_image)
    output_map = np.asarray(output_map)
    assert input_image.ndim == 3 and output_map.ndim == 2 and input_image.shape[-2:] == output_map.shape, (input_image.shape, output_map.shape)
    assert 0.0 < blend_factor < 1.0
    input_image = input_image.astype(np.uint8)
    palette = np.zeros((256, input_image.shape[0]), dtype=np.uint8)         # one 256-entry look-up table per channel
    for label, rgb in class_rgb_color.items():
        palette[int(label) & 0xff] = rgb
    colours = np.ascontiguousarray(palette[output_map.astype(np.uint8)].transpose(2, 0, 1))
    blend = (1. - blend_factor) * input_image.astype(np.float64) + blend_factor * colours.astype(np.float64)
    overlay = np.minimum(blend, 255.).astype(np.uint8)
    return np.concatenate((input_image, colours, overlay), axis=2)


def make_input_output_visualization_device(rgb_u8, classes, class_rgb_color, mask=None, ignore_index=255, blend_factor=0.4):
    """The same panels built on the device (functional.class_map_visualize): rgb_u8 (N,H,W,3) uint8, classes (N,H,W) uint8, mask (N,H,W) uint8 or None
    (where mask == ignore_index the class is drawn as ignore_index), all on the GPU -> device uint8 (N,H,3W,3); `out[n]` holds the bytes of
    make_input_output_visualization(rgb_u8[n] as (3,H,W), classes[n], class_rgb_color, blend_factor) transposed to (H,3W,3)."""
    from . import functional as HF
    return HF.class_map_visualize(rgb_u8, classes, HF.palette_tensor(class_rgb_color, rgb_u8.device), mask=mask, ignore_index=ignore_index,
                                  blend_factor=blend_factor)

"""Write a compiled model file for `test --compiled-model` / `benchmark` - counterpart of the reference's command_handlers/compile_model.py (same
`compile_model(...)` signature).

What differs by design: the reference traces the network with TorchScript and saves code; here the kernels are reached through ctypes and a hipGraph
cannot be serialised, so the file holds DATA only - the stage-1 state dict, the shape and conv arithmetic to capture, and the dataset constants the
commands need - and inference.load_compiled_model freezes the operands and captures the graph when it loads the file.  Runs on the CPU."""
import os

import torch as t

from .. import settings
from ..inference import FORMAT, FORMAT_VERSION
from ..models import DSRL
from ..utils import load_checkpoint_or_weights


@t.no_grad()
def compile_model(weights, output_file, dataset, **other_args):
    from .. import _lib, functional as HF
    ds = dataset['settings']
    model = DSRL(stage=1, dataset_settings=ds, init_weights=False).eval()
    try:
        model.load_state_dict(load_checkpoint_or_weights(weights, map_location='cpu')['model_state_dict'], strict=True)
    except RuntimeError as e:
        raise RuntimeError(f"compile_model: '{weights}' does not load strictly into the stage-1 model - a stage-2/3 file has to go through the "
                           f'prune_weights command first ({str(e)[:300]})') from e
    precision = other_args.get('conv_precision') or HF.get_conv_precision()
    if precision not in HF.CONV_PRECISION_MODES:
        raise RuntimeError(f'compile_model: unknown conv arithmetic {precision!r} (one of {sorted(HF.CONV_PRECISION_MODES)})')
    out = {'format': FORMAT, 'format_version': FORMAT_VERSION, 'abi_version': int(_lib.load().dsrl_version()),
           'model_state_dict': {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()},
           'model_input_size': [int(v) for v in other_args.get('model_input_size', settings.MODEL_INPUT_SIZE)],
           'batch_size': int(other_args.get('batch_size', 1)), 'conv_precision': str(precision),
           'NUM_CLASSES': int(ds.NUM_CLASSES), 'MEAN': [float(v) for v in ds.MEAN], 'STD': [float(v) for v in ds.STD],
           'IGNORE_CLASS_LABEL': int(ds.IGNORE_CLASS_LABEL), 'CLASS_RGB_COLOR': {int(k): [int(c) for c in v] for k, v in ds.CLASS_RGB_COLOR.items()}}
    os.makedirs(os.path.dirname(output_file) or '.', exist_ok=True)
    t.save(out, output_file)
    print('Compiled model saved to specified file.')
    return output_file

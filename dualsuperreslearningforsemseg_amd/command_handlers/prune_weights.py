"""Drop from a weights / checkpoint file what inference does not need - counterpart of the reference's command_handlers/prune_weights.py (same
`prune_weights(...)` signature): the state dict of a stage-2/3 model carries the SISR decoder and the feature transformers, a stage-1 model has
neither, and the compile_model command loads strictly.

What differs by design: the source is loaded with strict=False - dropping the keys stage 1 does not have is the command's purpose, and a strict load
(as the reference writes it) refuses exactly the files the command exists for.  Runs on the CPU."""
import os

import torch as t

from ..models import DSRL
from ..utils import load_checkpoint_or_weights


@t.no_grad()
def prune_weights(src_weights, dest_weights, dataset, **other_args):
    model = DSRL(stage=1, dataset_settings=dataset['settings'], init_weights=False).eval()
    src = load_checkpoint_or_weights(src_weights, map_location='cpu', ema=other_args.get('ema', False))      # ema=True: the averaged weights of a checkpoint
    missing, _dropped = model.load_state_dict(src['model_state_dict'], strict=False)
    missing = [k for k in missing if not k.endswith('num_batches_tracked')]
    if missing:
        raise RuntimeError(f"'{src_weights}' lacks {len(missing)} entries of the stage-1 model (first: {missing[0]}): not a DSRL weights file")
    os.makedirs(os.path.dirname(dest_weights) or '.', exist_ok=True)
    t.save({'model_state_dict': model.state_dict(), 'mixed_precision': src.get('mixed_precision'), 'amp_state_dict': src.get('amp_state_dict')}, dest_weights)
    print("Output weight saved in '{:s}'.".format(dest_weights))
    return dest_weights

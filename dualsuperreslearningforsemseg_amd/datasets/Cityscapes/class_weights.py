"""Per-class loss weights from the class frequencies of the cached label maps (the ENet rule most Cityscapes recipes use against the
imbalance between road / building and rider / train / motorcycle)."""
import json
import os

import numpy as np
import torch

from ... import functional as HF
from ..._lib import call
from .loader import CityscapesCache

COUNTS_FILE = 'class_counts_{split}.json'
COUNTS_VERSION = 1
CHUNK_IMAGES = 32


def class_counts(cache_dir, split, lut=None, device='cuda'):
    """-> numpy int64 [256]: how many pixels of the cached `split` label maps carry each label byte, after the remap through `lut` (256 uint8, or
    None for the raw ids).  Counted on the device by dsrl_class_histogram, CHUNK_IMAGES images at a time; the result is written beside the cache
    (class_counts_{split}.json, data only) and reused while the image count and the remap table still match."""
    lut_list = None if lut is None else [int(v) for v in torch.as_tensor(lut).reshape(-1).tolist()]
    if lut_list is not None and len(lut_list) != 256:
        raise ValueError(f'class_counts: the remap table has {len(lut_list)} entries, expected 256')
    cache = CityscapesCache(cache_dir, split)
    n = len(cache)
    path = os.path.join(cache_dir, COUNTS_FILE.format(split=split))
    if os.path.isfile(path):
        try:
            with open(path) as f:
                rec = json.load(f)
            if rec.get('version') == COUNTS_VERSION and rec.get('images') == n and rec.get('lut') == lut_list and len(rec.get('counts', ())) == 256:
                return np.asarray(rec['counts'], dtype=np.int64)
        except (OSError, ValueError):
            pass                                    # unreadable: count again
    device = torch.device(device)
    counts = torch.zeros(256, dtype=torch.int64, device=device)
    lut_dev = None if lut_list is None else torch.tensor(lut_list, dtype=torch.uint8, device=device)
    HF._need_gpu(counts)
    for i0 in range(0, n, CHUNK_IMAGES):
        chunk = torch.from_numpy(np.ascontiguousarray(cache.labels[i0:i0 + CHUNK_IMAGES])).to(device)
        call('dsrl_class_histogram', chunk.data_ptr(), chunk.numel(), None if lut_dev is None else lut_dev.data_ptr(), counts.data_ptr(), HF._stream())
    out = counts.cpu().numpy()
    tmp = f'{path}.{os.getpid()}.tmp'          # (every rank may count: each writes its own file and renames it over the same data)
    with open(tmp, 'w') as f:
        json.dump({'version': COUNTS_VERSION, 'split': split, 'images': n, 'lut': lut_list, 'counts': [int(v) for v in out]}, f)
    os.replace(tmp, path)
    return out


def enet_weights(counts):
    """w_c = 1 / ln(1.02 + n_c / sum n) in float64 (Paszke et al., ENet, 2016); a class that never occurs gets 1 / ln 1.02."""
    n = np.asarray(counts, dtype=np.float64)
    if n.ndim != 1 or n.size == 0 or (n < 0).any():
        raise ValueError('enet_weights: expected a vector of non-negative class counts')
    total = n.sum()
    f = n / total if total > 0 else np.zeros_like(n)
    return 1.0 / np.log(1.02 + f)

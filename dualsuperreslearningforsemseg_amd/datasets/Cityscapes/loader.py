"""Cityscapes reader, pre-decoded uint8 cache and device-fed loaders (the reference's torchvision Cityscapes + DataLoader, train_or_resume.py:139-170).

* pairs(): leftImg8bit/{split}/*/*_leftImg8bit.png with gtFine/{split}/*/*_gtFine_labelIds.png, sorted (torchvision Cityscapes, mode 'fine',
  target_type 'semantic').
* build_cache(): one PIL decode of every pair into two raw uint8 arrays per split ({split}_rgb.npy (n,H,W,3), {split}_labels.npy (n,H,W)) and a small
  index.json, written last, so a cache with an index is complete.  Only this step needs PIL; the read path needs numpy and torch.
* CityscapesLoader: a background thread gathers the memmap rows of the next batches into pinned buffers; the host->device copy and the augmentation
  run on a side stream and hand over to the training step with an event.  The train order is a permutation drawn from (seed, epoch), partitioned
  across ranks like DistributedSampler(shuffle=True, drop_last=True).  The reference never calls DistributedSampler.set_epoch, so when distributed it
  repeats the epoch-0 order in every epoch; here every epoch has its own order, with one rank or many."""
import glob
import json
import math
import os
import queue
import threading

import numpy as np
import torch

from ...models.transforms import DeviceBatchPreparation, DeviceJointAugmentation
from ...models.transforms.augment import pack_table, philox, table_bytes

INDEX = 'index.json'
CACHE_VERSION = 1
_PHILOX_STREAM_ORDER = 2


def has_tree(root):
    return os.path.isdir(os.path.join(root, 'leftImg8bit')) and os.path.isdir(os.path.join(root, 'gtFine'))


def has_cache(cache_dir):
    return os.path.isfile(os.path.join(cache_dir, INDEX))


def pairs(root, split):
    """(image, labelIds) paths of a split in sorted order."""
    out = []
    for img in sorted(glob.glob(os.path.join(root, 'leftImg8bit', split, '*', '*_leftImg8bit.png'))):
        city = os.path.basename(os.path.dirname(img))
        stem = os.path.basename(img)[:-len('_leftImg8bit.png')]
        lab = os.path.join(root, 'gtFine', split, city, stem + '_gtFine_labelIds.png')
        if not os.path.isfile(lab):
            raise FileNotFoundError(f'{lab} (the label map of {img}) is missing')
        out.append((img, lab))
    return out


def build_cache(root, cache_dir, splits=('train', 'val')):
    """Decodes every pair of `splits` once into the raw uint8 cache under cache_dir.  Every image of a split must have one size."""
    from PIL import Image
    os.makedirs(cache_dir, exist_ok=True)
    index = {'version': CACHE_VERSION, 'splits': {}}
    for split in splits:
        pr = pairs(root, split)
        if not pr:
            continue
        with Image.open(pr[0][0]) as im:
            W, H = im.size
        rgb = np.lib.format.open_memmap(os.path.join(cache_dir, f'{split}_rgb.npy'), mode='w+', dtype=np.uint8, shape=(len(pr), H, W, 3))
        lab = np.lib.format.open_memmap(os.path.join(cache_dir, f'{split}_labels.npy'), mode='w+', dtype=np.uint8, shape=(len(pr), H, W))
        for i, (pi, pl) in enumerate(pr):
            with Image.open(pi) as im:
                a = np.asarray(im.convert('RGB'))
            with Image.open(pl) as im:
                b = np.asarray(im)
            if a.shape != (H, W, 3) or b.shape != (H, W):
                raise ValueError(f'{pi}: image {a.shape} / labels {b.shape}, expected ({H}, {W}) like the first image of the split')
            if b.dtype != np.uint8:
                if b.min() < 0 or b.max() > 255:
                    raise ValueError(f'{pl}: label ids outside [0, 255]')
                b = b.astype(np.uint8)
            rgb[i] = a
            lab[i] = b
        rgb.flush()
        lab.flush()
        del rgb, lab
        index['splits'][split] = {'count': len(pr), 'height': H, 'width': W,
                                  'images': [os.path.relpath(p, root) for p, _ in pr], 'labels': [os.path.relpath(p, root) for _, p in pr]}
    tmp = os.path.join(cache_dir, INDEX + '.tmp')
    with open(tmp, 'w') as f:
        json.dump(index, f)
    os.replace(tmp, os.path.join(cache_dir, INDEX))
    return index


class CityscapesCache:
    """Read side of the cache: memory-mapped uint8 arrays of one split."""

    def __init__(self, cache_dir, split):
        with open(os.path.join(cache_dir, INDEX)) as f:
            index = json.load(f)
        if index.get('version') != CACHE_VERSION:
            raise ValueError(f'{cache_dir}: cache version {index.get("version")} != {CACHE_VERSION}: rebuild it')
        if split not in index['splits']:
            raise KeyError(f'{cache_dir} holds no {split!r} split')
        s = index['splits'][split]
        self.count, self.height, self.width = s['count'], s['height'], s['width']
        self.images, self.label_files = s['images'], s['labels']
        self.rgb = np.load(os.path.join(cache_dir, f'{split}_rgb.npy'), mmap_mode='r')
        self.labels = np.load(os.path.join(cache_dir, f'{split}_labels.npy'), mmap_mode='r')
        if self.rgb.shape != (self.count, self.height, self.width, 3) or self.labels.shape != (self.count, self.height, self.width):
            raise ValueError(f'{cache_dir}: {split} arrays {self.rgb.shape} / {self.labels.shape} do not match the index')

    def __len__(self):
        return self.count


def rank_indices(n, epoch, seed, rank, world, shuffle=True, drop_last=True):
    """Sample indices of `rank` for `epoch`: torch DistributedSampler's partition (strided slices of one permutation, drop_last trims the tail to a
    multiple of world, otherwise the head is repeated to pad) of a permutation drawn from (seed, epoch)."""
    order = philox(seed, _PHILOX_STREAM_ORDER, epoch, 0).permutation(n) if shuffle else np.arange(n)
    if drop_last and n % world != 0:
        per = math.ceil((n - world) / world)
    else:
        per = math.ceil(n / world)
    total = per * world
    if total > n:
        order = np.concatenate([order, np.resize(order, total - n)])
    return order[:total][rank:total:world]


class _Slot:
    __slots__ = ('rgb', 'labels', 'table', 'copied')

    def __init__(self, bs, H, W, table_bytes):
        self.rgb = torch.empty((bs, H, W, 3), dtype=torch.uint8, pin_memory=True)
        self.labels = torch.empty((bs, H, W), dtype=torch.uint8, pin_memory=True)
        self.table = torch.empty((max(table_bytes, 1),), dtype=torch.uint8, pin_memory=True)
        self.copied = None            # event recorded behind the host->device copies that read this slot


class CityscapesLoader:
    """Device batches ((input_image, input_org), (target, _)) of one split from the cache.

    train: per-epoch permutation partitioned across ranks, drop_last, DeviceJointAugmentation (parameters drawn per (seed, epoch, sample index);
           with dataset['color_jitter'] its colour jitter as well);
    val:   file order, every sample (drop_last=False), DeviceBatchPreparation only."""

    def __init__(self, cache, batch_size, device, transform, rank=0, world=1, train=True, seed=0, prefetch=2):
        self.cache, self.bs, self.device, self.transform = cache, int(batch_size), torch.device(device), transform
        self.rank, self.world, self.train, self.seed = rank, world, train, seed
        self.augment = isinstance(transform, DeviceJointAugmentation)
        self.jitter = self.augment and transform.jitter          # the batch table then carries the colour-jitter rows as a third section
        self.prefetch = max(1, int(prefetch))
        self.epoch = 0
        self._slots = None
        self._stream = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self, epoch):
        n = len(self.cache)
        if self.train:
            return rank_indices(n, epoch, self.seed, self.rank, self.world, shuffle=True, drop_last=True)
        return np.arange(n)

    def _batches(self, epoch):
        idx = self.indices(epoch)
        nb = len(idx) // self.bs if self.train else math.ceil(len(idx) / self.bs)
        return [idx[k * self.bs:(k + 1) * self.bs] for k in range(nb)]

    def __len__(self):
        return len(self._batches(self.epoch))

    def _fill(self, slot, ids, epoch):
        c = self.cache
        rgb, lab = slot.rgb.numpy(), slot.labels.numpy()
        for j, i in enumerate(ids):
            rgb[j] = c.rgb[i]
            lab[j] = c.labels[i]
        if self.augment:
            rows = pack_table(self.transform.draw(epoch, ids, (c.height, c.width)), c.width, c.height, self.jitter)
            slot.table.numpy()[:rows.size] = rows

    def _worker(self, batches, epoch, free, ready, stop):
        try:
            for k, ids in enumerate(batches):
                while True:
                    if stop.is_set():
                        return
                    try:
                        slot = free.get(timeout=0.1)
                        break
                    except queue.Empty:
                        continue
                if slot.copied is not None:
                    slot.copied.synchronize()          # the previous host->device copy out of this slot has finished
                self._fill(slot, ids, epoch)
                ready.put((k, slot, ids))
        except BaseException as e:          # noqa: BLE001  (re-raised in the consumer)
            ready.put((None, e, None))

    def _launch(self, slot, ids):
        """Host->device copy + augmentation of one batch on the side stream; returns the batch and the event that completes it."""
        n, dev = len(ids), self.device
        with torch.cuda.stream(self._stream):
            rgb = slot.rgb[:n].to(dev, non_blocking=True)
            lab = slot.labels[:n].to(dev, non_blocking=True)
            table = slot.table[:table_bytes(n, self.cache.width, self.cache.height, self.jitter)].to(dev, non_blocking=True) if self.augment else None
            slot.copied = torch.cuda.Event()
            slot.copied.record(self._stream)
            if self.augment:
                (img, org), (tgt, aux) = self.transform(rgb, lab, params=table)
            else:
                (img, org), (tgt, aux) = self.transform(rgb, lab)
            done = torch.cuda.Event()
            done.record(self._stream)
        return ((img, org), (tgt, aux)), done

    def __iter__(self):
        epoch = self.epoch
        batches = self._batches(epoch)
        if self.train:
            self.epoch += 1                  # a loader iterated again without set_epoch moves on to the next order
        if not batches:
            return
        c = self.cache
        if self._slots is None:
            self._stream = torch.cuda.Stream(self.device)
            self._slots = [_Slot(self.bs, c.height, c.width, table_bytes(self.bs, c.width, c.height, self.jitter)) for _ in range(self.prefetch + 2)]
        free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()
        for s in self._slots:
            free.put(s)
        th = threading.Thread(target=self._worker, args=(batches, epoch, free, ready, stop), daemon=True)
        th.start()
        inflight = []

        def launch_next():
            k, slot, ids = ready.get()
            if k is None:
                raise slot
            out = self._launch(slot, ids)
            free.put(slot)
            inflight.append(out)

        try:
            with torch.cuda.device(self.device):
                for _ in range(min(self.prefetch, len(batches))):
                    launch_next()
                for k in range(len(batches)):
                    if k + self.prefetch < len(batches):
                        launch_next()              # the batch after next is prepared while this one trains
                    batch, done = inflight.pop(0)
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(done)
                    (img, org), (tgt, aux) = batch
                    for x in (img, org, tgt, aux):
                        if isinstance(x, torch.Tensor):
                            x.record_stream(cur)
                    yield batch
        finally:
            stop.set()
            th.join()


def cache_dir_of(dataset):
    return dataset.get('cache_path') or os.path.join(dataset['path'], 'dsrl_u8_cache')


def loader_factory(dataset, model_input_size, seed, distributed=False):
    """callable(split, batch_size, device, rank, world) over the Cityscapes cache of `dataset` (built from the tree under dataset['path'] first when
    it is missing: rank 0 decodes, the other ranks wait at a barrier)."""
    cache_dir = cache_dir_of(dataset)
    if not has_cache(cache_dir):
        if not has_tree(dataset['path']):
            raise FileNotFoundError(f"neither a Cityscapes tree (leftImg8bit/, gtFine/) under '{dataset['path']}' nor a cache in '{cache_dir}'")
        import torch.distributed as dist
        rank0 = not (distributed and dist.is_initialized()) or dist.get_rank() == 0
        if rank0:
            build_cache(dataset['path'], cache_dir)
        if distributed and dist.is_initialized():
            dist.barrier()
    ds = dataset['settings']

    def factory(split, batch_size, device, rank, world):
        cache = CityscapesCache(cache_dir, split)
        if split == 'train':
            tf = DeviceJointAugmentation(ds.LABEL_MAPPING_DICT, ds.MEAN, ds.STD, model_input_size, ds.IGNORE_CLASS_LABEL, seed=seed,
                                         color_jitter=dataset.get('color_jitter'))
            return CityscapesLoader(cache, batch_size, device, tf, rank, world, train=True, seed=seed)
        tf = DeviceBatchPreparation(ds.LABEL_MAPPING_DICT, ds.MEAN, ds.STD, model_input_size, ds.IGNORE_CLASS_LABEL)
        return CityscapesLoader(cache, batch_size, device, tf, 0, 1, train=False, seed=seed)
    return factory

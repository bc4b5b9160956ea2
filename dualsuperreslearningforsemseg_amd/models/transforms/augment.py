"""Random head of the reference's training transform (command_handlers/train_or_resume.py:128-137) on the device.

JointRandomRotate(15, fill=(0, 255)), JointRandomCrop(1.0, 3.5), JointHFlip, JointRandomGaussianBlur(3, p=0.5) and JointRandomGrayscale(0.1) run as two
HIP calls on decoded uint8 batches: dsrl_augment_geometry (rotate + crop-zoom, Pillow-exact) and dsrl_prepare_batch_augmented (flip, blur and
grayscale folded into the deterministic tail of DeviceBatchPreparation).  The random parameters are drawn on the host from (seed, epoch, sample id)
with numpy's Philox generator, so a sample's augmentation does not depend on batch size, rank count or loader threads.  Everything Pillow and
torchvision compute from a parameter before touching pixels (the rotation matrix, its fixed-point form, the crop box, the blur weights) is computed
here with their formulas and shipped in one 128-byte row per sample (include/dsrl_hip.h: dsrl_augment_params).

JointColorJitter (models/transforms/JointColorJitter.py; commented out in the reference's compose between JointImageAndLabelTensor and JointHFlip)
is opt-in: DeviceJointAugmentation(color_jitter=(0.4, 0.4, 0.4, 0.4)).  Its draws (a permutation of the four operations, then the four factors) come
from a Philox stream of their own, so the other parameters of a sample do not change when it is switched on; its 64-byte rows
(dsrl_colour_jitter_params) are a third section of the batch table, and the batch runs dsrl_colour_jitter_means + dsrl_prepare_batch_jittered
instead of dsrl_prepare_batch_augmented."""
import math
import numbers
from collections import namedtuple

import numpy as np
import torch

from ... import functional as HF
from ..._lib import call, query
from . import DeviceBatchPreparation

AUG_HFLIP, AUG_BLUR, AUG_GRAY = 1, 2, 4
# include/dsrl_hip.h: dsrl_augment_params
PARAMS_DTYPE = np.dtype([('rot', '<f8', 6), ('rot_fix', '<i4', 6), ('box', '<i4', 4), ('flags', '<i4'), ('blur', '<f4', 9)])
assert PARAMS_DTYPE.itemsize == 128

# include/dsrl_hip.h: dsrl_colour_jitter_params
JITTER_DTYPE = np.dtype([('order', '<i4', 4), ('brightness', '<f4'), ('contrast', '<f4'), ('saturation', '<f4'), ('hue', '<f4', 9)])
assert JITTER_DTYPE.itemsize == 64
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3

# order: a permutation of (0, 1, 2, 3) = (brightness, contrast, saturation, hue), the order of application; a factor of None: that operation is off
ColourJitterParams = namedtuple('ColourJitterParams', 'order brightness contrast saturation hue')
# angle (degrees), scale factor, crop box (x, y, w, h) in the rotated image, flip / blur / gray decisions, blur sigma, ColourJitterParams or None
AugmentParams = namedtuple('AugmentParams', 'angle scale box flip blur sigma gray jitter', defaults=(None,))

_PHILOX_STREAM_AUGMENT = 1
_PHILOX_STREAM_JITTER = 3         # 2 is the loader's sample order


def philox(seed, stream, epoch, index):
    """numpy Generator on Philox4x64 keyed by `seed`, counter (0, stream, epoch, index): independent streams per (stream, epoch, index)."""
    return np.random.Generator(np.random.Philox(key=int(seed) % (1 << 64), counter=[0, stream, int(epoch) % (1 << 64), int(index) % (1 << 64)]))


def rotate_matrix(angle, W, H):
    """PIL Image.rotate(angle, expand=False, center=None): the inverse affine matrix (output pixel centre -> source point)."""
    angle = angle % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix_fixed(m):
    """Pillow's 16.16 fixed-point form of the matrix for the nearest path (Geometry.c affine_fixed): a0, a1, a2, a3, a4, a5."""
    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def gaussian_weights(sigma, kernel_size=3):
    """torchvision 0.8.1 GaussianBlur kernel (functional_tensor._get_gaussian_kernel2d) in fp32: 9 weights, row-major."""
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = pdf / pdf.sum()
    return torch.mm(k1[:, None], k1[None, :]).reshape(-1).numpy()


def crop_box(scale, u, v, W, H):
    """JointRandomCrop's PIL branch (JointRandomCrop.py:26-33) for scale factor `scale` and the two offset draws u, v in [0, 1).  The offsets span only
    [0, (W - cw) // 2) x [0, (H - ch) // 2): the reference draws them from half the admissible range, so a crop never touches the right / bottom
    quarter of the slack.  That quirk is reproduced."""
    if not scale > 1.0:
        return (0, 0, W, H)
    cw, ch = int(1.0 / scale * W), int(1.0 / scale * H)
    x = int(u * ((W - cw) // 2))
    y = int(v * ((H - ch) // 2))
    return (x, y, cw, ch)


def jitter_range(value, name, center=1.0, bound=(0.0, float('inf')), clip_first_on_zero=True):
    """The factor range of one JointColorJitter argument (its _check_input): a number v gives [center - v, center + v] (the lower end not below 0
    for brightness, contrast and saturation), a (min, max) pair is taken as given within `bound`; None when the range is the neutral value alone.
    Stricter than the reference in two places: a single number is held to `bound` as well (the reference lets hue=0.7 through although it documents
    0 <= hue <= 0.5), and a bool is not a number."""
    if isinstance(value, numbers.Number):
        if isinstance(value, bool):
            raise TypeError(f'{name} should be a number, not a bool')
        if value < 0:
            raise ValueError(f'If {name} is a single number, it must be non negative.')
        if center + float(value) > bound[1]:       # the reference checks only pairs against the bound: hue=0.7 would pass there as (-0.7, 0.7)
            raise ValueError(f'{name} values should be between {bound}')
        lo, hi = center - float(value), center + float(value)
        if clip_first_on_zero:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = value
        if not bound[0] <= lo <= hi <= bound[1]:
            raise ValueError(f'{name} values should be between {bound}')
    else:
        raise TypeError(f'{name} should be a single number or a list/tuple with length 2.')
    return None if lo == hi == center else (float(lo), float(hi))


def jitter_ranges(color_jitter):
    """(brightness, contrast, saturation, hue) ranges of a `color_jitter` argument - None, a mapping with those keys (a missing key is 0) or a
    4-tuple, each value in JointColorJitter's forms - or None when nothing is left enabled."""
    if color_jitter is None:
        return None
    names = ('brightness', 'contrast', 'saturation', 'hue')
    if hasattr(color_jitter, 'keys'):
        unknown = set(color_jitter.keys()) - set(names)
        if unknown:
            raise TypeError(f'color_jitter: unknown keys {sorted(unknown)}')
        values = [color_jitter.get(k, 0) for k in names]
    elif isinstance(color_jitter, (tuple, list)) and len(color_jitter) == 4:
        values = list(color_jitter)
    else:
        raise TypeError('color_jitter should be None, a mapping or a 4-tuple of brightness, contrast, saturation, hue')
    ranges = tuple(jitter_range(v, k) for v, k in zip(values[:3], names[:3])) + (jitter_range(values[3], 'hue', 0.0, (-0.5, 0.5), False),)
    return None if all(r is None for r in ranges) else ranges


def hue_matrix(hue_factor):
    """The reference's hue rotation (JointColorJitter.py:88-96) for hue_factor * 2 pi, computed in float64: (3, 3) float32, out = x_row @ M."""
    a = float(hue_factor) * 2.0 * np.pi
    cos, sin = np.cos(a), np.sin(a)
    d, p, m = cos + (1.0 - cos) / 3.0, (1.0 - cos) / 3.0 + np.sqrt(1.0 / 3.0) * sin, (1.0 - cos) / 3.0 - np.sqrt(1.0 / 3.0) * sin
    return np.array([[d, m, p], [p, d, m], [m, p, d]], dtype=np.float64).astype(np.float32)


def pack_jitter(params):
    """Rows of dsrl_colour_jitter_params for a batch of AugmentParams: a sample without jitter, or a disabled operation, gets -1 in its slot."""
    rows = np.zeros(len(params), dtype=JITTER_DTYPE)
    rows['order'] = -1
    rows['brightness'] = rows['contrast'] = rows['saturation'] = 1.0
    rows['hue'] = np.eye(3, dtype=np.float32).ravel()
    for i, p in enumerate(params):
        j = p.jitter
        if j is None:
            continue
        if sorted(int(k) for k in j.order) != [0, 1, 2, 3]:
            raise ValueError(f'jitter order {tuple(j.order)} is not a permutation of (0, 1, 2, 3)')
        factors = (j.brightness, j.contrast, j.saturation, j.hue)
        rows[i]['order'] = [int(k) if factors[int(k)] is not None else -1 for k in j.order]
        for name, f in zip(('brightness', 'contrast', 'saturation'), factors):
            if f is not None:
                rows[i][name] = f
        if j.hue is not None:
            rows[i]['hue'] = hue_matrix(j.hue).ravel()
    return rows


def pack(params, W, H):
    """Rows of dsrl_augment_params for a batch of AugmentParams."""
    rows = np.zeros(len(params), dtype=PARAMS_DTYPE)
    for i, p in enumerate(params):
        m = rotate_matrix(p.angle, W, H)
        rows[i]['rot'] = m
        rows[i]['rot_fix'] = rotate_matrix_fixed(m)
        rows[i]['box'] = p.box if p.box is not None else (0, 0, W, H)
        rows[i]['flags'] = (AUG_HFLIP if p.flip else 0) | (AUG_BLUR if p.blur else 0) | (AUG_GRAY if p.gray else 0)
        if p.blur:
            rows[i]['blur'] = gaussian_weights(p.sigma)
    return rows


def label_source_index(box, W, H):
    """Source column of every output column, then source row of every output row, of Image.resize((W, H), NEAREST, box) (Geometry.c
    ImagingScaleAffine): xo_0 = x + 0.5 * w / W, xo_{i+1} = xo_i + w / W as sequential double sums (np.add.accumulate is sequential), int()."""
    x, y, w, h = box if box is not None else (0, 0, W, H)
    out = []
    for b0, n_box, n_out in ((x, w, W), (y, h, H)):
        a = n_box / n_out
        steps = np.full(n_out, a, dtype=np.float64)
        steps[0] = b0 + a * 0.5
        v = np.add.accumulate(steps)
        out.append(np.where(v < 0, -1, v.astype(np.int64)))
    return np.concatenate(out).astype(np.int32)


def table_bytes(N, W, H, jitter=False):
    """Size of the device table of N samples: N dsrl_augment_params rows, then N x (W + H) int32 label source indices; with `jitter`, then N
    dsrl_colour_jitter_params rows."""
    return N * (PARAMS_DTYPE.itemsize + 4 * (W + H) + (JITTER_DTYPE.itemsize if jitter else 0))


def jitter_offset(N, W, H):
    """Byte offset of the jitter rows in a table that has them."""
    return table_bytes(N, W, H)


def pack_table(params, W, H, jitter=False):
    """The device table of a batch as uint8: pack() rows followed by label_source_index() of every sample; with `jitter`, then pack_jitter() rows."""
    rows = pack(params, W, H)
    idx = np.stack([label_source_index(p.box, W, H) for p in params])
    parts = [rows.view(np.uint8).ravel(), idx.view(np.uint8).ravel()]
    if jitter:
        parts.append(pack_jitter(params).view(np.uint8).ravel())
    return np.concatenate(parts)


def identity_params():
    return AugmentParams(0.0, 1.0, None, False, False, 1.0, False)


class DeviceJointAugmentation:
    """The reference's random training augmentations + DeviceBatchPreparation's deterministic tail, on the device.

    Defaults are the reference's (train_or_resume.py:128-137).  draw(epoch, sample_ids) is a pure function of (seed, epoch, sample id);
    __call__(rgb_u8, labels_u8, params) returns ((input_image, input_org), (target, None)) like DeviceBatchPreparation (the reference's loop discards
    the second target element, train_or_resume.py:404)."""

    def __init__(self, label_mapping_dict, mean, std, model_input_size, ignore_label=255, seed=0, degrees=15.0, min_scale=1.0, max_scale=3.5,
                 flip_p=0.5, blur_p=0.5, blur_sigma=(0.1, 2.0), gray_p=0.1, color_jitter=None):
        self.prep = DeviceBatchPreparation(label_mapping_dict, mean, std, model_input_size, ignore_label)
        self.seed = seed
        self.degrees, self.min_scale, self.max_scale = float(degrees), float(min_scale), float(max_scale)
        self.flip_p, self.blur_p, self.blur_sigma, self.gray_p = flip_p, blur_p, tuple(blur_sigma), gray_p
        # JointColorJitter's (brightness, contrast, saturation, hue) ranges, None: no jitter stage (also when every range is neutral)
        self.color_jitter = jitter_ranges(color_jitter)
        self._jitter_buffers = {}     # (device, stream, N, Hs, Ws) -> (workspace, means), allocated once and reused on that stream
        self._calls = 0

    @property
    def jitter(self):
        """Whether batches carry jitter rows and run the jittered kernels."""
        return self.color_jitter is not None

    def draw_jitter(self, epoch, sample_id):
        """ColourJitterParams of one sample from its own Philox stream: a permutation of the four operations, then one uniform per factor (drawn
        for a disabled operation too, so a factor does not depend on which others are enabled), each rounded through fp32."""
        g = philox(self.seed, _PHILOX_STREAM_JITTER, epoch, sample_id)
        order = tuple(int(k) for k in g.permutation(4))
        u = g.random(4)
        factors = [None if r is None else float(np.float32(r[0] + u[i] * (r[1] - r[0]))) for i, r in enumerate(self.color_jitter)]
        return ColourJitterParams(order, *factors)

    def draw_one(self, epoch, sample_id, W, H):
        g = philox(self.seed, _PHILOX_STREAM_AUGMENT, epoch, sample_id)
        u = g.random(8)
        f32 = lambda v: float(np.float32(v))      # the reference draws each of these with torch's fp32 uniform_
        angle = f32(-self.degrees + u[0] * 2 * self.degrees)
        scale = f32(self.min_scale + u[1] * (self.max_scale - self.min_scale))
        box = crop_box(scale, u[2], u[3], W, H)
        sigma = f32(self.blur_sigma[0] + u[6] * (self.blur_sigma[1] - self.blur_sigma[0]))
        jitter = self.draw_jitter(epoch, sample_id) if self.jitter else None
        return AugmentParams(angle, scale, box, bool(u[4] < self.flip_p), bool(u[5] < self.blur_p), sigma, bool(u[7] < self.gray_p), jitter)

    def draw(self, epoch, sample_ids, size=(1024, 2048)):
        """Per-sample parameters for images of `size` (H, W)."""
        H, W = size
        return [self.draw_one(epoch, int(i), W, H) for i in sample_ids]

    def table(self, params, W, H, device):
        """Device table (uint8) of a batch: pack_table(), with the jitter rows when the transform jitters."""
        if not self.jitter and any(p.jitter is not None for p in params):
            raise ValueError('parameters carry a colour jitter but the transform was built without color_jitter')
        host = torch.from_numpy(pack_table(params, W, H, self.jitter)).pin_memory()
        return host.to(device, non_blocking=True)

    def geometry(self, rgb_u8, labels_u8, table):
        """Rotate + crop-zoom only: uint8 (N,Hs,Ws,3) and raw label ids (N,Hs,Ws) out."""
        HF._need_gpu(rgb_u8, labels_u8)
        N, Hs, Ws, _ = rgb_u8.shape
        rgb_out = torch.empty_like(rgb_u8)
        lab_out = torch.empty_like(labels_u8) if labels_u8 is not None else None
        src = None if labels_u8 is None else table.data_ptr() + N * PARAMS_DTYPE.itemsize
        call('dsrl_augment_geometry', rgb_u8.contiguous().data_ptr(), None if labels_u8 is None else labels_u8.contiguous().data_ptr(), table.data_ptr(),
             src, rgb_out.data_ptr(), None if lab_out is None else lab_out.data_ptr(), N, Hs, Ws, HF._stream())
        return rgb_out, lab_out

    def prepare(self, rgb_u8, labels_u8, table):
        """Flip / blur / grayscale + ToTensor, Normalize, label remap and the dual-scale resize (the rows' flags select); with jitter rows in the
        table, the colour jitter in front of them."""
        return self._prepare(rgb_u8, labels_u8, table, None)

    def _prepare(self, rgb_u8, labels_u8, table, means):
        """prepare(); `means`: jitter_means() of this very batch when it has been run already (tools/augment_bench.py times the two calls apart)."""
        prep = self.prep
        HF._need_gpu(rgb_u8, labels_u8)
        N, Hs, Ws, _ = rgb_u8.shape
        H, W = prep.size
        dev = rgb_u8.device
        lut = prep._lut.get(dev)
        if lut is None:
            lut = prep._lut[dev] = prep.lut_host.to(dev)
        img_in = torch.empty((N, H, W, 4), device=dev, dtype=torch.float32)
        img_org = torch.empty((N, 2 * H, 2 * W, 3), device=dev, dtype=torch.float32)
        target = torch.empty((N, 2 * H, 2 * W), device=dev, dtype=torch.uint8) if labels_u8 is not None else None
        rgb_u8 = rgb_u8.contiguous()
        args = (rgb_u8.data_ptr(), None if labels_u8 is None else labels_u8.contiguous().data_ptr(), lut.data_ptr(), prep.mean, prep.std, img_in.data_ptr(),
                img_org.data_ptr(), None if target is None else target.data_ptr(), N, Hs, Ws, H, W, table.data_ptr())
        if self.jitter:
            rows = table.data_ptr() + jitter_offset(N, Ws, Hs)
            if means is None:
                means = self.jitter_means(rgb_u8, rows)
            call('dsrl_prepare_batch_jittered', *args, rows, means.data_ptr(), HF._stream())
        else:
            call('dsrl_prepare_batch_augmented', *args, HF._stream())
        return (img_in.permute(0, 3, 1, 2)[:, :3], img_org.permute(0, 3, 1, 2)), (target, None)

    def jitter_means(self, rgb_u8, rows):
        """Contrast's per-sample mean (dsrl_colour_jitter_means) of a contiguous batch for the jitter rows at device address `rows`: float (N,), a
        buffer owned by the transform that the next call on the same stream with the same shape overwrites."""
        N, Hs, Ws, _ = rgb_u8.shape
        stream = HF._stream()
        key = (rgb_u8.device, stream, N, Hs, Ws)
        buf = self._jitter_buffers.get(key)
        if buf is None:
            nbytes = query('dsrl_colour_jitter_workspace_bytes', N, Hs, Ws)
            buf = self._jitter_buffers[key] = (torch.empty((nbytes // 8,), device=rgb_u8.device, dtype=torch.float64),
                                               torch.zeros((N,), device=rgb_u8.device, dtype=torch.float32))
        ws, means = buf
        call('dsrl_colour_jitter_means', rgb_u8.data_ptr(), rows, means.data_ptr(), ws.data_ptr(), ws.numel() * 8, N, Hs, Ws, stream)
        return means

    def __call__(self, rgb_u8, labels_u8, params=None):
        """rgb_u8 (N,Hs,Ws,3) uint8 and labels_u8 (N,Hs,Ws) raw label ids on the device.  `params`: a list of AugmentParams, a device table from
        table(), or None (draws for sample ids 0..N-1 of an internal call counter used as the epoch)."""
        N, Hs, Ws, _ = rgb_u8.shape
        if params is None:
            params = self.draw(self._calls, range(N), (Hs, Ws))
            self._calls += 1
        table = params if isinstance(params, torch.Tensor) else self.table(params, Ws, Hs, rgb_u8.device)
        if table.numel() != table_bytes(N, Ws, Hs, self.jitter) or table.device != rgb_u8.device or table.dtype != torch.uint8:
            raise ValueError(f'parameter table of {table.numel()} bytes on {table.device} for {N} samples on {rgb_u8.device}')
        rgb2, lab2 = self.geometry(rgb_u8, labels_u8, table)
        return self.prepare(rgb2, lab2, table)


__all__ = ['DeviceJointAugmentation', 'AugmentParams', 'ColourJitterParams', 'PARAMS_DTYPE', 'JITTER_DTYPE', 'pack', 'pack_jitter', 'pack_table', 'jitter_range',
           'jitter_ranges', 'hue_matrix', 'jitter_offset', 'table_bytes', 'label_source_index', 'rotate_matrix', 'rotate_matrix_fixed', 'gaussian_weights',
           'crop_box', 'philox', 'identity_params', 'AUG_HFLIP', 'AUG_BLUR', 'AUG_GRAY']

"""Writes tests/golden/augment.npz: the reference's random training augmentations (command_handlers/train_or_resume.py:128-137) for one batch of
five 48x96 samples with fixed, mixed parameters, computed by Pillow (rotate + crop-zoom) and torch on the CPU (flip, blur, grayscale, normalise,
dual-scale resize).  Run from the repository root: python tests/golden/make_augment_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import augment_ref as R  # noqa: E402
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs  # noqa: E402
from dualsuperreslearningforsemseg_amd.models.transforms import augment as A  # noqa: E402

H, W = 48, 96
MODEL_INPUT = (16, 32)
# angle, scale, offset draws (u, v), flip, blur, sigma, gray: angles 0 and +-15, scale 1 and near 3.5, each float flag on its own
CASES = [
    (0.0, 1.0, 0.0, 0.0, True, False, 1.0, False),
    (15.0, 3.45, 0.9, 0.6, False, True, 1.3, False),
    (-15.0, 1.0, 0.0, 0.0, False, False, 1.0, True),
    (8.5, 2.0, 0.5, 0.99, False, False, 1.0, False),
    (-3.7, 3.4, 0.2, 0.4, True, True, 0.35, True),
]


def params():
    return [A.AugmentParams(a, s, A.crop_box(s, u, v, W, H), f, b, sg, g) for a, s, u, v, f, b, sg, g in CASES]


def make():
    rng = np.random.default_rng(2024)
    n = len(CASES)
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    ids = np.array(sorted(k for k in cs.LABEL_MAPPING_DICT if 0 <= k < 256), dtype=np.uint8)
    labels = ids[rng.integers(0, len(ids), (n, H, W))]
    lut = R.lut_of(cs.LABEL_MAPPING_DICT)
    ps = params()
    geo_rgb, geo_lab, img_in, img_org, target = [], [], [], [], []
    for i, p in enumerate(ps):
        g, gl = R.geometry_pillow(rgb[i], labels[i], p)
        a, b, c = R.tail_torch(g, gl, p, lut, cs.MEAN, cs.STD, MODEL_INPUT)
        geo_rgb.append(g); geo_lab.append(gl); img_in.append(a); img_org.append(b); target.append(c)
    return {'rgb': rgb, 'labels': labels, 'angle': np.array([p.angle for p in ps]), 'scale': np.array([p.scale for p in ps]),
            'box': np.array([p.box for p in ps], dtype=np.int32), 'flip': np.array([p.flip for p in ps]), 'blur': np.array([p.blur for p in ps]),
            'sigma': np.array([p.sigma for p in ps]), 'gray': np.array([p.gray for p in ps]),
            'geo_rgb': np.stack(geo_rgb), 'geo_labels': np.stack(geo_lab),
            'img_in': np.stack(img_in), 'img_org': np.stack(img_org), 'target': np.stack(target)}


def params_of(g):
    """The AugmentParams stored in a fixture."""
    return [A.AugmentParams(float(a), float(s), tuple(int(v) for v in b), bool(f), bool(bl), float(sg), bool(gr))
            for a, s, b, f, bl, sg, gr in zip(g['angle'], g['scale'], g['box'], g['flip'], g['blur'], g['sigma'], g['gray'])]


if __name__ == '__main__':
    out = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(out, **make())
    print(out, os.path.getsize(out), 'bytes')

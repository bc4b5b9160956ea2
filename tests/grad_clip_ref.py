"""Plain numpy float64 reference of gradient-norm clipping (csrc/gradclip.hip, ddp.FlatParams.enable_grad_clip): the sums of squares of the
1024-float tiles of an arena, S, the norm and the clip coefficient by torch.nn.utils.clip_grad_norm_'s formula, the grad_scale the optimiser reads,
and the running fields of the device record."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TILE = 1024


def tile_sums(g):
    """sum of squares of every 1024-float tile of the float32 arena `g` (the last one may be short), float64; math.fsum: correctly rounded"""
    g = np.asarray(g, F32).astype(F64)
    sq = g * g                                    # exact: 24 x 24 bits
    return np.array([math.fsum(sq[i:i + TILE]) for i in range(0, len(g), TILE)], F64)


def total(tiles):
    return F64(math.fsum(np.asarray(tiles, F64))) if np.isfinite(tiles).all() else F64(np.sum(np.asarray(tiles, F64)))


def norm_coef(S, gs, max_norm):
    """norm = gs sqrt(S), coef = min(1, max_norm / (norm + 1e-6)) as torch's clamp(max=1) forms it: a NaN stays a NaN"""
    with np.errstate(invalid='ignore', over='ignore'):
        norm = F64(F32(gs)) * np.sqrt(F64(S))
        coef = F64(F32(max_norm)) / (norm + F64(1e-6))
    if coef > 1.0:
        coef = F64(1.0)
    return norm, coef


def grad_scale(gs, coef):
    """what the finish leaves in hyper_out[3]: gs itself at coef == 1, else the float64 product rounded once"""
    return F32(gs) if coef == 1.0 else F32(F64(F32(gs)) * coef)


def new_record(max_norm):
    return {'sumsq': 0.0, 'norm_sum': 0.0, 'norm': 0.0, 'coef': 0.0, 'max_norm': float(F32(max_norm)), 'norm_max': 0.0, 'steps': 0, 'clipped': 0,
            'nonfinite': 0}


def record_step(rec, S, gs):
    """the record after one more finish on the sum of squares S; -> (record, grad_scale the optimiser reads)"""
    norm, coef = norm_coef(S, gs, rec['max_norm'])
    out = dict(rec)
    with np.errstate(over='ignore'):
        out.update(sumsq=float(S), norm=float(F32(norm)), coef=float(F32(coef)), steps=rec['steps'] + 1)
        if np.isfinite(norm):
            out['norm_sum'] = rec['norm_sum'] + float(norm)
            out['norm_max'] = max(rec['norm_max'], float(F32(norm)))
            out['clipped'] = rec['clipped'] + int(coef < 1.0)
        else:
            out['nonfinite'] = rec['nonfinite'] + 1
    return out, grad_scale(gs, coef)

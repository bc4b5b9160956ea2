"""CPU checks of the colour jitter's host side: JointColorJitter's range handling, the hue matrix, the draws (their own Philox stream: the other
parameters of a sample do not move), the 64-byte rows, and the batch table with and without jitter rows."""
import math

import numpy as np
import pytest

from dualsuperreslearningforsemseg_amd.models.transforms import augment as A
from dualsuperreslearningforsemseg_amd.models.transforms import DeviceJointAugmentation
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs

REFERENCE_VALUES = (0.4, 0.4, 0.4, 0.4)          # the reference's commented-out compose entry


def _aug(color_jitter=None, seed=54321, **kw):
    return DeviceJointAugmentation(cs.LABEL_MAPPING_DICT, cs.MEAN, cs.STD, (256, 512), seed=seed, color_jitter=color_jitter, **kw)


def test_ranges_follow_the_reference_constructor():
    assert A.jitter_range(0.4, 'brightness') == (0.6, 1.4)
    assert A.jitter_range(1.5, 'contrast') == (0.0, 2.5)                       # the lower end is clipped at 0
    assert A.jitter_range((0.2, 3.0), 'saturation') == (0.2, 3.0)
    assert A.jitter_range([0.5, 0.5], 'saturation') == (0.5, 0.5)              # a collapsed range off the neutral value stays enabled
    assert A.jitter_range(0.4, 'hue', 0.0, (-0.5, 0.5), False) == (-0.4, 0.4)  # hue is not clipped at 0
    assert A.jitter_range((-0.5, 0.25), 'hue', 0.0, (-0.5, 0.5), False) == (-0.5, 0.25)
    # a range that collapses onto the neutral value disables the operation
    assert A.jitter_range(0, 'brightness') is None and A.jitter_range((1.0, 1.0), 'contrast') is None
    assert A.jitter_range(0.0, 'hue', 0.0, (-0.5, 0.5), False) is None and A.jitter_range((0, 0), 'hue', 0.0, (-0.5, 0.5), False) is None
    assert A.jitter_ranges(REFERENCE_VALUES) == ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.4, 0.4))
    assert A.jitter_ranges({'contrast': 0.2, 'hue': (0.0, 0.1)}) == (None, (0.8, 1.2), None, (0.0, 0.1))
    assert A.jitter_ranges(None) is None and A.jitter_ranges((0, 0, 0, 0)) is None and A.jitter_ranges({'brightness': (1, 1)}) is None


@pytest.mark.parametrize('value,kind', [
    (-0.1, ValueError), ((1.2, 0.8), ValueError), ((-0.1, 1.0), ValueError), ('0.4', TypeError), ((0.1, 0.2, 0.3), TypeError), (None, TypeError)])
def test_bad_ranges_raise_like_the_reference(value, kind):
    with pytest.raises(kind):
        A.jitter_range(value, 'brightness')


def test_bad_hue_and_bad_arguments_raise():
    for bad in ((-0.6, 0.0), (0.0, 0.6), (0.3, 0.1)):
        with pytest.raises(ValueError):
            A.jitter_range(bad, 'hue', 0.0, (-0.5, 0.5), False)
    with pytest.raises(ValueError):
        _aug((0.4, 0.4, 0.4, -0.1))
    with pytest.raises(ValueError):
        _aug((0.4, 0.4, 0.4, (0.0, 0.7)))
    for bad in ((0.4, 0.4, 0.4), 0.4, {'brightnes': 0.4}):
        with pytest.raises(TypeError):
            _aug(bad)
    # a disabled operation is None in the transform and draws None
    aug = _aug({'brightness': 0.4, 'hue': 0.1})
    assert aug.jitter and aug.color_jitter == ((0.6, 1.4), None, None, (-0.1, 0.1))
    j = aug.draw(0, [0])[0].jitter
    assert j.contrast is None and j.saturation is None and j.brightness is not None and j.hue is not None
    assert not _aug().jitter and not _aug((0, 0, 0, 0)).jitter and _aug().draw(0, [0])[0].jitter is None


def test_single_numbers_are_held_to_the_bound_and_bools_are_refused():
    """Stricter than the reference's _check_input, which bound-checks only pairs: hue=0.7 is outside the documented 0 <= hue <= 0.5."""
    with pytest.raises(ValueError):
        A.jitter_range(0.7, 'hue', 0.0, (-0.5, 0.5), False)
    with pytest.raises(ValueError):
        _aug((0.4, 0.4, 0.4, 0.51))
    assert A.jitter_range(0.5, 'hue', 0.0, (-0.5, 0.5), False) == (-0.5, 0.5)
    assert A.jitter_range(7.0, 'brightness') == (0.0, 8.0)                      # no upper bound for the other three
    for bad in (True, False):
        with pytest.raises(TypeError):
            A.jitter_range(bad, 'brightness')


def _reference_hue_matrix(h):
    """JointColorJitter.py:88-96 written out: rotation by h * 2 pi about the grey axis."""
    a = h * 2.0 * math.pi
    c, s, r = math.cos(a), math.sin(a), math.sqrt(1.0 / 3.0)
    t = (1.0 - c) / 3.0
    return np.array([[c + t, t - r * s, t + r * s], [t + r * s, c + t, t - r * s], [t - r * s, t + r * s, c + t]])


@pytest.mark.parametrize('h', [0.0, 0.25, -0.25, 0.5, -0.5])
def test_hue_matrix_is_the_reference_formula(h):
    M = A.hue_matrix(h)
    assert M.dtype == np.float32 and M.shape == (3, 3)
    assert np.array_equal(M, _reference_hue_matrix(h).astype(np.float32))
    assert np.allclose(M.sum(0), 1, atol=1e-6) and np.allclose(M.sum(1), 1, atol=1e-6)        # grey stays grey
    if h == 0.0:
        assert np.array_equal(M, np.eye(3, dtype=np.float32))
    if abs(h) == 0.5:
        assert np.allclose(M, (2.0 / 3.0) - np.eye(3), atol=1e-6)                                # half a turn: the same matrix either way


def test_draw_is_a_pure_function_of_seed_epoch_and_sample():
    aug = _aug(REFERENCE_VALUES)
    a = aug.draw(3, [5, 9, 11])
    assert a == aug.draw(3, [5, 9, 11]) == _aug(REFERENCE_VALUES).draw(3, [5, 9, 11])
    assert a[1:] == aug.draw(3, [9, 11]) and a[0] == aug.draw(3, [5])[0]                          # independent of the batch
    assert all(x.jitter != y.jitter for x, y in zip(a, aug.draw(4, [5, 9, 11])))                   # epoch
    assert a[0].jitter != a[1].jitter                                                              # sample id
    assert _aug(REFERENCE_VALUES, seed=1).draw(3, [5])[0].jitter != a[0].jitter                    # seed


def test_jitter_leaves_the_other_seven_fields_alone():
    plain, jit = _aug(), _aug(REFERENCE_VALUES)
    for epoch, size in ((0, (1024, 2048)), (7, (48, 96))):
        a, b = plain.draw(epoch, range(200), size), jit.draw(epoch, range(200), size)
        assert [p[:7] for p in a] == [p[:7] for p in b]
        assert all(p.jitter is None for p in a) and all(p.jitter is not None for p in b)


def test_factors_stay_in_range_and_every_order_occurs():
    ranges = {'brightness': (0.5, 1.1), 'contrast': 0.4, 'saturation': (0.0, 3.0), 'hue': (-0.5, 0.2)}
    aug = _aug(ranges)
    js = [p.jitter for p in aug.draw(2, range(2000), (48, 96))]
    for name, (lo, hi) in zip(('brightness', 'contrast', 'saturation', 'hue'), aug.color_jitter):
        v = np.array([getattr(j, name) for j in js])
        assert v.min() >= np.float32(lo) and v.max() <= np.float32(hi), name
        assert v.min() < lo + 0.02 * (hi - lo) and v.max() > hi - 0.02 * (hi - lo), name          # and span it
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), name                   # rounded through float32
    orders = {j.order for j in js}
    assert len(orders) == 24 and all(sorted(o) == [0, 1, 2, 3] for o in orders)


def test_rows_are_64_bytes_at_the_documented_offsets():
    dt = A.JITTER_DTYPE
    assert dt.itemsize == 64
    assert {k: dt.fields[k][1] for k in dt.names} == {'order': 0, 'brightness': 16, 'contrast': 20, 'saturation': 24, 'hue': 28}
    j = A.ColourJitterParams((3, 0, 2, 1), 1.25, None, 0.5, -0.25)
    ps = [A.identity_params()._replace(jitter=j), A.identity_params()]
    rows = A.pack_jitter(ps)
    raw = rows.view(np.uint8).reshape(2, 64)
    assert list(raw[0, :16].view('<i4')) == [3, 0, 2, -1]                                        # the disabled contrast's slot
    assert list(raw[0, 16:28].view('<f4')) == [1.25, 1.0, 0.5]
    assert np.array_equal(raw[0, 28:].view('<f4').reshape(3, 3), A.hue_matrix(-0.25))
    assert list(raw[1, :16].view('<i4')) == [-1] * 4                                             # a sample without jitter: every slot off
    with pytest.raises(ValueError):
        A.pack_jitter([A.identity_params()._replace(jitter=j._replace(order=(0, 1, 2, 2)))])


def test_tables_without_jitter_are_what_they_were():
    W, H = 96, 48
    aug = _aug()
    ps = aug.draw(1, range(3), (H, W))
    t = A.pack_table(ps, W, H)
    assert A.table_bytes(3, W, H) == 3 * (128 + 4 * (W + H)) == t.size
    rows = A.pack(ps, W, H)
    idx = np.stack([A.label_source_index(p.box, W, H) for p in ps])
    assert np.array_equal(t, np.concatenate([rows.view(np.uint8).ravel(), idx.view(np.uint8).ravel()]))
    # seven positional fields and _replace still build a parameter set
    p = A.AugmentParams(0.0, 1.0, None, False, False, 1.0, False)
    assert p == A.identity_params() and p.jitter is None and p._replace(flip=True).flip
    # with jitter: the same bytes, then the 64-byte rows
    jit = _aug(REFERENCE_VALUES)
    pj = jit.draw(1, range(3), (H, W))
    tj = A.pack_table(pj, W, H, jitter=True)
    assert A.table_bytes(3, W, H, jitter=True) == t.size + 3 * 64 == tj.size and A.jitter_offset(3, W, H) == t.size
    assert np.array_equal(tj[:t.size], t) and np.array_equal(tj[t.size:], A.pack_jitter(pj).view(np.uint8).ravel())
    assert np.array_equal(A.pack_table(pj, W, H), t)                                             # rows are added only on request

"""The premises of tests/test_amax_records_gpu.py, proved on the CPU from the fp64 oracle: the record helpers do what they say, and in every parametrised
case the planted element is the reference's unique maximum by at least 4x when it is kept - and is not the maximum when the Dropout drops it."""
import numpy as np
import pytest

import amax_ref as A


def test_record_helpers():
    rec = np.zeros(A.AMAX_WORDS, np.uint32)
    assert A.record_max(rec) == 0 and A.record_spare_words_zero(rec)
    rec[3 * 16] = 0x42000000
    rec[15 * 16] = 0x41000000
    assert A.record_max(rec) == 0x42000000 and A.record_spare_words_zero(rec)
    for w in (1, 15, 17, 255):
        bad = rec.copy()
        bad[w] = 1
        assert not A.record_spare_words_zero(bad), w
        assert A.record_max(bad) == 0x42000000          # a ticket word is no shard
    with pytest.raises(AssertionError):
        A.record_max(rec.view(np.int32))


def test_abs_bits_max_orders_like_the_kernels():
    f = lambda *v: np.array(v, np.float32)          # noqa: E731
    assert A.abs_bits_max(f(1.0, -3.0, 2.0)) == np.float32(3.0).view(np.uint32)
    assert A.abs_bits_max(f(-0.0, 0.0)) == 0
    assert A.abs_bits_max(f(1e-40, -2e-40)) == np.float32(2e-40).view(np.uint32) and A.abs_bits_max(f(2e-40)) < 0x00800000       # subnormal
    assert A.abs_bits_max(f(3e38, np.inf)) == A.INF_BITS and A.abs_bits_max(f(-np.inf)) == A.INF_BITS
    assert A.abs_bits_max(f(np.inf, np.nan)) > A.INF_BITS and A.abs_bits_max(f(-np.nan, 1.0)) > A.INF_BITS
    assert A.abs_bits_max(np.zeros((0, 4), np.float32)) == 0
    with pytest.raises(AssertionError):
        A.abs_bits_max(np.zeros(4))


SHAPES = sorted({(c.P, c.C) for c in A.FWD_CASES + A.BWD_CASES} | {(1, 1), (1, 3), (7, 19), (300, 256)})


@pytest.mark.parametrize('P,C', SHAPES)
def test_plants_are_distinct_and_inside(P, C):
    pl = A.PLANTS(P, C)
    assert len(set(pl)) == len(pl) and all(0 <= p < P and 0 <= c < C for p, c in pl)
    assert (0, 0) in pl and (P - 1, C - 1) in pl
    if P >= 4 and C >= 8:
        assert len(pl) == 7
        assert (P - 1, C - 1 - (C % 4 or 4)) in pl and (P - 2, 1) in pl and (P // 2, C // 2) in pl
        assert (C - 1 - (C % 4 or 4)) % 4 == 3          # the last lane of the last full group of four in front of the tail


def test_case_tables_cover_every_publishing_kernel():
    kernels = {c.kernel for c in A.FWD_CASES} | {c.kernel for c in A.BWD_CASES}
    assert kernels == {'bn_apply_kernel', 'bn_apply_flat_kernel', 'bn_apply4_kernel', 'bn_fused_fwd_kernel', 'bn_stats_apply_kernel', 'bn_bwd_apply_kernel',
                       'bn_bwd_apply4_kernel', 'bn_fused_bwd_kernel', 'bn_bwd_stats_apply_kernel'}
    assert len(A.FWD_CASES) == 2 * 9 + 3 + 2 * 4 and len(A.BWD_CASES) == 6 + 2 * 4
    assert len(A.FWD_PARAMS) == (2 * 9 + 3 + 4) * 8 + 4 * 4
    assert all(v.relu for c, v in A.FWD_PARAMS if c.entry.endswith('_mask'))
    assert all(v.dres for c, v in A.BWD_PARAMS if c.entry.endswith('_res'))
    assert all(v.relu or c.entry == 'dsrl_bn_bwd' for c, v in A.BWD_PARAMS)


def test_dropout_seeds_keep_and_drop_the_planted_element():
    import oracle as O
    for P, C in ((105, 19), (521, 256), (2, 64)):
        for pos in A.PLANTS(P, C):
            kept, dropped = A.drop_seeds(P, C, pos)
            for seed, want in ((kept, True), (dropped, False)):
                m = O.dropout_mask((1, C, P, 1), A.DROP_P, seed, A.RNG_STREAM)
                assert bool(m[0, pos[1], pos[0], 0]) == want, (P, C, pos, seed)
                u = O.philox.uniform_for_elements(P * C, seed, A.RNG_STREAM)[pos[0] * C + pos[1]]
                assert float(u) == A.uniform_at(P, C, pos, seed)


# what the reference of a case depends on: the shape and the variant, not the entry point, the row stride or the kernel
FWD_PREMISES = sorted({(c.P, c.C, v) for c, v in A.FWD_PARAMS})
BWD_PREMISES = sorted({(c.P, c.C, v) for c, v in A.BWD_PARAMS})


@pytest.mark.parametrize('P,C,v', FWD_PREMISES, ids=lambda x: '-'.join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_forward_plant_is_the_unique_maximum(P, C, v):
    for pos in A.PLANTS(P, C):
        d = A.forward_inputs(P, C, v.res, pos)
        for seed, kept in A.seeds_of(P, C, pos, v.drop):
            y, _, _, _ = A.forward_reference(d, v, seed)
            assert np.isfinite(y).all()
            ok, text = A.premise(y, pos, kept)
            assert ok, (pos, seed, kept, text)
            if v.drop:
                assert bool(A.keep_mask(P, C, seed)[pos]) == kept and (kept or y[pos] == 0.0)


@pytest.mark.parametrize('P,C,v', BWD_PREMISES, ids=lambda x: '-'.join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_backward_plant_is_the_unique_maximum(P, C, v):
    fv = A.backward_forward_variant(v)
    for pos in A.PLANTS(P, C):
        d = A.backward_inputs(P, C, pos)
        for seed, kept in A.seeds_of(P, C, pos, v.drop):
            y, _, _, _ = A.forward_reference(d, fv, seed)
            g = A.masked_gradient(d, v, y)
            assert (g[pos] != 0.0) == kept, (pos, seed, 'the planted gradient passes the mask exactly when the element is kept')
            dx = A.backward_reference(d, v, g)
            ok, text = A.premise(dx, pos, kept)
            assert ok, (pos, seed, kept, text)


@pytest.mark.parametrize('case,v', A.FWD_LONG[:len(A.LONG_STATS_SHAPES)] + A.BWD_LONG[::3], ids=lambda x: '-'.join(map(str, x)))
def test_long_slab_plants_are_the_unique_maximum(case, v):
    """one entry point per shape: the reference does not depend on it"""
    P, C = case.P, case.C
    for pos in A.long_plants(P, C):
        assert 0 <= pos[0] < P and 0 <= pos[1] < C
        if isinstance(v, A.FwdVariant):
            ref = A.forward_reference(A.forward_inputs(P, C, v.res, pos), v, 1)[0]
        else:
            d = A.backward_inputs(P, C, pos)
            y = A.forward_reference(d, A.backward_forward_variant(v), 1)[0]
            ref = A.backward_reference(d, v, A.masked_gradient(d, v, y))
        ok, text = A.premise(ref, pos, True)
        assert ok, (pos, text)


def test_nan_plant_reaches_the_output():
    for P, C in ((105, 19), (70, 32)):
        pos = (P // 2, C // 2)
        d = A.forward_inputs(P, C, False, pos, nan=True)
        stats = (np.zeros(C, np.float32), np.ones(C, np.float32))
        y, _, _, _ = A.forward_reference(d, A.FwdVariant(False, 0, 0.0), 1, stats)
        assert np.isnan(y[pos]) and np.isnan(y).sum() == 1 and A.abs_bits_max(y.astype(np.float32)) > A.INF_BITS


def test_backward_partials_sum_to_the_oracle_sums():
    P, C, parts = 70, 32, 3
    d = A.backward_inputs(P, C, (P - 1, C - 1))
    g = d['dy'].astype(np.float64)
    part = A.bwd_partials(g, A.xhat_of(d), parts)
    import oracle as O
    x = A._nchw(d['x'].astype(np.float64))
    _, (mean, invstd), _ = O.batchnorm_train(x, d['gamma'].astype(np.float64), d['beta'].astype(np.float64), eps=A.EPS)
    _, dgamma, dbeta = O.batchnorm_train_bwd(x, d['gamma'].astype(np.float64), mean, invstd, A._nchw(g))
    assert np.allclose(part[0].sum(0), dbeta, rtol=1e-5, atol=1e-5) and np.allclose(part[1].sum(0), dgamma, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('widths,strided', A.CAT_CASES)
def test_concatenation_plants(widths, strided):
    for plant in A.cat_plants(widths):
        xs = A.cat_inputs(widths, plant)
        ref = np.concatenate(xs, 1)
        off = sum(widths[:plant[0]]) + plant[2]
        ok, text = A.premise(ref, (plant[1], off), True)
        assert ok, (plant, text)
    pl = A.cat_plants(widths)
    assert len(set(pl)) == 3 and pl[2][2] // 4 == widths[pl[2][0]] // 4 - 1        # three places; the third is in the last float4 of its source

"""CPU checks of tests/conv_guard_ref.py: the guards detect what they are there to detect, and the case lists of tests/test_conv_guard_gpu.py have the
edges they claim - asserted on the lists themselves, from a copy of the tile table of csrc/conv_igemm.hip."""
import collections

import numpy as np
import pytest
import torch

import conv_guard_ref as R

TILE_SET = {(128, 128), (256, 64), (256, 32), (64, 64), (128, 64), (64, 128), (128, 32), (256, 128), (256, 256)}


# ------------------------------------------------------------------------------------------------ the guard helper
@pytest.mark.parametrize('nbytes', [0, 4, 1000, 64 * 1024, 200000])
def test_guarded_layout(nbytes):
    g = R.Guarded(nbytes, 'cpu', 'buf')
    assert g.ptr % 256 == 0 and g.payload.numel() == nbytes
    assert g.front.numel() >= max(nbytes, 64 * 1024) and g.back.numel() >= max(nbytes, 64 * 1024)
    assert g.front.data_ptr() + g.front.numel() == g.ptr and g.back.data_ptr() == g.ptr + nbytes       # the guards touch the payload: no slack
    assert g.damage() is None
    g.assert_guards()
    assert len(set(g.back[:251].tolist())) > 200           # a pattern, not one repeated byte


@pytest.mark.parametrize('side,where', [('front', -1), ('front', 0), ('back', 0), ('back', -1), ('back', 40000)])
def test_guard_detects_one_planted_byte(side, where):
    g = R.Guarded(1000, 'cpu', 'buf').put(np.zeros(250, np.float32)).keep()
    guard = g.front if side == 'front' else g.back
    guard[where] ^= 1
    assert g.damage() is not None and side in g.damage()
    with pytest.raises(AssertionError, match='1 bytes changed'):
        g.assert_guards()
    g.assert_unchanged()                    # the payload itself was not touched
    guard[where] ^= 1
    g.assert_guards()


def test_payload_change_is_detected():
    g = R.of_bytes(np.arange(64, dtype=np.float32), 'cpu', 'operand')
    g.assert_unchanged()
    g.payload[17] ^= 0x80
    with pytest.raises(AssertionError, match='changed the payload'):
        g.assert_unchanged()
    g.assert_guards()


def test_rows_span_nan_and_gap_columns():
    rows, ld, C = 7, 24, 19
    t = R.Rows(rows, ld, C, 'cpu', name='y')
    assert t.nbytes == 4 * ((rows - 1) * ld + C)            # rows * ld floats minus the unused tail of the last row
    assert np.isnan(t.matrix()).all() and t.matrix().shape == (rows, C)
    t.assert_gaps()
    flat = t.payload.view(torch.float32)
    flat[2 * ld + C] = 1.0                                   # the first gap column of row 2
    assert not t.gaps_intact()
    with pytest.raises(AssertionError, match='gap column'):
        t.assert_gaps()
    flat[2 * ld + C] = float(R.SENTINEL)
    t.assert_gaps()
    flat[(rows - 2) * ld + ld - 1] = 0.0        # the last gap column of the row before last
    assert not t.gaps_intact()
    dense = R.Rows(5, 8, 8, 'cpu', data=np.arange(40, dtype=np.float32).reshape(5, 8), name='x')
    assert dense.nbytes == 160 and np.array_equal(dense.matrix(), np.arange(40, dtype=np.float32).reshape(5, 8))
    dense.assert_gaps(); dense.assert_unchanged()


def test_record_helpers():
    rec = np.zeros(R.AMAX_WORDS, np.uint32)
    rec[32] = np.float32(3.5).view(np.uint32)
    assert R.record_max(rec) == R.abs_bits_max(np.float32([1.0, -3.5, 2.0])) and R.tickets_zero(rec)
    rec[33] = 1
    assert not R.tickets_zero(rec)


def test_check_matrix_sees_a_tail_error_under_the_range_of_the_body():
    want = np.ones((279, 136)); want[:256] *= 1000.0         # the body's range is 1000 times the tail's
    got = want.copy(); got[270, 5] += 1e-2                   # 1e-5 of the whole range, 1e-2 of the tail's
    assert R.range_error(got, want) <= 1e-4
    with pytest.raises(AssertionError, match='last tile of 256 rows'):
        R.check_matrix(got, want, 1e-4, ((256, 64),), 'y')
    got = want.copy(); got[3, 0] = np.nan
    with pytest.raises(AssertionError, match='never written'):
        R.check_matrix(got, want, 1e-4, ((256, 64),), 'y')


# ------------------------------------------------------------------------------------------------ the case lists
def test_tile_table_is_the_librarys():
    assert set(R.TILES) == TILE_SET and len(R.TILES) == 9


def test_case_ids_unique():
    ids = [R.case_id(c) for c in R.ALL_CASES]
    assert len(ids) == len(set(ids)), [i for i, n in collections.Counter(ids).items() if n > 1][:5]


def test_every_forced_tile_has_an_m_tail_an_n_tail_and_two_row_tiles():
    for c in R.ALL_CASES:
        if c.cfg is None:
            continue
        if c.op == 'group':          # one forced tile for a whole group: at least one problem of the group has the edges (the all-taps 3x3 problem keeps its own tile)
            assert any(R.tail_ok('group', R.SHAPES[n], c.cfg) for n in R.GROUP), R.case_id(c)
        else:
            assert R.tail_ok(c.op, R.SHAPES.get(c.shape), c.cfg), R.case_id(c)


def test_channel_chunk_tail_in_every_pass():
    for op in ('fwd', 'dgrad'):
        names = {c.shape for c in (R.FWD_CASES if op == 'fwd' else R.DGRAD_CASES)}
        assert any(R.gemm(op, R.SHAPES[n])[2] % 32 != 0 for n in names)
        assert any(R.SHAPES[n][1] in (40, 72) for n in names)
        for c in (R.FWD_CASES if op == 'fwd' else R.DGRAD_CASES):        # every forced tile meets a chunk tail
            if c.cfg is not None:
                assert R.gemm(op, R.SHAPES[c.shape])[2] % 32 != 0, R.case_id(c)
    # the weight gradient reduces over pixels in chunks of 32: a pixel tail in every shape it runs on
    for c in R.WGRAD_CASES:
        N, C, H, W, K, R_, stride, pad, dil = R.SHAPES[c.shape]
        Ho, Wo = R.dims(R.SHAPES[c.shape])
        assert (N * Ho * Wo) % 32 != 0 or c.shape == 'w3', R.case_id(c)      # the all-taps kernel needs whole 32-pixel row pieces


def test_partials_shapes():
    for c in R.ALL_CASES:
        if c.stats:
            N, C, H, W, K = R.SHAPES[c.shape][:5]
            assert (K if c.op == 'fwd' else C) % 32 == 0 and c.mode != 'fp32', R.case_id(c)
    assert any(c.stats for c in R.FWD_CASES) and any(c.stats and c.drop > 0 for c in R.DGRAD_CASES) and any(c.stats and c.drop == 0 for c in R.DGRAD_CASES)


def test_shape_kinds_present():
    for cases, op in ((R.FWD_CASES, 'fwd'), (R.DGRAD_CASES, 'dgrad'), (R.WGRAD_CASES, 'wgrad')):
        shapes = {R.SHAPES[c.shape] for c in cases}
        assert any(s[5] == 3 and s[6] == 1 and s[8] == 1 for s in shapes), op                           # 3x3 stride 1
        assert any(s[5] == 3 and s[6] == 2 and s[2] % 2 == 1 and s[3] % 2 == 1 for s in shapes), op       # 3x3 stride 2 on odd H and W
        assert any(s[5] == 1 and s[6] == 2 for s in shapes), op                                         # 1x1 stride 2
        assert any(s[8] >= max(s[2], s[3]) and s[5] == 3 for s in shapes), op                             # a dilation as large as the map: dead taps
        assert any(s[4] == 19 for s in shapes), op                                                      # K = 19 (dgrad pads to 20)
    assert R.live_taps(R.SHAPES['dil']).sum() == 1 and R.live_taps(R.SHAPES['dil'])[1, 1]
    assert R.live_taps(R.SHAPES['s1']).all()
    N, C, H, W, K, Rk, stride, pad = R.STEM
    assert (C, Rk, stride) == (3, 7, 2) and H % 2 == 1 and W % 2 == 1
    assert any(c.op == 'rowfold_fwd' for c in R.ALL_CASES) and any(c.op == 'rowfold_wgrad' for c in R.ALL_CASES)
    # the planner's own split-K shapes run unforced only
    for c in R.ALL_CASES:
        if c.shape in ('splitk', 'fp32sk'):
            assert R.plan_kind(c) == 'planner', R.case_id(c)
    assert any(c.shape == 'splitk' for c in R.FWD_CASES)
    # rows stay small: above 256 only as far as the 256-row tiles and the strided maps need
    for n, s in R.SHAPES.items():
        if n != 'splitk':
            assert max(R.gemm('fwd', s)[0], R.gemm('dgrad', s)[0]) <= 1200, n


def test_every_tile_and_every_split_appears_for_every_pass():
    for mode in R.MODES:
        for op, cases in (('fwd', R.FWD_CASES), ('dgrad', R.DGRAD_CASES), ('wgrad', R.WGRAD_CASES), ('group', R.GROUP_CASES), ('rowfold_fwd', R.ROWFOLD_CASES)):
            if op == 'group' and mode == 'fp32':
                continue
            mine = [c for c in cases if c.mode == mode and c.op == op and not c.refused]
            assert {c.cfg for c in mine if c.cfg is not None} >= set(R.cfgs_of(mode, op)), (mode, op)
            assert any(R.plan_kind(c) == 'planner' for c in mine), (mode, op)
        for op, cases in (('fwd', R.FWD_CASES), ('dgrad', R.DGRAD_CASES)):
            mine = [c for c in cases if c.mode == mode]
            if mode != 'fp32':
                assert {c.kg for c in mine} >= {1, 2}, (mode, op)
            for strided in (False, True):
                got = {(c.splits, c.coop) for c in mine if c.splits and (R.SHAPES[c.shape][6] > 1) == strided}
                want = {(s, k) for s in (1, 2, 3) for k in ((1, 0) if mode in R.F16 else (1,))}
                assert got >= want, (mode, op, strided)
        assert {c.psplits for c in R.WGRAD_CASES if c.mode == mode} >= {1, 3}
    for mode in R.F16:          # every operand variant under the planner's choice and under every tile
        for cases in (R.FWD_CASES, R.DGRAD_CASES):
            for cfg in (None,) + tuple(range(8)):
                assert {c.operands for c in cases if c.mode == mode and c.cfg == cfg and c.kg is None and c.splits is None} == {'planes', 'amax', 'null'}, (mode, cfg)
    assert len(R.GROUP) >= 3 and 'w3' in R.GROUP


def test_refused_share_and_coverage():
    refused = [c for c in R.ALL_CASES if c.refused]
    assert 0 < len(refused) <= 0.10 * len(R.ALL_CASES), (len(refused), len(R.ALL_CASES))
    for c in refused:
        assert c.refused[0] < 0 and isinstance(c.refused[1], str) and c.refused[1]
    cov = R.coverage()
    for e in ('dsrl_conv2d_fwd_planes', 'dsrl_conv2d_dgrad_planes', 'dsrl_conv2d_wgrad_amax', 'dsrl_conv2d_rowfold_fwd', 'dsrl_conv2d_rowfold_wgrad'):
        for mode in R.MODES:
            assert sum(cov[(e, mode)].values()) > 0, (e, mode)
    for mode in R.MODES[:3]:
        assert sum(cov[('dsrl_conv2d_dgrad_planes_drop', mode)].values()) > 0 and sum(cov[('dsrl_conv2d_wgrad_group_plan+launch', mode)].values()) > 0
    assert len(R.ALL_CASES) <= 1500            # seconds per case, a few minutes in all


def test_references_are_frozen_and_shared():
    a, b = R.inputs('k19'), R.inputs('k19')
    assert all(u is v for u, v in zip(a, b)) and not a[0].flags.writeable
    assert R.ref_fwd('k19') is R.ref_fwd('k19') and not R.ref_fwd('k19').flags.writeable
    x, w = a[:2]
    y = R.ref_fwd('k19')
    assert y.shape == (1, 19, 9, 31) and y.dtype == np.float64
    np.testing.assert_allclose(y[0, :, 4, 5], w[:, :, 0, 0].astype(np.float64) @ x[0, :, 4, 5].astype(np.float64), rtol=1e-12)

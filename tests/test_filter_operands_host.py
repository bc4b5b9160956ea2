"""filter_operands.py, the host half: the int64 table rows of the batched filter kernels and the amax segment rows, from plain integers and fake
addresses - no device.  The expected values are written out here, not recomputed through the code under test."""
from dualsuperreslearningforsemseg_amd import filter_operands as FO

# (K, C, R*S) of the reduced-width head: a K padded 19 -> 20, a ragged channel tile (C = 40), one filter that is not plane-eligible (K = 19)
SHAPES = ((19, 32, 1), (32, 40, 9), (8, 32, 1), (32, 64, 9))
DIMS = [(K, RS, C) for K, C, RS in SHAPES]
W = [0x1000, 0x2000, 0x3000, 0x4000]            # fake addresses: filters, amax records, transposed outputs, forward outputs
REC = [0x100, 0x500, 0x900, 0xD00]
WT = [0x10000, 0x20000, 0x30000, 0x40000]
FWD = [0x50000, 0x60000, 0x70000, 0x80000]


def test_rules_and_padding():
    assert [FO.padded_k(K) for K, _, _ in SHAPES] == [20, 32, 8, 32]
    assert [FO.wt_floats(K, RS, C) for K, C, RS in SHAPES] == [32 * 20, 40 * 9 * 32, 32 * 8, 64 * 9 * 32]
    assert [FO.plane_eligible(K, C) for K, C, _ in SHAPES] == [False, True, True, True]
    assert FO.eligible(32, True) and FO.eligible(40, True) and not FO.eligible(3, True) and not FO.eligible(32, False) and not FO.eligible(1, True)
    assert [FO.align(n) for n in (0, 1, 4, 19, 20)] == [0, 4, 4, 20, 20] and FO.align(1025, 1024) == 2048


def test_transpose_and_split_tables():
    """columns {w, transposed-out, K, K-out, RS, C, first tile, ct, record, forward-out}; K-out padded to 4"""
    first, kp, ct = [0, 1, 19, 20], [20, 32, 8, 32], [1, 2, 1, 2]
    rows, tiles = FO.table_rows(DIMS, W, REC, transposed_out=WT)               # the fp32 transposes of a training step
    assert tiles == 38
    assert rows == [[W[i], WT[i], SHAPES[i][0], kp[i], SHAPES[i][2], SHAPES[i][1], first[i], ct[i], REC[i], 0] for i in range(4)]
    rows, tiles = FO.table_rows(DIMS, W, REC, transposed_out=WT, forward_out=FWD)      # both split forms
    assert tiles == 38
    assert rows == [[W[i], WT[i], SHAPES[i][0], kp[i], SHAPES[i][2], SHAPES[i][1], first[i], ct[i], REC[i], FWD[i]] for i in range(4)]
    # the forward-only form (frozen operands): the transposed column is null, everything else as above; and the measuring-only table
    rows, tiles = FO.table_rows(DIMS, W, REC, forward_out=FWD)
    assert tiles == 38 and [r[1] for r in rows] == [0, 0, 0, 0] and [r[9] for r in rows] == FWD and [r[6] for r in rows] == first
    rows, tiles = FO.table_rows(DIMS, W, REC)
    assert tiles == 38 and all(r[1] == 0 and r[9] == 0 for r in rows) and [r[3] for r in rows] == kp and [r[8] for r in rows] == REC


def test_plane_tables_use_k_itself():
    idx = [i for i, (K, C, _) in enumerate(SHAPES) if FO.plane_eligible(K, C)]
    assert idx == [1, 2, 3]
    rows, tiles = FO.table_rows([DIMS[i] for i in idx], [W[i] for i in idx], [REC[i] for i in idx], [WT[i] for i in idx], [FWD[i] for i in idx], pad_k=False)
    assert tiles == 37
    assert rows == [[0x2000, 0x20000, 32, 32, 9, 40, 0, 2, 0x500, 0x60000],
                    [0x3000, 0x30000, 8, 8, 1, 32, 18, 1, 0x900, 0x70000],
                    [0x4000, 0x40000, 32, 32, 9, 64, 19, 2, 0xD00, 0x80000]]
    # K-out is what differs from the split tables: a K that is no multiple of 4 would be padded there and is not here
    assert FO.table_row(1, 19, 1, 32, 0, 2, pad_k=False)[0][3] == 19 and FO.table_row(1, 19, 1, 32, 0, 2)[0][3] == 20
    # a K of 40 spans two 32-wide tiles, padded or not
    assert FO.table_row(1, 40, 9, 40, 5, 2)[1] == 9 * 2 * 2


def test_single_row():
    row, tiles = FO.table_row(0x1000, 19, 1, 32, 7, 0x100, 0x10000, 0x50000)
    assert row == [0x1000, 0x10000, 19, 20, 1, 32, 7, 1, 0x100, 0x50000] and tiles == 1


def test_amax_segment_rows():
    """{address of the segment's first float, floats, record}: a 32 x 9 x 40 filter is 11520 floats = 11 segments of 1024 and one of 256"""
    rows = FO.segment_rows(0x2000, 32 * 9 * 40, 0x500, 1024, 4)
    assert len(rows) == 12 and rows[0] == [0x2000, 1024, 0x500] and rows[1] == [0x2000 + 4096, 1024, 0x500]
    assert rows[11] == [0x2000 + 11 * 4096, 256, 0x500] and sum(r[1] for r in rows) == 11520
    assert FO.segment_rows(0x1000, 19 * 32, 0x100, 1024, 4) == [[0x1000, 608, 0x100]]          # shorter than one segment
    assert FO.segment_rows(0x1000, 2048, 0, 1024, 4) == [[0x1000, 1024, 0], [0x1000 + 4096, 1024, 0]]      # exactly two
    # arena indices (the optimiser's segment table): unit steps, and an empty range gives no row
    assert FO.segment_rows(100, 2500, 7, 1024) == [[100, 1024, 7], [1124, 1024, 7], [2148, 452, 7]]
    assert FO.segment_rows(100, 0, 7, 1024) == [] and FO.segment_rows(100, -8, 7, 1024) == []

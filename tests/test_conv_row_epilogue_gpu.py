"""The row epilogue of the one-group data-gradient builds (csrc/conv_common.h: RowEpilogue; switch DSRL_ROW_EPILOGUE) against the scalar epilogue it
replaces.  Every case runs its entry point twice on identical inputs - switch unset, switch = 0 - and the two runs must agree bit for bit (torch.equal)
on dx / y, on the BatchNorm-backward partials and on the forward statistics: the row pass performs the same floating-point operations in the same order.
Each run is also held against the fp64 oracle within its arithmetic's bound, and writes behind guards into a buffer of exactly the tensor's span whose
gap columns (and the floats in front of an offset tensor) must stay untouched.  Which cases take the row path is stated here from the rule
(expect_row) and compared with the library's own answer (dsrl_conv2d_row_epilogue_supported), so a case meant to fall back does, and the others do not.

Shapes are the smallest that can go wrong: M = 130 (a tail behind a 128-row tile, inside a 32-row piece) and M = 9; output channels 4 (one float4),
36 / 68 / 40 / 72 / 96 (tile tails, multiples of 4), 19 / 50 (fall back); reductions of 32, 40 and 96 channels (one chunk, a chunk tail, three chunks)."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_guard_ref as R                                   # noqa: E402
import oracle as O                                           # noqa: E402
from hip_helpers import DEV, HF                              # noqa: E402

TOL = dict(R.TOL, bf16x3=3e-5)                # bf16x3: 16 mantissa bits per operand (test_conv_precision_modes)
F16 = R.F16
Case = collections.namedtuple('Case', 'op mode N H W C K R stride acc sums drop gap shift cfg splits coop operands bias mean_shift')
# op: dgrad / fwd.  C: channels of the conv's input, K: of its output (dgrad writes C channels and reduces over K, forward the other way round).
# sums (dgrad): None, or bn_relu 0 / 1 / 2 of the BatchNorm-backward sums.  gap: floats between the rows of the written tensor; shift: floats the written
# tensor is offset by from a 256-byte boundary; mean_shift: the same for mean / invstd.  operands: 'amax' (records + pre-split filters), 'planes', 'null'.


def mk(op='dgrad', mode='f16x3', px=(2, 5, 13), C=36, K=40, Rk=1, stride=1, acc=1, sums=None, drop=0.0, gap=0, shift=0, cfg=4, splits=None, coop=None,
       operands=None, bias=0, mean_shift=0):
    operands = operands or ('amax' if mode in F16 else 'null')
    return Case(op, mode, px[0], px[1], px[2], C, K, Rk, stride, acc, sums, drop, gap, shift, cfg, splits, coop, operands, bias, mean_shift)


def cid(c):
    s = f'{c.op}-{c.mode}-{c.N}x{c.H}x{c.W}-C{c.C}-K{c.K}-{c.R}x{c.R}-cfg{c.cfg}-{c.operands}'
    for k, v in (('s', c.stride if c.stride > 1 else 0), ('acc', c.acc), ('relu', c.sums), ('drop', c.drop), ('gap', c.gap), ('shift', c.shift), ('sp', c.splits),
                 ('coop', c.coop), ('bias', c.bias), ('mshift', c.mean_shift)):
        if v not in (None, 0, 0.0) or (k == 'relu' and v == 0):
            s += f'-{k}{v}'
    return s


def _cases():
    out = []
    # output channels x filter x accumulate on 128x64 tiles; no sums
    for C in (4, 36, 68, 19, 50):
        for Rk in (1, 3):
            for acc in (0, 1):
                out.append(mk(C=C, Rk=Rk, acc=acc))
    # reduction length, BatchNorm sums of every kind, dropout scale
    for K in (32, 40, 96):
        for relu in (0, 1, 2):
            out.append(mk(C=96, K=K, sums=relu, acc=(K // 8 + relu) % 2, drop=0.25 if (relu and (relu + K // 32) % 2) else 0.0, Rk=3 if K == 40 else 1))     # a dropout scale needs the ReLU mask
    out.append(mk(C=64, K=96, sums=2, acc=1, drop=0.25))
    out.append(mk(C=64, K=32, sums=1, acc=0))
    # M = 9
    out += [mk(px=(1, 3, 3), C=36, Rk=3), mk(px=(1, 3, 3), C=64, sums=2, Rk=3), mk(px=(1, 3, 3), C=4, acc=1)]
    # output layout: row gaps, an offset that keeps 16-byte alignment, one that does not
    out += [mk(C=68, gap=12), mk(C=96, gap=12, sums=2), mk(C=68, shift=4), mk(C=96, shift=4, sums=1, gap=12), mk(C=68, shift=1), mk(C=96, shift=1, sums=2)]
    # mean / invstd off the 16-byte boundary: the sums lose their fast conditions and the whole launch falls back
    out.append(mk(C=96, sums=2, mean_shift=1))
    # every tile, register-staged and planes (8 = 256x256: no register-staged dgrad build; the planes build stays scalar)
    for cfg in range(8):
        out.append(mk(C=96, K=96, sums=2, acc=1, cfg=cfg, drop=0.25 if cfg % 2 else 0.0))
        out.append(mk(C=72, K=40, acc=1, cfg=cfg, Rk=3))
    for cfg in (0, 1, 3, 4, 5, 7, 8):
        out.append(mk(C=96, K=96, sums=2, acc=1, cfg=cfg, operands='planes'))
    # split-K on 128x128: reduced inside the launch (the last arriver runs the row epilogue) and through slabs (scalar, the reduce kernel accumulates)
    out += [mk(C=96, K=96, Rk=3, sums=2, acc=1, cfg=0, splits=2, coop=1), mk(C=96, K=96, Rk=3, acc=1, cfg=0, splits=2, coop=1),
            mk(C=96, K=96, Rk=3, acc=1, cfg=0, splits=2, coop=0)]
    # a stride-2 data gradient in parity order (64 pixels per class = one 64-row tile): scalar
    out.append(mk(px=(1, 4, 64), C=36, K=32, Rk=3, stride=2, acc=1, cfg=3))
    out.append(mk(px=(1, 5, 13), C=36, K=32, Rk=3, stride=2, acc=1, cfg=3))      # odd map: strided, row-major order - scalar as well
    # arithmetics
    for mode in ('f16x1', 'bf16x3', 'bf16x6'):
        out += [mk(mode=mode, C=96, sums=1, acc=1), mk(mode=mode, C=68, acc=1, Rk=3)]
    out.append(mk(mode='fp32', C=68, acc=1))
    # planes kernel: stride-1 data gradients and the forward, f16x3 and f16x1
    for mode in F16:
        for C in (40, 72):
            for Rk in (1, 3):
                out.append(mk(mode=mode, C=C, K=40, Rk=Rk, acc=1, operands='planes', gap=12 if C == 72 else 0))
        for relu in (0, 1, 2):
            out.append(mk(mode=mode, C=96, K=96 if relu else 32, sums=relu, acc=relu % 2, drop=0.25 if relu == 1 else 0.0, operands='planes', shift=4 if relu == 2 else 0))
        out.append(mk(mode=mode, px=(1, 3, 3), C=64, K=32, sums=2, acc=1, operands='planes'))
        out.append(mk(op='fwd', mode=mode, C=40, K=72, bias=1, operands='planes'))
    # forward launches keep the scalar epilogue: with and without bias, with the statistics
    for K in (36, 19):
        for bias in (0, 1):
            out.append(mk(op='fwd', C=40, K=K, bias=bias, Rk=3 if bias else 1, gap=12 if K == 36 else 0))
    out.append(mk(op='fwd', C=40, K=64, bias=1, sums=0))         # sums on a forward case: the (n, mean, M2) statistics
    return out


CASES = _cases()


def pad_of(c):
    return 1 if c.R == 3 else 0


def parity_order(c):
    """the host's rule for ordering the rows of a strided data gradient by parity class (csrc/conv_igemm.hip: dgrad_impl)"""
    bm = R.TILES[c.cfg][0]
    return c.stride > 1 and c.mode != 'fp32' and c.H % c.stride == 0 and c.W % c.stride == 0 and (c.W // c.stride) % 32 == 0 and \
        (c.N * (c.H // c.stride) * (c.W // c.stride)) % bm == 0


def expect_row(c):
    """the rule of the row epilogue, restated: a stride-1 data gradient of an fp16 arithmetic on a one-group build that writes finished values, 4-channel rows
    at 16-byte alignment, a tile of at most 128 KiB, something to fetch (old values or the sums' operands), and the sums' own 16-byte conditions"""
    bm, bn = R.TILES[c.cfg]
    if c.op != 'dgrad' or c.mode not in F16 or c.stride != 1 or bm * bn * 4 > 128 * 1024:
        return False
    if c.splits and c.splits > 1 and not (c.coop == 1 and c.cfg == 0 and c.operands != 'planes'):
        return False
    if c.C % 4 or c.gap % 4 or c.shift % 4:
        return False
    if c.sums is not None and c.mean_shift % 4:
        return False
    return bool(c.acc) or c.sums is not None


@functools.lru_cache(maxsize=None)
def data(N, H, W, C, K, Rk, stride):
    """inputs and fp64 references of a conv shape, drawn and computed once: x >= 0 [N,C,H,W] (also the BatchNorm output of the sums), w, bias, dy, the previous
    content of dx, the BatchNorm's input / mean / invstd; y = conv(x), dx = dgrad(dy)"""
    pad = 1 if Rk == 3 else 0
    rs = np.random.RandomState(N * 1000 + H * 100 + W * 10 + C + 7 * K + Rk + stride)
    x = np.maximum(rs.standard_normal((N, C, H, W)), 0).astype(np.float32)
    w = (rs.standard_normal((K, C, Rk, Rk)) / np.sqrt(C * Rk * Rk)).astype(np.float32)
    bias = rs.standard_normal(K).astype(np.float32)
    Ho, Wo = R.out_size(H, Rk, stride, pad, 1), R.out_size(W, Rk, stride, pad, 1)
    dy = rs.standard_normal((N, K, Ho, Wo)).astype(np.float32)
    dx0 = rs.standard_normal((N, C, H, W)).astype(np.float32)
    bx = rs.standard_normal((N * H * W, C)).astype(np.float32)
    mean, invstd = (rs.standard_normal(C) * 0.1).astype(np.float32), (1.0 + rs.rand(C)).astype(np.float32)
    y = O.conv2d(x.astype(np.float64), w.astype(np.float64), None, stride, pad, 1)
    dx = O.conv2d_bwd(x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64), stride, pad, 1, False)[0]
    out = (x, w, bias, dy, dx0, bx, mean, invstd, y, dx)
    for a in out:
        a.setflags(write=False)
    return out


class Out(R.Guarded):
    """the written tensor [rows][ld] with C channels in use, `shift` floats behind a 256-byte boundary, exactly as long as its span; everything that is
    not one of its elements - the shift, the gap columns - holds SENTINEL and must still hold it afterwards"""

    def __init__(self, rows, ld, C, shift, prev, name):
        n = shift + R.span_floats(rows, ld, C)
        super().__init__(4 * n, DEV, name)
        self.shape2 = (rows, C)
        self.used = shift + (np.arange(rows)[:, None] * ld + np.arange(C)[None, :]).reshape(-1)
        flat = np.full(n, R.SENTINEL, np.float32)
        flat[self.used] = np.nan if prev is None else np.asarray(prev, np.float32).reshape(-1)
        self.rest = np.ones(n, bool)
        self.rest[self.used] = False
        self.put(flat)
        self.at = self.ptr + 4 * shift

    def matrix(self):
        return self.f32()[self.used].reshape(self.shape2)

    def tensor(self):
        return self.payload.view(torch.int32).clone()          # bit patterns: torch.equal then also holds NaN against NaN to the bit

    def assert_rest(self):
        assert (self.f32()[self.rest].view(np.uint32) == R.SENTINEL.view(np.uint32)).all(), f'{self.name}: a float outside the tensor (gap column or offset) was written'


def shifted(a, shift, name, bufs):
    """a copy of a float vector `shift` floats behind a 256-byte boundary -> its address"""
    g = R.of_bytes(np.concatenate([np.zeros(shift, np.float32), np.asarray(a, np.float32)]), DEV, name)
    bufs.append(g)
    return g.ptr + 4 * shift


def filter_ops(c, bufs, w):
    """(record, forward split, transposed split, forward planes, transposed planes) as guarded copies of what functional prepares, or Nones"""
    if c.mode not in F16 or c.operands == 'null':
        return [None] * 5
    wt = torch.from_numpy(R.krsc(w)).to(DEV).permute(0, 3, 1, 2)
    rec, wsp, wtsp, _ = HF.split_filter(wt)
    out = [R.of_bytes(rec, DEV, 'w_amax'), R.of_bytes(wsp, DEV, 'w_split'), R.of_bytes(wtsp, DEV, 'wt_split'), None, None]
    if c.operands == 'planes':
        wp, wtp = HF.filter_planes(wt, rec)
        out[3], out[4] = R.of_bytes(wp, DEV, 'w_planes'), R.of_bytes(wtp, DEV, 'wt_planes')
    bufs += [g for g in out if g is not None]
    return out


def act_ops(c, bufs, src, ld, P, C, name):
    """(record, planes) of an activation operand"""
    if c.mode not in F16 or c.operands == 'null':
        return None, None
    rec = R.Guarded(4 * R.AMAX_WORDS, DEV, name + '_amax')
    rec.payload.zero_()
    HF.call('dsrl_amax', src.ptr, ld, P, C, rec.ptr, HF._stream())
    bufs.append(rec.keep())
    pl = None
    if c.operands == 'planes':
        npl = 2 if c.mode == 'f16x3' else 1
        pl = R.Guarded(int(HF.query('dsrl_planes_bytes', P * ld, npl)), DEV, name + '_planes')
        pl.payload.zero_()
        HF.call('dsrl_split_planes', src.ptr, ld, P, C, rec.ptr, pl.ptr, npl, HF._stream())
        bufs.append(pl.keep())
    return rec, pl


def ptr(g):
    return None if g is None else g.ptr


def finish(bufs, outs):
    torch.cuda.synchronize()
    for g in bufs + outs:
        g.assert_guards()
    for g in bufs:
        g.assert_unchanged()


def run_dgrad(c):
    x, w, _, dy, dx0, bx, mean, invstd, _, dx_ref = data(c.N, c.H, c.W, c.C, c.K, c.R, c.stride)
    pad = pad_of(c)
    shp = (c.N, c.H, c.W, c.C, c.K, c.R, c.R, c.stride, pad, 1)
    Ho, Wo = R.out_size(c.H, c.R, c.stride, pad, 1), R.out_size(c.W, c.R, c.stride, pad, 1)
    P, Po = c.N * c.H * c.W, c.N * Ho * Wo
    bufs = []
    dyg = R.Rows(Po, c.K, c.K, DEV, R.pixel_major(dy), 'dy')
    wg = R.of_bytes(R.krsc(w), DEV, 'w')
    bufs += [dyg, wg]
    wa, _, wtsp, _, wtp = filter_ops(c, bufs, w)
    dya, dypl = act_ops(c, bufs, dyg, c.K, Po, c.K, 'dy')
    lddx = c.C + c.gap
    dxg = Out(P, lddx, c.C, c.shift, R.pixel_major(dx0) if c.acc else None, 'dx')
    ws_bytes = int(HF.query('dsrl_conv2d_dgrad_workspace_bytes', *shp))
    wsg = R.Guarded(ws_bytes, DEV, 'workspace')
    wsg.payload.fill_(0xff)
    outs = [dxg, wsg]
    parts, sg, bnargs = 0, None, (None, 0, None, 0, None, None, 0)
    ypix = R.pixel_major(x)
    if c.sums is not None:
        parts = int(HF.query('dsrl_conv2d_dgrad_stats_parts', *shp))
        assert parts > 0, 'the case expects BatchNorm-backward sums from this launch, dsrl_conv2d_dgrad_stats_parts says it has none'
        bxg = R.Rows(P, c.C, c.C, DEV, bx, 'bn_x')
        bufs.append(bxg)
        if c.sums == 2:             # sign mask: uint32 [C / 32][ldm], bit c % 32 of word [c / 32][p] = y[p][c] > 0
            ldm = P + 3
            words = np.zeros((c.C // 32, ldm), np.uint32)
            for ch in range(c.C):
                words[ch // 32, :P] |= (ypix[:, ch] > 0).astype(np.uint32) << np.uint32(ch % 32)
            byg, bn_ldy = R.of_bytes(words, DEV, 'bn mask'), ldm
        else:
            byg, bn_ldy = R.Rows(P, c.C, c.C, DEV, ypix, 'bn_y'), c.C
        bufs.append(byg)
        sg = R.Guarded(4 * int(HF.query('dsrl_bn_stats_floats', 2, parts, c.C)), DEV, 'dgrad partials')
        sg.fill_nan()
        outs.append(sg)
        bnargs = (bxg.ptr, c.C, byg.ptr, bn_ldy, shifted(mean, c.mean_shift, 'bn_mean', bufs), shifted(invstd, c.mean_shift, 'bn_invstd', bufs), c.sums)
    head = (dyg.ptr, c.K, ptr(dya), ptr(dypl), wg.ptr, None, ptr(wa), ptr(wtsp), ptr(wtp), dxg.at, lddx) + shp + (wsg.ptr, ws_bytes)
    if c.sums is not None and c.drop > 0:
        HF.call('dsrl_conv2d_dgrad_planes_drop', *head, *bnargs, float(c.drop), ptr(sg), parts, int(c.acc), HF._stream())
    else:
        HF.call('dsrl_conv2d_dgrad_planes', *head, *bnargs, ptr(sg), parts, int(c.acc), HF._stream())
    finish(bufs, outs)
    dxg.assert_rest()
    dx = dxg.matrix()
    want = R.pixel_major(dx_ref) + (R.pixel_major(dx0).astype(np.float64) if c.acc else 0.0)
    e = R.check_matrix(dx, want, TOL[c.mode], (R.TILES[c.cfg],), 'dx')
    res = dict(out=dxg.tensor(), stats=None)
    if c.sums is not None:
        raw = sg.f32()
        assert not np.isnan(raw).any(), 'dgrad partials: elements never written'
        res['stats'] = sg.payload.view(torch.int32).clone()
        b2 = raw[:2 * parts * c.C].reshape(2, parts, c.C).astype(np.float64).sum(1)
        gs = float(np.float32(1.0) / (np.float32(1.0) - np.float32(c.drop))) if c.drop > 0 else 1.0
        g = dx.astype(np.float64) * ((ypix > 0) if c.sums else 1.0) * gs           # the (masked) gradient of the tensor the launch wrote
        xh = (bx.astype(np.float64) - mean[None, :]) * invstd[None, :]
        e0, e1 = R.range_error(b2[0], g.sum(0)), R.range_error(b2[1], (g * xh).sum(0))
        e += [e0, e1]
        assert e0 <= R.DGRAD_SUMS_TOL and e1 <= R.DGRAD_SUMS_TOL, f'dgrad partials: sum g {e0:.2e}, sum g xhat {e1:.2e} (bound {R.DGRAD_SUMS_TOL})'
    res['err'] = e
    bn_fast = c.sums is not None and c.mean_shift % 4 == 0
    res['row'] = int(HF.query('dsrl_conv2d_row_epilogue_supported', 1, R.TILES[c.cfg][0], R.TILES[c.cfg][1], 1, c.stride, int(parity_order(c)), c.splits or 1,
                              int(bool(c.coop) and c.cfg == 0 and c.operands != 'planes'), c.C, lddx, dxg.at, int(c.acc), int(c.sums is not None), int(bn_fast), 0))
    return res


def run_fwd(c):
    x, w, bias, _, _, _, _, _, y_ref, _ = data(c.N, c.H, c.W, c.C, c.K, c.R, c.stride)
    pad = pad_of(c)
    shp = (c.N, c.H, c.W, c.C, c.K, c.R, c.R, c.stride, pad, 1)
    Ho, Wo = R.out_size(c.H, c.R, c.stride, pad, 1), R.out_size(c.W, c.R, c.stride, pad, 1)
    P, M = c.N * c.H * c.W, c.N * Ho * Wo
    bufs = []
    xg = R.Rows(P, c.C, c.C, DEV, R.pixel_major(x), 'x')
    wg = R.of_bytes(R.krsc(w), DEV, 'w')
    bufs += [xg, wg]
    bg = None
    if c.bias:
        bg = R.of_bytes(bias, DEV, 'bias')
        bufs.append(bg)
    wa, wsp, _, wp, _ = filter_ops(c, bufs, w)
    xa, xp = act_ops(c, bufs, xg, c.C, P, c.C, 'x')
    ldy = c.K + c.gap
    yg = Out(M, ldy, c.K, c.shift, None, 'y')
    ws_bytes = int(HF.query('dsrl_conv2d_fwd_workspace_bytes', *shp))
    wsg = R.Guarded(ws_bytes, DEV, 'workspace')
    wsg.payload.fill_(0xff)
    outs = [yg, wsg]
    parts, sg = 0, None
    if c.sums is not None:
        parts = int(HF.query('dsrl_conv2d_fwd_stats_parts', *shp))
        assert parts > 0
        sg = R.Guarded(4 * int(HF.query('dsrl_bn_stats_floats', 3, parts, c.K)), DEV, 'partials')
        sg.fill_nan()
        outs.append(sg)
    HF.call('dsrl_conv2d_fwd_planes', xg.ptr, c.C, ptr(xa), ptr(xp), wg.ptr, ptr(wa), ptr(wsp), ptr(wp), ptr(bg), yg.at, ldy, *shp, wsg.ptr, ws_bytes, ptr(sg), parts,
            HF._stream())
    finish(bufs, outs)
    yg.assert_rest()
    y = yg.matrix()
    want = R.pixel_major(y_ref) + (bias.astype(np.float64)[None, :] if c.bias else 0.0)
    e = R.check_matrix(y, want, TOL[c.mode], (R.TILES[c.cfg],), 'y')
    res = dict(out=yg.tensor(), stats=None, err=e)
    if sg is not None:
        pt = sg.f32()[:3 * parts * c.K].reshape(3, parts, c.K).astype(np.float64)
        assert not np.isnan(pt).any(), 'partials: elements never written'
        res['stats'] = sg.payload.view(torch.int32).clone()
        n = pt[0].sum(0)
        assert np.all(n == M)
        mu = (pt[0] * pt[1]).sum(0) / n
        m2 = (pt[2] + pt[0] * (pt[1] - mu) ** 2).sum(0)
        em, ev = R.range_error(mu, y.astype(np.float64).mean(0)), R.range_error(m2 / n, y.astype(np.float64).var(0))
        assert em <= R.STATS_MEAN_TOL and ev <= R.STATS_VAR_TOL, (em, ev)
    res['row'] = int(HF.query('dsrl_conv2d_row_epilogue_supported', 0, R.TILES[c.cfg][0], R.TILES[c.cfg][1], 1, c.stride, 0, 1, 0, c.K, ldy, yg.at, 0, 0, 0,
                              int(c.sums is not None)))
    return res


@pytest.fixture(autouse=True)
def _default_mode():
    HF.set_conv_precision(None)
    yield
    HF.set_conv_precision(None)
    HF._query_cache.clear()


@pytest.mark.parametrize('c', CASES, ids=cid)
def test_row_epilogue_equals_scalar_epilogue(c, monkeypatch):
    monkeypatch.setenv('DSRL_PLANES', '1')
    monkeypatch.setenv('DSRL_SK_COOP1', '1')
    plan = dict(DSRL_FORCE_CFG=c.cfg, DSRL_FORCE_KG=1, DSRL_FORCE_SPLITS=c.splits, DSRL_SK_COOP=c.coop, DSRL_FORCE_PSPLITS=None)
    for k, v in plan.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    HF.set_conv_precision(c.mode)
    HF._query_cache.clear()
    run = run_dgrad if c.op == 'dgrad' else run_fwd
    monkeypatch.delenv('DSRL_ROW_EPILOGUE', raising=False)
    on = run(c)
    monkeypatch.setenv('DSRL_ROW_EPILOGUE', '0')
    off = run(c)
    print(cid(c), 'row' if on['row'] else 'scalar', ['%.1e' % v for v in on['err']])
    assert on['row'] == int(expect_row(c)), f"the library says row epilogue = {on['row']}, the rule says {expect_row(c)}"
    assert off['row'] == 0, 'DSRL_ROW_EPILOGUE=0 must give the scalar epilogue everywhere'
    assert torch.equal(on['out'], off['out']), 'the written tensor differs between the row and the scalar epilogue'
    assert (on['stats'] is None) == (off['stats'] is None)
    if on['stats'] is not None:
        assert torch.equal(on['stats'], off['stats']), 'the BatchNorm partials differ between the row and the scalar epilogue'

"""The ReLU sign mask of a BatchNorm output (dsrl_bn_train_fwd_from_stats_mask: uint32 [C / 32][P], bit j of word (g, p) = y[p][32 g + j] > 0) and its
readers (relu / bn_relu == 2 in dsrl_bn_bwd_from_stats_* and in the dsrl_conv2d_dgrad_* epilogues: the y pointer addresses the mask, ldy is its row
length P).  The bit is the very comparison the readers made on y, so every comparison here is bitwise."""
import numpy as np
import pytest
import torch

import gen                     # noqa: F401
from hip_helpers import DEV, HF, D, dev

gpu = pytest.mark.gpu          # every test but the size query at the end needs the GPU

# (P, C, row blocks of partials): ragged last pass; several slabs and groups; the 1024-thread variant (>= 128 partials); the reduce launch (> 256)
SHAPES = [(70, 32, 3), (521, 96, 5), (256, 32, 128), (600, 64, 300)]
VARIANTS = [(res, drop) for res in (False, True) for drop in (0.0, 0.2)]       # ReLU always (the mask exists behind a ReLU only)
EPS, MOM, SEED, RNG_STREAM = 1e-5, 0.1, 1234567, 3


@pytest.fixture(autouse=True)
def _default_conv_precision():
    HF.set_conv_precision(None)
    yield
    HF.set_conv_precision(None)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def pack_mask(y):
    """host reference: y [P][C] -> uint32 [C / 32][P]"""
    P, C = y.shape
    b = (y > 0).reshape(P, C // 32, 32).astype(np.uint64)
    return np.ascontiguousarray((b << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32).T)


def host_partials(x, parts, rows):
    """[rows][parts][C] partials over row blocks of x [P][C]: rows = 3: (n, mean, M2); rows = 2: (sum, sum of squares) - any finite values do for a bitwise A/B"""
    P, C = x.shape
    out = np.zeros((rows, parts, C), np.float32)
    for i, idx in enumerate(np.array_split(np.arange(P), parts)):
        blk = x[idx].astype(np.float64)
        if rows == 3:
            out[0, i], out[1, i], out[2, i] = len(idx), blk.mean(0), ((blk - blk.mean(0)) ** 2).sum(0)
        else:
            out[0, i], out[1, i] = blk.sum(0), (blk * blk).sum(0) * 0.25
    return out


def stats_buffer(part, C):
    rows, parts = part.shape[:2]
    buf = torch.zeros(int(HF.query('dsrl_bn_stats_floats', rows, parts, C)), device=DEV)
    buf[:part.size] = torch.from_numpy(part.reshape(-1)).to(DEV)
    return buf


_fwd_cache = {}


def forward_pair(shape, variant):
    """(inputs, outputs without mask, outputs with mask) of the from-statistics forward; computed once per case and shared by the tests, never modified"""
    key = (shape, variant)
    if key in _fwd_cache:
        return _fwd_cache[key]
    (P, C, parts), (res, drop) = shape, variant
    rs = np.random.RandomState(P + C + parts)
    x = rs.standard_normal((P, C)).astype(np.float32)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(np.float32), (rs.standard_normal(C) * 0.3).astype(np.float32)
    gamma[5], beta[5] = 0.0, 0.0                    # channel 5: y = fma(x, 0, 0 - mean * 0) is exactly (+-)0 before the residual
    r = rs.standard_normal((P, C)).astype(np.float32)
    r[::3, 5] = 0.0                                 # ... and stays exactly 0 in a third of the rows with a residual
    part = host_partials(x, parts, 3)               # statistics of the clean tensor
    x[P // 2, 9] = np.nan                           # one NaN: the ReLU's fmaxf stores 0 for it, bit clear
    xt, rt, gt, bt = dev(x), dev(r), dev(gamma), dev(beta)
    outs = []
    st = torch.cuda.current_stream().cuda_stream
    for with_mask in (False, True):
        y = torch.full((P, C), 7.0, device=DEV)
        mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        amax = torch.zeros(HF.AMAX_WORDS, dtype=torch.int32, device=DEV)
        stats = stats_buffer(part, C)
        words = int(HF.query('dsrl_bn_mask_words', P, C))
        assert words == (C // 32) * P
        mask = torch.full((words + 8,), -1, dtype=torch.int32, device=DEV)       # 8 guard words behind the mask
        args = (xt.data_ptr(), C, y.data_ptr(), C, P, C, EPS, MOM, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), gt.data_ptr(), bt.data_ptr(),
                rt.data_ptr() if res else None, C, 1, drop, SEED, RNG_STREAM, stats.data_ptr(), parts, amax.data_ptr())
        if with_mask:
            HF.call('dsrl_bn_train_fwd_from_stats_mask', *args, mask.data_ptr(), st)
        else:
            HF.call('dsrl_bn_train_fwd_from_stats', *args, st)
        torch.cuda.synchronize()
        outs.append(dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, amax=amax, mask=mask))
    _fwd_cache[key] = (dict(x=xt, r=rt, gamma=gt, x_host=x), outs[0], outs[1])
    return _fwd_cache[key]


@gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_with_mask_leaves_the_same_outputs_and_the_sign_bits_of_y(shape, variant):
    P, C, parts = shape
    _, plain, masked = forward_pair(shape, variant)
    for k in ('y', 'mean', 'invstd', 'rm', 'rv', 'amax'):
        assert same(plain[k], masked[k]), k
    y = masked['y'].cpu().numpy()
    assert not (y[P // 2, 9] > 0) and (y != 7.0).all()
    assert (y[::3, 5] == 0).all() and (y == 0).sum() > P           # exact zeros: channel 5, and what the ReLU (and the Dropout) cleared
    got = masked['mask'].cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:(C // 32) * P].reshape(C // 32, P), pack_mask(y))
    assert (got[(C // 32) * P:] == 0xffffffff).all()               # nothing behind the mask was touched
    assert (plain['mask'].cpu().numpy() == -1).all()               # and the plain entry point writes none


@gpu
@pytest.mark.parametrize('training', [0, 1])
@pytest.mark.parametrize('with_dres', [False, True])
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES)
def test_bn_backward_from_the_mask_is_bit_identical_to_backward_from_y(shape, variant, with_dres, training):
    """dsrl_bn_bwd_from_stats_drop, and dsrl_bn_bwd_from_stats_res (it needs dres), with relu = 2 and the mask against relu = 1 and y"""
    (P, C, parts), (res, drop) = shape, variant
    inp, _, fwd = forward_pair(shape, variant)
    rs = np.random.RandomState(P * 3 + C)
    dy = dev(rs.standard_normal((P, C)).astype(np.float32))
    x2 = dev((rs.standard_normal((P, C)) * 2 + 0.5).astype(np.float32))
    mean2, invstd2 = dev(rs.standard_normal(C).astype(np.float32)), dev(rs.uniform(0.5, 2, C).astype(np.float32))
    part = host_partials(np.nan_to_num(inp['x_host']) * 0.1, parts, 2)
    st = torch.cuda.current_stream().cuda_stream
    names = ['dsrl_bn_bwd_from_stats_drop'] + (['dsrl_bn_bwd_from_stats_res'] if with_dres else [])
    for name in names:
        rparts = int(HF.query('dsrl_bn_bwd_from_stats_res_parts', P, C, parts))
        assert rparts > 0
        got = []
        for mode in (1, 2):
            dx, dres = torch.full((P, C), 7.0, device=DEV), torch.full((P, C), 7.0, device=DEV)
            dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            amax = torch.zeros(HF.AMAX_WORDS, dtype=torch.int32, device=DEV)
            stats = stats_buffer(part, C)
            rst = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 2, rparts, C)), device=DEV)
            ym = (fwd['y'].data_ptr(), C) if mode == 1 else (fwd['mask'].data_ptr(), P)
            extra = (x2.data_ptr(), C, mean2.data_ptr(), invstd2.data_ptr(), rst.data_ptr(), rparts) if name.endswith('_res') else ()
            HF.call(name, inp['x'].data_ptr(), C, ym[0], ym[1], dy.data_ptr(), C, dx.data_ptr(), C, dres.data_ptr() if with_dres else None, C, P, C,
                    fwd['mean'].data_ptr(), fwd['invstd'].data_ptr(), inp['gamma'].data_ptr(), dg.data_ptr(), db.data_ptr(), mode, drop, training,
                    stats.data_ptr(), parts, amax.data_ptr(), *extra, st)
            torch.cuda.synchronize()
            got.append(dict(dx=dx, dres=dres, dgamma=dg, dbeta=db, dx_amax=amax, res_partials=rst))
        for k in got[0]:
            assert same(got[0][k], got[1][k]), (name, k)
        assert (got[1]['dx'] != 7.0).any() and (not with_dres or (got[1]['dres'] == 0).any())


def _dgrad_pair(shp, entry, accumulate, drop, planes, rs, want_parts=None):
    """dx and the BatchNorm-backward partials of one data-gradient launch with bn_relu = 1 (y) and = 2 (its sign mask)"""
    N, H, W, C, K, R, S, stride, pad, dil = shp
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    P = N * H * W
    w = dev((rs.standard_normal((K, C, R, S)) / np.sqrt(C * R * S)).astype(np.float32))
    dy = dev(rs.standard_normal((N, K, Ho, Wo)).astype(np.float32))
    by = np.maximum(rs.standard_normal((P, C)), 0).astype(np.float32)
    by[3, 7] = np.nan
    bx, byt = dev(rs.standard_normal((P, C)).astype(np.float32)), dev(by)
    mask = torch.from_numpy(pack_mask(by).view(np.int32)).to(DEV)
    mean, invstd = dev(rs.standard_normal(C).astype(np.float32) * 0.1), dev((1.0 + rs.rand(C)).astype(np.float32))
    dx0 = dev(rs.standard_normal((N, C, H, W)).astype(np.float32))
    parts = int(HF.query('dsrl_conv2d_dgrad_stats_parts', *shp))
    assert parts > 0, 'this launch cannot leave BatchNorm sums: the case tests nothing'
    assert want_parts is None or parts == want_parts, ('the forced tile plan was not taken', parts, want_parts)
    ws = torch.empty(int(HF.query('dsrl_conv2d_dgrad_workspace_bytes', *shp)) + 256, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p_ = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    rec = wtsp = dya = dyp = wtp = None
    if entry != 'dsrl_conv2d_dgrad_bnstats':
        rec, _, wtsp, _ = HF.split_filter(w)
        dya = HF.amax_for(dy)
        if planes:
            _, wtp = HF.filter_planes(w, rec)
            dyp = HF.planes_of(dy, K, dya)
    got = []
    for mode in (1, 2):
        dx = dx0.clone()
        bst = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 2, parts, C)), device=DEV)
        ym = (byt.data_ptr(), C) if mode == 1 else (mask.data_ptr(), P)
        bn = (bx.data_ptr(), C, ym[0], ym[1], mean.data_ptr(), invstd.data_ptr(), mode)
        tail = (bst.data_ptr(), parts, int(accumulate), st)
        if entry == 'dsrl_conv2d_dgrad_bnstats':
            HF.call(entry, dy.data_ptr(), K, w.data_ptr(), None, dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(), *bn, *tail)
        elif entry == 'dsrl_conv2d_dgrad_amax':
            HF.call(entry, dy.data_ptr(), K, p_(dya), w.data_ptr(), None, p_(rec), p_(wtsp), dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(), *bn, *tail)
        else:
            dropa = (drop,) if entry.endswith('_drop') else ()
            HF.call(entry, dy.data_ptr(), K, p_(dya), p_(dyp), w.data_ptr(), None, p_(rec), p_(wtsp), p_(wtp), dx.data_ptr(), C, *shp, ws.data_ptr(), ws.numel(),
                    *bn, *dropa, *tail)
        torch.cuda.synchronize()
        got.append((dx, bst))
    assert same(got[0][0], got[1][0]), 'dx'
    assert same(got[0][1], got[1][1]), 'BatchNorm-backward partials'
    assert (got[1][1][:2 * parts * C] != 0).any()
    assert accumulate or not same(got[1][0], dx0)


BASE = (1, 9, 13, 64, 48, 3, 3, 1, 1, 1)            # N, H, W, C, K, R, S, stride, pad, dil: 3x3 pad 1, dy has 48 channels, dx 64; M = 117 (ragged tile)
S2 = (2, 8, 128, 64, 96, 1, 1, 2, 0, 1)             # 1x1 stride 2: intended path = rows in parity order (W / 2 = 64 pixels per class row), the epilogue's 4-byte path
DGRAD_CASES = [
    # shape, entry point, accumulate, dropout p, forced (tile configuration, K groups), plane operands
    (BASE, 'dsrl_conv2d_dgrad_bnstats', 0, 0.0, None, False),
    (BASE, 'dsrl_conv2d_dgrad_amax', 0, 0.0, None, False),
    (BASE, 'dsrl_conv2d_dgrad_planes', 0, 0.0, None, False),
    (BASE, 'dsrl_conv2d_dgrad_planes_drop', 0, 0.2, None, False),
    (BASE, 'dsrl_conv2d_dgrad_amax', 1, 0.0, None, False),
    (BASE, 'dsrl_conv2d_dgrad_planes_drop', 1, 0.2, None, False),
    # forced plans: the tile is asserted through the number of partials; K groups and plane operands are the INTENDED path (the library has no query for them)
    (BASE, 'dsrl_conv2d_dgrad_amax', 0, 0.0, (0, 2), False),           # intended: two K groups, the 4-byte epilogue, shares through LDS
    (BASE, 'dsrl_conv2d_dgrad_bnstats', 1, 0.0, (0, 2), False),
    (S2, 'dsrl_conv2d_dgrad_amax', 0, 0.0, None, False),
    (S2, 'dsrl_conv2d_dgrad_bnstats', 1, 0.0, None, False),
    (BASE, 'dsrl_conv2d_dgrad_planes_drop', 0, 0.2, (3, 1), True),     # intended: conv_planes_kernel, 16-byte epilogue
    (BASE, 'dsrl_conv2d_dgrad_planes_drop', 1, 0.2, (3, 2), True),     # intended: conv_planes_kernel, two K groups
    (BASE, 'dsrl_conv2d_dgrad_planes', 0, 0.0, (3, 1), True),
]


@gpu
@pytest.mark.parametrize('shp,entry,accumulate,drop,forced,planes', DGRAD_CASES)
def test_dgrad_epilogue_sums_from_the_mask_are_bit_identical_to_sums_from_y(shp, entry, accumulate, drop, forced, planes, monkeypatch):
    monkeypatch.setenv('DSRL_PLANES', '1')
    monkeypatch.setenv('DSRL_DGRAD_PARITY', '1')
    if forced is not None:
        monkeypatch.setenv('DSRL_FORCE_CFG', str(forced[0]))
        monkeypatch.setenv('DSRL_FORCE_KG', str(forced[1]))
    HF._query_cache.clear()
    try:
        # partials = M tiles x wave rows of the tile: BASE (M = 117) leaves 2 on the forced 128x128 tile and 4 on the forced 64x64 tile
        want = None if forced is None else {0: 2, 3: 4}[forced[0]]
        _dgrad_pair(shp, entry, accumulate, drop, planes, np.random.RandomState(sum(shp) + accumulate), want)
    finally:
        HF._query_cache.clear()


@gpu
def test_mode_2_arguments_are_checked():
    """a mask row shorter than the tensor, C that is no multiple of 32 and a mask without ReLU semantics are refused before any launch"""
    P, C = 64, 32
    t = torch.zeros((P, C), device=DEV)
    v = torch.ones(C, device=DEV)
    mask = torch.zeros(P, dtype=torch.int32, device=DEV)
    stats = torch.zeros(int(HF.query('dsrl_bn_stats_floats', 2, 1, C)), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(HF.DsrlHipError):
        HF.call('dsrl_bn_bwd_from_stats_drop', t.data_ptr(), C, mask.data_ptr(), P - 1, t.data_ptr(), C, t.data_ptr(), C, None, C, P, C, v.data_ptr(), v.data_ptr(), v.data_ptr(),
                v.data_ptr(), v.data_ptr(), 2, 0.0, 1, stats.data_ptr(), 1, None, st)
    with pytest.raises(HF.DsrlHipError):
        HF.call('dsrl_bn_bwd_from_stats_drop', t.data_ptr(), C, mask.data_ptr(), P, t.data_ptr(), C, t.data_ptr(), C, None, C, P, C, v.data_ptr(), v.data_ptr(), v.data_ptr(),
                v.data_ptr(), v.data_ptr(), 3, 0.0, 1, stats.data_ptr(), 1, None, st)


@gpu
def test_whole_model_gradients_identical_with_and_without_the_mask(monkeypatch):
    """DSRL stage 3, B = 2 at 32x64, dropout on with a fixed key: every parameter gradient and the four outputs with HF.bn_mask_enabled on and off, bit for
    bit - and the from-statistics backward launches and the linked data gradients did take the mask (relu == 2)."""
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    torch.manual_seed(5)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    rs = np.random.RandomState(2)
    x = dev(rs.standard_normal((2, 3, 32, 64)).astype(np.float32), cl=False)
    tg = dev(rs.randint(0, 19, (2, 64, 128)).astype(np.uint8))
    org = dev(rs.standard_normal((2, 3, 64, 128)).astype(np.float32))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads, outs_, counts = {}, {}, {}
    orig = HF.call
    for on in (True, False):
        monkeypatch.setattr(HF, 'bn_mask_enabled', on)
        model.load_state_dict(state)
        for p_ in model.parameters():
            p_.grad = None
        HF.set_dropout_seed(77)
        c = counts[on] = {'fwd_mask': 0, 'bwd': 0, 'bwd2': 0, 'dgrad': 0, 'dgrad2': 0}

        def counting(name, *a, _c=c, _o=orig):
            if name == 'dsrl_bn_train_fwd_from_stats_mask' and a[-2] is not None:
                _c['fwd_mask'] += 1
            if name in ('dsrl_bn_bwd_from_stats_drop', 'dsrl_bn_bwd_from_stats_res'):
                _c['bwd'] += 1
                _c['bwd2'] += a[17] == 2                # relu
            if name == 'dsrl_conv2d_dgrad_planes_drop' and a[31] is not None:       # bstats: a linked data gradient
                _c['dgrad'] += 1
                _c['dgrad2'] += a[29] == 2              # bn_relu
            return _o(name, *a)
        monkeypatch.setattr(HF, 'call', counting)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        outs = model(x)
        vals = HF.fused_losses(outs, tg, org, 255, 0.1, 1.0, 3, flag)
        vals[3].backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(HF, 'call', orig)
        grads[on] = {k: p_.grad.clone() for k, p_ in model.named_parameters() if p_.grad is not None}
        outs_[on] = [o.detach().clone() for o in outs]
    assert counts[False]['fwd_mask'] == 0 and counts[False]['bwd2'] == 0 and counts[False]['dgrad2'] == 0, counts[False]
    c = counts[True]
    # bn1 / bn2 of the 33 bottlenecks alone are 66 BatchNorms with ReLU whose output feeds one conv: a run in which the from-statistics backward launches
    # and the linked data gradients did not take the mask (relu == 2) fails here, however equal its gradients are
    print('mask launches', c)
    assert c['fwd_mask'] >= 60 and c['bwd2'] >= 60 and c['dgrad2'] >= 60, c
    assert len(outs_[True]) == 4 and all(same(a, b) for a, b in zip(outs_[True], outs_[False]))
    assert grads[True].keys() == grads[False].keys() and len(grads[True]) > 300
    bad = [k for k in grads[True] if not same(grads[True][k], grads[False][k])]
    assert not bad, bad[:5]


def test_mask_size_query():
    """host side: (C / 32) * P words, and none for a channel count the mask cannot describe; depends on nothing but the shape"""
    assert HF.query('dsrl_bn_mask_words', 4096, 48) == 0
    assert HF.query('dsrl_bn_mask_words', 4096, 256) == 8 * 4096 and HF.query('dsrl_bn_mask_words', 70, 32) == 70
    assert HF.query('dsrl_bn_mask_words', 0, 32) == 0

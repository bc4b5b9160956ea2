"""The four cross-entropy paths of the training step at the edges of a softmax over fp32 logits, each against an INDEPENDENT reference:
torch.nn.functional.cross_entropy(ignore_index, 'mean') in float64 on CPU, fed the same fp32 values, gradient from CPU autograd.

    A  dsrl_ce_fwd / dsrl_ce_bwd        HF.cross_entropy (+ autograd)
    B  dsrl_ce_fused                    the loss pass of HF.fused_losses (value, gradient, NaN flag)
    C  dsrl_convt2x2_fwd_ce             the CE value evaluated inside the last ConvTranspose forward (HF.logits_target)
    D  dsrl_convt2x2_bwd_ce             d(CE)/d(logits) formed inside the ConvTranspose backward (HF.LogitsGrad), both builds

Edges: -inf logits (one class, a whole class, the target), a spread that overflows v - m, large common offsets, equal logits, near one-hot
pixels, +inf / NaN logits, ignore indices other than 255 (and one no uint8 label matches), ragged pixel counts, label buffers that start
off a 16-byte boundary, labels outside [0, C).  Then the hand-over of the CE gradient when the logits have a second consumer.

Tolerances (fixed, stated where they are used):
    loss       |L - ref| <= 1e-6 |ref| + 2 ulp of the largest |max logit| m of a live pixel (a pixel's m + log s - v rounds at ulp(m): with a common
               offset, or a small loss, that term is the larger one)
    gradient   |g - ref| <= 2^-20 * scale per element, scale = 1 / (pixels that count); ignored pixels exactly 0
    D          dx, dw, db against the fp64 gradient pushed through the fp64 ConvTranspose backward: 1e-5 of the range (check())
    exp sweep  4 ulp where the fp64 value is >= 2^-120, 2^-120 absolute below
B and D are also held bit for bit to each other (dsrl_ce_fused -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd against the one call)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gen                     # noqa: E402
import oracle as O             # noqa: E402
from hip_helpers import DEV, HF, check, dev, host, make_head   # noqa: E402

GRAD_TOL = 2.0 ** -20          # x scale, per gradient element
LOSS_REL = 1e-6
M_ULPS = 2

CASES = ['randn', 'neginf_some', 'neginf_class', 'neginf_target', 'spread', 'offset_1e4', 'offset_1e6', 'equal', 'onehot',
         'posinf_live', 'nan_live', 'nan_ignored', 'bad_label']
NAN_CASES = {'posinf_live': 1, 'nan_live': 1, 'bad_label': 2}          # -> NaN loss; the flag bit of B and C
IGNORES = [0, 18, 254, 255, -1, 300]


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def make_case(case, P, C, rs, ii=255):
    """-> logits (P, C) float32, labels (P,) uint8.  Labels in [0, C), 10 % set to ii when a uint8 can hold it."""
    lg = (rs.standard_normal((P, C)) * 3).astype(np.float32)
    tg = rs.randint(0, C, P).astype(np.int64)
    if 0 <= ii <= 255 and P > 1:
        tg[rs.uniform(size=P) < 0.1] = ii
    live = tg != ii
    some = rs.uniform(size=P) < 0.1
    if case == 'neginf_some':                   # -inf in a class other than the target
        idx = np.where(some)[0]
        lg[idx, (np.where(tg[idx] < C, tg[idx], 0) + 1) % C] = -np.inf
    elif case == 'neginf_class':                # a whole class -inf, never a target
        lg[:, 1 % C] = -np.inf
        tg[live & (tg == 1 % C)] = 0 if C > 1 else tg[live & (tg == 1 % C)]
    elif case == 'neginf_target':               # the target class -inf: loss +inf, finite gradient
        idx = np.where(some & live)[0]
        lg[idx, tg[idx]] = -np.inf
    elif case == 'spread':                      # +3e38 and -3e38 in one pixel: v - m overflows to -inf (the target is never the -3e38 class:
        idx = np.where(some)[0]                 # its fp32 pixel loss 6e38 would overflow, the fp64 reference's would not)
        a = rs.randint(0, C, idx.size); b = (a + 1) % C
        lg[idx, a] = 3e38; lg[idx, b] = -3e38
        bad = live[idx] & (tg[idx] == b)
        tg[idx[bad]] = a[bad]
    elif case in ('offset_1e4', 'offset_1e6'):
        lg = (float(case[-3:]) + rs.standard_normal((P, C)) * 3).astype(np.float32)
    elif case == 'equal':
        lg = np.repeat((rs.standard_normal((P, 1)) * 10).astype(np.float32), C, axis=1)
    elif case == 'onehot':
        lg = np.full((P, C), -100, np.float32)
        lg[np.arange(P), rs.randint(0, C, P)] = 100
    elif case == 'posinf_live':
        j = int(np.where(live)[0][0]) if live.any() else 0
        lg[j, 0] = np.inf
    elif case == 'nan_live':
        j = int(np.where(live)[0][0]) if live.any() else 0
        lg[j, C - 1] = np.nan
    elif case == 'nan_ignored':                 # NaN in a pixel the loss ignores: the flag still rises (the reference's NaN assert on the outputs)
        tg[0] = ii
        lg[0, 0] = np.nan
    elif case == 'bad_label':                   # labels outside [0, C) that are not the ignore index
        j = np.where(live)[0]
        tg[j[0]] = C
        if j.size > 1 and ii != 254:
            tg[j[1]] = 254
    return lg, tg.astype(np.uint8)


def reference(lg, tg, ii):
    """-> (loss, gradient (P, C), count): torch CPU float64 on the same fp32 values."""
    x = torch.tensor(lg.astype(np.float64), requires_grad=True)
    t = torch.tensor(tg.astype(np.int64))
    loss = F.cross_entropy(x, t, ignore_index=ii, reduction='mean')
    loss.backward()
    return float(loss), x.grad.numpy(), int((t != ii).sum())


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def check_loss(L, ref, lg, tg, ii, case):
    """m: the largest |max logit| of a live pixel (finite wherever the reference loss is)"""
    if math.isinf(ref):
        assert L == ref, (L, ref)
        return
    live = tg.astype(np.int64) != ii
    tol = LOSS_REL * abs(ref) + M_ULPS * ulp32(float(np.abs(lg[live].max(axis=1)).max()))
    assert abs(L - ref) <= tol, f'{case}: loss {L!r} vs {ref!r} (|d| = {abs(L - ref):.3e} > {tol:.3e})'


def check_grad(g, gref, tg, ii, count, case):
    live = tg.astype(np.int64) != ii
    assert np.all(g[~live] == 0), f'{case}: nonzero gradient on an ignored pixel'
    err = np.abs(g[live].astype(np.float64) - gref[live])
    bound = GRAD_TOL / count
    assert not np.isnan(err).any(), f'{case}: NaN in the gradient of a live pixel'
    assert err.max(initial=0.0) <= bound, f'{case}: gradient error {err.max():.3e} > {bound:.3e} (2^-20 / {count})'


def flag_bits(case):
    return {'nan_ignored': 1}.get(case, NAN_CASES.get(case, 0))


# ------------------------------------------------------------------------------------------------------------------------------ path A
def run_A(lg, tg, ii, layout='dense', tgt=None):
    P, C = lg.shape
    pad = 5 if layout == 'slice' else 0
    base = torch.full((1, 1, P, C + pad), 7.0, device=DEV)
    base[..., 2 if pad else 0:(2 if pad else 0) + C] = torch.tensor(lg, device=DEV).view(1, 1, P, C)
    base.requires_grad_(True)
    view = base[..., 2:2 + C] if pad else base
    target = torch.tensor(tg, device=DEV).view(1, 1, P) if tgt is None else tgt.view(1, 1, P)
    loss = HF.cross_entropy(view.permute(0, 3, 1, 2), target, ii)          # (1, C, 1, P) pixel-major, ld = C (+ 5)
    loss.backward()
    torch.cuda.synchronize()
    g = host(base.grad)[0, 0]
    if pad:
        assert np.all(g[:, :2] == 0) and np.all(g[:, 2 + C:] == 0)
        g = g[:, 2:2 + C]
    return float(loss), g


@pytest.mark.parametrize('C', [2, 3, 19])
@pytest.mark.parametrize('case', CASES)
def test_path_A_cross_entropy_edges(case, C):
    rs = np.random.RandomState(100 * C + CASES.index(case))
    lg, tg = make_case(case, 4099, C, rs)
    L, g = run_A(lg, tg, 255, layout='slice' if C == 3 else 'dense')
    if case in NAN_CASES:                       # A has no flag: the loss itself is NaN; for a bad label the pixel's gradient row too
        assert np.isnan(L), L
        if case == 'bad_label':
            bad = (tg != 255) & (tg >= C)
            assert np.isnan(g[bad]).all() and not np.isnan(g[~bad]).any()
        return
    ref, gref, count = reference(lg, tg, 255)
    check_loss(L, ref, lg, tg, 255, case)       # nan_ignored: finite, as torch
    check_grad(g, gref, tg, 255, count, case)
    if np.isfinite(lg).all():                   # the numpy oracle agrees where every logit is finite
        assert abs(O.cross_entropy(lg.astype(np.float64), tg, 255) - ref) <= 1e-12 * max(1.0, abs(ref))


# ------------------------------------------------------------------------------------------------------------------------------ path B
def run_B(lg, tg, ii, layout='dense', tgt=None):
    """dsrl_ce_fused.  layout: 'dense' (ld = lddl = C: the float4 loads and stores), 'slice' (the logits a channel slice of a wider tensor,
    ld = C + 5, 8 bytes past the base: scalar loads), 'lddl' (slice + a gradient buffer with lddl = C + 3: scalar stores), 'nodl' (no
    gradient buffer).  -> (loss, count, flag, gradient (P, C) or None)"""
    call, query = _lib()
    P, C = lg.shape
    if layout in ('slice', 'lddl'):
        buf = torch.full((P, C + 5), 7.0, device=DEV); buf[:, 2:2 + C] = torch.tensor(lg, device=DEV)
        ptr, ld = buf.data_ptr() + 8, C + 5
    else:
        buf = torch.tensor(lg, device=DEV); ptr, ld = buf.data_ptr(), C
    lddl = C + 3 if layout == 'lddl' else C
    dl = None if layout == 'nodl' else torch.full((P, lddl), 7.0, device=DEV)
    target = torch.tensor(tg, device=DEV) if tgt is None else tgt
    scal = torch.full((8,), 7.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(query('dsrl_ce_fused_workspace_bytes', P), dtype=torch.uint8, device=DEV)
    call('dsrl_ce_fused', ptr, ld, target.data_ptr(), P, C, ii, None if dl is None else dl.data_ptr(), lddl, scal.data_ptr(), flag.data_ptr(),
         ws.data_ptr(), ws.numel(), HF._stream())
    torch.cuda.synchronize()
    s = host(scal)
    g = None
    if dl is not None:
        g = host(dl)
        if lddl > C:
            assert np.all(g[:, C:] == 7.0), 'wrote past the C gradient columns'
            g = g[:, :C]
    return float(s[0]), float(s[1]), int(flag), g


@pytest.mark.parametrize('layout', ['dense', 'slice', 'lddl', 'nodl'])
@pytest.mark.parametrize('C', [2, 3, 19])
@pytest.mark.parametrize('case', CASES)
def test_path_B_fused_cross_entropy_edges(case, C, layout):
    rs = np.random.RandomState(100 * C + CASES.index(case))
    lg, tg = make_case(case, 4099, C, rs)
    L, n, fl, g = run_B(lg, tg, 255, layout)
    assert fl == flag_bits(case), (case, fl)
    assert n == float((tg != 255).sum())
    if case in NAN_CASES:
        assert np.isnan(L), L
        return
    ref, gref, count = reference(lg, tg, 255)
    check_loss(L, ref, lg, tg, 255, case)
    if g is not None:
        check_grad(g, gref, tg, 255, count, case)


# ------------------------------------------------------------------------------------------------------------------------------ A and B: ignore indices, sizes, label alignment
SIZES = [(1, 0), (1, 9), (17, 3), (259, 15), (4111, 1), (4111, 8), (300007, 7)]


@pytest.mark.parametrize('ii,P,off,pattern', [(ii, P, off, pat) for ii in IGNORES for P, off in SIZES for pat in ('mixed', 'one_live')
                                              if pat == 'mixed' or 0 <= ii <= 255])
def test_ignore_index_sizes_and_unaligned_labels(ii, P, off, pattern):
    # P not a multiple of 16 or 256, P = 1, more pixels than one grid of the loss kernel walks (300007 > 1024 x 256); the labels a view that starts
    # `off` bytes past a 16-byte boundary (the head and tail loops of count_valid_kernel); ignore indices that are a class (0, 18), 254, 255 and two
    # that no uint8 label can match.  'one_live': every pixel ignored but one (ignore indices a label can hold).  The exact count comes back in scal[1].
    C = 19
    rs = np.random.RandomState(P + off + (ii & 0xffff))
    lg, tg = make_case('randn', P, C, rs, ii)
    if pattern == 'one_live':
        tg[:] = ii; tg[rs.randint(P)] = (ii + 1) % C
    big = torch.zeros(P + 64, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    tgt = big[off:off + P]
    tgt.copy_(torch.tensor(tg, device=DEV))
    ref, gref, count = reference(lg, tg, ii)
    assert count == int((tg.astype(np.int64) != ii).sum())
    L, n, fl, g = run_B(lg, tg, ii, 'dense', tgt)
    assert n == float(count) and fl == 0
    check_loss(L, ref, lg, tg, ii, 'randn')
    check_grad(g, gref, tg, ii, count, 'B')
    La, ga = run_A(lg, tg, ii, tgt=tgt)
    check_loss(La, ref, lg, tg, ii, 'randn')
    check_grad(ga, gref, tg, ii, count, 'A')


def test_all_pixels_ignored_is_nan_and_writes_zero_gradient():
    lg, tg = make_case('randn', 300, 19, np.random.RandomState(3))
    tg[:] = 255
    L, n, fl, g = run_B(lg, tg, 255, 'dense')
    assert np.isnan(L) and n == 0.0 and fl == 0 and np.all(g == 0)
    La, ga = run_A(lg, tg, 255)
    assert np.isnan(La)


# ------------------------------------------------------------------------------------------------------------------------------ exp_nonpos
def test_exp_nonpos_accuracy_sweep_through_the_fused_loss():
    # common.h claims exp_nonpos is within 2 ulp of expf on [-87, 0] and 0 below.  Rows [0, x] with target 0: d(CE)/d(v_1) = scale e^x / (1 + e^x),
    # scale = 2^-17 exactly (2^17 rows, none ignored).  ~10^5 fp32 values in [-110, 0]: the integers, 2000 neighbours of -87.34 (expf's last
    # normal results) and of -103.3 (the last subnormal ones), the rest spread evenly.
    P = 1 << 17
    xs = [np.arange(-110, 1, dtype=np.float32)]
    for c in (-87.34, -103.3):
        xs.append(np.float32(c) + np.arange(-1000, 1000, dtype=np.float32) * np.float32(2.0 ** -17))
    xs.append(np.float32(0.0)); xs.append(np.float32(-1e-30))
    head = np.concatenate([np.atleast_1d(a) for a in xs]).astype(np.float32)
    rest = np.linspace(-110, 0, P - head.size).astype(np.float32)
    x = np.concatenate([head, rest])
    assert x.size == P and x.max() <= 0
    lg = np.stack([np.zeros(P, np.float32), x], axis=1)
    tg = np.zeros(P, np.uint8)
    L, n, fl, g = run_B(lg, tg, 255, 'dense')
    assert n == P and fl == 0 and not np.isnan(g).any()
    x64 = x.astype(np.float64)
    ref = 2.0 ** -17 * np.exp(x64) / (1 + np.exp(x64))
    d = np.abs(g[:, 1].astype(np.float64) - ref)
    hi = ref >= 2.0 ** -120
    ulps = d[hi] / np.spacing(ref[hi].astype(np.float32)).astype(np.float64)
    assert ulps.max() <= 4, f'{ulps.max():.2f} ulp at x = {x[hi][np.argmax(ulps)]!r}'
    assert d[~hi].max(initial=0) <= 2.0 ** -120
    assert hi.sum() > P // 2 and (~hi).sum() > 1000


# ------------------------------------------------------------------------------------------------------------------------------ path C
C_CASES = ['randn', 'neginf_class', 'neginf_target', 'spread', 'offset_1e4', 'offset_1e6', 'equal', 'onehot', 'posinf_live', 'nan_live',
           'nan_ignored', 'bad_label']


@pytest.mark.parametrize('case,ii', [(c, 255) for c in C_CASES] + [(c, ii) for c in ('randn', 'spread', 'neginf_target') for ii in (0, 18, 254, -1)])
def test_path_C_cross_entropy_value_inside_the_convT_forward(case, ii, monkeypatch):
    # The logits come out of the conv (N = 1, 3 x 200 -> 6 x 400: a ragged 72-pixel segment); the edge values enter through the bias.  Every case with
    # ignore index 255, three with the others.
    call, query = _lib()
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    N, H, W, C = 1, 3, 200, 19
    P = N * 4 * H * W
    rs = np.random.RandomState(C_CASES.index(case) + 7 * (ii & 0xff))
    x = (rs.standard_normal((N, H, W, C)) * 0.5).astype(np.float32)
    w = (rs.standard_normal((C, C, 2, 2)) * 0.5).astype(np.float32)
    b = rs.standard_normal(C).astype(np.float32)
    tg = rs.randint(0, C, (N, 2 * H, 2 * W)).astype(np.int64)
    if 0 <= ii <= 255:
        tg[rs.uniform(size=tg.shape) < 0.1] = ii
    live = tg != ii
    if case == 'neginf_class':
        b[1] = -np.inf; tg[live & (tg == 1)] = 0
    elif case == 'neginf_target':
        b[1] = -np.inf
    elif case == 'spread':
        b[3] = 3e38; b[4] = -3e38; tg[live & (tg == 4)] = 3
    elif case.startswith('offset'):
        b += np.float32(float(case[-3:]))
    elif case == 'equal':
        w[:] = 0; b[:] = 5.0
    elif case == 'onehot':
        w[:] = 0; b[:] = -100; b[4] = 100
    elif case == 'posinf_live':
        b[3] = np.inf
    elif case == 'nan_live':
        x[0, 1, 7, 2] = np.nan
    elif case == 'nan_ignored':
        x[0, 1, 7, 2] = np.nan; tg[0, 2:4, 14:16] = ii          # the four outputs of that input pixel
    elif case == 'bad_label':
        tg[0, 0, 1] = 200 if ii != 200 else 201
    tg = tg.astype(np.uint8)
    xt = torch.tensor(x, device=DEV); wt = torch.tensor(w, device=DEV); bt = torch.tensor(b, device=DEV); target = torch.tensor(tg, device=DEV)
    assert query('dsrl_convt2x2_fwd_ce_supported', xt.data_ptr(), xt.data_ptr(), N, H, W, C, C) == 1
    ws = torch.empty(query('dsrl_convt2x2_fwd_ce_workspace_bytes', N, H, W), dtype=torch.uint8, device=DEV)
    st = HF._stream()
    y0 = torch.empty((N, 2 * H, 2 * W, C), device=DEV); y1 = torch.full_like(y0, 7.0)
    s1 = torch.full((8,), 7.0, device=DEV); f1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    call('dsrl_convt2x2_fwd', xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y0.data_ptr(), N, H, W, C, C, st)
    call('dsrl_convt2x2_fwd_ce', xt.data_ptr(), wt.data_ptr(), bt.data_ptr(), y1.data_ptr(), N, H, W, C, C, target.data_ptr(), ii, s1.data_ptr(),
         f1.data_ptr(), ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))          # the logits themselves, bit for bit (NaN patterns included)
    lg = host(y1).reshape(P, C)
    L, n, fl = float(host(s1)[0]), float(host(s1)[1]), int(f1)
    assert fl == flag_bits(case), (case, fl)
    assert n == float((tg.astype(np.int64) != ii).sum())
    LB, nB, flB, _ = run_B(lg, tg.reshape(P), ii, 'nodl')                  # path B on the same logits: same count and flag
    assert nB == n and flB == fl
    if case in NAN_CASES:
        assert np.isnan(L) and np.isnan(LB)
        return
    ref, _, _ = reference(lg, tg.reshape(P), ii)
    check_loss(L, ref, lg, tg.reshape(P), ii, case)
    check_loss(LB, ref, lg, tg.reshape(P), ii, case)


# ------------------------------------------------------------------------------------------------------------------------------ path D
D_CASES = ['randn', 'neginf_some', 'neginf_class', 'neginf_target', 'spread', 'offset_1e4', 'offset_1e6', 'equal', 'onehot', 'bad_label']


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('ft', [8, 0])
@pytest.mark.parametrize('waves', [None, '8'])
@pytest.mark.parametrize('case,ii', [(c, 255) for c in D_CASES] + [(c, ii) for c in ('randn', 'neginf_target') for ii in (0, 18, 254, -1)])
def test_path_D_cross_entropy_gradient_inside_the_convT_backward(case, ii, waves, ft, monkeypatch):
    # dsrl_convt2x2_bwd_ce, the default 12-wave build and DSRL_CONVT_CE_WAVES=8, with and without the feature transformer's g * w term:
    # bit for bit against dsrl_ce_fused -> dsrl_pointwise_strided_bwd -> dsrl_convt2x2_bwd, and against the fp64 CE gradient (torch autograd)
    # pushed through the fp64 ConvTranspose backward.  A label outside [0, C): the loss is NaN and flagged (paths B, C); here the launch completes.
    # Every case with ignore index 255, two with the others.
    call, query = _lib()
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    if waves is None:
        monkeypatch.delenv('DSRL_CONVT_CE_WAVES', raising=False)
    else:
        monkeypatch.setenv('DSRL_CONVT_CE_WAVES', waves)
    N, H, W, C = 1, 3, 128, 19
    P = N * 4 * H * W
    rs = np.random.RandomState(D_CASES.index(case) + 11 * (ii & 0xff) + ft)
    lg, tg = make_case(case, P, C, rs, ii)
    x = torch.tensor(rs.standard_normal((N, H, W, C)).astype(np.float32), device=DEV)
    w = torch.tensor(rs.standard_normal((C, C, 2, 2)).astype(np.float32), device=DEV)
    logits = torch.tensor(lg.reshape(N, 2 * H, 2 * W, C), device=DEV)
    target = torch.tensor(tg.reshape(N, 2 * H, 2 * W), device=DEV)
    Hf, Wf = ((2 * H - 1) // ft + 1, (2 * W - 1) // ft + 1) if ft else (0, 0)
    ftg = torch.tensor(rs.standard_normal((N, Hf, Wf)).astype(np.float32), device=DEV) if ft else None
    ftw = torch.tensor(rs.standard_normal(C).astype(np.float32), device=DEV) if ft else None
    st = HF._stream()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(query('dsrl_ce_fused_workspace_bytes', P), dtype=torch.uint8, device=DEV)
    wsb = torch.empty(query('dsrl_convt2x2_bwd_workspace_bytes', N, H, W, C, C), dtype=torch.uint8, device=DEV)
    assert query('dsrl_convt2x2_bwd_ce_supported', x.data_ptr(), logits.data_ptr(), target.data_ptr(), N, H, W, C, C) == 1
    scal = torch.zeros(8, device=DEV); dl = torch.empty_like(logits)
    call('dsrl_ce_fused', logits.data_ptr(), C, target.data_ptr(), P, C, ii, dl.data_ptr(), C, scal.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), st)
    dl_ce = dl.clone()
    if ft:
        dwf = torch.empty(C, device=DEV)
        wsf = torch.empty(query('dsrl_pointwise_strided_bwd_workspace_bytes', N, 2 * H, 2 * W, C, ft), dtype=torch.uint8, device=DEV)
        call('dsrl_pointwise_strided_bwd', logits.data_ptr(), ftw.data_ptr(), ftg.data_ptr(), dl.data_ptr(), dwf.data_ptr(), 1, N, 2 * H, 2 * W, C, ft,
             wsf.data_ptr(), wsf.numel(), st)
    dx = torch.empty_like(x); dw = torch.empty_like(w); db = torch.empty(C, device=DEV)
    call('dsrl_convt2x2_bwd', x.data_ptr(), w.data_ptr(), dl.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    dx2 = torch.full_like(x, 7.0); dw2 = torch.full_like(w, 7.0); db2 = torch.full((C,), 7.0, device=DEV)
    call('dsrl_convt2x2_bwd_ce', x.data_ptr(), w.data_ptr(), logits.data_ptr(), target.data_ptr(), ii, scal.data_ptr() + 4,
         None if not ft else ftg.data_ptr(), None if not ft else ftw.data_ptr(), ft, dx2.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
         N, H, W, C, C, wsb.data_ptr(), wsb.numel(), st)
    torch.cuda.synchronize()
    assert int(flag) == flag_bits(case)
    assert _bits_equal(dx, dx2) and _bits_equal(dw, dw2) and _bits_equal(db, db2)
    if case == 'bad_label':
        return
    ref, g64, count = reference(lg, tg, ii)
    check_grad(host(dl_ce).reshape(P, C), g64, tg, ii, count, case)
    g64 = g64.reshape(N, 2 * H, 2 * W, C)
    if ft:
        g64[:, ::ft, ::ft, :] += host(ftg).astype(np.float64)[..., None] * host(ftw).astype(np.float64)
    dxo, dwo, dbo = O.conv_transpose2d_k2s2_bwd(host(x).astype(np.float64).transpose(0, 3, 1, 2), host(w).astype(np.float64), g64.transpose(0, 3, 1, 2),
                                               has_bias=True)
    check(host(dx2).transpose(0, 3, 1, 2), dxo, 1e-5, 'dx'); check(host(dw2), dwo, 1e-5, 'dw'); check(host(db2), dbo, 1e-5, 'db')


# ------------------------------------------------------------------------------------------------------------------------------ hand-over with a second consumer
def _dense_pointwise(monkeypatch):
    """_PointwiseStrided.backward as if the holder were not there: its gradient goes to the logits as a dense tensor."""
    orig = HF._PointwiseStrided.backward

    def backward(ctx, dy):
        ctx.logits_grad = None
        return orig(ctx, dy)
    monkeypatch.setattr(HF._PointwiseStrided, 'backward', staticmethod(backward))


@pytest.mark.parametrize('consumer', ['aux', 'cross_entropy', 'dense_transformer'])
def test_logits_gradient_hand_over_with_a_second_consumer(consumer, monkeypatch):
    # SMALL head, stage 3, 64 x 256 logits (the last ConvTranspose sees W = 128: the hand-over qualifies).  A second consumer of outs[0]:
    # 'aux' (outs[0] * r).sum() as a second root; 'cross_entropy' HF.cross_entropy as a second root; 'dense_transformer' the stride-8 feature
    # transformer returning its gradient densely.  Every parameter gradient, with the hand-over (convt_ce_enabled) and without it, against the
    # plainest run (no hand-over, no gradient slots: autograd sums every gradient): 1e-6 of the range.  (Without the hand-over the gradient slot
    # of the logits is in play: a second root reaches autograd before the transformer has added its part.)  The holder ends disarmed, and a
    # following plain step matches too.
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    r = torch.tensor(np.random.RandomState(4).standard_normal((2, 19, 64, 256)).astype(np.float32), device=DEV)
    e3 = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=DEV)
    if consumer == 'dense_transformer':
        _dense_pointwise(monkeypatch)

    def step(second, enabled, slots):
        monkeypatch.setattr(HF, 'convt_ce_enabled', enabled)
        monkeypatch.setattr(HF, 'grad_slots_enabled', slots)
        head, _ = make_head(gen.SMALL, 3, 101, True)
        a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
        outs = head(a, b)
        tgt = dev(target)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        vals = HF.fused_losses(outs, tgt, dev(org), gen.IGNORE, 0.1, 1.0, 3, flag)
        h = getattr(outs[0], '_dsrl_logits_grad', None)
        assert (h is not None and h.armed) == enabled, 'the hand-over did not engage as configured'
        if second and consumer == 'aux':
            torch.autograd.backward([vals, (outs[0] * r).sum()], [e3, torch.ones((), device=DEV)])
        elif second and consumer == 'cross_entropy':
            torch.autograd.backward([vals, HF.cross_entropy(outs[0], tgt, gen.IGNORE)], [e3, torch.ones((), device=DEV)])
        else:
            vals[3].backward()
        torch.cuda.synchronize()
        assert h is None or not h.armed, 'holder left armed'
        assert int(flag) == 0
        return {k: host(p.grad) for k, p in head.named_parameters()}, host(a.grad), host(b.grad)

    second = consumer != 'dense_transformer'
    ref = step(second, False, False)
    for enabled in (True, False):
        got = step(second, enabled, True)
        for k in ref[0]:
            check(got[0][k], ref[0][k], 1e-6, f'{consumer} enabled={enabled} grad {k}')
        check(got[1], ref[1], 1e-6, 'dx16'); check(got[2], ref[2], 1e-6, 'dx4')
    # a plain step after it
    plain_ref = step(False, False, False)
    got = step(False, True, True)
    for k in plain_ref[0]:
        check(got[0][k], plain_ref[0][k], 1e-6, f'plain step after {consumer}: grad {k}')

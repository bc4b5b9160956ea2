"""The kernels of csrc/losses.hip between the cross-entropy family and the SGD tail - the feature-affinity loss (fa_sim / fa_pairs / fa_finalize /
fa_bwd), MSE (mse_fwd / mse_bwd / mse_fused), loss_mix and nan_check - at their edges, each against the plain float64 references of
tests/fa_ref.py (which tests/test_fa_ref_host.py holds against the recorded original module and float64 stock torch).  Every test is a few small
launches.

u = 2^-24 is the unit roundoff of float32; the library is built with -ffp-contract=off, so the operation counts are the ones written in the
kernels.  FA forward values are held to the first-order bound derived at fa_ref.forward_bounds; FA gradients to 8 x the error float32 stock
torch makes with the original module's formula on the same inputs (fa_ref.grad_bound), never less than 8 x 32 u.  Every tolerance-based test
prints its largest observed error / bound.

Largest error / bound observed on an MI355X: FA forward 0.060 (k = 1, uniform; 0.0001 to 0.04 elsewhere: the bound is a worst case over k^2
sequential roundings of one sign, which S = G / lambda largely cancels), FA gradients 0.072 (vec64_T4 behind strides; the bounds were 256 u, the
floor, for all but four cases and 515 u at most, where today's golden test allows 33 000 u), the clean slices beside a NaN slice 0.008, MSE
loss 0.42 and MSE gradient 0.84 of their 4 u and 3 u."""
import functools

import numpy as np
import pytest
import torch

import fa_ref as R
from hip_helpers import D, DEV, HF, host
from dualsuperreslearningforsemseg_amd._lib import DsrlHipError

pytestmark = pytest.mark.gpu

U = R.U
F64 = np.float64
NAN = float('nan')


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def worst_ratio(err, bound):
    """largest error / bound; an element whose bound is 0 has to be exact"""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    assert not np.isnan(err).any(), 'NaN where the reference is finite'
    assert not (err[bound == 0] != 0).any(), 'error on an element whose bound is 0'
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


# ================================================================================================ FA loss
def case_of(name):
    return R.FA_CASES[name][:2] if name in R.FA_CASES else ((2, 1, 64, 64), 8)


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    return R.special_inputs(name) if name in ('rank1', 'same') else R.fa_inputs(name, kind)


@functools.lru_cache(maxsize=None)
def forward_ref(name, kind):
    return R.forward_bounds(*inputs(name, kind), case_of(name)[1])


@functools.lru_cache(maxsize=None)
def grad_ref(name, kind, red, root):
    f1, f2 = inputs(name, kind)
    k = case_of(name)[1]
    ref = R.fa_grads(f1, f2, k, red, root)
    return ref, R.grad_bound(f1, f2, k, red, root, ref)


def run_forward(a, b, k):
    """-> (mean, sum, none) as host arrays"""
    return tuple(host(D.FALoss(k, reduction=red)(a, b)) for red in ('mean', 'sum', 'none'))


def run_grads(a, b, k, red, root):
    a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    (root * D.FALoss(k, reduction=red)(a, b)).backward()
    return host(a.grad), host(b.grad)


def check_forward(got, name, kind, what):
    """the three reductions against the float64 reference and the bound of fa_ref.forward_bounds -> largest error / bound"""
    mean, total, none = got
    none_ref, none_bound, total_ref, total_bound = forward_ref(name, kind)
    assert none.shape == none_ref.shape, (what, none.shape)
    count = none_ref.size
    r = max(worst_ratio(np.abs(none - none_ref), none_bound), worst_ratio(abs(float(total) - total_ref), total_bound),
            worst_ratio(abs(float(mean) - total_ref / count), total_bound / count))
    assert r <= 1.0, f'{what}: forward error {r:.3f} x the bound'
    return r


def check_grads(got, name, kind, red, root, what):
    (r1, r2), (b1, b2) = grad_ref(name, kind, red, root)
    ratios = []
    for g, ref, bound, s in ((got[0], r1, b1, 'd fm1'), (got[1], r2, b2, 'd fm2')):
        assert g.shape == ref.shape and np.isfinite(g).all(), f'{what}: {s}'
        ratios.append(R.range_rel(g, ref) / bound)
        assert ratios[-1] <= 1.0, f'{what}: {s} error {R.range_rel(g, ref) / U:.1f} u of the range, {ratios[-1]:.3f} x the bound of {bound / U:.0f} u'
    return max(ratios), max(b1, b2) / U


def assert_remainder_is_zero(g, k, what):
    """rows and columns past the last whole k x k cell take no part in the loss: their gradient is exactly zero"""
    H, W = g.shape[2:]
    assert not g[:, :, (H // k) * k:, :].any() and not g[:, :, :, (W // k) * k:].any(), f'{what}: a gradient outside the pooled area'


@pytest.mark.parametrize('kind', R.FA_KINDS)
@pytest.mark.parametrize('name', list(R.FA_CASES))
def test_fa_values_and_gradients_at_every_pooling_path_and_limit(name, kind):
    """All three reductions, and both input gradients of 1.0 * loss and 3.5 * loss for 'mean' and 'sum', on contiguous NCHW maps: the 16-byte
    pooling path with 4 and 8 lanes per cell and with a ragged edge, the scalar path (row stride 43, k = 4, 3, 1), hp < wp and a rank-deficient
    G, the 1 x 1 pooled map (everything exactly 0), hp = 64 and, forward only, hp = 64 with wp = 32."""
    (shape, k), gradient = case_of(name), (name, kind) in R.fa_gradient_cases()
    f1, f2 = inputs(name, kind)
    a, b = to_dev(f1), to_dev(f2)
    what = f'{name} {kind} {shape} k={k}'
    got = run_forward(a, b, k)
    rf = check_forward(got, name, kind, what)
    if name == 'pooled_1x1':
        assert got[0] == 0 and got[1] == 0 and not got[2].any(), what
    rg = gb = 0.0
    if gradient:
        for red in ('mean', 'sum'):
            for root in (1.0, 3.5):
                g = run_grads(a, b, k, red, root)
                r, bu = check_grads(g, name, kind, red, root, f'{what} {red} x{root}')
                rg, gb = max(rg, r), max(gb, bu)
                for t in g:
                    assert_remainder_is_zero(t, k, what)
                    if name == 'pooled_1x1':
                        assert not t.any(), what
    print(f'fa {what}: largest error / bound forward {rf:.4f}' + (f', gradients {rg:.3f} (bound up to {gb:.0f} u)' if gradient else ' (forward only)'))


@pytest.mark.parametrize('name', ['rank1', 'same'])
def test_fa_constant_map_and_identical_maps(name):
    """(2, 1, 64, 64), k = 8.  rank1: a constant map (G = c^2 J, one non-zero eigenvalue) against a random one.  same: two identical maps.  The loss
    compares every entry of S1 with every entry of S2, so identical maps give mean |S_i - S_j| > 0 and a non-zero gradient, as the recording of
    the original module does (tests/golden/fa_loss.npz 'same': mean 2.4e-3); what is exact is the symmetry: S1 = S2 bit for bit, so 'none' is a
    symmetric matrix with a zero diagonal and d fm1 = d fm2 bit for bit."""
    f1, f2 = inputs(name, 'uniform')
    a, b = to_dev(f1), to_dev(f2)
    got = run_forward(a, b, 8)
    rf = check_forward(got, name, 'uniform', name)
    rg = 0.0
    for red, root in (('mean', 1.0), ('sum', 3.5)):
        g = run_grads(a, b, 8, red, root)
        rg = max(rg, check_grads(g, name, 'uniform', red, root, f'{name} {red} x{root}')[0])
        if name == 'same':
            assert np.array_equal(g[0], g[1]) and g[0].any(), 'identical maps: the two gradients differ'
    if name == 'same':
        none = got[2].reshape(2, 1, 64, 64)
        assert np.array_equal(none, none.transpose(0, 1, 3, 2)) and not none[:, :, np.arange(64), np.arange(64)].any() and got[0] > 1e-3
    print(f'fa {name}: largest error / bound forward {rf:.4f}, gradients {rg:.3f}')


# ------------------------------------------------------------------------------------------------ layouts
def strided_view(vals, layout):
    """the values of `vals` (B, C, H, W) behind the strides of `layout`, in a storage whose every other float is NaN"""
    B, C, H, W = vals.shape
    v = to_dev(vals)

    def full(*shape):
        return torch.full(shape, NAN, device=DEV)
    if layout == 'nchw':
        return v
    if layout == 'channels_last':
        view = full(B, H, W, C).permute(0, 3, 1, 2)
    elif layout == 'channel_slice':                # channels 1 : 1 + C of a pixel-major buffer 5 channels wide
        view = full(B, H, W, 5).permute(0, 3, 1, 2)[:, 1:1 + C]
    elif layout in ('rows+4', 'rows+1'):
        view = full(B, C, H, W + int(layout[-1]))[..., :W]
    elif layout == 'slices_2mod4':                 # slice stride = 2 mod 4 floats: every other slice starts 8 bytes off a 16-byte boundary
        L = H * W + ((2 - H * W) % 4 or 4)
        view = torch.as_strided(full(B * C * L + 8), (B, C, H, W), (C * L, L, W, 1), 0)
    else:
        assert layout == 'offset1'                 # one float into its storage
        view = full(B * C * H * W + 8)[1:1 + B * C * H * W].view(B, C, H, W)
    view.copy_(v)
    assert view.untyped_storage().data_ptr() % 16 == 0
    return view


def pooling_path(t, k):
    """'vector' / 'scalar' / 'mixed' (by slice): the branch fa_pool takes for each (b, c) slice of `t`"""
    sb, sc, sh, sw = t.stride()
    if not (k == 8 and sw == 1 and sh % 4 == 0):
        return 'scalar', None
    aligned = np.array([[(t.data_ptr() // 4 + b_ * sb + c_ * sc) % 4 == 0 for c_ in range(t.shape[1])] for b_ in range(t.shape[0])])
    return ('vector' if aligned.all() else 'mixed' if aligned.any() else 'scalar'), aligned


LAYOUTS = ['nchw', 'channels_last', 'channel_slice', 'rows+4', 'rows+1', 'slices_2mod4', 'offset1', 'nchw|channels_last']
EXPECTED_PATH = {
    'vec8_T8_C2': dict(zip(LAYOUTS, ['vector', 'scalar', 'scalar', 'vector', 'scalar', 'mixed', 'scalar', 'vector'])),
    # one channel: channels-last IS row-major with unit column stride
    'vec64_T4': dict(zip(LAYOUTS, ['vector', 'vector', 'scalar', 'vector', 'scalar', 'mixed', 'scalar', 'vector'])),
    'k3': dict.fromkeys(LAYOUTS, 'scalar'),
}


@pytest.mark.parametrize('name', list(EXPECTED_PATH))
def test_fa_any_input_strides(name):
    """The same values as contiguous NCHW, channels-last, a channel slice of a wider pixel-major buffer (how fused_losses hands over the feature
    transformers' outputs), NCHW with rows padded by 4 and by 1 floats, slices 2 mod 4 floats apart, a view one float into its storage, and
    fm1 NCHW with fm2 channels-last (the wrapper then makes both contiguous); every float of the storage outside the view is NaN, so a read
    outside the view shows.  Each layout against the reference; the pooling arithmetic does not depend on the strides, so all layouts on the
    scalar path agree bit for bit, all on the 16-byte path do, and where the slices of one tensor alternate between the two (slices_2mod4)
    each slice's 'none' rows equal those of the layout that takes that slice's path everywhere."""
    kind = 'normal'
    (shape, k), (f1, f2) = case_of(name), inputs(name, kind)
    results, paths, worst = {}, {}, [0.0, 0.0]
    for layout in LAYOUTS:
        la, _, lb = layout.partition('|')
        a, b = strided_view(f1, la), strided_view(f2, lb or la)
        handed = (a.contiguous(), b.contiguous()) if a.stride() != b.stride() else (a, b)          # what _FALoss.forward hands to the library
        paths[layout] = pooling_path(handed[0], k)
        assert paths[layout][0] == EXPECTED_PATH[name][layout] == pooling_path(handed[1], k)[0], (layout, paths[layout][0])
        what = f'{name} {layout}'
        fwd = run_forward(a, b, k)
        worst[0] = max(worst[0], check_forward(fwd, name, kind, what))
        grads = []
        for red, root in (('mean', 1.0), ('sum', 3.5)):
            g = run_grads(a, b, k, red, root)
            worst[1] = max(worst[1], check_grads(g, name, kind, red, root, f'{what} {red} x{root}')[0])
            grads += list(g)
        results[layout] = list(fwd) + grads
    for path in ('scalar', 'vector'):
        group = [lay for lay in LAYOUTS if paths[lay][0] == path]
        for lay in group[1:]:
            for x, y, s in zip(results[group[0]], results[lay], ('mean', 'sum', 'none', 'd fm1 mean', 'd fm2 mean', 'd fm1 sum', 'd fm2 sum')):
                assert np.array_equal(x, y), f'{name}: {s} of {lay} differs from {group[0]}, both on the {path} path'
    if name != 'k3':
        aligned = paths['slices_2mod4'][1]
        assert aligned.any() and not aligned.all()
        for (b_, c_), al in np.ndenumerate(aligned):
            twin = 'nchw' if al else 'offset1'
            assert np.array_equal(results['slices_2mod4'][2][b_, c_], results[twin][2][b_, c_]), f'{name}: slice {(b_, c_)} of slices_2mod4 vs {twin}'
    print(f'fa layouts {name}: largest error / bound forward {worst[0]:.4f}, gradients {worst[1]:.3f}')


# ------------------------------------------------------------------------------------------------ scaling, determinism
@pytest.mark.parametrize('name', ['vec64_T4', 'ragged_scalar', 'k3'])
def test_fa_is_exactly_invariant_under_power_of_two_scaling_and_deterministic(name):
    """fm1 x 2^40 or x 2^-40, and both maps by the same factor: the loss and 'none' bit-identical, the gradient of a scaled map the unscaled
    one times the inverse factor exactly, that of an unscaled map unchanged.  Every operation of the kernels commutes with a power-of-two scaling
    (sums, products, the division by the largest diagonal entry, sqrt of an even power) or acts on scale-free quantities (S, u, v, the sign
    counts), and nothing under- or overflows at these magnitudes.  Two runs of one call give the same bits."""
    (shape, k), (f1, f2) = case_of(name), inputs(name, 'normal')

    def everything(x1, x2):
        out = list(run_forward(to_dev(x1), to_dev(x2), k))
        for red, root in (('mean', 1.0), ('sum', 3.5)):
            out += list(run_grads(to_dev(x1), to_dev(x2), k, red, root))
        return out
    base = everything(f1, f2)
    again = everything(f1, f2)
    for x, y in zip(base, again):
        assert np.array_equal(x, y), f'{name}: two runs differ'
    for e in (40, -40):
        s, inv = np.float32(2.0 ** e), np.float32(2.0 ** -e)
        for both in (False, True):
            got = everything(f1 * s, f2 * s if both else f2)
            what = f'{name} x 2^{e} {"both maps" if both else "fm1"}'
            for i in range(3):
                assert np.array_equal(got[i], base[i]), f'{what}: {("mean", "sum", "none")[i]} changed'
            for i in (3, 5):
                assert np.array_equal(got[i], base[i] * inv), f'{what}: d fm1 is not the unscaled gradient / 2^{e}'
                assert np.array_equal(got[i + 1], base[i + 1] * inv if both else base[i + 1]), f'{what}: d fm2'
                assert np.isfinite(got[i]).all() and got[i].any()


# ------------------------------------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize('name,where', [('vec8_T8_C2', (1, 0)), ('k3', (0, 1))])
def test_fa_nan_or_inf_poisons_its_own_slice_only(name, where):
    """One NaN, then one +inf, in one slice of fm1, in pooled column 0 and in another column.  The original module divides the whole pooled map
    by its (then NaN) spectral norm: every 'none' row of that slice is NaN and so are 'mean' and 'sum'; every other slice stays finite and
    within the bound.  (The all-zero slice, 0 / 0, is test_fa_zero_sample_nan_and_shape_asserts.)"""
    (shape, k), (f1, f2) = case_of(name), inputs(name, 'normal')
    none_ref, none_bound = forward_ref(name, 'normal')[:2]
    keep = np.ones(shape[:2], bool); keep[where] = False
    r = 0.0
    for bad in (np.nan, np.inf):
        for pos in ((0, 1), (2 * k + 1, k + 1)):
            f = f1.copy(); f[where + pos] = bad
            mean, total, none = run_forward(to_dev(f), to_dev(f2), k)
            what = f'{name} {bad} at {where + pos}'
            want = R.fa_loss(f, f2, k, 'none')
            assert np.isnan(want[where]).all() and np.array_equal(want[keep], none_ref[keep])
            assert np.isnan(mean) and np.isnan(total), what
            assert np.array_equal(np.isnan(none), np.isnan(want)), f'{what}: {int(np.isnan(none[where]).sum())} of {none[where].size} rows of the slice are NaN'
            r = max(r, worst_ratio(np.abs(none[keep] - none_ref[keep]), none_bound[keep]))
            assert r <= 1.0, what
    print(f'fa non-finite {name}: largest error / bound on the clean slices {r:.4f}')


# ------------------------------------------------------------------------------------------------ refusals
def _valid_call_still_right():
    name, kind = 'vec8_T8_C2', 'normal'
    f1, f2 = inputs(name, kind)
    check_forward(run_forward(to_dev(f1), to_dev(f2), 8), name, kind, 'the valid call after a refusal')


def _fa_fwd_direct(a, b, k, red, ws_bytes=None):
    B, C, H, W = a.shape
    n = max(W // max(k, 1), 1) ** 2
    out = torch.empty((B, C, n * n) if red == 2 else (1,), device=DEV)
    saved = torch.empty(max(int(HF.cquery('dsrl_fa_saved_floats', B, C, H, W, k)), 64), device=DEV)
    need = int(HF.cquery('dsrl_fa_workspace_bytes', B, C, H, W, k))
    ws = torch.empty(max(need, 256), device=DEV, dtype=torch.uint8)
    HF.call('dsrl_fa_fwd', a.data_ptr(), b.data_ptr(), B, C, H, W, *a.stride(), k, red, out.data_ptr(), saved.data_ptr(), ws.data_ptr(),
            need if ws_bytes is None else ws_bytes(need), HF._stream())
    return out, saved


@pytest.mark.parametrize('shape,k,reason', [((1, 1, 8, 264), 8, 'pooled map 1x33 exceeds 64x32'), ((1, 1, 130, 16), 2, 'pooled map 65x8 exceeds 64x32'),
                                            ((1, 1, 4, 16), 8, 'subsample factor 8 larger than the 4x16 map'),
                                            ((1, 1, 16, 4), 8, 'subsample factor 8 larger than the 16x4 map'),
                                            ((1, 1, 16, 16), 0, 'subsample factor 0 must be positive'),
                                            ((1, 1, 16, 16), -8, 'subsample factor -8 must be positive')])
def test_fa_refuses_what_it_cannot_pool(shape, k, reason):
    """W / k = 33, H / k = 65, k > H, k > W, k = 0, k < 0: DsrlHipError with the reason, from the module, from a direct forward and from a direct
    backward call; and a valid call right after gives the right answer."""
    a = torch.ones(shape, device=DEV)
    for red in ('mean', 'none'):
        with pytest.raises(DsrlHipError, match=reason):
            D.FALoss(k, reduction=red)(a, a)
    with pytest.raises(DsrlHipError, match=reason):
        _fa_fwd_direct(a, a, k, 0)
    one = torch.ones(1, device=DEV)
    d = torch.empty(shape, device=DEV)
    with pytest.raises(DsrlHipError, match=reason):
        HF.call('dsrl_fa_bwd', a.data_ptr(), a.data_ptr(), *shape, *a.stride(), k, 0, one.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), None, 0, HF._stream())
    _valid_call_still_right()


def test_fa_refuses_a_backward_pass_through_none_and_a_short_workspace():
    f1, f2 = inputs('vec8_T8_C2', 'normal')
    a, b = to_dev(f1).requires_grad_(True), to_dev(f2).requires_grad_(True)
    none = D.FALoss(8, reduction='none')(a, b)
    with pytest.raises(DsrlHipError, match="reduction='none'.* has no backward kernel"):
        none.sum().backward()
    assert a.grad is None and b.grad is None
    _valid_call_still_right()
    a, b = a.detach(), b.detach()
    one = torch.ones(1, device=DEV)
    out, saved = _fa_fwd_direct(a, b, 8, 2)
    assert np.array_equal(host(out), host(none))            # the direct call with exactly the workspace the query asks for
    d1, d2 = torch.empty_like(a), torch.empty_like(b)
    with pytest.raises(DsrlHipError, match="only 'mean' and 'sum' reductions have a backward kernel"):
        HF.call('dsrl_fa_bwd', a.data_ptr(), b.data_ptr(), *a.shape, *a.stride(), 8, 2, one.data_ptr(), saved.data_ptr(), d1.data_ptr(), d2.data_ptr(), None, 0,
                HF._stream())
    with pytest.raises(DsrlHipError, match='fa_fwd: workspace too small'):
        _fa_fwd_direct(a, b, 8, 0, ws_bytes=lambda need: need - 1)
    with pytest.raises(DsrlHipError, match='fa_fwd: bad arguments'):
        _fa_fwd_direct(a, b, 8, 3)
    _valid_call_still_right()


# ================================================================================================ MSE
MSE_SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1048579]         # the last: more than 4 x 256 x 1024 floats, the capped grid loops
PAD = 8                                                                     # floats of NaN on either side of every buffer: keeps 16-byte alignment


def mse_inputs(n, mag):
    rs = np.random.RandomState(n % 9973 + 17)
    return (rs.uniform(size=n) * mag).astype(np.float32), (rs.uniform(size=n) * mag).astype(np.float32)


def padded(vals, off, n=None):
    """-> (storage, view): `vals` (or n floats of NaN) `off` floats past a 16-byte boundary, NaN on both sides"""
    n = len(vals) if vals is not None else n
    st = torch.full((n + 2 * PAD,), NAN, device=DEV)
    view = st[PAD + off:PAD + off + n]
    if vals is not None:
        view.copy_(to_dev(vals))
    assert st.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    return st, view


def pads_are_nan(st, off, n):
    h = st.cpu().numpy()
    return np.isnan(h[:PAD + off]).all() and np.isnan(h[PAD + off + n:]).all()


def mse_fused(a, b, n, grad_scale, da, flag):
    out = torch.full((3,), NAN, device=DEV)
    ws = torch.empty(max(int(HF.cquery('dsrl_mse_workspace_bytes', n)), 256), device=DEV, dtype=torch.uint8)
    HF.call('dsrl_mse_fused', a.data_ptr(), b.data_ptr(), n, grad_scale, da.data_ptr() if da is not None else None, out[1:].data_ptr(),
            flag.data_ptr() if flag is not None else None, ws.data_ptr(), int(HF.cquery('dsrl_mse_workspace_bytes', n)), HF._stream())
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[2]), 'mse_fused wrote beside its loss'
    return float(o[1])


# Bounds, from the kernel text.  A term is d = a - b and d * d, two float32 operations: (1 + u)^3 of the exact (a - b)^2; the sum and the division by n
# are float64 and the result is rounded to float32 once: the loss is within (1 + u)^4 - 1 < 4.01 u of the reference, relative (all terms are positive).
# A gradient element is d * sc with sc = 2 s / (float) n: 2 s is exact for the scales used, the division, the difference and the product round once
# each: within (1 + u)^3 - 1 < 3.01 u of (a - b) 2 s / n.
LOSS_TOL, GRAD_TOL = 4.01 * U, 3.01 * U


@pytest.mark.parametrize('n', MSE_SIZES)
def test_mse_loss_forward_and_backward(n):
    """HF.mse_loss (mse_fwd_kernel, mse_finalize_kernel, mse_bwd_kernel) with roots 1 and 0.25, on uniform inputs of magnitude 1, 1e-15 and 1e15"""
    worst = [0.0, 0.0]
    for mag in (1.0, 1e-15, 1e15):
        a, b = mse_inputs(n, mag)
        ref = R.mse(a, b)
        for root in (1.0, 0.25):
            at = to_dev(a).reshape(1, 1, 1, n).requires_grad_(True)
            loss = HF.mse_loss(at, to_dev(b).reshape(1, 1, 1, n))
            (root * loss).backward()
            worst[0] = max(worst[0], abs(loss.item() - ref) / (LOSS_TOL * ref))
            want = R.mse_grad(a, b, root)
            worst[1] = max(worst[1], worst_ratio(np.abs(host(at.grad).reshape(n) - want), GRAD_TOL * np.abs(want)))
            assert max(worst) <= 1.0, f'n={n} magnitude {mag} root {root}: error / bound loss {worst[0]:.3f}, gradient {worst[1]:.3f}'
    print(f'mse n={n}: largest error / bound loss {worst[0]:.3f}, gradient {worst[1]:.3f}')


# name: offsets in floats of a, b, da from a 16-byte boundary (None: a null da)
MSE_FUSED_LAYOUTS = {'aligned': (0, 0, 0), 'a+1': (1, 0, 0), 'b+2': (0, 2, 0), 'da+3': (0, 0, 3), 'all+1': (1, 1, 1), 'no da': (0, 0, None), 'no da, a+3': (3, 0, None)}


@pytest.mark.parametrize('n', MSE_SIZES)
def test_mse_fused_vector_body_tail_scalar_branch_and_null_gradient(n):
    """dsrl_mse_fused with all three pointers 16-byte aligned (float4 body and its tail), each of a, b, da in turn off the boundary (the scalar
    branch), a null da, grad_scale 1 and 0.1; NaN pads on both sides of every buffer are neither read into the result nor overwritten; da of
    the two branches is the same per-element arithmetic: bit-identical.  The flag stays as it was."""
    worst = [0.0, 0.0]
    for mag, scale in ((1.0, 1.0), (1.0, 0.1), (1e-15, 0.1), (1e15, 1.0)):
        a, b = mse_inputs(n, mag)
        ref, want = R.mse(a, b), R.mse_grad(a, b, float(np.float32(scale)))
        das = {}
        for name, (oa, ob, od) in MSE_FUSED_LAYOUTS.items():
            (sa, va), (sb_, vb) = padded(a, oa), padded(b, ob)
            sd, vd = padded(None, od, n) if od is not None else (None, None)
            flag = torch.full((1,), 2, dtype=torch.int32, device=DEV)
            loss = mse_fused(va, vb, n, scale, vd, flag)
            what = f'n={n} magnitude {mag} scale {scale} {name}'
            assert int(flag) == 2, what + ': the flag changed'
            assert np.array_equal(va.cpu().numpy(), a) and np.array_equal(vb.cpu().numpy(), b) and pads_are_nan(sa, oa, n) and pads_are_nan(sb_, ob, n), what
            worst[0] = max(worst[0], abs(loss - ref) / (LOSS_TOL * ref))
            if vd is not None:
                assert pads_are_nan(sd, od, n), what + ': da written outside its n floats'
                das[name] = vd.cpu().numpy()
                worst[1] = max(worst[1], worst_ratio(np.abs(das[name] - want), GRAD_TOL * np.abs(want)))
                assert np.array_equal(das[name], das['aligned']), what + ': da differs from the aligned call'
            assert max(worst) <= 1.0, f'{what}: error / bound loss {worst[0]:.3f}, gradient {worst[1]:.3f}'
    print(f'mse_fused n={n}: largest error / bound loss {worst[0]:.3f}, gradient {worst[1]:.3f}')


@pytest.mark.parametrize('n', MSE_SIZES)
def test_mse_fused_nan_flag_checks_a_only(n):
    """The comment on mse_fused_kernel: the NaN check is of `a`.  A NaN in a at element 0, at the first tail element 4 * (n / 4) and at n - 1 sets
    bit 0 and makes the loss NaN, in the float4 and in the scalar branch, with and without da; a NaN only in b makes the loss NaN and leaves the
    flag; a flag that holds 2 ends as 3; a null flag is accepted."""
    a, b = mse_inputs(n, 1.0)
    for oa, od in ((0, 0), (1, 0), (0, None)):
        for pos in sorted({0, min(4 * (n // 4), n - 1), n - 1}):
            for start in (0, 2):
                x = a.copy(); x[pos] = np.nan
                flag = torch.full((1,), start, dtype=torch.int32, device=DEV)
                vd = padded(None, od, n)[1] if od is not None else None
                loss = mse_fused(padded(x, oa)[1], padded(b, 0)[1], n, 1.0, vd, flag)
                what = f'n={n} NaN in a[{pos}], a off by {oa}, da {"null" if od is None else "given"}, flag {start}'
                assert np.isnan(loss) and int(flag) == (start | 1) == R.nan_flag(x) | start, what
                if vd is not None:
                    assert np.array_equal(np.isnan(vd.cpu().numpy()), np.isnan(x)), what + ': da'
            y = b.copy(); y[pos] = np.nan
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            loss = mse_fused(padded(a, oa)[1], padded(y, 0)[1], n, 1.0, None, flag)
            assert np.isnan(loss) and int(flag) == 0, f'n={n} NaN in b[{pos}], a off by {oa}'
        x = a.copy(); x[n - 1] = np.nan
        assert np.isnan(mse_fused(padded(x, oa)[1], padded(b, 0)[1], n, 1.0, None, None))


# ================================================================================================ loss mix
def test_loss_mix_is_the_float32_expressions_as_written():
    """dsrl_loss_mix with all three terms, with mse null, with mse and fa null, with a null flag: c, w1 * m, w2 * f, (c + m) + f and the flag,
    bit for bit (no contraction); a NaN term reaches its own value and the total only; the floats around the five stay untouched."""
    def scalar(v, dtype=torch.float32):
        return torch.tensor([v], dtype=dtype, device=DEV) if v is not None else None

    def ptr(t):
        return t.data_ptr() if t is not None else None
    cases = [(1.2345678, 0.3371, 0.0071234, 0.1, 1.0, 0), (1.2345678, 0.3371, 0.0071234, 0.3, 0.7, 1), (1.2345678, None, 0.0071234, 0.1, 0.7, 3),
             (1.2345678, 0.3371, None, 0.1, 0.7, 0), (0.1, None, None, 0.1, 1.0, 2), (1e-8, 1.0, 3.0, 1.0, 1.0, None), (16777216.0, 10.0, 1.0, 0.1, 1.0, 0),
             (NAN, 0.3371, 0.0071234, 0.1, 1.0, 1), (1.2345678, NAN, 0.0071234, 0.1, 1.0, 0), (1.2345678, 0.3371, NAN, 0.1, 1.0, 0),
             (1.2345678, float('inf'), 0.0071234, 0.0, 1.0, 0)]
    for ce, ms, fa, w1, w2, flag in cases:
        vals = torch.full((7,), -7.0, device=DEV)
        t = [scalar(ce), scalar(ms), scalar(fa), scalar(flag, torch.int32)]
        HF.call('dsrl_loss_mix', ptr(t[0]), ptr(t[1]), ptr(t[2]), w1, w2, ptr(t[3]), vals[1:].data_ptr(), HF._stream())
        got = vals.cpu().numpy()
        want = R.loss_mix(ce, ms, fa, w1, w2, flag)
        assert got[0] == -7.0 and got[6] == -7.0
        assert np.array_equal(got[1:6], want, equal_nan=True), ((ce, ms, fa, w1, w2, flag), got[1:6], want)
        nan_terms = [i for i, v in enumerate((ce, ms, fa)) if v is not None and np.isnan(np.float32(v) * np.float32((1.0, w1, w2)[i]))]
        assert [i for i in range(5) if np.isnan(got[1 + i])] == (nan_terms + [3] if nan_terms else [])
    with pytest.raises(DsrlHipError, match='loss_mix: bad arguments'):
        HF.call('dsrl_loss_mix', None, None, None, 0.1, 1.0, None, vals.data_ptr(), HF._stream())


# ================================================================================================ NaN check
def _bits(pattern):
    return torch.tensor([pattern - (1 << 32) if pattern >= (1 << 31) else pattern], dtype=torch.int32, device=DEV).view(torch.float32)


NANS = {'+NaN': 0x7fc00000, '-NaN': 0xffc00000, 'payload': 0x7f800001, '-payload': 0xffbadbad}
NOT_NANS = {'+inf': 0x7f800000, '-inf': 0xff800000, 'denormal': 0x00000001, '-denormal': 0x807fffff, 'largest': 0x7f7fffff, '-0': 0x80000000}


def _flag_after(*tensors, start=0):
    flag = torch.full((1,), start, dtype=torch.int32, device=DEV)
    HF.nan_check_(flag, *tensors)
    return int(flag)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 2047, 2048, 2049, 2048 * 4096 + 1])
def test_nan_check_finds_one_nan_at_either_end_of_any_size(n):
    """HF.nan_check_ on n floats, up to one more than 4096 blocks x 2048 floats (the grid-stride loop wraps): nothing flagged on finite values with
    +-inf, denormals and the largest float at both ends; the only NaN at the last element, then at the first, with either sign and a payload."""
    x = torch.ones(n, device=DEV)
    assert _flag_after(x) == 0
    for end in (n - 1, 0):
        for name, pattern in NOT_NANS.items():
            x[end] = _bits(pattern)[0]
            assert _flag_after(x) == 0, f'n={n}: {name} at {end} flagged'
        for name, pattern in NANS.items():
            x[end] = _bits(pattern)[0]
            assert bool(torch.isnan(x[end])) and int((x != x).sum()) == 1
            assert _flag_after(x) == 1, f'n={n}: {name} at {end} not flagged'
        x[end] = 1.0
    assert _flag_after(x) == 0
    x[n // 2] = NAN
    assert _flag_after(x, start=2) == 3 and _flag_after(x, start=1) == 1


def test_nan_check_arguments_none_several_channels_last_and_views():
    """a None argument is skipped; several tensors in one call; a channels-last tensor; a channel slice of a wider buffer is checked as the view it
    is: NaN in the hidden channels only leaves the flag, NaN in the view only sets it"""
    clean, dirty = torch.ones(300, device=DEV), torch.ones(70, device=DEV)
    dirty[69] = NAN
    assert _flag_after(None) == 0 and _flag_after(None, clean, None) == 0 and _flag_after() == 0
    assert _flag_after(clean, dirty) == 1 and _flag_after(dirty, clean) == 1 and _flag_after(clean, None, clean, dirty, clean) == 1
    cl = torch.ones(2, 5, 3, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and _flag_after(cl) == 0
    cl[1, 4, 2, 6] = NAN
    assert _flag_after(cl) == 1 and _flag_after(clean, cl) == 1
    big = torch.ones(2, 3, 7, 8, device=DEV).permute(0, 3, 1, 2)          # (2, 8, 3, 7) pixel-major, 8 channels wide
    view = big[:, 2:5]
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    big[:, :2] = NAN; big[:, 5:] = NAN
    assert _flag_after(view) == 0 and _flag_after(big) == 1
    big = torch.ones(2, 3, 7, 8, device=DEV).permute(0, 3, 1, 2)
    view = big[:, 2:5]
    view[1, 2, 2, 6] = NAN
    assert _flag_after(view) == 1 and _flag_after(big[:, :2]) == 0 and _flag_after(big[:, 5:]) == 0 and _flag_after(big[:, :2], big[:, 5:], view) == 1
    hidden = torch.ones(4, 1, 6, 9, device=DEV)                           # padded rows: NaN in the pad column only
    hidden[..., 8] = NAN
    assert _flag_after(hidden[..., :8]) == 0 and _flag_after(hidden) == 1

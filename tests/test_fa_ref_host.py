"""The float64 references of tests/fa_ref.py against the recorded values of the original FALoss module (tests/golden/fa_loss.npz) and against
float64 stock torch, on the inputs tests/test_loss_edges_gpu.py uses; and the condition that makes those inputs valid gradient cases: every pair
|S1_i - S2_j| at least GAP_FLOOR apart by the reference alone, so that no tolerance has to absorb a flipped sign.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
import fa_ref as R

F64 = np.float64
ALL_CASES = [(c, kd) for c in R.FA_CASES for kd in R.FA_KINDS]


def rel(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), 'NaN pattern differs'
    return float(np.nanmax(np.abs(a - b))) / max(float(np.nanmax(np.abs(b))), 1e-300) if a.size else 0.0


# ------------------------------------------------------------------------------------------------ against the original module's recording
@pytest.mark.parametrize('case', ['rand', 'c3', 'big', 'signed', 'relu_like', 'same', 'near_degenerate'])
def test_reference_reproduces_the_recorded_module(golden, case):
    """values and gradients the original module gave in float32, at the tolerances test_fa_golden holds the kernels to"""
    g = golden('fa_loss')
    f1, f2 = g[f'{case}.fm1'], g[f'{case}.fm2']
    for red in ('mean', 'sum'):
        assert rel(R.fa_loss(f1, f2, 8, red), g[f'{case}.{red}']) <= 2e-5, red
    none = R.fa_loss(f1, f2, 8, 'none')
    assert tuple(none.shape) == tuple(g[f'{case}.none_shape'])
    assert rel(gen.strided_sample(none), g[f'{case}.none_sample']) <= 1e-4
    g1, g2 = R.fa_grads(f1, f2, 8, 'mean')
    assert rel(g1, g[f'{case}.g1']) <= (2e-2 if case == 'near_degenerate' else 2e-3)
    assert rel(g2, g[f'{case}.g2']) <= 2e-3


def test_reference_all_zero_slice_is_nan_like_the_module(golden):
    g = golden('fa_loss')
    assert np.isnan(g['zero_sample.mean']) and np.isnan(R.fa_loss(g['zero_sample.fm1'], g['zero_sample.fm2']))
    none = R.fa_loss(g['zero_sample.fm1'], g['zero_sample.fm2'], 8, 'none')
    assert np.isnan(none[1]).all() and np.isfinite(none[0]).all()


def test_identical_maps_do_not_give_a_zero_loss(golden):
    """The loss compares EVERY entry of S1 with EVERY entry of S2, so two identical maps give mean |S_i - S_j| > 0, and the same non-zero
    gradient twice; the recording of the original module says so too.  What IS exact is the symmetry: 'none' is a symmetric matrix with a
    zero diagonal and d fm1 = d fm2."""
    g = golden('fa_loss')
    assert g['same.mean'] > 1e-3 and np.abs(g['same.g1']).max() > 0 and np.array_equal(g['same.g1'], g['same.g2'])
    f1, f2 = R.special_inputs('same')
    n = 64
    none = R.fa_loss(f1, f2, 8, 'none').reshape(2, 1, n, n)
    assert np.array_equal(none, none.transpose(0, 1, 3, 2)) and not none[:, :, np.arange(n), np.arange(n)].any() and none.mean() > 1e-3
    g1, g2 = R.fa_grads(f1, f2, 8, 'mean')
    assert np.array_equal(g1, g2) and np.abs(g1).max() > 0


# ------------------------------------------------------------------------------------------------ numpy against float64 torch
@pytest.mark.parametrize('case,kind', ALL_CASES)
def test_numpy_reference_is_float64_torch(case, kind):
    """the numpy formula, its torch twin (whose autograd gives the reference gradients) and the original module's formula on stock ops
    (avg_pool2d, spectral norm, repeat_interleave / repeat, l1_loss) agree to 1e-12 in float64, ragged shapes and every k included"""
    shape, k, _ = R.FA_CASES[case]
    f1, f2 = R.fa_inputs(case, kind)
    a, b = torch.from_numpy(f1).double(), torch.from_numpy(f2).double()
    for red in ('mean', 'sum', 'none'):
        want = R.fa_loss(f1, f2, k, red)
        if case == 'pooled_1x1':
            assert not np.asarray(want).any()
        for fn in (R.fa_loss_torch64, R.fa_loss_stock):
            got = fn(a, b, k, red).numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), (fn.__name__, red)


@pytest.mark.parametrize('name', ['rank1', 'same'])
def test_numpy_reference_is_float64_torch_on_the_special_maps(name):
    f1, f2 = R.special_inputs(name)
    a, b = torch.from_numpy(f1).double(), torch.from_numpy(f2).double()
    for red in ('mean', 'sum', 'none'):
        want = R.fa_loss(f1, f2, 8, red)
        assert np.abs(R.fa_loss_torch64(a, b, 8, red).numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), red


def test_reference_nan_and_inf_poison_one_slice_only():
    """one NaN or one +inf in a slice of fm1: every 'none' row of that slice is NaN (the original divides the whole map by its norm), the other
    slices are untouched"""
    f1, f2 = R.fa_inputs('vec8_T8_C2', 'normal')
    clean = R.fa_loss(f1, f2, 8, 'none')
    for bad in (np.nan, np.inf):
        f = f1.copy(); f[1, 0, 9, 11] = bad
        none = R.fa_loss(f, f2, 8, 'none')
        assert np.isnan(none[1, 0]).all()
        keep = np.ones((2, 2), bool); keep[1, 0] = False
        assert np.array_equal(none[keep], clean[keep])
        assert np.isnan(R.fa_loss(f, f2, 8, 'mean')) and np.isnan(R.fa_loss(f, f2, 8, 'sum'))


# ------------------------------------------------------------------------------------------------ the gap floor
@pytest.mark.parametrize('case,kind', [ck for ck in R.fa_gradient_cases() if not R.fa_exempt(ck[0])])
def test_gradient_cases_meet_the_gap_floor(case, kind):
    """the 1 x 1 pooled map is exempt: S1 = S2 = 1, every pair an exact tie with sign 0 on both sides"""
    shape, k, _ = R.FA_CASES[case]
    gap = R.min_gap(*R.fa_inputs(case, kind), k)
    print(f'{case} {kind}: min gap {gap:.2e}')
    assert gap >= R.GAP_FLOOR


def test_gradient_case_table_is_what_the_seed_search_allows():
    """every (case, kind) with a gradient is in the table, bar the one the seed table documents as impossible"""
    want = {(c, kd) for c, (_, _, grad) in R.FA_CASES.items() if grad for kd in R.FA_KINDS}
    assert want - set(R.fa_gradient_cases()) == {('wide_rank4', 'uniform')}
    assert R.min_gap(*R.special_inputs('rank1'), 8) >= R.GAP_FLOOR


def test_forward_bound_holds_a_host_model_of_the_kernels():
    """the first-order bound of forward_bounds is no blank cheque: it stays within 1e-2 of the loss even on signed inputs, whose pooled cells cancel to an eighth of mean |x|; and it does hold
    the arithmetic it was derived for: pooling by float32 additions in the scalar kernel's order and one float32 multiplication, G, lambda and
    G / lambda in float64, S rounded to float32, float32 differences"""
    f32 = np.float32
    for case, kind in ALL_CASES:
        shape, k, _ = R.FA_CASES[case]
        f1, f2 = R.fa_inputs(case, kind)
        none, bound, total, total_bound = R.forward_bounds(f1, f2, k)
        assert np.array_equal(none, R.fa_loss(f1, f2, k, 'none'))
        if case == 'pooled_1x1':
            assert not none.any()
            continue
        assert total_bound <= 1e-2 * total, (case, kind, total_bound / total)
        S = []
        for f in (f1, f2):
            B, C, H, W = f.shape
            hp, wp = H // k, W // k
            acc = np.zeros((B, C, hp, wp), f32)
            for r in range(k):
                for q in range(k):
                    acc = acc + f[:, :, r:hp * k:k, q:wp * k:k]
            X = (acc * (f32(1) / f32(k * k))).astype(F64)
            G = R.gram(X)
            S.append((G / R.top_eigenvalue(G)[:, :, None, None]).astype(f32).reshape(B, C, -1))
        got = np.abs(S[0][:, :, :, None] - S[1][:, :, None, :]).reshape(none.shape)
        assert got.dtype == f32
        ratio = float((np.abs(got - none) / bound).max())
        print(f'{case} {kind}: host model error / bound {ratio:.3f}, bound / loss {total_bound / total:.1e}')
        assert ratio <= 1.0, (case, kind, ratio)


# ------------------------------------------------------------------------------------------------ MSE, loss mix, NaN flag
def test_mse_loss_mix_and_nan_flag_references():
    rs = np.random.RandomState(3)
    a, b = rs.standard_normal(1025).astype(np.float32), rs.standard_normal(1025).astype(np.float32)
    at = torch.from_numpy(a).double().requires_grad_(True)
    loss = F.mse_loss(at, torch.from_numpy(b).double())
    (0.25 * loss).backward()
    assert abs(R.mse(a, b) - loss.item()) <= 1e-14 * loss.item()
    assert np.abs(R.mse_grad(a, b, 0.25) - at.grad.numpy()).max() <= 1e-15 * np.abs(at.grad.numpy()).max()
    b2 = b.copy(); b2[7] = np.nan
    assert np.isnan(R.mse(a, b2)) and R.nan_flag(a, None) == 0 and R.nan_flag(a, b2) == 1 and R.nan_flag(np.float32([np.inf, -np.inf, 1e-45])) == 0
    v = R.loss_mix(1.5, 0.25, 3.0, 0.1, 2.0, 3)
    assert v.dtype == np.float32 and np.array_equal(v, np.float32([1.5, np.float32(0.1) * np.float32(0.25), 6.0,
                                                                   np.float32(np.float32(1.5) + np.float32(0.1) * np.float32(0.25)) + np.float32(6.0), 3.0]))
    assert np.array_equal(R.loss_mix(1.5, None, None, 0.1, 2.0, None), np.float32([1.5, 0, 0, 1.5, 0]))
    v = R.loss_mix(1.5, np.nan, 3.0, 0.1, 2.0, 0)
    assert np.isnan(v[1]) and np.isnan(v[3]) and v[0] == 1.5 and v[2] == 6.0 and v[4] == 0

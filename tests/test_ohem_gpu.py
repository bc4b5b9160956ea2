"""OHEM cross entropy on the device: hard-pixel selection as a rewrite of the target, against tests/ohem_ref.py.

    dsrl_ohem_select + dsrl_ohem_apply   on uploaded p: stats and the rewritten target equal the exact float32 reference (OR.select), byte for byte
    dsrl_ohem_prob                       |p - p64| <= (C + 3) 2^-23 p64 + 2^-149 C against the float64 probability of the same fp32 logits; the
                                         sentinel 2.0 exactly on the pixels that are no candidates; the NaN flag only where the float64 sum is NaN
    dsrl_ohem_target / HF.ohem_target    on guarded cases (OR.make_case: no p within 1e-5 of thr): the target of OR.rewrite, byte for byte
    HF.fused_losses / cross_entropy      with ohem= : loss, dx, dw, db bit-identical to the same call without ohem on the reference's rewritten target
    TrainStep(ohem=), train_or_resume    captured == eager, off == absent, validation unmined, the unfused path, dataset['ohem']

Where a case cannot be guarded (the TrainStep's own logits: tens of thousands of probabilities around 1 / 19), the loss is compared within a
bound formed from the reference alone: the pixels whose float64 p lies within the guard of thr may fall either side, each moves the mean by at
most (largest - smallest nll) / (kept - such pixels); the fp32 loss itself gets test_cross_entropy_edges' bound."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gen                     # noqa: E402
import ohem_ref as OR          # noqa: E402
from hip_helpers import DEV, HF, dev, host, make_head   # noqa: E402
from test_class_weighted_ce_gpu import _five, make_weights     # noqa: E402
from test_cross_entropy_edges import LOSS_REL, M_ULPS, make_case, ulp32     # noqa: E402

import dualsuperreslearningforsemseg_amd as D                  # noqa: E402

SIZES = [1, 2, 255, 257, 4097, 70001]
THRESHES = [0.0, 0.7, 1.0]


def _lib():
    from dualsuperreslearningforsemseg_amd._lib import call, query
    return call, query


def _bits32(x):
    return np.asarray(x, np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------ select + apply
class SelectRig:
    """p and the labels uploaded once (at an offset of p_off floats / t_off bytes from a 16-byte boundary); run() is dsrl_ohem_select +
    dsrl_ohem_apply.  The workspace is pre-filled with 0xAB (nothing in it needs zeroing), stats with -1, the output buffer with 7."""

    def __init__(self, p32, tg, ii, p_off=0, t_off=0, inplace=False):
        _, query = _lib()
        self.p32, self.tg, self.ii, self.P, self.inplace = p32, tg, ii, p32.size, inplace
        P = self.P
        self.pbuf = torch.zeros(P + 8, dtype=torch.float32, device=DEV)
        assert self.pbuf.data_ptr() % 16 == 0
        self.p = self.pbuf[p_off:p_off + P]
        self.p.copy_(torch.from_numpy(p32.view(np.int32)).to(DEV).view(torch.float32))       # (as integers: a NaN keeps its bits)
        self.tbuf = torch.zeros(P + 8, dtype=torch.uint8, device=DEV)
        self.t = self.tbuf[t_off:t_off + P]
        self.obuf = torch.zeros(P + 8, dtype=torch.uint8, device=DEV)
        self.o = self.t if inplace else self.obuf[t_off:t_off + P]
        self.t_off = t_off
        self.ws = torch.empty(query('dsrl_ohem_workspace_bytes', P), dtype=torch.uint8, device=DEV)
        self.stats = torch.empty(4, dtype=torch.int32, device=DEV)

    def run(self, thresh, min_kept):
        call, _ = _lib()
        P, st = self.P, HF._stream()
        self.t.copy_(torch.from_numpy(self.tg).to(DEV))
        self.obuf.fill_(7); self.ws.fill_(0xAB); self.stats.fill_(-1)
        call('dsrl_ohem_select', self.p.data_ptr(), P, thresh, min_kept, self.stats.data_ptr(), self.ws.data_ptr(), self.ws.numel(), st)
        call('dsrl_ohem_apply', self.p.data_ptr(), self.t.data_ptr(), P, self.ii, self.stats.data_ptr(), self.o.data_ptr(), st)
        torch.cuda.synchronize()
        if not self.inplace:
            ob = self.obuf.cpu().numpy()
            assert np.all(ob[:self.t_off] == 7) and np.all(ob[self.t_off + P:] == 7), 'wrote outside target_out'
            assert np.array_equal(self.t.cpu().numpy(), self.tg), 'the input target changed'
        return self.stats.cpu().numpy().view(np.uint32).copy(), self.o.cpu().numpy().copy()

    def check(self, thresh, min_kept, name):
        bits, n, kept, below, keep = OR.select(self.p32, thresh, min_kept)
        stats, out = self.run(thresh, min_kept)
        want = np.where(keep, self.tg, np.uint8(self.ii)).astype(np.uint8)
        assert stats.tolist() == [bits, n, kept, below], (name, thresh, min_kept, stats.tolist(), [bits, n, kept, below])
        assert np.array_equal(out, want), (name, thresh, min_kept, int((out != want).sum()))
        return stats, out


def _min_kepts(n):
    return sorted({0, 1, max(n - 1, 0), n, 10 * n})


def _random_p(P, rs, sentinels=0.2):
    p = (rs.uniform(0, 1, P) ** rs.choice([0.3, 1.0, 3.0])).astype(np.float32)
    if P > 4:
        p[rs.uniform(size=P) < 0.2] = p[rs.randint(P)]                         # ties
    p[rs.uniform(size=P) < sentinels] = OR.SENTINEL
    return p


@pytest.mark.parametrize('P', SIZES)
def test_select_and_apply_equal_the_reference_at_every_size(P):
    rs = np.random.RandomState(P)
    for ii, trial in ((255, 0), (0, 1)):
        p = _random_p(P, rs)
        if trial == 0:
            p[0] = np.float32(0.25)                                             # at least one candidate
        tg = rs.randint(0, 19, P).astype(np.uint8)
        rig = SelectRig(p, tg, ii)
        n = int((p < 2).sum())
        for thresh in THRESHES:
            for mk in _min_kepts(n):
                rig.check(thresh, mk, f'P={P} ii={ii}')


def _value_cases():
    P = 4097
    rs = np.random.RandomState(99)
    cases = {}
    p = np.full(P, 0.3, np.float32); p[rs.uniform(size=P) < 0.1] = OR.SENTINEL
    cases['all_equal'] = p
    p = _random_p(P, rs); p[rs.uniform(size=P) < 0.6] = np.float32(0.5)
    cases['ties_at_kth'] = p                                                    # the median is 0.5: thr = 0.5, none of the ties is kept
    cases['lowest_digit'] = _bits32(0x3F000000 + rs.randint(0, 4, P))
    edges = np.array([0x3EFFFFFF, 0x3F000000, 0x3F0000FF, 0x3F000100, 0x3EFFFF00, 0x3F00FFFF, 0x3F010000, 0x3EFF0000, 0x3F333333, 0x3F333334], np.uint32)
    cases['digit_boundaries'] = _bits32(edges[rs.randint(0, edges.size, P)])
    sp = np.concatenate([np.zeros(1, np.uint32), np.arange(1, 300, dtype=np.uint32), np.array([0x007FFFFF, 0x00800000, 0x3F800000, 0x7FC00000,
                         0x80000000, 0x7FC00001], np.uint32)])                  # 0, denormals, the smallest normal, 1.0, NaNs, -0
    p = _random_p(P, rs).view(np.uint32).copy(); idx = rs.permutation(P)[:3 * sp.size]; p[idx] = np.tile(sp, 3)
    cases['specials'] = _bits32(p)
    p = _random_p(P, rs); p[7] = np.float32('nan')
    cases['one_nan'] = p
    cases['n0'] = np.full(P, OR.SENTINEL, np.float32)
    p = np.full(P, OR.SENTINEL, np.float32); p[4000] = np.float32(0.9)
    cases['n1'] = p
    return cases


VALUE_CASES = _value_cases()


@pytest.mark.parametrize('name', sorted(VALUE_CASES))
def test_select_and_apply_on_hard_values(name):
    p = VALUE_CASES[name]
    tg = np.random.RandomState(5).randint(0, 19, p.size).astype(np.uint8)
    rig = SelectRig(p, tg, 255)
    with np.errstate(invalid='ignore'):
        n = int((~(p >= 2)).sum())
    for thresh in THRESHES + [0.5, 0.3]:
        for mk in sorted(set(_min_kepts(n)) | {n // 2, n // 3}):
            stats, out = rig.check(thresh, mk, name)
    if name == 'ties_at_kth':
        stats, out = rig.check(0.0, n // 2, name)
        assert stats[0] == int(np.float32(0.5).view(np.uint32)) and np.all(out[p == np.float32(0.5)] == 255), 'a tie at thr was kept'
    if name == 'one_nan':
        stats, out = rig.check(0.0, 5, name)
        assert out[7] == tg[7], 'the NaN pixel was not kept'


def test_select_and_apply_repeat_unaligned_and_in_place():
    P = 70001
    rs = np.random.RandomState(3)
    p = _random_p(P, rs)
    tg = rs.randint(0, 19, P).astype(np.uint8)
    n = int((p < 2).sum())
    want = None
    for p_off, t_off, inplace in ((0, 0, False), (1, 3, False), (3, 1, False), (0, 0, True), (2, 5, True)):
        rig = SelectRig(p, tg, 255, p_off, t_off, inplace)
        a = rig.check(0.7, n // 4, f'offsets {p_off} {t_off} {inplace}')
        b = rig.run(0.7, n // 4)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), 'two calls differ'
        if want is None:
            want = a
        assert a[0].tobytes() == want[0].tobytes() and a[1].tobytes() == want[1].tobytes(), 'the placement of the buffers changed the result'


# ------------------------------------------------------------------------------------------------------------------------------ probabilities
PROB_CASES = ['randn', 'spread', 'offset_1e4', 'onehot', 'neginf_some', 'bad_label', 'nan_live']


def run_prob(lg, tg, ii, layout):
    """dsrl_ohem_prob -> (p, flag).  dense: ld == C on an aligned base; offset4: ld == C, the base 4 bytes past a 16-byte boundary; slice: a channel
    slice of a wider tensor (ld = C + 5, 8 bytes past the base)"""
    call, _ = _lib()
    P, C = lg.shape
    if layout == 'slice':
        buf = torch.full((P, C + 5), 7.0, device=DEV); buf[:, 2:2 + C] = torch.tensor(lg, device=DEV)
        ptr, ld = buf.data_ptr() + 8, C + 5
    elif layout == 'offset4':
        buf = torch.full((P * C + 4,), 7.0, device=DEV); buf[1:1 + P * C] = torch.tensor(lg.reshape(-1), device=DEV)
        ptr, ld = buf.data_ptr() + 4, C
    else:
        buf = torch.tensor(lg, device=DEV)
        ptr, ld = buf.data_ptr(), C
        assert ptr % 16 == 0
    target = torch.tensor(tg, device=DEV)
    out = torch.full((P + 2,), 7.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    call('dsrl_ohem_prob', ptr, ld, target.data_ptr(), P, C, ii, out.data_ptr() + 4, flag.data_ptr(), HF._stream())
    torch.cuda.synchronize()
    o = host(out)
    assert o[0] == 7.0 and o[-1] == 7.0, 'wrote outside p_out'
    return o[1:-1], int(flag)


@pytest.mark.parametrize('C', [1, 19, 60])
@pytest.mark.parametrize('case', PROB_CASES)
def test_probabilities_against_float64(case, C):
    P = 300                                                                         # two blocks, the second one partial
    for ii in ((255, 0) if C > 1 else (255, 7)):                                    # (C == 1 with ignore 0 has no live pixel)
        rs = np.random.RandomState(1000 * C + 10 * PROB_CASES.index(case) + (ii & 1))
        lg, tg = make_case(case, P, C, rs, ii)
        p64, cand = OR.target_probability64(lg, tg, ii)
        with np.errstate(invalid='ignore', over='ignore'):
            x = lg.astype(np.float64)
            nan_sum = bool(np.isnan(np.exp(x - x.max(axis=1, keepdims=True)).sum(axis=1)).any())
        # the float64 sum is NaN in the NaN case alone (and where the only class of C == 1 is -inf: -inf - -inf)
        assert nan_sum == (case == 'nan_live' or (case == 'neginf_some' and C == 1)), (case, C)
        if case == 'bad_label':
            assert (~cand & (tg != ii)).any()
        got = {}
        for layout in ('dense', 'offset4', 'slice'):
            p, flag = run_prob(lg, tg, ii, layout)
            got[layout] = p
            assert np.array_equal(p == OR.SENTINEL, ~cand), f'{case} C={C} {layout}: the sentinel is not exactly on the pixels that are no candidates'
            err = np.abs(p[cand].astype(np.float64) - p64[cand])
            bound = (C + 3) * 2.0 ** -23 * p64[cand] + 2.0 ** -149 * C
            print(f'{case} C={C} ii={ii} {layout}: max error / bound = {float((err / bound).max(initial=0.0)):.3f}')
            assert not np.isnan(p).any() and np.all(err <= bound), f'{case} C={C} {layout}: error {err.max():.3e} beyond the bound'
            assert flag == (1 if nan_sum else 0), (case, C, layout, flag)
        assert got['dense'].tobytes() == got['offset4'].tobytes() == got['slice'].tobytes(), 'the layout changed the bits'


# ------------------------------------------------------------------------------------------------------------------------------ the rewritten target
@pytest.mark.parametrize('ii', [255, 0, 18])
def test_ohem_target_on_guarded_cases_is_the_reference_byte_for_byte(ii):
    call, query = _lib()
    N, H, W, C = 3, 40, 70, 19                                                       # 8400 pixels: three histogram blocks, 33 tiles
    P = N * H * W
    for thresh, mk in ((0.7, P // 4), (0.9, P // 4), (0.0, P // 2), (0.3, P // 2)):
        lg, tg, thresh, mk, _ = OR.make_case(P, C, 11 + ii, ii, thresh, mk)
        want, thr, n, kept = OR.rewrite(lg, tg, ii, thresh, mk)
        # the entry point itself
        lgd = torch.tensor(lg, device=DEV); tgd = torch.tensor(tg, device=DEV)
        out = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
        stats = torch.full((4,), -1, dtype=torch.int32, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.full((query('dsrl_ohem_workspace_bytes', P),), 0xAB, dtype=torch.uint8, device=DEV)
        call('dsrl_ohem_target', lgd.data_ptr(), C, tgd.data_ptr(), P, C, ii, thresh, mk, out.data_ptr(), stats.data_ptr(), flag.data_ptr(),
             ws.data_ptr(), ws.numel(), HF._stream())
        torch.cuda.synchronize()
        s = stats.cpu().numpy().view(np.uint32)
        assert np.array_equal(out.cpu().numpy(), want), (ii, thresh, mk, int((out.cpu().numpy() != want).sum()))
        assert (int(s[1]), int(s[2])) == (n, kept) and int(flag) == 0
        assert abs(float(s[:1].view(np.float32)[0]) - thr) <= OR.GUARD
        # the Python call, on (N, C, H, W) logits and an int64 target
        logits = dev(lg.reshape(N, H, W, C).transpose(0, 3, 1, 2))
        st2 = torch.zeros(4, dtype=torch.int32, device=DEV)
        got = HF.ohem_target(logits, torch.tensor(tg.reshape(N, H, W).astype(np.int64), device=DEV), ii, thresh, mk, flag=flag, stats=st2)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W) and not got.requires_grad
        assert np.array_equal(got.cpu().numpy().reshape(-1), want)
        assert st2.cpu().numpy().tobytes() == stats.cpu().numpy().tobytes() and int(flag) == 0


# ------------------------------------------------------------------------------------------------------------------------------ end to end: the last layer
def _last_layer_inputs(N, H, ii, thresh, mk_frac, seed):
    """The layer that produces the logits at the smallest shapes its hand-over takes (W = 128): x (N, 19, H, 128), w (19, 19, 2, 2), b (19) with logits
    of a few units, labels that follow the logits' own ranking in part (the top class lifted through the bias is not possible per pixel: the easy
    share comes from the ranking alone), 10 % ignored.  Seeds are retried until the guard holds ON THE DEVICE'S OWN LOGITS."""
    C, W = 19, 128
    P = N * 4 * H * W
    mk = int(P * mk_frac)
    for s in range(seed, seed + 50):
        rs = np.random.RandomState(s)
        x = rs.standard_normal((N, C, H, W)).astype(np.float32)
        w = (rs.standard_normal((C, C, 2, 2)) * 1.5).astype(np.float32)
        b = rs.standard_normal(C).astype(np.float32)
        with torch.no_grad():
            y = HF.conv_transpose2d_k2s2(dev(x), torch.tensor(w, device=DEV), torch.tensor(b, device=DEV))
        lg = host(y).transpose(0, 2, 3, 1).reshape(P, C)
        order = np.argsort(-lg, axis=1)
        pick = rs.randint(0, 3, P)
        tg = np.where(pick < 2, order[:, 0], rs.randint(0, C, P))
        tg[rs.uniform(size=P) < 0.1] = ii
        if OR.guard_holds(lg, tg, ii, thresh, mk):
            break
    else:
        raise AssertionError('no seed satisfied the guard')
    want, thr, n, kept = OR.rewrite(lg, tg, ii, thresh, mk)
    assert (n - kept) >= 0.25 * n, f'only {n - kept} of {n} candidates dropped'
    plain, mined = OR.ce64(lg, tg, ii), OR.ce64(lg, want, ii)
    assert abs(mined - plain) > 0.05 * abs(plain), (mined, plain)
    return x, w, b, tg.astype(np.uint8).reshape(N, 2 * H, 2 * W), want.reshape(N, 2 * H, 2 * W), mk


def _last_layer_step(x, w, b, tgt, ii, weight, ohem, path, monkeypatch):
    """forward through the logits layer, the loss (fused_losses at stage 1, or cross_entropy), backward -> bytes of (loss, dx, dw, db), calls made"""
    xd = dev(x).requires_grad_(True); wd = torch.tensor(w, device=DEV, requires_grad=True); bd = torch.tensor(b, device=DEV, requires_grad=True)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    calls = []
    orig = HF.call
    monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
    try:
        h = HF.LogitsGrad() if path == 'fused' else None
        y = HF.conv_transpose2d_k2s2(xd, wd, bd, h)
        if path == 'fused':
            vals = HF.fused_losses((y, None, None, None), tgt, None, ii, 0.1, 1.0, 1, flag, weight=weight, ohem=ohem)
            assert h.armed, 'the hand-over did not engage'
            assert (h.target.data_ptr() != tgt.data_ptr()) == (ohem is not None)           # the layer is handed the rewritten target
            vals[3].backward()
            assert not h.armed
            loss = vals[0]
        else:
            loss = HF.cross_entropy(y, tgt, ii, weight=weight, ohem=ohem)
            loss.backward()
    finally:
        monkeypatch.setattr(HF, 'call', orig)
    torch.cuda.synchronize()
    assert int(flag) == 0
    return [host(t).tobytes() for t in (loss, xd.grad, wd.grad, bd.grad)], calls


@pytest.mark.parametrize('weights', ['weights', 'none'])
@pytest.mark.parametrize('N,H', [(1, 3), (2, 5)])
def test_losses_with_ohem_equal_the_call_on_the_reference_target_bit_for_bit(N, H, weights, monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    monkeypatch.setattr(HF, 'convt_ce_enabled', True)
    ii, thresh = 255, 0.7
    x, w, b, tg, want, mk = _last_layer_inputs(N, H, ii, thresh, 0.25, 40 + N)
    wt = make_weights(19, np.random.RandomState(17)) if weights == 'weights' else None
    sfx = '_w' if wt is not None else ''
    tgt, ref_t = torch.tensor(tg, device=DEV), torch.tensor(want, device=DEV)
    for path in ('fused', 'cross_entropy'):
        got, calls = _last_layer_step(x, w, b, tgt, ii, wt, (thresh, mk), path, monkeypatch)
        ref, ref_calls = _last_layer_step(x, w, b, ref_t, ii, wt, None, path, monkeypatch)
        off, _ = _last_layer_step(x, w, b, tgt, ii, wt, None, path, monkeypatch)
        assert calls.count('dsrl_ohem_target') == 1 and not [c for c in ref_calls if 'ohem' in c]
        assert [c for c in calls if 'ohem' not in c] == ref_calls, 'ohem changed the calls behind the rewrite'
        if path == 'fused':
            assert 'dsrl_convt2x2_bwd_ce' + sfx in calls and 'dsrl_ce_fused' + sfx in calls and 'dsrl_convt2x2_fwd' in calls
        for name, a, r, o in zip(('loss', 'dx', 'dw', 'db'), got, ref, off):
            assert a == r, f'{path} {weights}: {name} differs from the call on the reference target'
            assert a != o, f'{path} {weights}: {name} is what the call without ohem gives'


def test_nothing_kept_is_the_all_ignored_target(monkeypatch):
    monkeypatch.setattr(HF, 'convt_ce_enabled', True)
    ii = 255
    x, w, b, tg, _, _ = _last_layer_inputs(1, 3, ii, 0.7, 0.25, 41)
    tgt = torch.tensor(tg, device=DEV)
    none = torch.full_like(tgt, ii)
    for path in ('fused', 'cross_entropy'):
        got, _ = _last_layer_step(x, w, b, tgt, ii, None, (0.0, 0), path, monkeypatch)     # k = 0, thr = the smallest p: no p is below it
        ref, _ = _last_layer_step(x, w, b, none, ii, None, None, path, monkeypatch)
        assert got == ref, path
        assert np.isnan(np.frombuffer(got[0], np.float32)).all() and not np.frombuffer(got[1], np.float32).any()


def test_fused_losses_with_ohem_on_the_head_hands_over(monkeypatch):
    """the whole head: tens of thousands of probabilities near 1 / 19 cannot be guarded, so the value is held to the bound of the module docstring;
    the byte-exact statements are those of the last-layer tests above"""
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    monkeypatch.setattr(HF, 'convt_ce_enabled', True)
    x16, x4, target, org = gen.make_head_inputs(303, 2, 2, 8, gen.SMALL)
    w = make_weights(19, np.random.RandomState(17))
    ohem = (0.0, target.size // 4)
    head, _ = make_head(gen.SMALL, 3, 101, True)
    a = dev(x16).requires_grad_(True); b = dev(x4).requires_grad_(True)
    tgt = dev(target); o = dev(org)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with HF.logits_target(tgt, gen.IGNORE, flag, w, ohem=ohem):
        outs = head(a, b)
    h = getattr(outs[0], '_dsrl_logits_grad', None)
    assert h is not None and h.value is None                    # with ohem the producer's forward evaluates nothing
    vals = HF.fused_losses(outs, tgt, o, gen.IGNORE, 0.1, 1.0, 3, flag, weight=w, ohem=ohem)
    assert h.armed and h.weight is not None and h.target.data_ptr() != tgt.data_ptr(), 'the hand-over did not engage on the rewritten target'
    vals[3].backward()
    torch.cuda.synchronize()
    assert int(flag) == 0 and not h.armed
    ref, plain = _check_mined_loss(float(vals[0].detach()), outs, tgt, ohem, w, 'head')
    assert abs(ref - plain) > 0.05 * abs(plain)
    assert all(np.isfinite(host(p.grad)).all() for p in head.parameters()) and np.isfinite(host(a.grad)).all() and np.isfinite(host(b.grad)).all()


# ------------------------------------------------------------------------------------------------------------------------------ TrainStep, train_or_resume
ABSENT = object()


def _model_and_step(graph, ohem=ABSENT, w=None):
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import TrainStep
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    from dualsuperreslearningforsemseg_amd.ddp import FlatParams
    torch.manual_seed(77)
    model = D.DSRL(3, cs).to(DEV).to(memory_format=torch.channels_last).train()
    flat = FlatParams(model)
    HF.set_dropout_seed(1234)
    kw = {} if ohem is ABSENT else {'ohem': ohem}
    return model, TrainStep(model, flat, 3, 0.1, 1.0, cs.IGNORE_CLASS_LABEL, graph=graph, class_weights=w, **kw)


def _batch():
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import SyntheticCityscapes
    (img, org), (tgt, _) = next(iter(SyntheticCityscapes(2, (64, 128), torch.device(DEV), length=1)))
    return img, org, tgt


def _step_ohem(tgt):
    """thresh below every p of a freshly initialised model, min_kept a quarter of the batch: thr is the k-th smallest p and about three quarters
    of the pixels are dropped"""
    return (0.0, tgt.numel() // 4)


def _check_mined_loss(ce, outs, tgt, ohem, w, name):
    """the step's CE against the float64 OHEM loss of its own logits, within the bound of the module docstring; -> (reference, plain CE)"""
    lg = host(outs[0]).transpose(0, 2, 3, 1).reshape(-1, 19)
    tgh = tgt.cpu().numpy().reshape(-1)
    p64, cand = OR.target_probability64(lg, tgh, 255)
    if ohem is None:
        want, near, kept = tgh, 0, int(cand.sum())
    else:
        want, thr, n, kept = OR.rewrite(lg, tgh, 255, *ohem)
        near = int((np.abs(p64[cand] - thr) <= OR.GUARD).sum())
    ref, plain = OR.ce64(lg, want, 255, w), OR.ce64(lg, tgh, 255, w)
    nll = -np.log(p64[cand])
    wa = np.ones(19) if w is None else np.asarray(w, np.float64)
    d_ref = float(wa[want[want != 255]].sum())                  # a pixel that falls the other side moves the mean by at most max w * (nll range) / D
    flip = near * float(wa.max()) * float(nll.max() - nll.min()) / max(d_ref - near * float(wa.max()), 1e-30)
    tol = LOSS_REL * abs(ref) + M_ULPS * ulp32(float(np.abs(lg).max())) + flip
    print(f'{name}: CE {ce!r} ref {ref!r} plain {plain!r} near {near} kept {kept} error / bound = {abs(ce - ref) / tol:.3f}')
    assert abs(ce - ref) <= tol, f'{name}: CE {ce!r} vs {ref!r} (|d| = {abs(ce - ref):.3e} > {tol:.3e})'
    return ref, plain


def test_train_step_with_ohem_captured_equals_eager(monkeypatch):
    img, org, tgt = _batch()
    ohem = _step_ohem(tgt)
    res = {}
    for graph in (False, True):
        model, step = _model_and_step(graph, ohem)
        assert step.ohem == ohem and step._graph_key(img, org, tgt)[-1] == ohem
        n = step.GRAPH_WARMUP + 3                                       # graph: the eager iterations, the capture, then replays
        res[graph] = [_five(step, img, org, tgt)[0] for _ in range(n)]
        if graph:
            assert step.graph_replays >= 2, 'the OHEM step was not captured and replayed'
        step.release()
    for a, b in zip(res[False], res[True]):
        assert a.tobytes() == b.tobytes(), (res[False], res[True])
    assert all(np.isfinite(v).all() and v[4] == 0 for v in res[True])


def test_train_step_mines_in_training_only_and_off_is_absent(monkeypatch):
    for k in ('DSRL_CONVT_CE', 'DSRL_CONVT_DMA', 'DSRL_CONVT_MFMA'):
        monkeypatch.setenv(k, '1')
    monkeypatch.setattr(HF, 'convt_ce_enabled', True)
    img, org, tgt = _batch()
    ohem = _step_ohem(tgt)
    calls = []
    orig = HF.call
    monkeypatch.setattr(HF, 'call', lambda name, *args: (calls.append(name), orig(name, *args))[1])
    first, val = {}, {}
    for tag, oh in (('absent', ABSENT), ('none', None), ('false', False), ('ohem', ohem)):
        model, step = _model_and_step(False, oh)
        del calls[:]
        val[tag] = _five(step, img, org, tgt, do_train=False)[0]                    # validation first: the same weights in every run
        assert not [c for c in calls if 'ohem' in c], 'do_train=False mined'
        del calls[:]
        five, outs = _five(step, img, org, tgt)
        first[tag] = five
        assert calls.count('dsrl_ohem_target') == (1 if tag == 'ohem' else 0)
        assert ('dsrl_convt2x2_fwd_ce' in calls) == (tag != 'ohem') and 'dsrl_convt2x2_bwd_ce' in calls     # the hand-over of the gradient stays
        if tag == 'ohem':
            ref, plain = _check_mined_loss(float(five[0]), outs, tgt, ohem, None, 'do_train=True')
            assert abs(ref - plain) > 0.05 * abs(plain), 'mining does not move the loss of this batch'
        step.release()
    assert first['absent'].tobytes() == first['none'].tobytes() == first['false'].tobytes()
    assert first['ohem'][0] != first['absent'][0]
    assert val['absent'].tobytes() == val['none'].tobytes() == val['false'].tobytes() == val['ohem'].tobytes(), 'validation depends on ohem'


@pytest.mark.parametrize('weights', ['weights', 'none'])
def test_unfused_losses_of_the_train_step_use_ohem(weights):
    img, org, tgt = _batch()
    ohem = _step_ohem(tgt)
    w = make_weights(19, np.random.RandomState(23)) if weights == 'weights' else None
    for fused in (True, False):
        model, step = _model_and_step(False, ohem, w)
        step.fused_losses = fused
        five, outs = _five(step, img, org, tgt)
        ref, plain = _check_mined_loss(float(five[0]), outs, tgt, ohem, w, f'fused_losses={fused} {weights}')
        assert abs(ref - plain) > 0.05 * abs(plain)
        five, outs = _five(step, img, org, tgt, do_train=False)
        _check_mined_loss(float(five[0]), outs, tgt, None, w, f'fused_losses={fused} {weights} do_train=False')
        step.release()


def test_train_or_resume_passes_the_datasets_ohem_to_the_step(tmp_path, monkeypatch):
    from test_augment_gpu import _cache_tree
    from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as cs
    data, _ = _cache_tree(tmp_path)
    seen = []

    class Spy(TR.TrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append(self.ohem)

    monkeypatch.setattr(TR, 'TrainStep', Spy)

    def run(tag, **ds):
        torch.manual_seed(1234)
        HF.set_dropout_seed(77)
        kw = dict(device='gpu', distributed=None, mixed_precision=None, disable_cudnn_benchmark=False, num_workers=0,
                  dataset=dict({'path': data, 'settings': cs}, **ds), val_interval=1, checkpoint_interval=1, checkpoint_history=2,
                  init_weights=None, batch_size=2, epochs=1, learning_rate=0.006, end_learning_rate=0.0005, momentum=0.9, weights_decay=5e-4,
                  poly_power=0.9, stage=3, w1=0.1, w2=1.0, freeze_batch_norm=False, experiment_id=str(tmp_path / tag), description='test',
                  early_stopping=False, pretrained_backbone=False, model_input_size=(32, 64))
        return TR.train_or_resume(is_resuming_training=False, **kw)

    h1 = run('a', ohem={'thresh': 0.0, 'min_kept': 500})
    assert seen == [(0.0, 500)]
    assert all(np.isfinite(v) for v in h1[0]['train'][:4]) and h1[0]['train'][0] > 0 and np.isfinite(h1[0]['val'][3])
    h0 = run('b')
    assert seen[1] is None
    assert h0[0]['train'][0] != h1[0]['train'][0]                      # mining changes the training loss
    with pytest.raises(ValueError, match='ohem'):
        run('c', ohem=(0.7, -5))
    with pytest.raises(ValueError, match='ohem'):
        run('d', ohem=True, focal_gamma=2.0)
    assert len(seen) == 2 and not os.path.exists(str(tmp_path / 'c')) and not os.path.exists(str(tmp_path / 'd'))

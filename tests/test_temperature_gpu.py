"""GPU checks of temperature scaling: the record of dsrl_temperature_stats against tests/temperature_ref.py (float64, and the float32 restatement
that sets the accuracy bound), its flags and argument checks; beta applied in the fused tails (dsrl_sssr_tail_predict_t / _flip_t), in
dsrl_calibration_from_logits_t and in the module-by-module fall-back; the fit_temperature command and benchmark(temperature=) end to end."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import calibration_ref as CR
import gen
import predict_flip_ref as PFR
import temperature_ref as R

pytestmark = pytest.mark.gpu

NC = gen.NUM_CLASSES
IGNORE = gen.IGNORE
B = CR.DEFAULT_BINS
# (N, H, W): 265 pixels = two tiles with a short last one; 30720 = 120 tiles, one per block; 266240 = 1040 tiles > 1024 blocks: a second round for 16 of them
SHAPES = [(1, 5, 53), (2, 96, 160), (1, 512, 520)]
MARGIN = 4.0            # exp_nonpos is within 2 ulp where numpy's float32 exp is within 1, and C of them are summed


def _helpers():
    import hip_helpers as H
    return H


def _grid16():
    from dualsuperreslearningforsemseg_amd import functional as HF
    return HF.temperature_grid(0.25, 4.0, 16)


K1 = 9                  # the K = 1 cases take this point of the 16-point grid (beta = 1.32), so that one reference serves both


@functools.lru_cache(maxsize=None)
def _case(shape, C):
    """rows (P, C) float32 logits, labels (P,) with ~10 % ignored, and the float64 / float32 reference records over the 16-point grid with the
    magnitudes the errors are measured against; computed once and shared: read-only"""
    N, Hh, W = shape
    P = N * Hh * W
    rs = np.random.RandomState(P + C)
    rows = (3.0 * rs.standard_normal((P, C))).astype(np.float32)
    labels = rs.randint(0, C, P).astype(np.uint8)
    labels[rs.uniform(size=P) < 0.1] = IGNORE
    b = _grid16()
    rec64, mag = R.record(rows, labels, b, IGNORE)
    rec32, _ = R.record(rows, labels, b, IGNORE, dtype=np.float32)
    return rows, labels, b, rec64, rec32, mag


def _pick(rec, ks):
    return np.concatenate([rec[:1]] + [rec[1 + 3 * k:4 + 3 * k] for k in ks])


def _dev_rows(rows, ld):
    """the rows on the device as a pixel-major buffer with pixel stride ld; pad columns hold 1e30"""
    H = _helpers()
    buf = np.full((rows.shape[0], ld), 1e30, np.float32)
    buf[:, :rows.shape[1]] = rows
    return torch.from_numpy(buf).to(H.DEV)


def _stats(logits, ld, target, C, betas, record=None, flag=None, ignore=IGNORE):
    """dsrl_temperature_stats straight through the C entry point; -> the record tensor"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    K = len(betas)
    bt = betas if isinstance(betas, torch.Tensor) else torch.tensor(np.asarray(betas, np.float32)).to(H.DEV)
    rec = torch.zeros(1 + 3 * K, dtype=torch.float64, device=H.DEV) if record is None else record
    P = target.numel()
    nbytes = HF.cquery('dsrl_temperature_workspace_bytes', P, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=H.DEV)
    HF.call('dsrl_temperature_stats', logits.data_ptr(), ld, target.data_ptr(), P, C, ignore, bt.data_ptr(), K, rec.data_ptr(),
            None if flag is None else flag.data_ptr(), ws.data_ptr(), nbytes, HF._stream())
    return rec


def _flag():
    return torch.zeros((), dtype=torch.int32, device=_helpers().DEV)


def _np(t):
    return t.cpu().numpy()


def _entry_errors(rec, rec64, mag):
    """per term (L, G, H): the maximum over the betas of |entry - float64| / sum over the pixels of |term|"""
    e = np.abs(rec[1:] - rec64[1:]) / mag[1:]
    return e[0::3].max(), e[1::3].max(), e[2::3].max()


# ---------------------------------------------------------------------------------------------- the record against the reference
@pytest.mark.parametrize('pad', [0, 5], ids=['dense', 'ld_C_plus_5'])
@pytest.mark.parametrize('K', [1, 16])
@pytest.mark.parametrize('C', [19, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '{}x{}x{}'.format(*s))
def test_record_against_the_reference(shape, C, K, pad):
    """For each of L, G and H: the error of an entry is |device - float64| / sum over the pixels of |term|, and its maximum over the betas must be at
    most 4 x the same figure of the float32 restatement (tests/temperature_ref.py: float32 terms with numpy's float32 exp, sums in float64).  The
    margin is 4 because exp_nonpos is within 2 ulp where numpy's float32 exp is within 1, and C of them are summed.  [0] is exact.
    Measured on the MI355X when this test first passed (device | restatement, dense and padded rows alike):
      265 px     C=19 K=16  L 6.7e-9 | 6.7e-9    G 6.3e-9 | 7.3e-9    H 2.1e-8 | 2.4e-8       C=2 K=16  L 4.6e-9 | 5.4e-9   G 4.1e-9 | 3.6e-9   H 1.4e-8 | 1.9e-8
      30720 px   C=19 K=1   L 4.0e-10 | 4.4e-10  G 1.3e-10 | 5.1e-11  H 2.2e-9 | 2.4e-9       C=19 K=16 L 1.6e-9 | 1.6e-9   G 3.9e-9 | 2.7e-9   H 5.5e-9 | 5.8e-9
      266240 px  C=19 K=1   L 2.6e-10 | 1.8e-10  G 8.8e-12 | 4.5e-11  H 1.6e-9 | 1.4e-9       C=19 K=16 L 1.5e-9 | 1.5e-9   G 1.7e-9 | 4.3e-10  H 5.3e-9 | 5.1e-9
    The worst ratio of the 24 cases is 3.96 (G at 266240 px, C=19, K=16).  With the device's logf in place of log_ge1 (csrc/common.h) the L entries
    were 1.9e-9 ... 2.3e-8 against 1.8e-10 ... 6.7e-9, up to 15 x the restatement: logf is 3.1e-8 relative low on average, and the sum keeps it."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    rows, labels, b, rec64, rec32, mag = _case(shape, C)
    ks = list(range(16)) if K == 16 else [K1]
    betas = b[ks]
    if pad:
        rec = _stats(_dev_rows(rows, C + pad), C + pad, torch.from_numpy(labels).to(H.DEV), C, betas)
    else:
        # the wrapper: (N, C, H, W) logits in channels-last memory are the rows as they are
        N, Hh, W = shape
        L4 = H.dev(np.ascontiguousarray(rows.reshape(N, Hh, W, C).transpose(0, 3, 1, 2)))
        rec = torch.zeros(1 + 3 * K, dtype=torch.float64, device=H.DEV)
        flag = _flag()
        assert HF.temperature_stats_(rec, L4, H.dev(labels.reshape(N, Hh, W)), betas, IGNORE, flag) is rec and int(flag.item()) == 0
    got = _np(rec)
    want64, want32, m = _pick(rec64, ks), _pick(rec32, ks), _pick(mag, ks)
    assert got[0] == want64[0] == (labels != IGNORE).sum()
    dev, ref = _entry_errors(got, want64, m), _entry_errors(want32, want64, m)
    print(f'{shape} C={C} K={K} pad={pad}: device L {dev[0]:.3e} G {dev[1]:.3e} H {dev[2]:.3e} | float32 restatement L {ref[0]:.3e} G {ref[1]:.3e} H {ref[2]:.3e}')
    for name, d, r in zip('LGH', dev, ref):
        assert d <= MARGIN * r, f'{name}: device {d:.3e} > {MARGIN:g} x restatement {r:.3e}'


def test_fit_on_the_device_record_matches_the_reference_solution():
    """the solver on the device's record lands where it lands on the float64 record: the record's error is far below the solver's"""
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.metrices import TemperatureFit
    H = _helpers()
    shape, C = SHAPES[1], 19
    rows, labels, b, rec64, _, _ = _case(shape, C)
    N, Hh, W = shape
    L4 = H.dev(np.ascontiguousarray(rows.reshape(N, Hh, W, C).transpose(0, 3, 1, 2)))
    tg = H.dev(labels.reshape(N, Hh, W))
    fit = TemperatureFit(b, IGNORE)
    fit.update_from_logits(L4[:1], tg[:1])
    fit.update_from_logits(L4[1:], tg[1:])
    other = TemperatureFit(b, IGNORE)
    other.merge(fit)
    f = other.result()
    # random labels: the NLL falls all the way to beta -> 0, the fit ends at the lower bound
    assert f['at_bound'] and f['beta'] == 0.25 and f['temperature'] == 4.0 and f['pixels'] == rec64[0]
    assert HF.temperature_solve(b, rec64) == (0.25, True)
    assert np.allclose(f['nll'], rec64[1::3] / rec64[0], rtol=1e-6)
    fit.reset()
    assert not _np(fit.record).any() and fit.result()['pixels'] == 0


# ---------------------------------------------------------------------------------------------- determinism, accumulation, flags
def test_identical_bits_accumulation_and_all_ignored():
    H = _helpers()
    rows, labels, b, _, _, _ = _case(SHAPES[2], 19)
    lg, tg = _dev_rows(rows, 19), torch.from_numpy(labels).to(H.DEV)
    one = _stats(lg, 19, tg, 19, b)
    two = _stats(lg, 19, tg, 19, b)
    assert _np(one).tobytes() == _np(two).tobytes()
    _stats(lg, 19, tg, 19, b, record=two)
    assert np.array_equal(_np(two), 2.0 * _np(one)) and np.isfinite(_np(two)).all()
    flag = _flag()
    zero = _stats(lg, 19, torch.full_like(tg, IGNORE), 19, b, flag=flag)
    assert _np(zero).tobytes() == np.zeros(49).tobytes() and int(flag.item()) == 0


def test_extreme_logits_stay_finite():
    """Logits scaled to +-1e4 with beta = 4: every exponential but the maximum's underflows (s = 1, a = q = 0), so L = -beta d_t and G = -d_t: one
    rounded difference and one rounded product per pixel, each within 2^-24 relative - the sums are held to 2^-22 of the magnitude, H to finite."""
    H = _helpers()
    rows, labels, _, _, _, _ = _case(SHAPES[0], 19)
    big = (rows * np.float32(1e4 / np.abs(rows).max())).astype(np.float32)
    assert np.abs(big).max() > 9.9e3
    flag = _flag()
    got = _np(_stats(_dev_rows(big, 19), 19, torch.from_numpy(labels).to(H.DEV), 19, [4.0, 1.0], flag=flag))
    want, mag = R.record(big, labels, [4.0, 1.0], IGNORE)
    assert np.isfinite(got).all() and int(flag.item()) == 0 and got[0] == want[0]
    for k in (0, 1):
        for j in (1, 2):            # L, G
            assert abs(got[3 * k + j] - want[3 * k + j]) <= 2.0 ** -22 * mag[3 * k + j], (k, j, got, want)
    assert got[1] > 1e4 * got[0]


def test_nan_logit_foreign_label_and_bad_betas():
    H = _helpers()
    C = 19
    rows, labels, b, rec64, _, mag = _case(SHAPES[0], C)
    tg = torch.from_numpy(labels).to(H.DEV)
    live = np.nonzero(labels != IGNORE)[0]
    # a NaN logit of a live pixel: bit 0, and the NaN reaches every sum (the count stays)
    bad = rows.copy()
    bad[live[3], 7] = np.nan
    flag = _flag()
    got = _np(_stats(_dev_rows(bad, C), C, tg, C, b[:4], flag=flag))
    assert int(flag.item()) == 1 and got[0] == live.size and np.isnan(got[1:]).all()
    # of an ignored pixel: nothing
    dead = np.nonzero(labels == IGNORE)[0]
    bad = rows.copy()
    bad[dead[0], 0] = np.nan
    flag = _flag()
    clean = _np(_stats(_dev_rows(rows, C), C, tg, C, b[:4]))
    got = _np(_stats(_dev_rows(bad, C), C, tg, C, b[:4], flag=flag))
    assert int(flag.item()) == 0 and got.tobytes() == clean.tobytes()
    # a label C (and 200) that is not the ignore label: bit 1, left out of [0] and of the sums
    foreign = labels.copy()
    foreign[live[5]] = C
    foreign[live[200]] = 200
    flag = _flag()
    got = _np(_stats(_dev_rows(rows, C), C, torch.from_numpy(foreign).to(H.DEV), C, b[:4], flag=flag))
    without = labels.copy()
    without[live[5]] = without[live[200]] = IGNORE
    want = _np(_stats(_dev_rows(rows, C), C, torch.from_numpy(without).to(H.DEV), C, b[:4]))
    assert int(flag.item()) == 2 and got[0] == live.size - 2 and got.tobytes() == want.tobytes()
    # a beta of 0 / inf / NaN passed straight to the C entry point: its own entries NaN, the others those of a call without it
    betas = np.array([0.5, 0.0, 1.0, np.inf, np.nan, 2.0, -1.0], np.float32)
    flag = _flag()
    got = _np(_stats(_dev_rows(rows, C), C, tg, C, betas, flag=flag))
    good = _np(_stats(_dev_rows(rows, C), C, tg, C, betas[[0, 2, 5]]))
    assert int(flag.item()) == 0 and got[0] == good[0]
    for k in (1, 3, 4, 6):
        assert np.isnan(got[1 + 3 * k:4 + 3 * k]).all(), k
    for j, k in enumerate((0, 2, 5)):
        assert got[1 + 3 * k:4 + 3 * k].tobytes() == good[1 + 3 * j:4 + 3 * j].tobytes(), k


def test_every_argument_check_returns_its_code_without_a_launch():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import _lib, functional as HF
    lib = _lib.load()
    C, P, K = 19, 300, 4
    lg = torch.zeros((P, C + 1), device=H.DEV)
    tg = torch.zeros(P, dtype=torch.uint8, device=H.DEV)
    bt = torch.ones(16, device=H.DEV)
    sentinel = np.arange(1 + 3 * 16, dtype=np.float64) + 0.5
    rec = torch.from_numpy(sentinel.copy()).to(H.DEV)
    nbytes = HF.cquery('dsrl_temperature_workspace_bytes', P, K)
    ws = torch.zeros(nbytes + 64, dtype=torch.uint8, device=H.DEV)
    flag = _flag()
    st = HF._stream()
    BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3

    def run(**kw):
        a = dict(logits=lg.data_ptr(), ld=C + 1, target=tg.data_ptr(), P=P, C=C, betas=bt.data_ptr(), K=K, record=rec.data_ptr(), ws=ws.data_ptr(),
                 ws_bytes=nbytes)
        a.update(kw)
        return lib.dsrl_temperature_stats(a['logits'], a['ld'], a['target'], a['P'], a['C'], IGNORE, a['betas'], a['K'], a['record'], flag.data_ptr(),
                                          a['ws'], a['ws_bytes'], st)

    assert run() == 0
    torch.cuda.synchronize()
    after = _np(rec).copy()
    assert after[0] == sentinel[0] + P and np.array_equal(after[1 + 3 * K:], sentinel[1 + 3 * K:])       # K entries and no more
    for kw, code in (({'logits': None}, BADARG), ({'target': None}, BADARG), ({'betas': None}, BADARG), ({'record': None}, BADARG), ({'ws': None}, BADARG),
                     ({'P': 0}, BADARG), ({'K': 0}, BADARG), ({'K': 17}, BADARG), ({'K': -1}, BADARG), ({'ld': C - 1}, BADARG), ({'C': 0}, BADARG),
                     ({'C': 61, 'ld': 61}, UNSUPPORTED), ({'record': rec.data_ptr() + 4}, BADARG), ({'logits': lg.data_ptr() + 2}, BADARG),
                     ({'ws_bytes': nbytes - 1}, WORKSPACE), ({'ws': ws.data_ptr() + 4}, WORKSPACE), ({'ld': 2 ** 23}, UNSUPPORTED)):
        assert run(**kw) == code, kw
        assert lib.dsrl_last_error().decode().startswith('temperature_'), kw
    torch.cuda.synchronize()
    assert np.array_equal(_np(rec), after) and int(flag.item()) == 0                # nothing was launched
    # the _t entry points check beta before anything else
    for beta in (0.0, -1.0, float('inf'), float('nan')):
        conf = torch.full((P,), -1.0, device=H.DEV)
        assert lib.dsrl_calibration_from_logits_t(lg.data_ptr(), C + 1, None, P, C, IGNORE, 1, None, conf.data_ptr(), None, ctypes.c_float(beta), st) == BADARG
        assert (_np(conf) == -1.0).all()


# ---------------------------------------------------------------------------------------------- applying beta: the fused tails
TAILS = [PFR.TAIL_FIXTURES[1], PFR.TAIL_FIXTURES[3]]           # (2,5,7): 70 / 140 pixels, a partial tile; (2,3,1): W = 1


def _tail_modules(p, bias1=None):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.nn_modules import HipBatchNorm2d, HipConvTranspose2d
    nc = p['w1'].shape[0]
    c1 = HipConvTranspose2d(nc, nc, kernel_size=2, stride=2, padding=0, bias=bias1 is not None)
    bn = HipBatchNorm2d(nc)
    c2 = HipConvTranspose2d(nc, nc, kernel_size=2, stride=2, padding=0, bias=p['b2'] is not None)
    with torch.no_grad():
        c1.weight.copy_(torch.from_numpy(p['w1'])); c2.weight.copy_(torch.from_numpy(p['w2']))
        bn.weight.copy_(torch.from_numpy(p['gamma'])); bn.bias.copy_(torch.from_numpy(p['beta']))
        bn.running_mean.copy_(torch.from_numpy(p['mean'])); bn.running_var.copy_(torch.from_numpy(p['var']))
        if p['b2'] is not None:
            c2.bias.copy_(torch.from_numpy(p['b2']))
        if bias1 is not None:
            c1.bias.copy_(torch.from_numpy(bias1))
    return [m.to(H.DEV).eval() for m in (c1, bn, c2)]


def _module_logits(x, mods):
    from dualsuperreslearningforsemseg_amd import functional as HF
    with torch.no_grad():
        return mods[2](HF.batch_norm_act(mods[0](x), mods[1], relu=True))


def _conf_from_logits_t(logits, beta):
    """dsrl_calibration_from_logits_t on (N, C, H, W) logits: the confidence map alone"""
    from dualsuperreslearningforsemseg_amd import functional as HF
    N, C, Hh, W = logits.shape
    lg, ld = HF.pm(logits)
    conf = torch.empty((N, Hh, W), device=logits.device, dtype=torch.float32)
    HF.call('dsrl_calibration_from_logits_t', lg.data_ptr(), ld, None, N * Hh * W, C, IGNORE, 1, None, conf.data_ptr(), None, beta, HF._stream())
    return conf


def _ce64(L, target):
    return float(torch.nn.functional.cross_entropy(torch.from_numpy(np.ascontiguousarray(L, dtype=np.float64)), torch.from_numpy(target.astype(np.int64)),
                                                   ignore_index=IGNORE))


@pytest.mark.parametrize('T', [0.5, 2.0])
@pytest.mark.parametrize('fixture', TAILS, ids=PFR.tail_fixture_id)
def test_single_view_keeps_the_class_map_and_scales_the_rest(fixture, T):
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    p, x, L64, _ = PFR.tail_fixture(fixture)
    n = x.shape[0]
    mods = _tail_modules(p)
    xd = H.dev(x)
    target = PFR.make_target(fixture[0] + 5, (n, 4 * fixture[3], 4 * fixture[4]))
    td = H.dev(target)
    beta = HF.temperature_beta(T)
    counts0, cm0 = (torch.zeros(k, dtype=torch.int64, device=H.DEV) for k in (3 * NC + 2, NC * NC))
    flag = _flag()
    pred0, ce0 = HF.sssr_tail_predict(xd, *mods, target=td, counts=counts0, confusion=cm0, nan_flag=flag)
    counts, cm, rec = (torch.zeros(k, dtype=torch.int64, device=H.DEV) for k in (3 * NC + 2, NC * NC, 3 * B))
    pred, ce, conf = HF.sssr_tail_predict(xd, *mods, target=td, counts=counts, confusion=cm, nan_flag=flag, calibration=rec, confidence=True, temperature=T)
    assert int(flag.item()) == 0
    # the class map and everything counted from it: byte-equal with and without a temperature
    assert _np(pred).tobytes() == _np(pred0).tobytes() and torch.equal(counts, counts0) and torch.equal(cm, cm0)
    # the confidence map is what the logits kernel makes of the module-path logits, bit for bit
    logits = _module_logits(xd, mods)
    want_conf = _conf_from_logits_t(logits, beta)
    assert _np(conf).tobytes() == _np(want_conf).tobytes()
    # the record is the binning of the map returned with it
    assert np.array_equal(_np(rec), CR.record_of(_np(conf), _np(pred), target, B, NC, IGNORE))
    # the loss is that of the scaled logits: the budget of test_predict_gpu.test_cross_entropy_of_the_unwritten_logits
    ref = _ce64(L64 * beta, target)
    unfused = float(torch.nn.functional.cross_entropy(logits * beta, td.long(), ignore_index=IGNORE))
    e_unfused, e_fused = abs(unfused - ref), abs(float(ce) - ref)
    budget = max(4 * e_unfused, 1e-6 * abs(ref))
    print(f'{PFR.tail_fixture_id(fixture)} T={T}: ce {float(ce0):.6f} -> {float(ce):.6f}, ref {ref:.9f}, unfused error {e_unfused:.3e}, fused {e_fused:.3e}, budget {budget:.3e}')
    assert e_fused <= budget and abs(float(ce) - float(ce0)) > 1e-3
    # every other combination of outputs: other instantiations, the same bits
    pred1, ce1 = HF.sssr_tail_predict(xd, *mods, target=td, temperature=T)
    pred2, none2, conf2 = HF.sssr_tail_predict(xd, *mods, confidence=True, temperature=T)
    rec3 = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
    pred3, ce3 = HF.sssr_tail_predict(xd, *mods, target=td, calibration=rec3, temperature=T)
    pred4, none4 = HF.sssr_tail_predict(xd, *mods, temperature=T)
    assert all(torch.equal(q, pred0) for q in (pred1, pred2, pred3, pred4)) and none2 is None and none4 is None
    assert _np(ce1).tobytes() == _np(ce).tobytes() == _np(ce3).tobytes() and _np(conf2).tobytes() == _np(conf).tobytes() and torch.equal(rec3, rec)


@pytest.mark.parametrize('fixture', TAILS, ids=PFR.tail_fixture_id)
def test_temperature_one_and_none_are_the_calls_of_today(fixture):
    """tests/hip_helpers.py offers no call log: byte-equal outputs, and the entry point a temperature reaches is exercised above"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    p, x, _, _ = PFR.tail_fixture(fixture)
    mods = _tail_modules(p)
    xd = H.dev(x)
    n = x.shape[0]
    for flip in (False, True):
        m = n // 2 if flip else n
        td = H.dev(PFR.make_target(fixture[0] + 6, (m, 4 * fixture[3], 4 * fixture[4])))
        outs = []
        for kw in ({}, {'temperature': None}, {'temperature': 1}, {'temperature': 1.0}):
            rec = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
            pred, ce, conf = HF.sssr_tail_predict(xd, *mods, target=td, flip=flip, calibration=rec, confidence=True, **kw)
            outs.append(_np(pred).tobytes() + _np(ce).tobytes() + _np(conf).tobytes() + _np(rec).tobytes())
        assert outs[0] == outs[1] == outs[2] == outs[3]
        rec = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV)
        pred, ce, conf = HF.sssr_tail_predict(xd, *mods, target=td, flip=flip, calibration=rec, confidence=True, temperature=2.0)
        assert _np(ce).tobytes() != outs[0][pred.numel():pred.numel() + 4]           # and a temperature is not


@pytest.mark.parametrize('T', [0.5, 2.0])
@pytest.mark.parametrize('fixture', TAILS, ids=PFR.tail_fixture_id)
def test_flip_ensemble_of_the_scaled_views(fixture, T):
    """pred, ce and the confidence against tests/predict_flip_ref.py fed beta-scaled logits: the class map inside its band rule, the loss within
    max(4 |unfused - ref|, 1e-6 |ref|), the confidence within max(4 x the unfused composition's error, 4 (C + 1) 2^-24: the float32 softmax bound of
    test_calibration_gpu.test_from_logits_record_map_stride_and_foreign_labels)."""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    p, x, L64, _ = PFR.tail_fixture(fixture)
    n = x.shape[0] // 2
    beta = HF.temperature_beta(T)
    Ls = L64 * beta
    E = PFR.ensemble_of_views(Ls)
    mods = _tail_modules(p)
    xd = H.dev(x)
    target = PFR.make_target(fixture[0] + 7, (n, 4 * fixture[3], 4 * fixture[4]))
    td = H.dev(target)
    rec, flag = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV), _flag()
    pred, ce, conf = HF.sssr_tail_predict(xd, *mods, target=td, flip=True, nan_flag=flag, calibration=rec, confidence=True, temperature=T)
    assert int(flag.item()) == 0
    PFR.check_class_map(_np(pred), E, Ls, 'flip tail with a temperature vs the fp64 ensemble of the scaled logits')
    assert np.array_equal(_np(rec), CR.record_of(_np(conf), _np(pred), target, B, NC, IGNORE))
    scores = HF._flip_ensemble(_module_logits(xd, mods) * beta)
    ref = PFR.ce(E, target)
    e_unfused = abs(float(torch.nn.functional.nll_loss(scores, td.long(), ignore_index=IGNORE)) - ref)
    e_fused = abs(float(ce) - ref)
    budget = max(4 * e_unfused, 1e-6 * abs(ref))
    c64 = np.exp(E).max(axis=1)
    c_unfused = np.abs(_np(scores.exp().max(dim=1)[0]).astype(np.float64) - c64).max()
    c_fused = np.abs(_np(conf).astype(np.float64) - c64).max()
    c_budget = max(4 * c_unfused, 4 * (NC + 1) * 2.0 ** -24)
    print(f'{PFR.tail_fixture_id(fixture)} T={T}: ce ref {ref:.9f} unfused {e_unfused:.3e} fused {e_fused:.3e} budget {budget:.3e}; '
          f'confidence unfused {c_unfused:.3e} fused {c_fused:.3e} budget {c_budget:.3e}')
    assert e_fused <= budget and c_fused <= c_budget
    pred1, ce1 = HF.sssr_tail_predict(xd, *mods, target=td, flip=True, temperature=T)
    assert torch.equal(pred1, pred) and _np(ce1).tobytes() == _np(ce).tobytes()


def test_fallback_head_multiplies_its_logits():
    """a head the tail kernel does not implement (a bias on convt1): modules -> logits -> the reductions of today on the scaled logits"""
    H = _helpers()
    from dualsuperreslearningforsemseg_amd import functional as HF
    f = TAILS[0]
    p, x, _, _ = PFR.tail_fixture(f)
    mods = _tail_modules(p, bias1=(0.1 * np.random.RandomState(5).standard_normal(NC)).astype(np.float32))
    xd = H.dev(x)
    n = x.shape[0]
    T = 2.0
    beta = HF.temperature_beta(T)
    target = PFR.make_target(77, (n, 4 * f[3], 4 * f[4]))
    td = H.dev(target)
    logits = _module_logits(xd, mods)
    counts0, counts = (torch.zeros(3 * NC + 2, dtype=torch.int64, device=H.DEV) for _ in range(2))
    pred0, ce0 = HF.sssr_tail_predict(xd, *mods, target=td, counts=counts0)
    rec, flag = torch.zeros(3 * B, dtype=torch.int64, device=H.DEV), _flag()
    pred, ce, conf = HF.sssr_tail_predict(xd, *mods, target=td, counts=counts, nan_flag=flag, calibration=rec, confidence=True, temperature=T)
    assert int(flag.item()) == 0 and torch.equal(pred, pred0) and torch.equal(counts, counts0)
    assert torch.equal(pred, torch.argmax(logits, dim=1).to(torch.uint8))
    assert _np(conf).tobytes() == _np(_conf_from_logits_t(logits, beta)).tobytes()
    assert np.array_equal(_np(rec), CR.record_of(_np(conf), _np(pred), target, B, NC, IGNORE))
    assert _np(ce).tobytes() == _np(HF.cross_entropy(logits * beta, td, IGNORE)).tobytes() and abs(float(ce) - float(ce0)) > 1e-3
    # the map alone, and the flip form: the ensemble of the scaled views
    _, none, conf1 = HF.sssr_tail_predict(xd, *mods, confidence=True, temperature=T)
    assert none is None and _np(conf1).tobytes() == _np(conf).tobytes()
    tf = H.dev(PFR.make_target(78, (n // 2, 4 * f[3], 4 * f[4])))
    predf, cef, conff = HF.sssr_tail_predict(xd, *mods, target=tf, flip=True, confidence=True, temperature=T)
    scores = HF._flip_ensemble(logits * beta)
    assert torch.equal(predf, torch.argmax(scores, dim=1).to(torch.uint8))
    assert abs(float(cef) - float(torch.nn.functional.nll_loss(scores, tf.long(), ignore_index=IGNORE))) <= 1e-6 * abs(float(cef))
    assert np.abs(_np(conff) - _np(scores.exp().max(dim=1)[0])).max() <= 4 * (NC + 1) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- the model and the commands
@pytest.fixture(scope='module')
def model():
    H = _helpers()
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    from dualsuperreslearningforsemseg_amd.models.DSRL import DSRL
    torch.manual_seed(1234)
    return DSRL(3, CS).to(H.DEV).to(memory_format=torch.channels_last).eval()


def _image(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(_helpers().DEV).contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope='module')
def split(model):
    """two synthetic batches at 64 x 128 whose labels are drawn from softmax(1.6 x the model's own logits) (~10 % ignored), so that the fit has
    an interior minimum near beta = 1.6; -> (batches in the loader protocol, logits rows (P, C) float32, labels (P,))"""
    H = _helpers()
    rs = np.random.RandomState(99)
    batches, rows, labels = [], [], []
    for i, n in enumerate((2, 1)):
        x = _image(300 + i, (n, 3, 64, 128))
        with torch.no_grad():
            L = _np(model._eval_sssr_logits(x))
        r = np.moveaxis(L, 1, -1).reshape(-1, L.shape[1])
        z = 1.6 * r.astype(np.float64)
        pr = np.exp(z - z.max(1, keepdims=True))
        pr /= pr.sum(1, keepdims=True)
        t = np.minimum((pr.cumsum(1) < rs.uniform(size=(r.shape[0], 1))).sum(1), L.shape[1] - 1).astype(np.uint8)
        t[rs.uniform(size=t.shape) < 0.1] = IGNORE
        batches.append(((x, None), (H.dev(t.reshape(n, L.shape[2], L.shape[3])), None)))
        rows.append(r); labels.append(t)
    return batches, np.concatenate(rows), np.concatenate(labels)


def test_predict_with_a_temperature(model, split):
    batches, _, _ = split
    (x, _), (td, _) = batches[0]
    rec0, rec = (torch.zeros(3 * B, dtype=torch.int64, device=x.device) for _ in range(2))
    pred0, counts0, ce0, conf0 = model.predict(x, td, calibration=rec0, confidence=True)
    pred, counts, ce, conf = model.predict(x, td, calibration=rec, confidence=True, temperature=0.5)
    assert torch.equal(pred, pred0) and torch.equal(counts, counts0)
    assert np.array_equal(_np(rec), CR.record_of(_np(conf), _np(pred), _np(td), B, NC, IGNORE))
    with torch.no_grad():
        logits = model._eval_sssr_logits(x)
    # the eval forward path forms the tail's logits in another summation order than the fused kernel (bit equality holds on the logits of the
    # tail's own modules: test_single_view_keeps_the_class_map_and_scales_the_rest); here the float32 softmax bound of test_calibration_gpu
    assert np.abs(_np(conf) - _np(_conf_from_logits_t(logits, 2.0))).max() <= 4 * (NC + 1) * 2.0 ** -24
    # a sharper softmax: every maximum grows (to the float32 softmax bound of test_calibration_gpu: 4 (C + 1) 2^-24)
    assert (_np(conf) >= _np(conf0) - 4 * (NC + 1) * 2.0 ** -24).all() and float(conf.mean()) > float(conf0.mean())
    same = model.predict(x, td, calibration=torch.zeros_like(rec), confidence=True, temperature=1)
    assert _np(same[2]).tobytes() == _np(ce0).tobytes() and _np(same[3]).tobytes() == _np(conf0).tobytes()
    predf, _, cef = model.predict(x, td, flip=True, temperature=0.5)
    assert tuple(predf.shape) == tuple(pred.shape) and np.isfinite(float(cef))
    with pytest.raises(ValueError, match='scales'):
        model.predict(x, td, temperature=0.5, scales=(0.75, 1.0))
    cp = model.compile_predict()
    try:
        with pytest.raises(ValueError, match='temperature'):
            cp(x, td, temperature=0.5)
        assert torch.equal(cp(x, td, temperature=1)[0], pred0)
    finally:
        cp.release()


def test_fit_temperature_and_benchmark_end_to_end(model, split, tmp_path):
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.benchmark import benchmark
    from dualsuperreslearningforsemseg_amd.command_handlers.fit_temperature import fit_temperature
    from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
    batches, rows, labels = split
    weights = str(tmp_path / 'final.weights')
    torch.save({'model_state_dict': model.state_dict()}, weights)
    asked = []
    dataset = {'settings': CS, 'split': 'val', 'path': str(tmp_path / 'nothing'),
               'loader_factory': lambda split, batch_size, device, rank, world: asked.append(split) or batches}
    kw = dict(model_input_size=(64, 128))
    fit = fit_temperature(weights, dataset, 'gpu', 0, 2, output_dir=str(tmp_path / 'fit'), **kw)
    assert set(fit) == {'temperature', 'beta', 'at_bound', 'nll_before', 'nll_after', 'pixels', 'passes'}
    assert asked == ['val', 'val'] and fit['passes'] == 2 and not fit['at_bound'] and fit['pixels'] == (labels != IGNORE).sum()
    # the same two passes on reference records of the same logits
    b1 = HF.temperature_grid(0.25, 4.0, 16)
    r1, _ = R.record(rows, labels, b1, IGNORE)
    i, at = HF.temperature_bracket(b1, r1)
    assert not at
    b2 = HF.temperature_grid(b1[i], b1[i + 1], 16, log=False)
    r2, _ = R.record(rows, labels, b2, IGNORE)
    want, _ = HF.temperature_solve(b2, r2)
    print(f"fitted T {fit['temperature']:.6f} (beta {fit['beta']:.6f}), reference beta {want:.6f}; NLL {fit['nll_before']:.5f} -> {fit['nll_after']:.5f}")
    assert abs(fit['temperature'] - 1.0 / want) <= 1e-4 / want and abs(fit['beta'] - 1.6) < 0.1
    assert fit['nll_after'] < fit['nll_before']
    assert abs(fit['nll_before'] - HF.temperature_nll_at(b1, r1, 1.0)) <= 1e-5 and abs(fit['nll_after'] - HF.temperature_nll_at(b2, r2, want)) <= 1e-5
    path = os.path.join(str(tmp_path / 'fit'), 'temperature.json')
    saved = json.load(open(path))
    assert saved['temperature'] == fit['temperature'] and saved['passes'] == 2 and saved['split'] == 'val'
    # benchmark: without the key, with 'fit', with the file
    plain = benchmark(weights, dataset, 'gpu', 0, 2, output_dir=str(tmp_path / 'plain'), calibration=True, **kw)
    assert 'temperature' not in plain and 'Temperature scaling' not in open(os.path.join(str(tmp_path / 'plain'), 'benchmark.txt')).read()
    fitted = benchmark(weights, dataset, 'gpu', 0, 2, output_dir=str(tmp_path / 'fitted'), calibration=True, temperature='fit', **kw)
    assert fitted['temperature'] == fit['temperature'] and set(fitted) - set(plain) == {'temperature'}
    assert fitted['CE'] <= plain['CE'] and fitted['CE'] < plain['CE'] - 1e-3
    for k in ('mIoU', 'accuracy', 'mIoU_dataset', 'pixel_accuracy', 'confusion_matrix'):
        assert fitted[k] == plain[k], k
    assert fitted['mean_confidence'] > plain['mean_confidence'] and sum(fitted['reliability']['n']) == sum(plain['reliability']['n'])
    text = open(os.path.join(str(tmp_path / 'fitted'), 'benchmark.txt')).read()
    assert 'Temperature scaling: T = {:.4f}'.format(fit['temperature']) in text and 'in-sample' in text
    loaded = benchmark(weights, dataset, 'gpu', 0, 2, output_dir=str(tmp_path / 'loaded'), calibration=True, temperature=path, **kw)
    assert json.dumps(loaded, sort_keys=True) == json.dumps(fitted, sort_keys=True)          # (empty bins hold NaN: compared as text)
    text = open(os.path.join(str(tmp_path / 'loaded'), 'benchmark.txt')).read()
    assert 'Temperature scaling: T = {:.4f}'.format(fit['temperature']) in text and 'in-sample' not in text
    number = benchmark(weights, dataset, 'gpu', 0, 2, output_dir=str(tmp_path / 'number'), temperature=fit['temperature'], flip=True, **kw)
    assert number['temperature'] == fit['temperature'] and 'ECE' not in number and np.isfinite(number['CE'])

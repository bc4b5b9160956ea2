"""The host side of the weight average, without a GPU: the dataset['ema'] parser, the numpy reference against its closed
form, ddp.FlatParams' EMA state on a CPU model, and the file layouts."""
import numpy as np
import pytest
import torch

import ema_ref as E

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ dataset['ema']
@pytest.mark.parametrize('given,expected', [
    (None, None), (False, None), (np.bool_(False), None),
    (True, (0.999, True)), (np.bool_(True), (0.999, True)),
    (0.9, (0.9, True)), (np.float32(0.5), (0.5, True)), (0.9999, (0.9999, True)),
    ((0.99, False), (0.99, False)), ([0.99, True], (0.99, True)),
    ({'decay': 0.9, 'warmup': False}, (0.9, False)), ({'decay': 0.9}, (0.9, True)), ({'warmup': False}, (0.999, False)),
])
def test_ema_value_accepts(given, expected):
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import check_ema
    assert HF.ema_value(given) == expected
    assert check_ema({'ema': given}) == expected
    assert check_ema({}) is None


@pytest.mark.parametrize('given', [
    0, 0.0, -0.5, 1, 1.0, 1.5, float('nan'), float('inf'), 1.0 - 1e-12,       # decay <= 0, >= 1 (also once rounded to fp32), NaN
    (True, True), (False, False), (0.9, 1), (0.9, None), (0.9, 'yes'),        # a bool in place of the decay; a warm-up that is no bool
    (0.9,), (0.9, True, 1), {}, {'decay': 0.9, 'momentum': 0.1}, {'decay': True}, {'decay': 1.0}, {'warmup': 0},
    '0.9', object(), ('0.9', True), (float('nan'), True),
])
def test_ema_value_refuses(given):
    from dualsuperreslearningforsemseg_amd import functional as HF
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import check_ema
    with pytest.raises(ValueError):
        HF.ema_value(given)
    with pytest.raises(ValueError):
        check_ema({'ema': given})


def test_package_decay_matches_reference_schedule():
    """functional.ema_decay / ema_record (what the host writes into the device record) against tests/ema_ref.py, bit for bit."""
    from dualsuperreslearningforsemseg_amd import functional as HF
    for dmax, warm in ((0.9, True), (0.9999, True), (0.999, False)):
        for t in list(range(40)) + [10 ** 4, 10 ** 6, 2 ** 24]:
            assert F32(HF.ema_decay(t, dmax, warm)).tobytes() == E.decay(t, dmax, warm).tobytes()
            rec = HF.ema_record_read(HF.ema_record(dmax, warm, t, 'cpu'))
            assert rec == {'omd': float(E.omd(t, dmax, warm)), 'decay_max': float(F32(dmax)), 'updates': t, 'warmup': warm}
    assert E.decay(0, 0.9, True) == F32(0.1) and E.decay(10 ** 6, 0.9, True) == F32(0.9) and E.decay(0, 0.9, False) == F32(0.9)
    # warm-up ends where (1 + t) / (10 + t) reaches the limit: t = 80 for 0.9 (81 / 90), t = 8 for 0.5 (9 / 18)
    assert E.decay(79, 0.9, True) < F32(0.9) and E.decay(80, 0.9, True) == F32(0.9) and E.decay(81, 0.9, True) == F32(0.9)
    assert E.decay(7, 0.5, True) < F32(0.5) and E.decay(8, 0.5, True) == F32(0.5)


# ------------------------------------------------------------------------------------------------ the reference against its closed form
@pytest.mark.parametrize('dmax,warm', [(0.9, True), (0.9999, True), (0.5, False)])
def test_reference_recursion_matches_closed_form(dmax, warm):
    rs = np.random.RandomState(7)
    e0 = rs.standard_normal(257)
    snaps = [e0 + 0.1 * (j + 1) * rs.standard_normal(257) for j in range(25)]
    run = E.ema_run(e0, snaps, dmax, warm)
    for k in (1, 2, 10, 25):
        closed = E.ema_closed_form(e0, snaps[:k], dmax, warm)
        # float64 on both sides: k fused steps against k-term sums of numbers of size max |p|
        assert np.abs(run[k - 1] - closed).max() <= 4 * k * 2.0 ** -53 * max(np.abs(s).max() for s in snaps[:k])
    # one step is the textbook form d e + (1 - d) p
    d0 = F64(1) - F64(E.omd(0, dmax, warm))
    assert np.abs(run[0] - (d0 * e0 + (1 - d0) * snaps[0])).max() <= 4 * 2.0 ** -53 * np.abs(snaps[0]).max()
    # float32 inputs: the difference is taken in float32
    e32, p32 = e0.astype(F32), snaps[0].astype(F32)
    assert np.array_equal(E.ema_step(e32, p32, F32(0.25)), e32.astype(F64) + 0.25 * (p32 - e32).astype(F64))


# ------------------------------------------------------------------------------------------------ FlatParams on a CPU model
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, bias=True)
        self.bn = torch.nn.BatchNorm2d(8)
        self.fc = torch.nn.Linear(8, 2)


def _tiny():
    from dualsuperreslearningforsemseg_amd import ddp
    torch.manual_seed(5)
    model = _Tiny().to(memory_format=torch.channels_last)
    with torch.no_grad():
        model.bn.running_mean.copy_(torch.arange(8.0))
        model.bn.num_batches_tracked.fill_(3)
    assert model.conv.weight.is_contiguous(memory_format=torch.channels_last) and not model.conv.weight.is_contiguous()
    return model, ddp.FlatParams(model)


def test_enable_ema_state_round_trip_on_cpu():
    from dualsuperreslearningforsemseg_amd import functional as HF
    model, flat = _tiny()
    with pytest.raises(HF.DsrlHipError):
        flat.ema_state_dict()                       # not enabled
    flat.enable_ema(0.9, warmup=True)
    with pytest.raises(HF.DsrlHipError):
        flat.enable_ema(0.9)                        # a second time
    assert torch.equal(flat.e_flat, flat.p_flat) and flat.e_flat.data_ptr() != flat.p_flat.data_ptr()
    assert torch.equal(flat.eb_flat, flat.b_flat) and flat.eb_flat.data_ptr() != flat.b_flat.data_ptr()
    assert flat.ema_rec.numel() * flat.ema_rec.element_size() == 16
    assert HF.ema_record_read(flat.ema_rec) == {'omd': float(E.omd(0, 0.9, True)), 'decay_max': float(F32(0.9)), 'updates': 0, 'warmup': True}
    # the average and the model part ways; the integer buffer follows the live model
    with torch.no_grad():
        flat.e_flat.mul_(0.5)
        flat.eb_flat.add_(1.0)
        model.bn.num_batches_tracked.fill_(7)
    live = model.state_dict()
    sd = flat.ema_state_dict()
    assert list(sd)[:len(live)] == list(live) and set(sd) == set(live) | {'ema_updates', 'ema_decay'}
    assert sd['ema_updates'] == 0 and isinstance(sd['ema_updates'], int) and sd['ema_decay'] == float(F32(0.9)) and isinstance(sd['ema_decay'], float)
    for k, v in live.items():
        assert tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype, k
        assert sd[k].data_ptr() != v.data_ptr()
    assert tuple(sd['conv.weight'].shape) == (8, 3, 3, 3)
    assert torch.equal(sd['conv.weight'], 0.5 * live['conv.weight']) and torch.equal(sd['fc.bias'], 0.5 * live['fc.bias'])
    assert torch.equal(sd['bn.running_mean'], live['bn.running_mean'] + 1.0) and torch.equal(sd['bn.running_var'], live['bn.running_var'] + 1.0)
    assert sd['bn.num_batches_tracked'].item() == 7
    # into a fresh twin: arenas and the record come back, omd recomputed from the update count
    model2, flat2 = _tiny()
    flat2.enable_ema(0.9, warmup=True)
    sd['ema_updates'] = 17
    sd = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in sd.items()}        # as a file would hold it
    flat2.load_ema_state_dict(sd)
    assert torch.equal(flat2.e_flat, flat.e_flat) and torch.equal(flat2.eb_flat, flat.eb_flat)
    assert not torch.equal(flat2.e_flat, flat2.p_flat)                                      # the live weights of the twin were not touched
    assert model2.bn.num_batches_tracked.item() == 3
    assert HF.ema_record_read(flat2.ema_rec) == {'omd': float(E.omd(17, 0.9, True)), 'decay_max': float(F32(0.9)), 'updates': 17, 'warmup': True}
    assert flat2.ema_state_dict()['ema_updates'] == 17 and flat2.ema_updates() == 17
    with pytest.raises(ValueError):
        flat2.load_ema_state_dict({k: v for k, v in sd.items() if k != 'conv.weight'})
    with pytest.raises(ValueError):
        flat2.load_ema_state_dict({k: v for k, v in sd.items() if k != 'ema_updates'})


def test_invalidate_filter_amax_and_state_load():
    model, flat = _tiny()
    flat._amax_key = ('stale',)
    flat.invalidate_filter_amax()
    assert flat._amax_key is None
    flat._amax_key = ('stale',)
    flat.load_state_dict(flat.state_dict(0.1, 0.9, 0.0))
    assert flat._amax_key is None
    # no kernel for the swap on the CPU, and no fallback
    from dualsuperreslearningforsemseg_amd import functional as HF
    flat.enable_ema(0.5)
    with pytest.raises(HF.DsrlHipError):
        with flat.ema_weights():
            pass


# ------------------------------------------------------------------------------------------------ files
def test_load_checkpoint_or_weights_ema(tmp_path):
    from dualsuperreslearningforsemseg_amd.utils import load_checkpoint_or_weights
    model, flat = _tiny()
    flat.enable_ema(0.9)
    with torch.no_grad():
        flat.e_flat.mul_(0.25)
    with_ema, without = str(tmp_path / 'a.checkpoint'), str(tmp_path / 'b.checkpoint')
    torch.save({'model_state_dict': model.state_dict(), 'epoch': 3, 'ema_state_dict': flat.ema_state_dict()}, with_ema)
    torch.save({'model_state_dict': model.state_dict(), 'epoch': 3}, without)
    d = load_checkpoint_or_weights(with_ema, ema=True)
    assert set(d['model_state_dict']) == set(model.state_dict()) and d['epoch'] == 3
    assert torch.equal(d['model_state_dict']['conv.weight'], 0.25 * model.state_dict()['conv.weight'])
    _Tiny().load_state_dict(d['model_state_dict'], strict=True)
    d = load_checkpoint_or_weights(with_ema)                      # the default reads the live weights, as before
    assert torch.equal(d['model_state_dict']['conv.weight'], model.state_dict()['conv.weight'])
    assert load_checkpoint_or_weights(without)['epoch'] == 3
    with pytest.raises(RuntimeError, match='ema_state_dict'):
        load_checkpoint_or_weights(without, ema=True)


def test_checkpoint_without_ema_keeps_its_keys():
    from dualsuperreslearningforsemseg_amd import settings
    from dualsuperreslearningforsemseg_amd.command_handlers.train_or_resume import checkpoint_dict
    have = {k: i for i, k in enumerate(settings.VARIABLES_IN_CHECKPOINT)}
    have['something_else'] = 1
    out = checkpoint_dict(have)
    assert set(out) == set(settings.VARIABLES_IN_CHECKPOINT) and list(out) == list(dict.fromkeys(settings.VARIABLES_IN_CHECKPOINT))
    assert 'ema_state_dict' not in settings.VARIABLES_IN_CHECKPOINT
    with_ema = checkpoint_dict(have, {'ema_updates': 0})
    assert set(with_ema) == set(settings.VARIABLES_IN_CHECKPOINT) | {'ema_state_dict'} and with_ema['model_state_dict'] == have['model_state_dict']

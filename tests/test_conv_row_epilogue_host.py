"""The host rule of the row epilogue (csrc/conv_common.h: row_epilogue_ok, through dsrl_conv2d_row_epilogue_supported), condition by condition.  No GPU:
the query fills an argument block and asks the helper every launcher uses."""
import pytest

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF

BASE = dict(dgrad=1, bm=128, bn=64, kg=1, stride=1, parity=0, splits=1, coop=0, channels=1024, ldy=1024, y_addr=1 << 20, accumulate=1, bn_sums=0, bn_fast=0,
            fwd_stats=0)
ORDER = ('dgrad', 'bm', 'bn', 'kg', 'stride', 'parity', 'splits', 'coop', 'channels', 'ldy', 'y_addr', 'accumulate', 'bn_sums', 'bn_fast', 'fwd_stats')


def ask(**kw):
    a = dict(BASE, **kw)
    return int(_lib.query('dsrl_conv2d_row_epilogue_supported', *[a[k] for k in ORDER]))


@pytest.fixture(autouse=True)
def _mode(monkeypatch):
    monkeypatch.delenv('DSRL_ROW_EPILOGUE', raising=False)
    HF.set_conv_precision('f16x3')
    yield
    HF.set_conv_precision(None)


def test_the_accumulating_wide_data_gradient_is_eligible():
    assert ask() == 1
    assert ask(accumulate=0, bn_sums=1, bn_fast=1) == 1          # sums without accumulate: their operands are what is fetched
    assert ask(bn_sums=1, bn_fast=1) == 1
    assert ask(channels=4, ldy=4) == 1                           # one float4
    assert ask(channels=36, ldy=48, y_addr=(1 << 20) + 16) == 1  # a tile tail, a row gap and an offset, all multiples of 4 floats


@pytest.mark.parametrize('kw', [dict(channels=19, ldy=20), dict(channels=50, ldy=52), dict(ldy=1026), dict(y_addr=(1 << 20) + 4), dict(y_addr=(1 << 20) + 8),
                                dict(stride=2), dict(stride=2, parity=1), dict(kg=2), dict(kg=4), dict(splits=2, coop=0), dict(dgrad=0), dict(dgrad=0, fwd_stats=1),
                                dict(bm=256, bn=256), dict(bn_sums=1, bn_fast=0), dict(accumulate=0), dict(accumulate=1, fwd_stats=1)],
                         ids=lambda kw: '-'.join(f'{k}{v}' for k, v in kw.items()))
def test_everything_else_keeps_the_scalar_epilogue(kw):
    assert ask(**kw) == 0


def test_every_tile_up_to_256x128_and_the_cooperative_split():
    for bm, bn in ((128, 128), (256, 64), (256, 32), (64, 64), (128, 64), (64, 128), (128, 32), (256, 128)):
        assert ask(bm=bm, bn=bn) == 1, (bm, bn)
    assert ask(bm=128, bn=128, splits=3, coop=1) == 1            # the last arriver writes finished values


def test_fp16_arithmetics_only_and_the_switch(monkeypatch):
    for mode, want in (('f16x3', 1), ('f16x1', 1), ('bf16x3', 0), ('bf16x6', 0), ('fp32', 0)):
        HF.set_conv_precision(mode)
        assert ask() == want, mode
    HF.set_conv_precision('f16x3')
    monkeypatch.setenv('DSRL_ROW_EPILOGUE', '0')
    assert ask() == 0 and ask(bn_sums=1, bn_fast=1) == 0
    monkeypatch.setenv('DSRL_ROW_EPILOGUE', '1')
    assert ask() == 1

"""Host side of the class-weighted cross entropy: the weight table's validation, the ENet rule, what train_or_resume accepts as
dataset['class_weights'] - nothing here needs a GPU."""
import math
import os

import numpy as np
import pytest
import torch

from dualsuperreslearningforsemseg_amd import functional as HF
from dualsuperreslearningforsemseg_amd.command_handlers import train_or_resume as TR
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes import settings as CS
from dualsuperreslearningforsemseg_amd.datasets.Cityscapes.class_weights import enet_weights

C = CS.NUM_CLASSES


def test_table_layout_and_zero_weights_allowed():
    w = np.linspace(0.25, 8.0, C)
    w[3] = 0.0
    tab = HF.class_weight_table(w, 'cpu', C)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (256,)
    assert np.array_equal(tab[:C].numpy(), w.astype(np.float32))
    assert np.all(tab[C:].numpy() == 0)                         # a label byte >= C reads a zero, never past the table
    assert HF.class_weight_table(list(w), 'cpu') is tab         # equal weights: one tensor (the hand-over is keyed by its pointer)
    assert HF.class_weight_table(tab, 'cpu', C) is tab
    all_zero = HF.class_weight_table(np.zeros(C), 'cpu', C)     # allowed: the loss is then 0 / 0 = NaN, as torch
    assert np.all(all_zero.numpy() == 0)


@pytest.mark.parametrize('bad', ['short', 'long', 'negative', 'nan', 'inf', 'fp32_overflow', 'empty', 'matrix', 'words', 'table_of_other_width'])
def test_table_rejects(bad):
    w = np.ones(C)
    if bad == 'short':
        w = w[:-1]
    elif bad == 'long':
        w = np.ones(C + 1)
    elif bad == 'negative':
        w[5] = -1e-3
    elif bad == 'nan':
        w[0] = np.nan
    elif bad == 'inf':
        w[C - 1] = np.inf
    elif bad == 'fp32_overflow':
        w[2] = 1e39                                             # finite in float64, +inf in the table's fp32
    elif bad == 'empty':
        w = np.ones(0)
    elif bad == 'matrix':
        w = np.ones((C, 2))
    elif bad == 'words':
        w = ['road'] * C
    elif bad == 'table_of_other_width':
        w = HF.class_weight_table(np.ones(3), 'cpu')
    with pytest.raises(ValueError):
        HF.class_weight_table(w, 'cpu', C)


def test_enet_weights_against_the_formula():
    counts = np.array([5_000_000, 0, 120_000, 37, 1, 900_000], dtype=np.int64)
    f = counts.astype(np.float64) / counts.sum()
    ref = 1.0 / np.log(1.02 + f)
    got = enet_weights(counts)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    assert got[1] == 1.0 / math.log(1.02)                      # a class that never occurs
    assert np.all(np.diff(got[np.argsort(counts)]) <= 0)        # rarer classes weigh more
    assert np.array_equal(enet_weights(np.zeros(4)), np.full(4, 1.0 / math.log(1.02)))
    with pytest.raises(ValueError):
        enet_weights([3, -1])


def _dataset(**kw):
    return dict({'settings': CS, 'path': '/nonexistent'}, **kw)


def test_check_class_weights_accepts():
    assert TR.check_class_weights(_dataset(), C) is None
    assert TR.check_class_weights(_dataset(class_weights=None), C) is None
    w = [0.5 + 0.25 * i for i in range(C)]
    got = TR.check_class_weights(_dataset(class_weights=w), C)
    assert got.dtype == np.float32 and np.array_equal(got, np.asarray(w, np.float32))
    assert TR.check_class_weights(_dataset(class_weights='enet'), C) == 'enet'     # the project's own loader: counted once its cache exists


@pytest.mark.parametrize('value', ['median', [1.0] * (C - 1), [1.0] * (C - 1) + [-2.0], [float('nan')] * C, 3.5])
def test_check_class_weights_refuses(value):
    with pytest.raises(ValueError):
        TR.check_class_weights(_dataset(class_weights=value), C)


def test_enet_needs_a_cache(tmp_path):
    with pytest.raises(ValueError, match='cache'):
        TR.check_class_weights(_dataset(class_weights='enet', loader_factory=lambda *a: []), C)
    with pytest.raises(ValueError, match='cache'):
        TR.check_class_weights({'settings': CS, 'class_weights': 'enet', 'loader_factory': lambda *a: [], 'cache_path': str(tmp_path)}, C)


def _train_args(dataset):
    return dict(is_resuming_training=False, device='gpu', distributed=None, mixed_precision='O0', disable_cudnn_benchmark=False, num_workers=0,
                dataset=dataset, val_interval=1, checkpoint_interval=1, checkpoint_history=1, init_weights=None, batch_size=1, epochs=1,
                learning_rate=0.01, end_learning_rate=0.001, momentum=0.9, weights_decay=5e-4, poly_power=0.9, stage=1, w1=0.1, w2=1.0,
                freeze_batch_norm=False, experiment_id=os.devnull, description='', early_stopping=False)


@pytest.mark.parametrize('value', ['balanced', [1.0] * 7])
def test_train_or_resume_refuses_bad_class_weights_before_touching_a_device(value):
    with pytest.raises(ValueError, match='class'):
        TR.train_or_resume(**_train_args(_dataset(class_weights=value, loader_factory=lambda *a: [])))


def test_train_or_resume_refuses_enet_without_a_cache():
    with pytest.raises(ValueError, match='cache'):
        TR.train_or_resume(**_train_args(_dataset(class_weights='enet', loader_factory=lambda *a: [])))

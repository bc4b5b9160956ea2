"""bench.py as the driver invokes it (CPU-only checks): `--gpus N` without WORLD_SIZE becomes the launcher of N ranks - a plain child process
running `python -m torch.distributed.run ... bench.py <same flags>` on 127.0.0.1 - before anything imports torch.cuda, and relays the exit code."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_gpus_n_self_launches_ranks_and_relays_exit_code(monkeypatch):
    import bench
    seen = {}

    class Done:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen['cmd'], seen['env'] = cmd, env
        return Done()
    monkeypatch.setattr(bench.subprocess, 'run', fake_run)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3', '--warmup', '1'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                    # the ranks' exit code is ours
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run'] and '--nproc-per-node=4' in cmd and '--nnodes=1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and 0 < int(cmd[cmd.index('--master-port') + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:] == ['--gpus', '4', '--steps', '3', '--warmup', '1']          # the same flags reach every rank
    assert seen['env'].get('HSA_ENABLE_IPC_MODE_LEGACY') == '0'


def test_rank_count_mismatch_is_refused(monkeypatch):
    import bench
    monkeypatch.setenv('WORLD_SIZE', '2'); monkeypatch.setenv('RANK', '0'); monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4'])
    with pytest.raises(SystemExit, match='WORLD_SIZE=2'):
        bench.main()


def test_host_cores_respects_override(monkeypatch):
    import bench
    monkeypatch.setenv('DSRL_CPU_BASELINE_THREADS', '3')
    assert bench.host_cores() == 3


def test_plain_run_is_lean_and_steps_are_checked(monkeypatch):
    """A plain run measures the headline only; everything else is behind --full.  --steps sets the timed steps and must be at least 1."""
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == 'out'
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse_args()


def test_dump_outputs_writes_fixed_float_samples(tmp_path):
    """--dump-outputs: one float .npy per output; a large output is sampled at positions of its logical (NCHW) order that depend on its size
    alone, whatever its memory format; a small one is written whole."""
    import numpy as np
    import torch
    import bench
    n_big = bench.DUMP_SAMPLE + 4096
    big = torch.randn((1, 4, 64, n_big // 256), generator=torch.Generator().manual_seed(0))
    outs = (big.contiguous(memory_format=torch.channels_last), torch.randn(2, 3, 4, 4), torch.zeros(1), torch.randn(2, 1, 8, 8))
    params, stats = torch.randn(1000), torch.rand(64)
    a = bench.dump_outputs(str(tmp_path / 'd'), [1.5, 0.25, 0.125, 1.875], outs, params, stats)
    names = {'losses', 'sssr_logits', 'sisr_output', 'sssr_transform', 'sisr_transform', 'params', 'bn_running_stats'}
    assert {p.name for p in (tmp_path / 'd').iterdir()} == {n + '.npy' for n in names}
    for n in names:
        x = np.load(tmp_path / 'd' / (n + '.npy'))
        assert x.dtype == (np.float64 if n == 'losses' else np.float32) and np.array_equal(x, a[n]), n
    idx = bench.sample_index(big.numel())
    assert idx.shape == (bench.DUMP_SAMPLE,) and np.array_equal(idx, bench.sample_index(big.numel()))
    assert np.array_equal(a['sssr_logits'], big.numpy().reshape(-1)[idx])
    assert np.array_equal(a['sisr_output'], outs[1].numpy()) and np.array_equal(a['params'], params.numpy())
    assert a['losses'].tolist() == [1.5, 0.25, 0.125, 1.875]

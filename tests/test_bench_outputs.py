"""bench.py --dump-outputs writes what the last timed step computed (same arguments -> same inputs -> comparable outputs), and a
plain run does only what its headline needs: the sections that take runs of their own come with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--batch', '2', '--img', '64', '--steps', '3', '--warmup', '2', '--preheat-seconds', '0.2']


def _bench(argv, timeout=600):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + argv, capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_bench_declares_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--full' in r.stdout and '--dump-outputs' in r.stdout


def test_dump_sample_is_fixed_and_bounded(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    small = torch.arange(1000, dtype=torch.float32)
    assert np.array_equal(bench._sample(small, 1), small.numpy())          # at the bound: every element, in order
    big = torch.randn(5000)
    a, b = bench._sample(big, 2), bench._sample(big.clone(), 2)
    assert a.shape == (1000,) and np.array_equal(a, b)                       # the same indices in every run
    assert not np.array_equal(a, bench._sample(big, 3))                      # ... chosen by the seed
    assert np.isin(a, big.numpy()).all()


@pytest.mark.gpu
def test_dump_outputs_repeat_for_the_same_arguments(tmp_path):
    dumps = []
    for name in ('a', 'b'):
        d = tmp_path / name
        j = _bench(SMALL + ['--dump-outputs', str(d)])
        assert j['steps'] == 3 and j['ms_per_step'] > 0 and j['preheat_steps'] == 20
        assert sorted(j['outputs_dumped']['arrays']) == sorted(f[:-4] for f in os.listdir(str(d)))
        dumps.append({f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))})
    a, b = dumps
    assert {'loss_g', 'loss_d', 'generated_images', 'discriminator_variables'} <= set(a)
    assert a['generated_images'].shape == (2, 3, 64, 64)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
        assert np.isfinite(v).all(), k
        assert np.allclose(v, b[k], rtol=1e-4, atol=1e-5), (k, float(np.abs(v.astype(np.float64) - b[k]).max()))


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_the_rest():
    plain = _bench(SMALL)
    assert plain['steps'] == 3 and plain['ms_per_step'] > 0 and plain['unit'] == 'images/sec'
    for k in ('roofline', 'generator_fwd_bwd', 'secondary', 'cpu_baseline', 'step_tflops_executed'):
        assert k not in plain, k
    full = _bench(SMALL + ['--full', '--no-secondary', '--no-cpu-baseline', '--prof-steps', '1'])
    assert full['roofline']['per_kernel'] and 'arithmetic_error_vs_f64' in full['roofline']
    assert full['generator_fwd_bwd']['ms'] > 0 and full['step_tflops_executed'] > 0

"""bench.py as a build-to-build comparison runs it: a plain run (headline line only) with --dump-outputs, twice with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '2', '--dump-outputs', out_dir]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_every_run(tmp_path):
    """same arguments -> same inputs -> the same loss, parameters and gradients up to float rounding (the library sums some gradients with
    float atomics, so the order of the additions, not their terms, changes from run to run); a plain run carries no extra legs"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    a_dir, b_dir = str(tmp_path / 'a'), str(tmp_path / 'b')
    for d in (_bench(a_dir), _bench(b_dir)):
        assert d['steps'] == 4 and d['warmup'] == 2 and d['ms_per_step'] > 0 and d['cpu_baseline'] is None
        assert not {'alt', 'other_configs'} & set(d) and 'alone' not in d['roofline']
    names = sorted(os.listdir(a_dir))
    assert names == sorted(os.listdir(b_dir)) and 'loss.npy' in names and len(names) == 1 + 2 * 24    # 25 tensors less att.b, twice
    total = 0
    for n in names:
        a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all(), n
        scale = float(np.abs(a).max())
        assert float(np.abs(a.astype(np.float64) - b).max()) <= 1e-4 * scale, (n, float(np.abs(a.astype(np.float64) - b).max()), scale)
    assert total <= 64e6

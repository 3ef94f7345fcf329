"""GPU (-m gpu): a plain `bench.py --gpus 1` run prints the headline line and nothing measured beside it, and `--dump-outputs`
writes what the last timed step computed: the loss and a fixed sample of the updated weights and of the gradient."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_bench_prints_the_headline_and_dumps_its_outputs(tmp_path):
    out_dir = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2', '--batch', '16',
           '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 2 and d['dtype'] == 'f32'
    assert d['unit'] == 'clips/s' and d['higher_is_better'] is True
    assert abs(d['value'] - 16 / (d['ms_per_step'] / 1e3)) <= 0.02 * d['value']
    assert d['config']['launch'] == 'hipGraph replay'
    # everything beyond the headline belongs to --full
    for k in ('roofline', 'kernel_time_ms_per_step', 'other_gemm_arithmetic', 'batch_128', 'cpu_baseline', 'vs_pytorch_rocm_eager'):
        assert k not in d, k

    names = sorted(os.listdir(out_dir))
    assert names == ['grads_sample.npy', 'loss.npy', 'weights_sample.npy'], names
    assert sum(os.path.getsize(os.path.join(out_dir, n)) for n in names) <= 64 << 20
    arr = {n[:-4]: np.load(os.path.join(out_dir, n)) for n in names}
    for n, x in arr.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
    assert arr['loss'].shape == (1,) and abs(float(arr['loss'][0]) - d['config']['final_loss']) <= 1e-5
    assert arr['weights_sample'].shape == arr['grads_sample'].shape and arr['weights_sample'].size > 1000
    assert np.abs(arr['grads_sample']).max() > 0

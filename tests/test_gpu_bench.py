"""GPU: the plain bench line (headline only) and --dump-outputs: float32 arrays of the last timed step, within 64 MB, the same in two runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', *extra],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])


def test_plain_line_and_dumped_outputs(cuda, tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f'run{i}'
        res = _bench('--dump-outputs', str(d))
        assert res['steps'] == 2 and res['warmup'] == 1 and res['value'] > 0 and res['ms_per_step'] > 0
        assert abs(res['value'] - 1e3 / res['ms_per_step']) < 1e-6 * res['value']
        assert res['unit'] == 'clips/s' and res['higher_is_better'] is True and res['dtype'] == 'bf16'
        assert not any(k in res for k in ('roofline', 'roofline_attention', 'host_enqueue_ms', 'cpu_baseline', 'fp16_mode', 'config3_long_forward'))
        files = sorted(os.listdir(d))
        assert {'loss.npy', 'grad_norm.npy', 'output_mask.npy', 'target_mask.npy', 'query_mask.npy', 'params.npy'} <= set(files)
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert abs(float(arrays['loss.npy']) - res['final_loss']) <= 1e-6 * abs(res['final_loss'])
        runs.append(arrays)
    # the same arguments give the same inputs (query / target masks are built from the seeded synthetic batch) and, with the drop-path
    # draws seeded too, the same step: logits, loss and updated parameters agree between the two runs
    for name in ('query_mask.npy', 'target_mask.npy', 'sel_occl_fracs.npy'):
        assert np.array_equal(runs[0][name], runs[1][name]), name
    for name in ('output_mask.npy', 'loss.npy', 'grad_norm.npy', 'params.npy'):
        assert np.allclose(runs[0][name], runs[1][name], rtol=0, atol=1e-4), (name, float(np.abs(runs[0][name] - runs[1][name]).max()))

"""GPU: a plain bench.py run times exactly --steps passes, prints the headline record only, and --dump-outputs writes what the last
timed pass returned, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ('secondary', 'strong_denominator', 'range_headroom', 'cpu_baseline', 'parity', 'gpu_over_cpu', 'weak_scaling')


def _bench(out_dir, warmup):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', str(warmup),
                        '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stderr or '')[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_dumps_the_last_timed_pass(tmp_path):
    rec = _bench(tmp_path / 'a', 1)
    assert rec['metric'] == 'mel_frames_per_sec' and rec['unit'] == 'mel-frames/s' and rec['higher_is_better'] is True
    assert rec['dtype'] == 'f32' and rec['steps'] == 2 and rec['warmup'] == 1 and rec['handoff_timeouts'] == 0
    assert rec['ms_per_step'] > 0 and abs(rec['value'] - 16 * 1000 * 1e3 / rec['ms_per_step']) <= 1e-6 * rec['value']
    assert 'kernel' in rec['roofline'] and not any(k in rec for k in FULL_ONLY), sorted(rec)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert 'mel_out.npy' in names and all(n.endswith('.npy') for n in names), names
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) <= 64 * 10**6
    a = {n[:-4]: np.load(tmp_path / 'a' / n) for n in names}
    assert a['mel_out'].shape == (16, 1000, 80) and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.isfinite(v).all() for v in a.values())
    # other warm-up, same timed passes: the last one computed the same
    _bench(tmp_path / 'b', 0)
    assert sorted(os.listdir(tmp_path / 'b')) == names
    for k, v in a.items():
        np.testing.assert_allclose(np.load(tmp_path / 'b' / (k + '.npy')), v, rtol=0, atol=1e-5, err_msg=k)

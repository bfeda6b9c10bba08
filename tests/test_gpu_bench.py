"""bench.py on one GPU as the driver runs it: a plain run computes the headline figure and nothing else; --full adds the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_is_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W`: the headline fields and --dump-outputs; the median pass, roofline, PCKh parity and
    CPU baseline stay null (they run with --full: tests/test_gpu_dist.py::test_bench_line_from_two_ranks)."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'POSEADV_DIST_INIT', 'POSEADV_FORCE_DIST')}
    out = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'].startswith('images/sec, 2-stack HG 256x256 bs=24 per GPU') and d['unit'] == 'images/sec' and d['higher_is_better'] is True
    assert d['dtype'] == 'bf16' and d['n_gpus'] == 1 and d['steps'] == 3 and d['warmup'] == 1
    assert d['value'] > 0 and abs(d['value'] - 24 * 1e3 / d['ms_per_step']) <= 0.01 * d['value']
    assert d['ms_per_step_median'] is None and d['pckh_parity'] is None and d['roofline'] is None and d['cpu_baseline'] is None
    assert np.isfinite(d['config']['loss']) and d['config']['loss'] > 0
    assert sorted(os.listdir(out)) == ['buffers.npy', 'heatmaps.npy', 'loss.npy', 'params.npy', 'pckh.npy', 'pckh_origin_res.npy']
    assert float(np.load(os.path.join(out, 'loss.npy'))) == pytest.approx(d['config']['loss'], rel=1e-6)

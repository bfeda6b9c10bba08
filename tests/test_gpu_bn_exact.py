"""Every BatchNorm, max pool and upsample-add of the hourglass net against a float64 recomputation from the engine's own stored tensors
after one real training step (checks and the derivation of every bound: tests/bn_exact.py).  The per-node tests
(tests/test_gpu_local.py) bound these operations only at 1e-2 / 4e-2 rel-rms; here a dropped, doubled or overwritten partial
statistics row, a wrong variance, a wrong summation order or a rounding error of the fused / split / streaming launches is a failure.

Legs: BASELINE configs[1] at full size (the only leg that reaches the fused low-resolution half of the upsample-add backward in the 1 x 1
data gradient's epilogue, the split upsample-add launches, 1536-row statistics and the consumer-prologue finalize at <= 128 rows); the
configs[4] geometry (384 x 384: the 24 x 24 / 12 x 12 tiled 3 x 3 variants, the masked 6 x 6 neck) at a ragged batch; tiny maps (2 x 2 neck,
8 values per channel: biased and unbiased variance differ by 14 %); and the IEEE-half build on the configs[4] geometry in a child process."""
import os
import subprocess
import sys

import pytest

from tests import bn_exact

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leg(stacks, chan, B, res, seed, **kw):
    worst, fails = bn_exact.run_leg(stacks, chan, B, res, seed, **kw)
    assert not fails, '%d checks outside their bound, first: %s (worst per kind: %s)' % (len(fails), fails[:12], worst)


def test_every_bn_pool_and_merge_is_exact_at_the_benchmark_size():
    """BASELINE configs[1]: 2 stacks, chan 256, B 24, 256 x 256."""
    _leg(2, 256, 24, 256, 31)


def test_every_bn_pool_and_merge_is_exact_on_the_384_geometry():
    """configs[4] geometry (maps 96 / 48 / 24 / 12 / 6) at B 3: partial-row counts that do not divide evenly."""
    _leg(2, 256, 3, 384, 32)


def test_every_bn_pool_and_merge_is_exact_on_tiny_maps():
    """chan 128, 128 x 128, B 2: the neck is 2 x 2 (8 values per channel), the last pool reads 2 x 2 pixels.  (No conv3 data gradient
    stores dz3 at these sizes -- the 1 x 1 row-tile kernel does not take them -- so only the stored dz2 are expected.)"""
    _leg(2, 128, 2, 128, 33, stored_expected=('.x2',))


# ---- a history in front of the checked step (tests/exact_history.py).  State does not depend on the map size: the smallest shapes
# that still reach every kernel family.
@pytest.mark.parametrize('history', ('warm', 'graph', 'phased', 'after_eval'))
def test_every_bn_pool_and_merge_is_exact_after_a_history_on_tiny_maps(history):
    """The tiny-maps size (chan 128, 128 x 128, B 2) with steps before the checked one, which runs through the benchmark's path."""
    _leg(2, 128, 2, 128, 35, stored_expected=('.x2',), history=history)


@pytest.mark.parametrize('history', ('warm', 'graph', 'after_half'))
def test_every_bn_pool_and_merge_is_exact_after_a_history_at_256(history):
    """chan 128, B 2, 256 x 256: 64 x 64 maps (the tile kernels, the grouped weight-gradient kernel).  'after_half' runs here and not on
    the tiny maps: the agent it needs accepts no res below 256."""
    _leg(2, 128, 2, 256, 36, history=history)


def _fp16_child(args):
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'bn_exact.py')] + args, env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 BN EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_every_bn_pool_and_merge_is_exact_after_warm_steps_in_the_fp16_build():
    """The IEEE-half library, 'warm' at chan 128, B 2, 256 x 256, in a child process."""
    _fp16_child(['2', '128', '2', '256', '37', 'warm'])


def test_every_bn_pool_and_merge_is_exact_in_the_fp16_build():
    """The IEEE-half library on the configs[4] geometry, in a child process (one storage type per process)."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'bn_exact.py'), '2', '256', '3', '384', '34'], env=env,
                       capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 BN EXACT PASSED' in r.stdout, out[-3000:]

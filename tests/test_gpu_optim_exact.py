"""The fused RMSprop step against a float64 evaluation of its formula, element by element, for p and for square_avg (reference and the
derivation of the bound: tests/optim_exact.py; tests/test_optim_exact_cpu.py shows which defects the bound excludes).
tests/test_gpu_pylib.py::test_rmsprop_matches_torch compares p alone at rtol 1e-6 on 98 workgroups with gscale 1: eps inside the root is
2.5e-10 there, the grid-stride loop never iterates and the 1 / world and 1 / pa_grad_scale() factors are never applied.

Cases: n from 1 (tail only) over the first vector chunk, 1023 and 100 003 to 2048 * 256 * 4 + {0, 1, 3, 5} (the capped launch's loop
iterates, with the tail behind it); both entry points; gscale 1, 1/2, 1/3, 1/32768; three consecutive steps from v = 0 and from a
non-zero v; guard elements around p and v; the real flat arrays of a pose net and of the agent on it after a backward pass (the agent's
has alignment padding, which must stay exactly 0; every tensor of the pose net has a multiple of 4 elements).  The IEEE-half
build (one storage type per process) runs the same cases in a child process, and there the skip of a step whose gradient holds an
inf / NaN at index 0, in the vector body, in the last tail element and beyond the first grid pass."""
import os
import subprocess
import sys

import pytest

from tests import optim_exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('entry', ('plain', 'state'))
@pytest.mark.parametrize('n', X.SIZES)
def test_rmsprop_step_is_exact(n, entry):
    """pa_rmsprop_step ('plain') / pa_rmsprop_step_state ('state') over n elements."""
    fails = X.run_case(n, entry)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


def test_rmsprop_is_exact_on_a_real_flat_array():
    """2-stack chan-128 pose net and its scale / rotation agent, each optimizer on its whole flat array (optim_exact.run_flat_array)"""
    fails = X.run_flat_array()
    assert not fails, fails[:12]


def test_skip_counter_reads_zero_in_the_bf16_build():
    """the bf16 build has no gradient scan: both counters read 0, before and after steps"""
    import torch
    p, g, v = X.make_inputs(1023, 3, 1.0, False)
    for entry in ('plain', 'state'):
        S = X.Stepper(entry, X._t(p), X._t(v))
        assert S.skipped() == 0
        S.step(X.Guarded(X._t(g), float('nan')), 1.0)
        torch.cuda.synchronize()
        assert S.skipped() == 0


def test_rmsprop_is_exact_and_skips_in_the_fp16_build():
    """The IEEE-half library: every case above, and the skipped steps (optim_exact.run_skip_case), in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'optim_exact.py')], env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 OPTIM EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]

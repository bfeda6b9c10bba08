"""Two data-parallel ranks with every optimizer option, gradient accumulation and the weight EMA on the REAL engine (recording, checks and
what each excludes: tests/dist_optim_exact.py; tests/test_dist_optim_cpu.py plants the defects).  Both ranks on the one GPU of the test
box with gloo carrying the exchange, or one rank per GPU over RCCL with POSEADV_TEST_DIST_BACKEND=nccl, as in tests/test_gpu_dist.py.

One spawn per test serves a whole list of cases; the ranks are joined with a deadline, so ranks that disagree on the number of
collectives fail the test instead of waiting for the process group's own timeout.  The smallest net the engine builds (1 stack, chan 128,
64 x 64, B 2), three optimizer steps per case; the overlapped exchange on the 2-stack 256 x 256 net of tests/test_gpu_dist.py, the fp16
build at 256 x 256 (at 64 x 64 the untrained net overflows IEEE half by itself: dist_optim_exact.FP16_CASES).

Clipping: max_grad_norm is 1e30 at a case's first step (the norm is recorded, the coefficient is exactly 1) and from the second step
on half the norm of that step's own exchanged gradient, so the coefficient is below 1 there, which is asserted.  Half the FIRST step's
norm would not clip: the norm of this untrained net moves by up to 80 times between steps (dist_optim_exact.check_clip has the figures).

Times on one MI355X, same run as test_two_process_data_parallel_step_on_the_engine: profiles/dist_optim_tests.txt."""
import os
import subprocess
import sys

import pytest
import torch

from tests import dist_optim_exact as D

pytestmark = pytest.mark.gpu

if os.environ.get('POSEADV_TEST_DIST_BACKEND') == 'nccl' and torch.cuda.device_count() < 2:
    pytestmark = [pytest.mark.gpu, pytest.mark.skip(reason='two ranks over RCCL need two GPUs (a GPU holds one RCCL rank)')]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(c, results):
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        for name, fails in results:
            print('%s %s: %s' % ('FAIL' if fails else 'PASS', c['name'], name))
    bad = [(c['name'], name, fails[:6]) for name, fails in results if fails]
    assert not bad, bad


def _run(cases, single=False, keep=False):
    """the cases on two ranks, every check of dist_optim_exact.check_case; single: also against one process accumulating both shards,
    run here after the ranks have ended; keep: return what check_same_run reads of every record"""
    seen = {}
    for c, recs in D.run_ranks(list(cases)):
        one = D.run_single(c, [st['max_norm'] for st in recs[0]['steps']]) if single else None
        _report(c, D.check_case(recs, one))
        assert D.skipped_steps_of(recs[0]) == [] and recs[0]['final']['skipped'] == 0
        seen[c['name']] = [dict(case=r['case'], rank=r['rank'], steps=[dict(after=st['after'], norm_out=st['norm_out'], adam=st['adam'])
                                                                       for st in r['steps']], start=r['start']) for r in recs] if keep else None
    assert sorted(seen) == sorted(c['name'] for c in cases)
    return seen


KINDS = (D.case('rmsprop'),
         D.case('rmsprop_opts_clip', kw=dict(momentum=0.9, centered=True, weight_decay=1e-4), clip='half'),
         D.case('adam_clip', 'Adam', clip='half'),
         D.case('adamw_amsgrad', 'AdamW', kw=dict(amsgrad=True)),
         D.case('adam_clip_large', 'Adam', clip='large'))


def test_every_optimizer_kind_on_two_ranks_is_one_process_accumulating_both_shards():
    """RMSprop(), RMSprop(momentum, centered, weight_decay, max_grad_norm), Adam(max_grad_norm), AdamW(amsgrad) and a max_grad_norm no
    gradient reaches: replicas, one exchange per step, g_sum = g_local[0] + g_local[1], every step in float64 with gscale = 1/2, the norm
    of the EXCHANGED gradient and its coefficient (below 1 from the second step on, exactly 1 with the large bound), last_grad_norm();
    and bit for bit the parameters and state of ONE process that accumulates the two shards."""
    _run(KINDS, single=True)


def test_accumulation_on_two_ranks():
    """N = 2 and 3 micro-batches per step: one exchange per GROUP, of the rank's own fold ((g1 + g2) + ...); gscale = 1 / (2 N) through the
    float64 checks; pending back to 0; _acc allocated once; replicas identical."""
    _run([D.case('rmsprop_accum%d' % N, N=N) for N in (2, 3)] + [D.case('adam_clip_accum%d' % N, 'Adam', clip='half', N=N) for N in (2, 3)])


def test_the_loop_of_stack_hg_on_two_ranks_with_a_short_trailing_group():
    """stack_hg.train over 3 batches with accum_steps 2 and an EMA: groups [2, 1] and two gradient exchanges on both ranks, two EMA
    updates, the effective-batch line once on rank 0, replicas identical.  Ranks that disagreed on the trailing group would hang: the
    deadline makes that a failure."""
    for c, recs in D.run_ranks([D.case('loop', loop=True)]):
        fails = D.check_loop(recs)
        assert not fails, fails[:8]


def test_the_ema_on_two_ranks():
    """ModelEma(decay 0.9, warm-up) and buffers='copy' behind RMSprop and behind Adam: the average and its counts identical on both
    ranks, its BatchNorm buffers per rank, every update in float64 (ema_exact.check_arrays / check_state)."""
    warm, copy = dict(decay=0.9, warmup=True), dict(decay=0.9, buffers='copy')
    seen = _run([D.case('rmsprop_ema_warmup', ema=warm), D.case('adam_ema_copy', 'Adam', ema=copy),
                 D.case('rmsprop_ema_copy', ema=copy), D.case('adam_ema_warmup', 'Adam', ema=warm)])
    assert len(seen) == 4


def test_the_overlapped_exchange_with_clipping_momentum_and_adam():
    """RMSprop(overlap=True, momentum, max_grad_norm) and Adam(overlap=True, max_grad_norm) on the 2-stack net of
    test_overlapped_gradient_exchange_gives_the_same_result: parameters, buffers, state and {norm, coefficient} bit for bit those of
    overlap=False (the norm must not be taken in front of the last bucket); 2 asynchronous buckets per step, every gradient once."""
    big = dict(stacks=2, res=256)
    rms, adam = dict(kw=dict(momentum=0.9), clip='half'), dict(opt='Adam', clip='half')
    cases = [D.case('rmsprop_plain_exchange', **dict(rms, **big)), D.case('rmsprop_overlap', overlap=True, **dict(rms, **big)),
             D.case('adam_plain_exchange', **dict(adam, **big)), D.case('adam_overlap', overlap=True, **dict(adam, **big))]
    seen = _run(cases, keep=True)
    for kind in ('rmsprop', 'adam'):
        for rank in (0, 1):
            fails = D.check_same_run(seen[kind + '_overlap'][rank], seen[kind + '_plain_exchange'][rank],
                                     '%s rank %d: overlap=True against overlap=False' % (kind, rank), buffers=True)
            assert not fails, fails[:8]


def test_two_ranks_in_the_fp16_build_skip_a_step_together():
    """The IEEE-half library, in a child process that spawns the two ranks itself: RMSprop(), Adam() and RMSprop() with N = 2, each with
    an EMA; rank 1 alone writes one inf into flat_grads at step 2 of 3.  Both ranks skip that step, bit for bit, and count it the same."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'dist_optim_exact.py')], env=env, capture_output=True, text=True,
                       timeout=D.deadline_for(D.FP16_CASES) + 60)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and D.FP16_MARKER + 'PASSED' in r.stdout, (r.stdout + r.stderr)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith(('PASS ', 'FAIL '))]
    assert lines and all(l.startswith('PASS ') for l in lines) and all(any(c['name'] in l for l in lines) for c in D.FP16_CASES)

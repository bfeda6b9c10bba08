"""The whole ASN agent against a float64 recomputation from the engine's own stored tensors after one agent step, element by element
(checks and the derivation of every bound: tests/asn_exact.py, which reuses the per-block and per-BatchNorm checks of
tests/conv_exact.py and tests/bn_exact.py).  tests/test_gpu_agent.py and tests/test_gpu_dropout.py keep guarding the wiring against the
oracle at rel-rms tolerances (25 % on the input blocks' conv1 weight gradients, 6 % on the BatchNorm beta gradients, 1e-2 on the heads);
here every element of every conv, BatchNorm, pool+add and head tensor is held to a derived bound or compared bit for bit.

Legs: the joint loop's size (chan 256, B 24, 256 x 256: shapes the grouped weight-gradient kernel takes); the 384 x 384 geometry at B 3
(maps 96 / 48 / 24 / 12 / 6: ragged streaming thread counts, and a 6 x 6 top map of which the head may only average the top-left 4 x 4
window); the 320 x 320 and 448 x 448 geometries (5 x 5 and 7 x 7 top maps, the largest the agent accepts; widths 20 / 28 / 10 / 14 that fit
no streaming row walk); chan 128 at B 4; the occlusion agent at chan 256 B 24 and chan 128 B 2; the IEEE-half build on the 384 and 448
geometries in child processes (one storage type per process; all gradient checks in units of pa_grad_scale()).  On every top map larger
than the window the head's input gradient outside it is exactly zero, element by element."""
import os
import subprocess
import sys

import pytest

from tests import asn_exact as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ok(worst_fails):
    worst, fails = worst_fails
    assert not fails, '%d checks outside their bound, first: %s (worst per kind: %s)' % (len(fails), fails[:12], worst)


def test_agent_is_exact_at_the_joint_loop_size():
    _ok(A.run_leg(256, 24, 256, 51, expect=('group',)))


def test_agent_is_exact_on_the_384_geometry():
    """6 x 6 top map: the head averages its top-left 4 x 4 window and sends no gradient outside it."""
    _ok_with_a_window(A.run_leg(256, 3, 384, 52))


def _ok_with_a_window(worst_fails):
    """a leg whose top map is larger than the head's 4 x 4 window: every element of the head's input gradient outside the window is exactly
    zero (asn_exact.outside_window counts them; run_leg also reports any as a failure)"""
    _ok(worst_fails)
    assert worst_fails[0]['head gradient outside the window'] == 0, worst_fails[0]


def test_agent_is_exact_on_the_320_geometry():
    """chan 256, B 3, 320 x 320 (maps 80 / 40 / 20 / 10 / 5): a 5 x 5 top map, the 3 x 3 layers of the two deepest levels on the generic
    kernel (10 x 10) and one masked 8 x 8 tile (5 x 5), pool+add and the streaming backward on widths that fit no row walk (20 / 10)."""
    _ok_with_a_window(A.run_leg(256, 3, 320, 91, expect=('group',)))


def test_agent_is_exact_on_the_448_geometry():
    """chan 128, B 2, 448 x 448 (maps 112 / 56 / 28 / 14 / 7): a 7 x 7 top map, the largest res the agent accepts."""
    _ok_with_a_window(A.run_leg(128, 2, 448, 92, expect=('group',)))


def test_agent_is_exact_on_the_448_geometry_in_the_fp16_build():
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'asn_exact.py'), '128', '2', '448', '93'], env=env,
                       capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 ASN EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_agent_is_exact_at_chan_128():
    _ok(A.run_leg(128, 4, 256, 53))


def test_occlusion_agent_is_exact_at_the_joint_loop_size():
    _ok(A.run_mask_leg(256, 24, 54, expect=('group',)))


def test_occlusion_agent_is_exact_at_chan_128():
    _ok(A.run_mask_leg(128, 2, 55))


# ---- chan 512: the agent's twelve blocks are 512 -> 256 -> 256 (3 x 3) -> 512 at every level, so every conv1 forward, every 3 x 3
# launch and every conv3 / conv2 data gradient is the generic K-stepping kernel at K = 512 / 2304 (B 2: <64,64> tiles), every
# 512-channel BatchNorm is finalized by a launch of its own, pooladd_fwd_kernel and the streaming backward launches run at 64 channel
# groups, and the heads read 512 features (asn_head_fwd_kernel: C fmas per logit; the mask head: 8 fmas per lane).  No launch of the
# agent stores dz2 / dz3 at this chan (stored_expected=()): no tile kernel takes these data gradients.
def test_agent_is_exact_at_chan_512():
    _ok(A.run_leg(512, 2, 256, 60, expect=('group',), stored_expected=()))


def test_occlusion_agent_is_exact_at_chan_512():
    _ok(A.run_mask_leg(512, 2, 61, expect=('group',), stored_expected=()))


def test_agent_is_exact_at_chan_512_in_the_fp16_build():
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'asn_exact.py'), '512', '2', '256', '62', 'fresh', 'stored='], env=env,
                       capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 ASN EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- a history in front of the checked agent step (tests/exact_history.py), at the smallest res the agent accepts
@pytest.mark.parametrize('history', ('warm', 'after_eval'))
def test_agent_is_exact_after_a_history(history):
    _ok(A.run_leg(128, 2, 256, 57, history=history))


@pytest.mark.parametrize('history', ('warm', 'after_eval'))
def test_occlusion_agent_is_exact_after_a_history(history):
    _ok(A.run_mask_leg(128, 2, 58, history=history))


def test_agent_is_exact_after_warm_steps_in_the_fp16_build():
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'asn_exact.py'), '128', '2', '256', '59', 'warm'], env=env,
                       capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 ASN EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_agent_is_exact_in_the_fp16_build():
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'asn_exact.py'), '256', '3', '384', '56'], env=env,
                       capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 ASN EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_agent_creation_refuses_a_top_map_without_one_pool_window():
    """AvgPool2d(4) + view + Linear(chan, K): a res / 64 top map below 4 x 4 has no window (the reference raises), from 8 x 8 on it has
    four and the Linear does not fit."""
    from pose_adv_aug_amd._lib import lib, PoseAdvError
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    L = lib()
    for res in (64, 128, 192, 512, 1024):
        assert not L.pa_asn_create(128, 7, 7, 2, res), res
        assert b'res' in L.pa_last_error()
    with pytest.raises(PoseAdvError):
        create_asn(128, 128, 7, 7, is_aug=True, res=128, default_batch=2).state_dict()
    for res in (256, 384, 448):
        h = L.pa_asn_create(128, 7, 7, 2, res)
        assert h, res
        L.pa_net_destroy(h)

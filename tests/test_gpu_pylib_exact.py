"""The stand-alone pose-library operators on the device, element by element: the forward bilinear warp, pa_affine_params,
pa_transform_pts(_sized), pa_gaussian_heatmap, pa_weighted_l2, the validation flips and the layout converters, through the C ABI.
References, bounds, cases and legs: tests/pylib_exact.py (its docstring derives every constant).  Every case takes a few seconds at the most;
POSEADV_TEST_VERBOSE=1 prints the worst error / bound of every leg."""
import os
import subprocess
import sys

import pytest

from tests import pylib_exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _done(fails):
    assert not fails, fails


@pytest.mark.parametrize('name', X.WARP_CASES)
def test_warp_forward_element_by_element(name):
    """outf within d + u32 (|ref| + d) of the float64 sampler evaluated on the device's own tinv, out4 = outf rounded to the storage type
    bit for bit with a +0 fourth channel, either output alone and a second call give the same bits, guards untouched.  a .. d: the cases of
    the backward pass (b: sized, padding bytes 200); int: integer centres; sat: clamped to exactly 1.0; out: windows outside / over the
    corner of their frames; tiny: res 1 and 3 on 1 x 1 and 2 x 3 frames; stride: 2 359 296 pixels, past the 8192 x 256 grid cap"""
    if name == 'stride':
        cs = X.warp_case(name)
        assert cs['params'].shape[0] * cs['res'] * cs['res'] > 8192 * 256
    _done(X.warp_leg(name))


def test_affine_params_element_by_element():
    """B 65 (a full block of 64 and a tail), rotations 0, -0.0, 90, 180, 360, 1e-9, +-37.5, scales 0.05 .. 10, four resolution pairs:
    t_out and tinv_in within the running bound of their operations, t(res) o tinv(res) the identity"""
    _done(X.affine_leg())


@pytest.mark.parametrize('J,sized', ((16, False), (16, True), (5, False), (5, True)))
def test_transform_pts_element_by_element(J, sized):
    """B * J = 65 * J joints on the device's own t: mixed flips (J 16: the six pairs swapped; J 5: mirrored, not swapped), the invalid
    rule at y == 0, x == 0, x == width under flip and just inside each, per-sample widths through sizes, pts_img bit-exact"""
    _done(X.pts_leg(J, sized))


@pytest.mark.parametrize('J', X.HEAT_JOINTS)
@pytest.mark.parametrize('H,Wd', X.HEAT_SHAPES)
def test_gaussian_heatmap_bit_exact_on_non_square_maps(H, Wd, J):
    """hand-placed points (every edge and corner, truncation toward zero, x == W, y == H, the next double above, one coordinate past its
    own limit) against oracle.pylib.pts2heatmap(...).astype(float32), bit for bit"""
    _done(X.heat_leg(H, Wd, J))


@pytest.mark.parametrize('n', X.L2_SIZES)
def test_weighted_l2_bound_and_sentinels(n):
    """weight NULL / given, *loss from 0 / 1.5 (the call accumulates): within u32 D sum |term| / n of the exactly rounded float64 sum; one
    non-zero term at the first / last element of a block, of the first grid pass, of the grid-stride pass and of the array: exactly
    fl32(3 / n), which a dropped or doubled element cannot give"""
    _done(X.l2_leg(n))


@pytest.mark.parametrize('shape', X.FLIP_LR_SHAPES)
def test_flip_lr_nhwc4_bit_exact(shape):
    _done(X.flip_lr_leg(shape))


@pytest.mark.parametrize('shape', X.TTA_SHAPES)
def test_flip_tta_merge_bit_exact(shape):
    _done(X.tta_leg(shape))


@pytest.mark.parametrize('shape', X.CONVERT_SHAPES)
def test_layout_converters_bit_exact(shape):
    _done(X.convert_leg(shape))


def test_refused_calls_write_nothing():
    """refusals tests/test_pylib_exact_cpu.py has shown to return before any launch: non-zero, the message names the argument, the
    pre-filled outputs stay untouched"""
    _done(X.refusal_leg())


def test_half_precision_build():
    """every leg above in the IEEE-half build (out4, the converters and the input flip are where the storage type shows): one child
    process, the storage type is per process"""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'pylib_exact.py')], env=env, capture_output=True, text=True, timeout=600)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'PYLIB EXACT PASSED' in r.stdout and 'the fp16 build (pa_dtype 1)' in r.stdout, (r.stdout + r.stderr)[-3000:]

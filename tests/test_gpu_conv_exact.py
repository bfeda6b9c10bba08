"""Every convolution of the hourglass net against a float64 recomputation from the engine's own operands after one real training step,
element by element (checks and the derivation of every bound: tests/conv_exact.py).  tests/test_gpu_local.py bounds these convs at
1e-2 / 4e-2 rel-rms and tests/test_gpu_conv.py at 4e-3 rel-rms: a dropped halo tap, a shifted tile, a wrong rounding mode, a wrong
bias or addend or an 8-channel group with its neighbour's constants is a few percent in a few hundred elements, below both; here it is
a failure.

Legs (as tests/test_gpu_bn_exact.py): BASELINE configs[1] at full size; the configs[4] geometry (maps 96 / 48 / 24 / 12 / 6) at B 3; tiny
maps; the IEEE-half build on the configs[4] geometry in a child process; 1, 3 and 8 stacks; the step with occlusion masks; chan 512 at
the smallest batch that reaches each tile of the generic kernel; the input resolutions 320, 448, 192 and 64 (odd and 1 x 1 necks, 10 x 10 /
14 x 14 maps on the generic kernel, B 1 and B 5).  Then every shape of tests/test_gpu_conv.SHAPES through pa_conv2d
in all three modes, and the split-count mirror against the library's workspace sizes.

What a leg guards is geometric only: it has the map sizes that conv3x3_tile.hip's dispatch sends to the tiled 24 x 24 / 12 x 12 and masked
6 x 6 variants (the 384 leg) and shapes the grouped weight-gradient kernel takes ('group', from the split mirror), and it checks every conv
there; nothing the engine reports says which kernel ran.  The standalone shapes name those variants one by one (tests/test_gpu_conv.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conv_exact as X
from tests import inputs
from tests.test_gpu_conv import SHAPES, run_conv
from tests import conv_plan_query as Q

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leg(stacks, chan, B, res, seed, **kw):
    # the engine's launch log: the leg still makes every convolution launch tests/test_conv_plan_cpu.py counts it for
    with Q.launches('conv_exact %d stacks chan %d B %d res %d %s' % (stacks, chan, B, res, ' '.join('%s=%s' % (k, kw[k]) for k in sorted(kw) if k != 'expect'))):
        worst, fails = X.run_leg(stacks, chan, B, res, seed, **kw)
    assert not fails, '%d checks outside their bound, first: %s (worst per kind: %s)' % (len(fails), fails[:12], worst)


def test_every_conv_is_exact_at_the_benchmark_size():
    """BASELINE configs[1]: 2 stacks, chan 256, B 24, 256 x 256 (the grouped weight-gradient kernel takes the 64 x 64 layers)."""
    _leg(2, 256, 24, 256, 41, expect=('group',))


def test_every_conv_is_exact_on_the_384_geometry():
    """configs[4] geometry (maps 96 / 48 / 24 / 12 / 6) at B 3."""
    _leg(2, 256, 3, 384, 42, expect=('group',))


def test_every_conv_is_exact_on_tiny_maps():
    """chan 128, 128 x 128, B 2: 2 x 2 neck, the generic kernels."""
    _leg(2, 128, 2, 128, 43)


# ---- a history in front of the checked step (tests/exact_history.py)
@pytest.mark.parametrize('history', ('warm', 'graph', 'phased', 'after_eval'))
def test_every_conv_is_exact_after_a_history_on_tiny_maps(history):
    """The tiny-maps size with steps before the checked one: the weight copies the convs read were repacked by the optimizer steps
    (Checker.W rounds the current fp32 parameters), the loss accumulators were used and cleared by earlier forward passes."""
    _leg(2, 128, 2, 128, 45, history=history)


@pytest.mark.parametrize('history', ('warm', 'graph', 'after_half'))
def test_every_conv_is_exact_after_a_history_at_256(history):
    """chan 128, B 2, 256 x 256: the 64 x 64 maps give 2 * 8 * 4 = 64 tiles of 8 x 16 (>= 48), so the grouped weight-gradient kernel
    takes the 3 x 3 layers there ('group', from the split mirror), beside the tile kernels.  'after_half' runs here: the agent accepts
    no res below 256."""
    _leg(2, 128, 2, 256, 46, expect=('group',), history=history)


# ---- stack counts other than two (as tests/test_gpu_bn_exact.py): no inner head; a middle stack, whose xin<i> is written by
# in_conv.<i-1> and read in the backward pass by forth_conv.<i> and in_conv.<i>; the configs[4] depth
@pytest.mark.parametrize('stacks', (1, 3, 8))
def test_every_conv_is_exact_on_tiny_maps_at_other_stack_counts(stacks):
    _leg(stacks, 128, 2, 128, 61)


def test_every_conv_is_exact_with_a_middle_stack_in_the_phased_backward():
    _leg(3, 128, 2, 128, 62, history='phased')


def test_every_conv_is_exact_with_a_middle_stack_after_warm_steps_at_256():
    _leg(3, 128, 2, 256, 63, expect=('group',), history='warm')


# ---- the step with occlusion masks (loss_and_backward(dropout_masks=...)): up4 reads maskedneck, the decoder's merges hold masked skips
@pytest.mark.parametrize('history', ('fresh', 'warm'))
def test_every_conv_is_exact_in_a_masked_step(history):
    _leg(2, 128, 2, 256, 64, expect=('group',), history=history, masks=640)


def test_every_conv_is_exact_in_the_step_after_a_masked_one():
    _leg(2, 128, 2, 256, 65, expect=('group',), history='after_masked')


def test_every_conv_is_exact_in_a_masked_step_with_a_middle_stack():
    _leg(3, 128, 2, 256, 66, expect=('group',), masks=660)


# ---- chan 512 (C / 8 = 64 channel groups, the most the networks admit).  Not a wider run of the kernels above: no tile or one-shot
# instance exists for 512 input channels or for a 3 x 3 layer with 256, so every 512 -> 256, 512 -> 512 and 64 -> 512 forward, every
# 256 -> 512 and 256 -> 256 (3 x 3) data gradient and every 3 x 3 forward is a launch of the generic K-stepping kernel (conv_igemm.hip
# launch_taps) with the net's BNRELU / LIN2 loads and statistics / BatchNorm-backward epilogues, at K = 512 (8 steps) or 2304; the
# 256 -> 512 forward and the 512 -> 256 data gradient (256 input channels) take the one-shot kernel below 12288 pixels and the row-tile
# kernel from there.  The weight-gradient plans have 8 (1 x 1) and 16 (3 x 3) channel blocks.  Each leg is the smallest batch that
# reaches its tile of the generic kernel, which the leg asserts through the planner's query (_tier); the stem blocks (64 -> 128,
# 128 -> 128) run as at every chan.
def _tier(B, H, Cin, Cout, taps=1):
    """tiling of a forward launch of the net (BatchNorm + ReLU on load, statistics epilogue, bias) on an H x H map"""
    return Q.plan(B, H, H, Cin, Cout, taps, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)['tiling']


@pytest.mark.parametrize('history', ('fresh', 'warm'))
def test_every_conv_is_exact_at_chan_512_on_tiny_maps(history):
    """2 stacks, chan 512, B 2, 128 x 128: maps 32 x 32 ... 2 x 2, every generic launch on the <64,64> instance (M <= 2048), the inner
    head (forth_conv 512 -> 512, in_conv 64 -> 512); 'warm': the weight copies repacked by optimizer steps."""
    assert {_tier(2, H, 512, 256) for H in (32, 16, 8, 4, 2)} == {'G64x64_1'} and _tier(2, 32, 256, 256, 9) == 'G64x64_9'
    _leg(2, 512, 2, 128, 71, expect=('group',), history=history)


def test_every_conv_is_exact_at_chan_512_on_the_64x128_tiles():
    """1 stack, chan 512, B 4, 256 x 256: the 64 x 64 maps have M = 16384, the <64,128> instance of the generic kernel."""
    assert (_tier(4, 64, 512, 256), _tier(4, 64, 256, 256, 9)) == ('G64x128_1', 'G64x128_9')
    _leg(1, 512, 4, 256, 72, expect=('group',))


def test_every_conv_is_exact_at_chan_512_on_the_128_row_tiles():
    """1 stack, chan 512, B 8, 256 x 256: the 64 x 64 maps have M = 32768 (bigM), the <128,128> instance (and <128,64> for out_conv's
    forward, 512 -> 64) with the net's load and epilogue modes; the 32 x 32 maps (M = 8192) stay on <64,64>."""
    assert (_tier(8, 64, 512, 256), _tier(8, 64, 512, 64), _tier(8, 64, 256, 256, 9), _tier(8, 32, 512, 256)) == ('G128x128_1', 'G128x64_1', 'G128x128_9', 'G64x64_1')
    _leg(1, 512, 8, 256, 73, expect=('group',))


def test_every_conv_is_exact_at_chan_512_in_a_masked_step():
    """2 stacks, chan 512, B 2, 256 x 256 with occlusion masks: the <64,64> instance at M = 8192 behind the cell mask and the masked
    merges at 64 channel groups; up4 reads maskedneck."""
    _leg(2, 512, 2, 256, 74, expect=('group',), masks=740)


# ---- input resolutions other than 128 / 256 / 384 (every res % 64 == 0 is accepted): map sides 80 / 40 / 20 / 10 / 5 (320), 112 / 56 / 28 /
# 14 / 7 (448), 48 / 24 / 12 / 6 / 3 (192) and 16 / 8 / 4 / 2 / 1 (64).  What each side reaches, by csrc/conv_plan.h (asserted through the
# planner's query, not re-derived; tests/test_conv_plan_cpu.py::test_documented_examples_of_the_other_resolutions states the rules): the
# 3 x 3 layers on 10 x 10 and 14 x 14 maps take the generic K-stepping kernel with the net's BatchNorm loads (a side above 8 that is no
# multiple of 4: its 64-pixel M tiles wrap image rows of width 10 / 14); 5 x 5, 7 x 7, 3 x 3 and 1 x 1 maps are one masked 8 x 8 tile, two
# images per workgroup; 40 / 56 take the 8 x 8 halo tiles, 20 / 28 the 4 x 4 ones.  The weight-gradient plans (the mirror, wgrad_plan) have
# ragged last tiles (1 * 56 * 56 pixels = 24.5 tiles of 128) and generic plans of fewer pixels than one 32-pixel MFMA step (M = 3 ... 49).
def _path3(B, H, Cin):
    """(path, tiling without its channel suffix) of a 3 x 3 forward launch of the net on an H x H map with Cin = Cout"""
    d = Q.plan(B, H, H, Cin, Cin, 9, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)
    return d['path'], d['tiling'].split('_')[0]


def test_every_conv_is_exact_on_the_320_geometry():
    """2 stacks, chan 256, B 2, 320 x 320 (maps 80 / 40 / 20 / 10 / 5).  The upsample-add data gradient on the 80 x 80 maps (2 * 80 * 80 / 64 =
    200 row tiles, W % 32 != 0) is refused with its second output and re-planned without it (Net::conv_dgrad)."""
    assert [_path3(2, H, 128) for H in (40, 20, 10, 5)] == [(Q.TILE3, 'TS8'), (Q.TILE3, 'TS4'), (Q.GENERIC, 'G64x64'), (Q.TILE3, 'TS8')]
    up = dict(in_=Q.LIN2, a1=Q.PLAIN, ep=Q.OUT_PLAIN)
    assert Q.plan(2, 80, 80, 128, 256, 1, ep2=Q.OUT_BWD, flags=Q.OUT2, **up)['path'] == Q.REFUSED and Q.plan(2, 80, 80, 128, 256, 1, **up)['path'] == Q.ROW
    _leg(2, 256, 2, 320, 81, expect=('group',))


def test_every_conv_is_exact_on_the_448_geometry_at_batch_1():
    """2 stacks, chan 128, B 1, 448 x 448 (maps 112 / 56 / 28 / 14 / 7): one image, 64 mid channels, ragged weight-gradient tiles."""
    assert [_path3(1, H, 64) for H in (56, 28, 14, 7)] == [(Q.TILE3, 'TS8'), (Q.TILE3, 'TS4'), (Q.GENERIC, 'G64x64'), (Q.TILE3, 'TS8')]
    assert X.wgrad_plan(1, 56, 56, 64, 128, 1)[:4] == ('tile', 128, 64, 25) and 1 * 56 * 56 % 128 != 0
    _leg(2, 128, 1, 448, 82, expect=('group',))


def test_every_conv_is_exact_on_the_192_geometry_at_batch_5():
    """2 stacks, chan 128, B 5, 192 x 192 (maps 48 / 24 / 12 / 6 / 3): an odd batch above 3, the 3 x 3 neck (45 pixels)."""
    assert _path3(5, 3, 64) == (Q.TILE3, 'TS8') and Q.plan(5, 3, 3, 64, 64, 9, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)['gx'] == 3
    assert X.wgrad_plan(5, 3, 3, 64, 64, 9)[:2] == ('generic', 64) and X.wgrad_plan(5, 3, 3, 64, 64, 9).splits == 1
    _leg(2, 128, 5, 192, 83, expect=('group',))


def test_every_conv_is_exact_on_the_64_geometry():
    """2 stacks, chan 256, B 4, 64 x 64 (maps 16 / 8 / 4 / 2 / 1): the 1 x 1 neck, where only the centre tap of a 3 x 3 layer meets a
    pixel and a BatchNorm normalises one value per image.  B 4 is the smallest batch whose operands leave the bounds of
    tests/test_gpu_bn_exact.py's leg of the same arguments meaningful (B 3 was degenerate there); the two files keep the same arguments."""
    assert _path3(4, 1, 128) == (Q.TILE3, 'TS8') and Q.plan(4, 1, 1, 128, 128, 9, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)['gx'] == 2
    _leg(2, 256, 4, 64, 84)


def test_every_conv_is_exact_at_chan_512_on_the_320_geometry():
    """1 stack, chan 512, B 2, 320 x 320: the generic kernel at K = 512 / 2304 on maps of width 80 ... 5 (M = 12800 ... 50)."""
    assert {_tier(2, H, 512, 256) for H in (80, 40, 20, 10, 5)} == {'G64x64_1'} and {_tier(2, H, 256, 256, 9) for H in (80, 40, 20, 10, 5)} == {'G64x64_9'}
    _leg(1, 512, 2, 320, 85, expect=('group',))


@pytest.mark.parametrize('history', ('warm', 'graph'))
def test_every_conv_is_exact_after_a_history_on_the_320_geometry(history):
    """chan 128, B 2, 320 x 320 behind optimizer steps (repacked weight copies) and in a graph replay."""
    _leg(2, 128, 2, 320, 86, history=history)


def _fp16_child(args):
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'conv_exact.py')] + args, env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 CONV EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_every_conv_is_exact_with_a_middle_stack_in_the_fp16_build():
    """The IEEE-half library, 3 stacks on the 96 / 48 / 24 / 12 / 6 geometry at chan 128, B 2."""
    _fp16_child(['3', '128', '2', '384', '67'])


def test_every_conv_is_exact_in_a_masked_step_in_the_fp16_build():
    _fp16_child(['2', '128', '2', '256', '68', 'fresh', '680'])


def test_every_conv_is_exact_at_chan_512_in_the_fp16_build():
    """The IEEE-half library on the chan-512 tiny-maps leg (2 stacks, B 2, 128 x 128): the generic <64,64> instance at K = 512 / 2304."""
    _fp16_child(['2', '512', '2', '128', '75'])


def test_every_conv_is_exact_on_the_320_geometry_in_the_fp16_build():
    """The IEEE-half library at chan 128, B 2, 320 x 320 (maps 80 / 40 / 20 / 10 / 5)."""
    _fp16_child(['2', '128', '2', '320', '87'])


def test_every_conv_is_exact_after_warm_steps_in_the_fp16_build():
    """The IEEE-half library, 'warm' at chan 128, B 2, 256 x 256, in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'conv_exact.py'), '2', '128', '2', '256', '47', 'warm'], env=env,
                       capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 CONV EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_every_conv_is_exact_in_the_fp16_build():
    """The IEEE-half library on the configs[4] geometry, in a child process (one storage type per process)."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'conv_exact.py'), '2', '256', '3', '384', '44'], env=env,
                       capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 CONV EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Cin,Cout,H,W,k', SHAPES)
def test_standalone_conv_shapes_are_exact(B, Cin, Cout, H, W, k):
    """pa_conv2d forward (with bias), data gradient and weight + bias gradient of every tests/test_gpu_conv shape, each element within
    its bound.  (pa_conv2d declares the layer without a BatchNorm behind it: S is the layer's split count, grouped where the grouped
    kernel takes the shape -- Net::layout_conv with the batch set.)"""
    from pose_adv_aug_amd._lib import act_dtype
    dt = act_dtype()
    g = inputs.rng(500, B, Cin, Cout, H, W, k)
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    x, dy = f(B, Cin, H, W), f(B, Cout, H, W)
    w = f(Cout, Cin, k, k) / float(np.sqrt(Cin * k * k))
    bias = f(Cout)
    xd, dyd, wd = X.rnd(x.double(), dt).cuda(), X.rnd(dy.double(), dt).cuda(), X.rnd(w.double(), dt).cuda()
    worst = {}
    y, _ = run_conv(0, x, None, w, bias, B, Cin, Cout, H, W, k)
    worst['forward'] = X.check16(y.cuda(), X.conv_term(xd, wd, Cin * k * k, bias.double().cuda()), dt)
    dx, _ = run_conv(1, dy, None, w, None, B, Cin, Cout, H, W, k)
    worst['data gradient'] = X.check16(dx.cuda(), X.dgrad_term(dyd, wd, Cout * k * k), dt)
    dw, db = run_conv(2, dy, x, w, None, B, Cin, Cout, H, W, k)
    S = X.layer_splits(B, H, W, Cin, Cout, k)
    worst['weight gradient'] = X.wgrad_check(dw.cuda(), xd, dyd, k, S)
    worst['bias gradient'] = X.bgrad_check(db.cuda(), dyd, S)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print('conv_exact %s: S %d, worst error / bound, degenerate fraction: %s' % ((B, Cin, Cout, H, W, k), S, worst))
    for kind, (r, deg) in worst.items():
        assert r <= 1.0, (kind, r, worst)
        assert deg <= X.DEGENERATE, ('degenerate bound', kind, deg)


# ---------------------------------------------------------------------------------------------------------------------------------
def _al(v):
    return (v + 255) & ~255


def _arena(sizes):
    """bytes of an Arena after these takes (net.h Arena::take: each take starts 256-aligned), plus the final take(0)."""
    off = 0
    for s in sizes:
        off = _al(off) + s
    return _al(off)


# the job tables at the front of ConvOp::build / WgradGroupOp::build (api.hip): PaPrepJob, PaWgradReduceJob, PaBnEvalJob, each < 256 bytes
_TABLES = [48, 56, 56]


@pytest.mark.parametrize('B,Cin,Cout,H,W,k', sorted(set(
    [s for s in SHAPES] +
    # the layers of the legs: 64 x 64 / 96 x 96 ... 4 x 4, 1 x 1 and 3 x 3, chan 128 / 256, the head's 16-channel layers padded to 64
    [(24, 256, 128, 64 >> j, 64 >> j, 1) for j in range(5)] + [(24, 128, 128, 64 >> j, 64 >> j, 3) for j in range(5)] +
    [(24, 128, 256, 64 >> j, 64 >> j, 1) for j in range(5)] + [(3, 256, 128, 96 >> j, 96 >> j, 1) for j in range(5)] +
    [(3, 128, 128, 96 >> j, 96 >> j, 3) for j in range(5)] + [(2, 64, 64, 32 >> j, 32 >> j, 3) for j in range(4)] +
    [(24, 256, 64, 64, 64, 1), (24, 64, 256, 64, 64, 1), (3, 64, 256, 96, 96, 1), (2, 64, 128, 32, 32, 1)] +
    # the layers of the chan-512 legs: B 2 at 32 x 32 ... 2 x 2, B 2 / 4 / 8 at 64 x 64 ... 4 x 4; residual3 (128 -> 256 -> 512, adapter
    # 128 -> 512) and the head (512 -> 512, 512 -> 16 and 16 -> 512 padded to 64)
    [(2, ci, co, 32 >> j, 32 >> j, k) for ci, co, k in ((512, 256, 1), (256, 256, 3), (256, 512, 1)) for j in range(5)] +
    [(B, ci, co, 64 >> j, 64 >> j, k) for B in (2, 4, 8) for ci, co, k in ((512, 256, 1), (256, 256, 3), (256, 512, 1)) for j in range(5)] +
    [(B, ci, co, H, H, 1) for B, H in ((2, 32), (2, 64), (4, 64), (8, 64))
     for ci, co in ((128, 256), (128, 512), (512, 512), (512, 64), (64, 512))])))
def test_split_mirror_matches_the_library(B, Cin, Cout, H, W, k):
    """S of tests/conv_exact.py (wgrad_plan, the mirror of pa_wgrad_plan) against the split counts the library's workspace sizes reveal:
    pa_conv2d_workspace_bytes lays the layer out without a batch (no grouped split: PaWgradPlan::splits), pa_wgrad_group_workspace_bytes
    with it (group_splits where the grouped kernel takes the shape).  Both workspaces hold S slabs of Cout * taps * Cin floats.  No HIP
    call is made: tests/test_conv_exact_cpu.py runs this test without a GPU as well."""
    from pose_adv_aug_amd._lib import lib
    L = lib()
    M, wn = B * H * W, Cout * k * k * Cin
    # ConvOp::build: tables, wf, wb, part [S][wn], dbpart [S][Cout] (declared without a BatchNorm behind it), xin, yout
    fixed = lambda S, db: _arena(_TABLES + [2 * wn, 2 * wn, 4 * S * wn] + ([4 * S * Cout] if db else []) + [2 * M * Cin, 2 * M * Cout])
    got = L.pa_conv2d_workspace_bytes(B, Cin, Cout, H, W, k)
    S1 = [S for S in range(1, 4097) if fixed(S, True) == got]
    assert S1 == [X.wgrad_splits(M, H, W, Cin, Cout, k * k)], (got, S1)

    class Job(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int) for n in ('B', 'Cin', 'Cout', 'H', 'W', 'k')] + \
                   [(n, ctypes.c_void_p) for n in ('dy', 'dy_q', 'dy_k', 'x', 'x_k', 'dw', 'db')]
    j = Job(B, Cin, Cout, H, W, k)
    got = L.pa_wgrad_group_workspace_bytes(ctypes.addressof(j), 1)
    nparams = ((Cout * Cin * k * k + 3) & ~3) + Cout
    # WgradGroupOp::build (one job, no bias gradient): tables, wf, wb, part [S][wn], dy, x, pbuf, gbuf
    grp = lambda S: _arena(_TABLES + [2 * wn, 2 * wn, 4 * S * wn, 2 * M * Cout, 2 * M * Cin, 4 * (nparams + 8), 4 * (nparams + 8)])
    S2 = [S for S in range(1, 4097) if grp(S) == got]
    assert S2 == [X.layer_splits(B, H, W, Cin, Cout, k)], (got, S2)


@pytest.mark.parametrize('B,Cin,Cout,H,W,k,alone,grouped', [(2, 64, 64, 16, 16, 1, 4, 2), (3, 64, 64, 32, 64, 3, 48, 12)])
def test_conv2d_weight_gradient_stays_inside_its_workspace(B, Cin, Cout, H, W, k, alone, grouped):
    """pa_conv2d_workspace_bytes lays the layer out without the batch (the slab count of a launch alone), pa_conv2d with it (the smaller
    grouped count): the smallest shapes where the two differ, run inside exactly the reported bytes with 64 MB guard regions on both
    sides.  With a bias gradient (the layout of the size query; a 3 x 3 launch then takes the generic kernel at the grouped count) and
    without one (fewer bytes; the tile kernels).  The guards stay untouched and the gradients are within their bounds at S = grouped."""
    import ctypes as C
    from pose_adv_aug_amd._lib import lib, check, ptr, stream, act_dtype
    L = lib()
    dt = act_dtype()
    assert (X.wgrad_splits(B * H * W, H, W, Cin, Cout, k * k), X.layer_splits(B, H, W, Cin, Cout, k)) == (alone, grouped)
    g = inputs.rng(501, B, Cin, Cout, H, W, k)
    f = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32))
    x, dy, w = f(B, Cin, H, W).cuda(), f(B, Cout, H, W).cuda(), f(Cout, Cin, k, k).cuda()
    xd, dyd = X.rnd(x.double(), dt), X.rnd(dy.double(), dt)
    nws = L.pa_conv2d_workspace_bytes(B, Cin, Cout, H, W, k)
    SL = 64 << 20
    for want_db in (True, False):
        big = torch.zeros(nws + 2 * SL, dtype=torch.uint8, device='cuda')
        big[:SL] = 0x5A; big[SL + nws:] = 0x5A
        dw = torch.empty((Cout, Cin, k, k), device='cuda')
        db = torch.empty(Cout, device='cuda') if want_db else None
        check(L.pa_conv2d(2, ptr(dy), ptr(x), ptr(w), None, ptr(dw), ptr(db), B, Cin, Cout, H, W, k,
                          C.c_void_p(big.data_ptr() + SL), stream()), 'pa_conv2d')
        torch.cuda.synchronize()
        assert bool((big[:SL] == 0x5A).all()) and bool((big[SL + nws:] == 0x5A).all()), want_db
        worst = {'weight gradient': X.wgrad_check(dw, xd, dyd, k, grouped)}
        if want_db:
            worst['bias gradient'] = X.bgrad_check(db, dyd, grouped)
        for kind, (r, deg) in worst.items():
            assert r <= 1.0, (kind, want_db, r, worst)
            assert deg <= X.DEGENERATE, ('degenerate bound', kind, want_db, deg)

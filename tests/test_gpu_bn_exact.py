"""Every BatchNorm, max pool and upsample-add of the hourglass net against a float64 recomputation from the engine's own stored tensors
after one real training step (checks and the derivation of every bound: tests/bn_exact.py).  The per-node tests
(tests/test_gpu_local.py) bound these operations only at 1e-2 / 4e-2 rel-rms; here a dropped, doubled or overwritten partial
statistics row, a wrong variance, a wrong summation order or a rounding error of the fused / split / streaming launches is a failure.

Legs: BASELINE configs[1] at full size (the only leg that reaches the fused low-resolution half of the upsample-add backward in the 1 x 1
data gradient's epilogue, the split upsample-add launches, 1536-row statistics and the consumer-prologue finalize at <= 128 rows); the
configs[4] geometry (384 x 384: the 24 x 24 / 12 x 12 tiled 3 x 3 variants, the masked 6 x 6 neck) at a ragged batch; tiny maps (2 x 2 neck,
8 values per channel: biased and unbiased variance differ by 14 %); and the IEEE-half build on the configs[4] geometry in a child process.
Then the tiny-maps size at 1, 3 and 8 stacks (no inner head; a middle stack -- a plain xin<i> with a nonzero gradient arriving from the
next stack; the configs[4] depth), 3 stacks behind a phased / warm history and in the IEEE-half build, and the step with occlusion masks
(loss_and_backward(dropout_masks=...), the occlusion agent's training path) at 256 x 256, the smallest size with a 4 x 4 neck.  Last,
chan 512 (64 channel groups, separate finalize launches) at the sizes of tests/test_gpu_conv_exact.py's chan-512 legs, and the input
resolutions 320, 448, 192 and 64 with that file's arguments (map widths that fit no streaming row walk, necks of 1 ... 49 pixels)."""
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


# ---- stack counts other than two.  One stack: forth / inc / dheat_in / lgrad_tmp are empty.  Three: stack 1 is neither first nor last
# (run_leg asserts that pool 1 of every middle stack met a nonzero addend over an input without a pending BatchNorm).  Eight: the depth
# of BASELINE configs[4].
@pytest.mark.parametrize('stacks', (1, 3, 8))
def test_every_bn_pool_and_merge_is_exact_on_tiny_maps_at_other_stack_counts(stacks):
    _leg(stacks, 128, 2, 128, 51, stored_expected=('.x2',))


def test_every_bn_pool_and_merge_is_exact_with_a_middle_stack_in_the_phased_backward():
    """3 stacks, tiny maps, RMSprop(overlap=True): four phases of pa_hg_backward_phase, phase 1 a middle stack."""
    _leg(3, 128, 2, 128, 52, stored_expected=('.x2',), history='phased')


def test_every_bn_pool_and_merge_is_exact_with_a_middle_stack_after_warm_steps_at_256():
    _leg(3, 128, 2, 256, 53, history='warm')


# ---- the step with occlusion masks: 2 stacks, chan 128, B 2, 256 x 256 as the history legs above.  Which blocks store dz2 / dz3 does not
# change under masks: Net::drop_mask switches x3_fin_ok off, which only moves x3's backward FINALIZE out of conv3's data-gradient prologue
# into a launch of its own; whether that data gradient stores dz3 (dz2) is the plan's stores_dz over shape and modes alone, which the
# first leg asserts for residual1's maps (128 x 128: both) and the hourglass blocks' (64 x 64: dz2).  So both kinds stay expected.
def _stores_dz(B, H, Cin, Cout, taps):
    from tests import conv_plan_query as Q
    return Q.plan(B, H, H, Cin, Cout, taps, in_=Q.LIN2, ep=Q.OUT_BWD, flags=Q.DZ)['stores_dz']


@pytest.mark.parametrize('history', ('fresh', 'warm'))
def test_every_bn_pool_merge_and_cell_mask_is_exact_in_a_masked_step(history):
    assert _stores_dz(2, 128, 128, 64, 1) and _stores_dz(2, 128, 64, 64, 9) and _stores_dz(2, 64, 64, 64, 9) and not _stores_dz(2, 64, 128, 64, 1)
    _leg(2, 128, 2, 256, 54, history=history, masks=540)


def test_every_bn_pool_and_merge_is_exact_in_the_step_after_a_masked_one():
    """'after_masked': a masked step and an optimizer step, then the checked step without masks."""
    _leg(2, 128, 2, 256, 55, history='after_masked')


def test_every_bn_pool_merge_and_cell_mask_is_exact_in_a_masked_step_with_a_middle_stack():
    _leg(3, 128, 2, 256, 56, masks=560)


# ---- chan 512: C / 8 = 64 channel groups, the most pa_stats_groups_ok admits -- a wave of a streaming kernel is exactly one pixel and
# flush_stats has no lane left to shuffle with.  The plan's takes_fin is false above 256 input channels, so the BatchNorm in front of
# every conv1 (512 -> 256) and of every conv3 data gradient (512 gradient channels) is finalized by a launch of its own
# (bn_finalize_kernel / the backward finalize, reduce_partial_rows in its <= 128-row order) where the nets above use the consumer
# prologue; the statistics and BatchNorm-backward epilogues run in the generic conv kernel's tiles (tests/test_gpu_conv_exact.py names the
# tier of each size).  Which blocks store dz2 / dz3: no tile instance takes 512 gradient channels or a 3 x 3 layer with 256, so only the
# stem's blocks (64 and 128 channels at every chan) can -- their 3 x 3 tile launches at every size (dz2), residual1's conv3 data
# gradient as a row-tile launch from 12288 pixels (dz3: the 256 x 256 legs, not the 128 x 128 ones).
@pytest.mark.parametrize('history', ('fresh', 'warm'))
def test_every_bn_pool_and_merge_is_exact_at_chan_512_on_tiny_maps(history):
    """2 stacks, chan 512, B 2, 128 x 128: maps 32 x 32 ... 2 x 2, <= 32 partial rows everywhere in the hourglasses (the finalize
    launches' small-row order), the inner head; 'warm': running estimates and weights from a non-initial state."""
    from tests import conv_plan_query as Q
    # no consumer prologue above 256 input channels: conv1's forward (512 -> 256) and conv3's data gradient (512 gradient channels); conv2's has one
    assert not Q.plan(2, 32, 32, 512, 256, 1, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)['takes_fin']
    assert not Q.plan(2, 32, 32, 512, 256, 1, in_=Q.LIN2, ep=Q.OUT_BWD, flags=Q.DZ)['takes_fin']
    assert Q.plan(2, 32, 32, 256, 256, 9, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)['takes_fin']
    _leg(2, 512, 2, 128, 71, stored_expected=('.x2',), history=history)


def test_every_bn_pool_and_merge_is_exact_at_chan_512_on_the_64x128_tiles():
    """1 stack, chan 512, B 4, 256 x 256: M = 16384 at 64 x 64, the generic kernel's <64,128> epilogues (256 rows: the finalize launches'
    sliced order), streaming launches of 512-thread workgroups."""
    _leg(1, 512, 4, 256, 72)


def test_every_bn_pool_and_merge_is_exact_at_chan_512_on_the_128_row_tiles():
    """1 stack, chan 512, B 8, 256 x 256: M = 32768 at 64 x 64, the <128,128> / <128,64> epilogues (128-pixel partial rows)."""
    _leg(1, 512, 8, 256, 73)


def test_every_bn_pool_merge_and_cell_mask_is_exact_at_chan_512_in_a_masked_step():
    """2 stacks, chan 512, B 2, 256 x 256 with occlusion masks: the cell mask's forward and backward launches (with their statistics
    epilogue) and the masked merges at 64 channel groups."""
    _leg(2, 512, 2, 256, 74, masks=740)


# ---- input resolutions other than 128 / 256 / 384: the legs of tests/test_gpu_conv_exact.py, argument for argument.  The statistics rows
# come from the kernels named there (64-pixel rows of the generic kernel on the 10 x 10 / 14 x 14 maps, one row per masked 8 x 8 workgroup
# of two images on the 5 x 5 / 7 x 7 / 3 x 3 / 1 x 1 necks).  The backward streaming launches (csrc/launch_plan.h: blockDim and the
# (W / 2) * (C / 8) items of a row must divide one another, over the tried sizes 512 / 256 / 384 / 192 / 128) fit the row walk at chan 256
# with 256 threads on the 80- and 112-wide maps (1280 / 1792 items) and with 128 on 40 / 56 (640 / 896), at chan 128 with 128 threads on
# 80 / 112 (640 / 896); 20 / 28 / 10 / 14 at chan 256 (320 / 448 / 160 / 224 items) and 40 / 56 / 20 / 28 / 10 / 14 at chan 128 fit no
# tried size and go to the generic max-pool and upsample-add kernels.  tests/bn_exact.py re-derives the depth D for these shapes:
# nothing changes.
def test_every_bn_pool_and_merge_is_exact_on_the_320_geometry():
    """2 stacks, chan 256, B 2, 320 x 320 (maps 80 / 40 / 20 / 10 / 5): the upsample-add backward of the 80 x 80 merges runs as a launch of
    its own behind the row-tile data gradient (the fused form is refused: W % 32 != 0)."""
    _leg(2, 256, 2, 320, 81)


def test_every_bn_pool_and_merge_is_exact_on_the_448_geometry_at_batch_1():
    """2 stacks, chan 128, B 1, 448 x 448 (maps 112 / 56 / 28 / 14 / 7): 49 values per channel at the neck."""
    _leg(2, 128, 1, 448, 82)


def test_every_bn_pool_and_merge_is_exact_on_the_192_geometry_at_batch_5():
    """2 stacks, chan 128, B 5, 192 x 192 (maps 48 / 24 / 12 / 6 / 3): 45 values per channel at the 3 x 3 neck, the last pool reads 6 x 6."""
    _leg(2, 128, 5, 192, 83)


def test_every_bn_pool_and_merge_is_exact_on_the_64_geometry():
    """2 stacks, chan 256, B 4, 64 x 64 (maps 16 / 8 / 4 / 2 / 1): BatchNorms over 4 values per channel at the 1 x 1 neck (biased and
    unbiased variance differ by a third), the last pool reads one 2 x 2 window per image.  B 3 -- three values per channel -- was
    DEGENERATE with this seed: the pooled, ReLU'd values of down4's input lie so close together in some channels (|mean| / sigma above
    about 45) that the invstd interval of hg.0.down4.0.bn1, hg.0.down4.0.bn3 and hg.1.down4.0.bn1 was 1.64 - 1.77 % wide, a property of the
    operands and not of the kernels; B 4 is the smallest batch that is not (widest interval 0.26 %; B 5: 0.28 %, B 6: 0.10 %).
    residual1's 32 x 32 maps are 64 row tiles, below the 192 the row-tile kernel takes: no dz3 is stored, the 3 x 3 tile launches store dz2."""
    assert not _stores_dz(4, 32, 128, 64, 1) and _stores_dz(4, 32, 64, 64, 9)
    _leg(2, 256, 4, 64, 84, stored_expected=('.x2',))


def test_every_bn_pool_and_merge_is_exact_at_chan_512_on_the_320_geometry():
    """1 stack, chan 512, B 2, 320 x 320: 64 channel groups on maps of width 80 ... 5, separate finalize launches; residual1's conv3 data
    gradient (160 x 160: 800 row tiles) stores dz3 as on the 256 x 256 legs."""
    assert _stores_dz(2, 160, 128, 64, 1) and _stores_dz(2, 160, 64, 64, 9)
    _leg(1, 512, 2, 320, 85)


@pytest.mark.parametrize('history', ('warm', 'graph'))
def test_every_bn_pool_and_merge_is_exact_after_a_history_on_the_320_geometry(history):
    """chan 128, B 2, 320 x 320 behind optimizer steps and in a graph replay."""
    _leg(2, 128, 2, 320, 86, history=history)


def test_every_bn_pool_and_merge_is_exact_on_the_320_geometry_in_the_fp16_build():
    """The IEEE-half library at chan 128, B 2, 320 x 320, in a child process."""
    _fp16_child(['2', '128', '2', '320', '87'])


def test_every_bn_pool_and_merge_is_exact_at_chan_512_in_the_fp16_build():
    """The IEEE-half library on the chan-512 tiny-maps leg, in a child process."""
    _fp16_child(['2', '512', '2', '128', '75', 'stored=x2'])


def _fp16_child(args):
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'bn_exact.py')] + args, env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 BN EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_every_bn_pool_and_merge_is_exact_after_warm_steps_in_the_fp16_build():
    """The IEEE-half library, 'warm' at chan 128, B 2, 256 x 256, in a child process."""
    _fp16_child(['2', '128', '2', '256', '37', 'warm'])


def test_every_bn_pool_and_merge_is_exact_with_a_middle_stack_in_the_fp16_build():
    """The IEEE-half library, 3 stacks on the 96 / 48 / 24 / 12 / 6 geometry at chan 128, B 2."""
    _fp16_child(['3', '128', '2', '384', '57'])


def test_every_bn_pool_merge_and_cell_mask_is_exact_in_a_masked_step_in_the_fp16_build():
    _fp16_child(['2', '128', '2', '256', '58', 'fresh', '580'])


def test_every_bn_pool_and_merge_is_exact_in_the_fp16_build():
    """The IEEE-half library on the configs[4] geometry, in a child process (one storage type per process)."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'bn_exact.py'), '2', '256', '3', '384', '34'], env=env,
                       capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 BN EXACT PASSED' in r.stdout, out[-3000:]

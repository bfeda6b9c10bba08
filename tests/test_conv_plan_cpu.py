"""The forward / data-gradient convolution planner (csrc/conv_plan.h) through the read-only query pa_conv_plan_describe: no device call, so
these run without a GPU.

* PINNED: the plan of the benchmark's launches (batch 24, chan 256) and of the documented chan-512 tiers.  The expected rows were recorded
  from the launchers of the commit BEFORE the planner existed (their launch macro replaced by a recorder), not from the planner.
* INVARIANTS over a grid of shapes and every combination of load / addend / epilogue modes.
* COVERAGE: every instance id the planner can return is run by tests/test_gpu_conv.py::SHAPES or by a recorded launch of a conv-exact or
  pool-route leg, or is listed with the reason why no numerical test can run it.
"""
import pytest

from tests.conv_plan_query import *  # noqa: F401,F403
from tests import conv_plan_query as Q


@pytest.fixture(scope='module')
def L():
    return Q.lib()


# (B, H, W, Cin, Cout, taps, in, add1, add2, ep, ep2, fin rows, flags, CUs):
#     (path, tiling, variant, grid x, grid y, threads, nbw, rows, rows2, xcd, stores dz, takes a finalize)
# variant: 0 plain, 1 BatchNorm + ReLU, 2 BatchNorm backward on load, 4 / 5 = 1 / 2 with the finalize prologue, 6 / 7 pool-routed second addend
# with the BatchNorm-backward / plain epilogue.  Forward launches carry a bias (flags 1); 4 = a dz buffer is offered.
PINNED = {
    (24, 64, 64, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'T16x8_128_128', 1, 768, 1, 256, 0, 768, 0, 1, 0, 0),
    (24, 32, 32, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'T16x4_128_64', 1, 384, 2, 256, 0, 384, 0, 1, 0, 1),
    (24, 16, 16, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'T16x4_128_64_T512', 1, 96, 2, 512, 0, 96, 0, 1, 0, 1),
    (24, 16, 16, 128, 128, 9, 1, -1, -1, 1, 0, 96, 1, 256): (5, 'T16x4_128_64_T512', 4, 96, 2, 512, 0, 96, 0, 1, 0, 1),
    (24, 8, 8, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'TS8_128_64_T512', 1, 12, 2, 512, 0, 12, 0, 0, 0, 1),
    (24, 4, 4, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'TS4_128_64_T512', 1, 3, 2, 512, 0, 3, 0, 0, 0, 1),
    (24, 64, 64, 256, 128, 1, 1, -1, -1, 1, 0, 0, 1, 256): (3, 'R256_64_128_K32', 1, 1536, 1, 256, 1, 1536, 0, 0, 0, 0),
    (24, 64, 64, 128, 256, 1, 1, -1, -1, 1, 0, 0, 1, 256): (3, 'R128_64_128', 1, 1536, 1, 256, 2, 1536, 0, 0, 0, 0),
    (24, 64, 64, 128, 256, 1, 1, 0, -1, 0, 0, 0, 1, 256): (3, 'R128_64_128', 1, 1536, 1, 256, 2, 1536, 0, 0, 0, 0),
    (24, 16, 16, 128, 256, 1, 1, -1, -1, 1, 0, 0, 1, 256): (2, 'OS2', 1, 96, 4, 256, 0, 96, 0, 0, 0, 1),
    (24, 16, 16, 128, 256, 1, 1, -1, -1, 1, 0, 96, 1, 256): (2, 'OS2', 4, 96, 4, 256, 0, 96, 0, 0, 0, 1),
    (24, 16, 16, 256, 128, 1, 1, -1, -1, 1, 0, 96, 1, 256): (2, 'OS4', 4, 96, 2, 256, 0, 96, 0, 0, 0, 1),
    (24, 64, 64, 256, 128, 1, 2, -1, -1, 2, 0, 0, 4, 256): (3, 'R256_64_128_K32', 2, 1536, 1, 256, 1, 1536, 0, 0, 1, 0),
    (24, 64, 64, 128, 128, 9, 2, -1, -1, 2, 0, 0, 4, 256): (5, 'T16x8_128_128', 2, 768, 1, 256, 0, 768, 0, 1, 1, 0),
    (24, 32, 32, 128, 128, 9, 2, -1, -1, 2, 0, 0, 4, 256): (5, 'T16x4_128_64', 2, 384, 2, 256, 0, 384, 0, 1, 1, 1),
    (24, 16, 16, 128, 128, 9, 2, -1, -1, 2, 0, 48, 4, 256): (5, 'T16x4_128_64_T512', 5, 96, 2, 512, 0, 96, 0, 1, 1, 1),
    (24, 8, 8, 128, 128, 9, 2, -1, -1, 2, 0, 12, 4, 256): (5, 'TS8_128_64_T512', 5, 12, 2, 512, 0, 12, 0, 0, 1, 1),
    (24, 64, 64, 128, 256, 1, 2, 0, -1, 2, 0, 0, 0, 256): (3, 'R128_64_128', 2, 1536, 1, 256, 2, 1536, 0, 0, 0, 0),
    (24, 64, 64, 128, 256, 1, 2, 0, -1, 0, 2, 0, 2, 256): (4, 'R128_64_128_UP', 2, 1536, 1, 256, 2, 1536, 1536, 0, 0, 0),
    (24, 64, 64, 128, 256, 1, 2, 0, 3, 2, 0, 0, 64, 256): (3, 'R128_64_128', 6, 1536, 1, 256, 2, 1536, 0, 0, 0, 0),
    (24, 16, 16, 128, 256, 1, 2, 0, 3, 2, 0, 0, 64, 256): (2, 'OS2', 6, 96, 4, 256, 0, 96, 0, 0, 0, 1),
    (24, 128, 128, 128, 64, 1, 3, -1, -1, 2, 0, 0, 60, 256): (3, 'R128_64_64_PIN', 2, 6144, 1, 256, 1, 6144, 0, 0, 1, 0),
    (24, 128, 128, 64, 64, 1, 1, -1, -1, 1, 0, 0, 1, 256): (3, 'R64_128_64', 1, 3072, 1, 256, 1, 3072, 0, 0, 0, 0),
    (24, 128, 128, 64, 128, 1, 1, -1, -1, 1, 0, 0, 1, 256): (3, 'R64_64_128', 1, 6144, 1, 256, 1, 6144, 0, 0, 0, 0),
    (24, 128, 128, 64, 64, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'T16x8_64_64', 1, 3072, 1, 256, 0, 3072, 0, 1, 0, 1),
    (16, 6, 6, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 256): (5, 'TS8_128_64_T512', 1, 8, 2, 512, 0, 8, 0, 0, 0, 1),
    (2, 16, 16, 512, 256, 1, 0, -1, -1, 0, 0, 0, 1, 256): (1, 'G64x64_1', 0, 8, 4, 256, 0, 8, 0, 0, 0, 0),
    (2, 16, 16, 256, 512, 1, 0, -1, -1, 0, 0, 0, 1, 256): (2, 'OS4', 0, 8, 8, 256, 0, 8, 0, 0, 0, 0),
    (4, 64, 64, 512, 256, 1, 0, -1, -1, 0, 0, 0, 1, 256): (1, 'G64x128_1', 0, 256, 2, 256, 0, 256, 0, 0, 0, 0),
    (8, 64, 64, 512, 256, 1, 0, -1, -1, 0, 0, 0, 1, 256): (1, 'G128x128_1', 0, 256, 2, 256, 0, 256, 0, 0, 0, 0),
    (8, 64, 64, 256, 512, 1, 0, -1, -1, 0, 0, 0, 1, 256): (3, 'R256_64_128_K32', 0, 512, 1, 256, 4, 512, 0, 0, 0, 0),
    (8, 64, 64, 256, 512, 1, 0, -1, -1, 0, 0, 0, 0, 256): (3, 'R256_64_128_K32', 0, 512, 1, 256, 4, 512, 0, 0, 0, 0),
    (8, 64, 64, 256, 256, 9, 0, -1, -1, 0, 0, 0, 1, 256): (1, 'G128x128_9', 0, 256, 2, 256, 0, 256, 0, 0, 0, 0),
    (2, 16, 16, 256, 256, 9, 0, -1, -1, 0, 0, 0, 1, 256): (1, 'G64x64_9', 0, 8, 4, 256, 0, 8, 0, 0, 0, 0),
    (24, 16, 16, 128, 128, 9, 1, -1, -1, 1, 0, 0, 1, 0): (5, 'T16x4_128_64', 1, 96, 2, 256, 0, 96, 0, 1, 0, 1),
    (24, 16, 16, 128, 128, 9, 1, -1, -1, 1, 0, 96, 1, 0): (5, 'T16x4_128_64', 4, 96, 2, 256, 0, 96, 0, 1, 0, 1),
    (24, 16, 16, 128, 128, 9, 2, -1, -1, 2, 0, 48, 4, 0): (5, 'T16x4_128_64', 5, 96, 2, 256, 0, 96, 0, 1, 1, 1),
    (2, 16, 16, 256, 256, 9, 0, -1, -1, 0, 0, 0, 1, 0): (1, 'G64x64_9', 0, 8, 4, 256, 0, 8, 0, 0, 0, 0),
}


def test_pinned_plans_of_the_benchmark_and_the_chan512_tiers(L):
    assert len(TILINGS) == 32
    for key, want in PINNED.items():
        d = describe(L, *key)
        got = (d['path'], d['tiling'], d['variant'], d['gx'], d['gy'], d['threads'], d['nbw'], d['rows'], d['rows2'], d['xcd'], d['stores_dz'],
               d['takes_fin'])
        assert got == want, (key, got, want)


def test_documented_examples(L):
    """DESIGN.md section 4 in words: batch 24, chan 256"""
    fwd3 = lambda H, cus=256: describe(L, 24, H, H, 128, 128, 9, BNRELU, ep=OUT_STATS, flags=BIAS, cus=cus)
    d = fwd3(64)
    assert (d['tiling'], d['gx'], d['gy'], d['xcd'] & 1, d['takes_fin']) == ('T16x8_128_128', 768, 1, 1, 0)
    d = fwd3(32)
    assert (d['tiling'], d['gx'], d['gy'], d['threads']) == ('T16x4_128_64', 384, 2, 256)
    assert (fwd3(16)['gx'], fwd3(16)['gy'], fwd3(16)['threads'], fwd3(16, cus=0)['threads']) == (96, 2, 512, 256)
    assert (fwd3(8)['tiling'], fwd3(8)['gx'], fwd3(8)['gy']) == ('TS8_128_64_T512', 12, 2)
    assert (fwd3(4)['tiling'], fwd3(4)['gx'], fwd3(4)['gy']) == ('TS4_128_64_T512', 3, 2)
    d = describe(L, 24, 64, 64, 256, 128, 1, BNRELU, ep=OUT_STATS, flags=BIAS)
    assert (d['tiling'], d['gx'], d['gy']) == ('R256_64_128_K32', 1536, 1)
    d = describe(L, 24, 64, 64, 128, 256, 1, BNRELU, ep=OUT_STATS, flags=BIAS)
    assert (d['path'], d['nbw'], d['gx'], d['gy']) == (ROW, 2, 1536, 1)
    d = describe(L, 24, 16, 16, 128, 256, 1, BNRELU, ep=OUT_STATS, flags=BIAS, fin=96)
    assert (d['path'], d['tiling'], d['variant'], d['gx'], d['gy'], d['takes_fin']) == (ONESHOT, 'OS2', 4, 96, 4, 1)
    assert describe(L, 24, 16, 16, 128, 256, 1, BNRELU, ep=OUT_STATS, flags=BIAS, fin=129)['path'] == REFUSED      # <= 128 rows


def test_documented_examples_of_the_other_resolutions(L):
    """The rules of csrc/conv_plan.h in words, on the maps of the 320 / 448 / 192 / 64 inputs (res / 4 ... res / 64): a 3 x 3 launch with 64 or 128
    input channels takes 8 x 8 halo tiles where both sides are multiples of 8 that the 16 x 8 tiles do not take (W % 16 != 0), 4 x 4 tiles where they
    are multiples of 4, ONE masked 8 x 8 tile for any other map up to 8 x 8, and no halo tile at all for any other map -- a side above 8 that is no
    multiple of 4 -- which leaves the generic kernel (its 64 x 64 tier below 128 * 256 pixels).  A workgroup holds 128 / side^2 sub-tiles: two
    images of a masked tile.  The row-tile instance with a second output needs W % 32 == 0; the launch without it is a plain row-tile launch from
    192 row tiles of 64 pixels on."""
    up = lambda a, b: -(-a // b)
    for cin in (128, 64):
        for B in (1, 2, 3, 5):
            for in_, ep, flags in ((BNRELU, OUT_STATS, BIAS), (LIN2, OUT_BWD, DZ)):          # the net's forward and data-gradient launches
                f = lambda H: describe(L, B, H, H, cin, cin, 9, in_, ep=ep, flags=flags)
                for H in (10, 14):
                    d = f(H)
                    assert (d['path'], d['tiling'], d['gx'], d['gy'], d['threads']) == (GENERIC, 'G64x64_9', up(B * H * H, 64), cin // 64, 256), (cin, B, H, d)
                    assert d['takes_fin'] and not d['stores_dz'], (cin, B, H, d)           # the 64 x 64 tier carries the finalize prologue; only tile kernels store dz
                for H in (1, 3, 5, 7):
                    d = f(H)
                    assert (d['path'], d['tiling'].split('_')[0], d['gx'], d['gy'], d['rows']) == (TILE3, 'TS8', up(B, 2), cin // 64, up(B, 2)), (cin, B, H, d)
                d = f(40)
                assert (d['path'], d['tiling'].split('_')[0], d['gx']) == (TILE3, 'TS8', up(B * 25, 2)), (cin, B, d)
                d = f(20)
                assert (d['path'], d['tiling'].split('_')[0], d['gx']) == (TILE3, 'TS4', up(B * 25, 8)), (cin, B, d)
                # (the 512-thread instances are the small tiles with 128 input channels)
                assert {f(H)['threads'] for H in (1, 3, 5, 7, 20, 40)} == {512 if cin == 128 else 256}, (cin, B)
    # the low-resolution half of the upsample-add backward in the 1 x 1 data gradient's second output: the 384 leg's launch (B 3, 96 x 96), and the
    # same launch on 80 x 80 (3 * 80 * 80 / 64 = 300 row tiles, W % 32 = 16)
    fused = lambda H, flags: describe(L, 3, H, H, 128, 256, 1, LIN2, PLAIN, ep=OUT_PLAIN, ep2=OUT_BWD if flags & OUT2 else OUT_PLAIN, flags=flags)
    assert fused(96, OUT2)['path'] == ROW_UP
    assert fused(80, OUT2)['path'] == REFUSED
    d = fused(80, 0)
    assert (d['path'], d['tiling'], d['gx'], d['rows2']) == (ROW, 'R128_64_128', 300, 0), d


# map sides of the 320 / 448 / 192 / 64 inputs that no power-of-two or 384 input has (the legs 'on the ... geometry' of tests/test_gpu_conv_exact.py)
OTHER_RES_MAPS = ((1, 1), (3, 3), (5, 5), (7, 7), (10, 10), (14, 14), (20, 20), (40, 40), (80, 80))


def max_stat_rows(M):
    return max(512, (M + 63) // 64)


def _grid():
    for B in (3, 24):
        for H, W in ((4, 4), (16, 16), (64, 64), (6, 6), (16, 32)) + OTHER_RES_MAPS:
            for Cin in (64, 128, 256, 512):
                for Cout in (64, 128, 256, 512):
                    for taps in (1, 9):
                        yield B, H, W, Cin, Cout, taps


FLAGSETS = (0, BIAS, OUT2, DZ, IN_MAP | IN_Q | EP2_AFFINE | ADD2_MAP | DZ, IN_MAP | IN_Q | EP2_AFFINE | ADD2_MAP, OUT2 | DZ)


def test_invariants_over_shapes_and_every_mode_combination(L):
    n = admitted = 0
    lds_modes = set()
    for shape in _grid():
        B, H, W, Cin, Cout, taps = shape
        M = B * H * W
        for in_ in (PLAIN, BNRELU, LIN2, POOL):
            for a1 in (NONE, PLAIN, BNRELU, LIN2, POOL):
                for a2 in (NONE, PLAIN, BNRELU, LIN2, POOL):
                    for ep in (OUT_PLAIN, OUT_STATS, OUT_BWD):
                        n += 1
                        flags = FLAGSETS[n % len(FLAGSETS)]
                        fin = (0, 0, 64, 200)[(n // 7) % 4]
                        cus = 256 if n % 3 else 0
                        d = describe(L, B, H, W, Cin, Cout, taps, in_, a1, a2, ep, OUT_BWD if flags & OUT2 else OUT_PLAIN, fin, flags, cus)
                        case = (shape, in_, a1, a2, ep, fin, flags, cus, d)
                        if d['path'] == REFUSED:                  # every refusal carries a message of its own (behind another call's message)
                            assert L.pa_copy_probe(None, None, 0, None) != 0 and L.pa_last_error().startswith(b'pa_copy_probe'), case
                            assert describe(L, *case[0], in_, a1, a2, ep, OUT_BWD if flags & OUT2 else OUT_PLAIN, fin, flags, cus)['path'] == REFUSED
                            assert L.pa_last_error().startswith(b'pa_launch_conv'), (case, L.pa_last_error())
                            assert not (d['takes_fin'] or d['stores_dz'] or d['pool_route'] or d['pool_in']), case
                            continue
                        admitted += 1
                        # ONE rule for the LDS form of the BatchNorm-backward epilogue: the planner's and the kernels' own copy agree
                        assert d['bwd_lds'] == d['kernel_lds'] == int(not flags & BIAS and a1 in (NONE, PLAIN, LIN2) and a2 in (NONE, PLAIN)), case
                        lds_modes.add((bool(flags & BIAS), a1, a2))
                        assert 1 <= d['rows'] <= max_stat_rows(M) and d['rows'] == d['gx'], case
                        assert d['gx'] >= 1 and d['gy'] >= 1 and d['threads'] in (256, 512), case
                        if d['path'] == ROW_UP:                  # the low tensor's BatchNorm is laid out with four times its own rows
                            assert d['rows2'] == d['rows'] <= max_stat_rows(4 * (M // 4)), case
                        else:
                            assert d['rows2'] == 0, case
                        if d['takes_fin']:
                            assert Cin <= 256 and in_ in (BNRELU, LIN2), case
                        if fin and d['path'] != TILE3:           # (the halo-tile launcher takes the caller's word: Net asks takes_fin first)
                            assert d['takes_fin'] and fin <= 128 and d['variant'] in (4, 5), case
                        # the host-side guarantee that the kernels' trap is unreachable: an instance without the direct BatchNorm-backward
                        # epilogue gets launches the LDS form takes only
                        if ep == OUT_BWD and not d['cannot_trap']:
                            assert d['bwd_lds'], case
                        if d['stores_dz']:
                            assert flags & DZ and in_ in (LIN2, POOL) and d['path'] in (ROW, TILE3), case
                        if d['pool_route'] or d['pool_in']:
                            assert taps == 1 and Cin == 128 and d['path'] in (ROW, ONESHOT), case
    assert 250000 <= n <= 300000 and admitted > n // 10, (n, admitted)
    # ... on every combination a launch can have (a pool-routed first addend is always refused)
    assert lds_modes >= {(b, a1, a2) for b in (False, True) for a1 in (NONE, PLAIN, BNRELU, LIN2) for a2 in (NONE, PLAIN, BNRELU, LIN2)}


def _name(inst):
    return '%s.%d' % (TILINGS[inst // VARIANTS], inst % VARIANTS)


def _reachable(L):
    """every instance id the planner returns at release values over batch, map, channels, taps, load / epilogue modes, the operand sets of
    the networks' launches (and those that force the direct BatchNorm-backward epilogue), with and without a known CU count"""
    operands = ((NONE, NONE, 0, 0), (PLAIN, NONE, 0, 0), (NONE, NONE, BIAS, 0), (BNRELU, NONE, 0, 0), (PLAIN, LIN2, 0, 0), (LIN2, PLAIN, 0, 0),
                (PLAIN, POOL, ADD2_MAP, 0), (PLAIN, NONE, OUT2, 0), (NONE, NONE, DZ, 0), (NONE, NONE, DZ | IN_MAP | IN_Q | EP2_AFFINE, 0), (NONE, NONE, 0, 64))
    reach = set()
    for B in (1, 4, 8, 16, 24):
        for H, W in ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (6, 6), (16, 32)) + OTHER_RES_MAPS:
            for Cin in (64, 128, 256, 512):
                for Cout in (64, 128, 256, 512):
                    for taps in (1, 9):
                        for in_ in (PLAIN, BNRELU, LIN2, POOL):
                            for ep in (OUT_PLAIN, OUT_STATS, OUT_BWD):
                                for a1, a2, flags, fin in operands:
                                    for cus in (256, 0):
                                        d = describe(L, B, H, W, Cin, Cout, taps, in_, a1, a2, ep, OUT_BWD if flags & OUT2 else OUT_PLAIN, fin, flags, cus)
                                        if d['path'] != REFUSED:
                                            reach.add(d['inst'])
    return reach


# Reachable, but run by no numerical GPU test -- each with its reason.  The test below asserts that this is EXACTLY the remainder.
NOT_COVERED = {
    # The fallbacks that keep a launch away from an instance without the direct BatchNorm-backward epilogue (the trap of pa_conv_epilogue_auto):
    # only a BatchNorm-backward epilogue the LDS form does not take (a bias, a BatchNorm + ReLU addend, a LIN2 second addend) selects them.  No
    # network makes such a launch and the operator-level entry pa_conv2d has plain operands and a plain epilogue, so nothing in the C ABI can
    # run them; they were as unreachable for a test before the planner.  Their tilings' kernel template runs in the K32 / 64-row instances.
    'a BatchNorm-backward epilogue that needs the direct form: no network launch, no operator-level entry':
        {'R256_64_128.0', 'R256_64_128.1', 'R256_64_128.2', 'R64_128_128.0', 'R64_128_128.1', 'R64_128_128.2', 'R128_128_128.2', 'R128_128_64.2'},
    # A tiling the networks of the suite reach with other load modes only (its shape class has no layer with this mode: 64-channel outputs
    # above 32768 pixels or on 256-channel row tiles, the 16 x 8 halo tiles with unequal channel counts, ...), or whose BatchNorm-on-load launches
    # always bring their finalize (the 512-thread halo tiles and the 64-channel small tiles' data gradients: variants 4 / 5 run instead) or never
    # do (the 256-thread 16 x 4 tiles, the generic small tier with 64 / 512 input channels: variants 1 / 2 run instead).  The plain variant of each
    # runs in tests/test_gpu_conv.py::SHAPES and the load transform in the covered instances of the same kernel template.  (The generic small
    # tier's 3 x 3 instances with a BatchNorm on load and no finalize, G64x64_9.1 / .2, and the 128 -> 64 row tile with BatchNorm + ReLU on load,
    # R128_64_64.1, left this list with the 320 / 448 legs: 80 x 80 maps at chan 512 have 200 statistics rows, too many for the prologue, and
    # chan 128 has a 128 -> 64 layer on >= 192 row tiles there.)
    'a load mode no layer of the networks of the suite has on this tiling (the plain variant and the finalize variants run)':
        {'G128x64_1.1', 'G128x64_1.2', 'G128x64_9.1', 'G128x64_9.2', 'G64x64_1.5', 'R256_64_64.1',
         'R256_64_64.2', 'T16x4_128_64.4', 'T16x4_128_64.5', 'T16x4_128_64_T512.1', 'T16x4_128_64_T512.2', 'T16x8_128_64.1', 'T16x8_128_64.2',
         'T16x8_64_128.1', 'T16x8_64_128.2', 'TS4_128_64_T512.1', 'TS4_128_64_T512.2', 'TS4_64_64.2', 'TS8_128_64_T512.1', 'TS8_128_64_T512.2',
         'TS8_64_64.2'},
}


def test_every_reachable_instance_is_run_by_a_numerical_gpu_test_or_listed_with_its_reason(L):
    """Every instance id (tiling * 8 + variant) the planner can return at release values is run by tests/test_gpu_conv.py::SHAPES (forward and
    data gradient of pa_conv2d: plain operands, the forward with a bias) or by a conv-exact / pool-route leg, whose launches -- shape and modes
    as the engine's launch log recorded them, tests/golden/conv_launches.json, which every such leg checks against the launches it makes --
    are fed through the planner here; what is left is exactly NOT_COVERED."""
    from tests.test_gpu_conv import SHAPES
    covered = set()
    for B, Cin, Cout, H, W, k in SHAPES:
        covered |= {describe(L, B, H, W, Cin, Cout, k * k, flags=BIAS)['inst'], describe(L, B, H, W, Cout, Cin, k * k)['inst']}
    legs = Q.recorded_launches()
    assert len(legs) >= 40
    for leg, launches in legs.items():
        for launch in launches:
            d = describe(L, *launch)
            assert d['path'] != REFUSED, (leg, launch)
            covered.add(d['inst'])
    reach = _reachable(L)
    assert covered <= reach, sorted(map(_name, covered - reach))
    listed = set().union(*NOT_COVERED.values())
    assert sum(len(v) for v in NOT_COVERED.values()) == len(listed)
    assert {_name(i) for i in reach - covered} == listed, (sorted({_name(i) for i in reach - covered} - listed), sorted(listed - {_name(i) for i in reach - covered}))
    assert len(reach) >= 110 and len(covered) >= 80

"""The conditions tests/test_gpu_metrics_exact.py relies on, checked without a GPU on the inputs of tests/metrics_cases.py: the
realistic maps give metrics strictly between 0 and 1, every adversarial case has the answer its construction says and the oracle
returns it, and the refinement cases take every branch.  A later change of seeds or sizes that hollowed the GPU test out fails
here.  These are conditions, not measurements: the oracle meets them with room to spare (10 .. 13 of 16 per-joint heat-map
accuracies and 11 .. 14 of 14 PCKh entries are fractional at the five sizes)."""
import math

import numpy as np
import pytest

from oracle import pylib as opl
from tests import metrics_cases as mc


def _fractional(acc):
    a = acc.numpy()[1:]
    return int(((a > 0) & (a < 1)).sum())


@pytest.mark.parametrize('variant', [0, 1])
@pytest.mark.parametrize('H', mc.REALISTIC_SIZES)
def test_realistic_maps_score_strictly_between_0_and_1(H, variant):
    maps, tgt, _ = mc.realistic(H, variant=variant)
    (c, s, res, r), (gpts, norm) = mc.meta_tensors(H, H, 16, None if variant == 0 else 500 + H + 1000 * variant)
    acc = opl.accuracy(mc.t(maps), mc.t(tgt), list(range(16)))
    assert _fractional(acc) >= 5, acc
    assert float(acc[0]) > 0.5, acc                     # what the in-net GPU test asserts of the engine's value
    pckh = opl.accuracy_origin_res(mc.t(maps), c, s, res, gpts, norm, r)
    assert _fractional(pckh) >= 5, pckh
    person = opl.per_person_pckh(mc.t(maps), mc.t(tgt), c, s, res, gpts, norm, r).numpy()
    assert person.min() < person.max(), person
    peaks = opl.get_preds(mc.t(maps)).numpy().reshape(-1, 2)
    assert len(peaks) == 80 and len({(x, y) for x, y in peaks}) >= 60
    if variant:                                         # a second forward's maps: a stale cached arg-max must show
        first = opl.get_preds(mc.t(mc.realistic(H)[0])).numpy().reshape(-1, 2)
        assert (first != peaks).any(1).sum() >= 60
        assert not np.array_equal(opl.accuracy(mc.t(mc.realistic(H)[0]), mc.t(tgt), list(range(16))).numpy(), acc.numpy())


def test_one_heatmap_pixel_is_several_image_pixels():
    """a quarter-pixel refinement step (0.25 * 200 s / W image pixels) is more than one image pixel for every person"""
    for H, W in mc.NHWC_SIZES + mc.NCHW_SIZES:
        s = mc.people(H, W, 16)[1]
        assert (0.25 * 200 * s / W > 1).all(), (H, W, s)


def _sizes():
    """(H, W, J, split) of every GPU run: joint-minor maps of 16 joints for their own kernel, and -- like those of 1, 3 and 17
    joints -- for the generic kernel they fall back to; joint-major maps"""
    return [(H, W, 16, mc.NHWC_SPLIT) for H, W in mc.NHWC_SIZES] + \
           [(H, W, J, mc.NCHW_SPLIT) for H, W in mc.NHWC_SIZES for J in (16, 1, 3, 17)] + \
           [(H, W, J, mc.NCHW_SPLIT) for H, W in mc.NCHW_SIZES for J in (1, 17) if (H, W) not in mc.NHWC_SIZES] + \
           [(H, W, 16, mc.NCHW_SPLIT) for H, W in mc.NCHW_SIZES if (H, W) not in mc.NHWC_SIZES]


def test_adversarial_cases_have_the_answer_written_by_hand():
    """the expected pixel of a tie case is the FIRST entry of its list by construction; it must be the lowest one (or -1 for
    (0, 0)), and the oracle's get_preds / torch.max must return exactly it and the map's own maximum 1 + m / 128"""
    for H, W, J, split in _sizes():
        T, U = split
        M = mc.B * J
        cases = mc.adversarial(H, W, J, split)
        assert set(mc.DEGENERATE_CASES) <= set(cases)
        for name, (maps, want) in cases.items():
            if name in mc.TIE_CASES:
                for m in range(M):
                    px = mc._tie_pixels(name, T, U, H * W, m, M)
                    assert px[0] == min(px) == want.reshape(-1)[m]
                    flat = maps.reshape(M, -1)[m]
                    assert (flat[px] == np.float32(1 + m / 128)).all() and (np.delete(flat, px) < 0).all()
            got = opl.get_preds(mc.t(maps)).numpy()
            assert np.array_equal(got, mc.expected_preds(want, H, W)), (H, W, J, name)
    # by hand, on the workload's map: p = 900 is (x, y) = (5, 15) and wins over p = 1030
    maps, want = mc.adversarial(64, 64, 16, mc.NHWC_SPLIT)['earlier_in_higher_thread']
    assert want[-1, -1] == 900 and maps[-1, -1].reshape(-1)[1030] == maps[-1, -1].reshape(-1)[900] == maps[-1, -1].max()
    assert opl.get_preds(mc.t(maps)).numpy()[-1, -1].tolist() == [900 % 64 + 1, 900 // 64 + 1] == [5.0, 15.0]
    for name, xy in (('plateau', [1, 1]), ('plateau_but_first_pixel', [2, 1]), ('all_zero', [0, 0]), ('all_negative', [0, 0]),
                     ('all_neg_inf', [0, 0]), ('first_pixel', [1, 1]), ('last_pixel', [64, 64])):
        assert (opl.get_preds(mc.t(mc.adversarial(64, 64, 16, mc.NHWC_SPLIT)[name][0])).numpy() == np.float32(xy)).all(), name


def test_adversarial_cases_aim_at_the_kernels_structure():
    """thread, slot, trip, lane and wave of the planted maxima are what each case's name says, for both kernels' splits"""
    def owner(p, T, U):
        return p % T, (p // T) % U, p // (T * U)            # thread, slot u, trip k

    for H, W, J, split in _sizes():
        T, U = split
        M = mc.B * J
        for name in mc.adversarial(H, W, J, split):
            if name not in mc.TIE_CASES or name in ('first_pixel', 'last_pixel', 'tail_of_a_partial_u'):
                continue
            for m in range(M):
                a, b = (owner(p, T, U) for p in mc._tie_pixels(name, T, U, H * W, m, M))
                if name == 'one_thread_two_u':
                    assert a[0] == b[0] and a[2] == b[2] == 0 and a[1] < b[1]
                elif name == 'one_thread_two_trips':
                    assert a[0] == b[0] and a[2] == 0 and b[2] == 1
                elif name == 'one_wave_earlier_in_lower_lane':
                    assert a[0] // 64 == b[0] // 64 and a[0] < b[0]
                elif name == 'one_wave_earlier_in_higher_lane':
                    assert a[0] // 64 == b[0] // 64 and a[0] > b[0]
                elif name == 'two_waves_earlier_in_lower_wave':
                    assert a[0] // 64 < b[0] // 64
                elif name == 'two_waves_earlier_in_higher_wave':
                    assert a[0] // 64 > b[0] // 64
                else:
                    assert name == 'earlier_in_higher_thread' and a[0] > b[0]
    # every case is held by some size of each kernel's list, and the listed sizes are the ones that split differently
    for sizes, split in ((mc.NHWC_SIZES, mc.NHWC_SPLIT), (mc.NCHW_SIZES, mc.NCHW_SPLIT)):
        T, U = split
        held = set()
        for H, W in sizes:
            held |= set(mc.adversarial(H, W, 16, split))
        assert held == set(mc.TIE_CASES + mc.DEGENERATE_CASES)
        hw = [H * W for H, W in sizes]
        assert min(hw) < T                                                  # fewer pixels than threads
        assert any(n > T * U and n % (T * U) for n in hw)                   # more than one trip, the last one ragged
        assert any(H != W for H, W in sizes)
    assert 64 * 64 == 4 * 1024 and 80 * 80 > 4096 and math.ceil(96 * 96 / 4096) == 3


def test_refinement_cases_take_every_branch():
    for H, W in sorted(set(mc.NHWC_SIZES + mc.NCHW_SIZES)):
        seen = set()
        for start in (0, 80):
            combos = [mc.refine_combo(H, W, 16, start, m) for m in range(80)]
            assert len(set(combos)) == 80
            assert {(sx, sy) for _, _, sx, sy in combos} == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
            for guard in (lambda px, py: px > 1, lambda px, py: px < W, lambda px, py: py > 1, lambda px, py: py < H):
                assert {guard(c[0], c[1]) for c in combos} == {True, False}
            seen |= set(combos)
            # the oracle sees the peak where it was put and the two differences with the signs asked for
            maps = mc.refinement(H, W, 16, start)
            got = opl.get_preds(mc.t(maps)).numpy().reshape(80, 2)
            for m, (px, py, sx, sy) in enumerate(combos):
                hm = maps.reshape(80, H, W)[m]
                qx, qy = px, (py - 1) * W + px - 1                              # the reference's y is floor(p / H) + 1
                assert got[m].tolist() == [qx, qy // H + 1]
                if 1 < px < W and 1 < py < H:
                    assert np.sign(hm[py - 1][px] - hm[py - 1][px - 2]) == sx and np.sign(hm[py][px - 1] - hm[py - 2][px - 1]) == sy
        assert len(seen) == mc.REFINE_COMBOS
    # the refinement is visible after the back-projection: final_preds differs from the unrefined back-projection for most
    # interior peaks with a nonzero sign
    H = W = 64
    maps = mc.refinement(H, W, 16, 0)
    (c, s, res, r), _ = mc.meta_tensors(H, W, 16)
    refined = opl.final_preds(mc.t(maps), c, s, res, r).numpy()
    flat = maps.copy().reshape(80, H, W)
    for m in range(80):
        px, py, sx, sy = mc.refine_combo(H, W, 16, 0, m)
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= px - 1 + dx < W and 0 <= py - 1 + dy < H:
                flat[m, py - 1 + dy, px - 1 + dx] = 0.5
    plain = opl.final_preds(mc.t(flat.reshape(maps.shape)), c, s, res, r).numpy()
    moved = (refined != plain).any(-1).reshape(-1)
    for m in range(80):
        px, py, sx, sy = mc.refine_combo(H, W, 16, 0, m)
        inside = 1 < px < W and 1 < py < H
        assert moved[m] == bool(inside and (sx or sy)), (m, px, py, sx, sy)

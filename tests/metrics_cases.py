"""Inputs of the exact metric tests (tests/test_metrics_cases_cpu.py, tests/test_gpu_metrics_exact.py): heat maps whose arg-max,
quarter-pixel refinement and PCK are known, with the expected values taken from oracle.pylib.  Plain numpy / torch, no GPU.

Three sets, each for any (H, W, J) at B = 5 (a test of B = 1 takes the first sample):
  realistic    Gaussian targets of inputs.person_meta people + noise 0.35: peaks near but not on the target, so PCK and PCKh
               take values strictly between 0 and 1 (at noise 0.2 the heat-map accuracy is 1.0 at every size and says nothing);
  adversarial  ties between equal maxima, placed by pixel index p = y * W + x against the way a kernel splits a map over its
               threads -- thread t of a workgroup of T threads with U loads in flight owns p = t + T u + T U k (the joint-minor
               kernel: T = 1024, U = 4; the one-map-per-workgroup kernel: T = 256, U = 8; a wave is 64 threads) -- and the
               degenerate maps (plateaus, all zero / negative / -inf).  torch.max returns the first maximum: the lowest p;
  refinement   single peaks on and next to the border with both neighbour differences set to +, - or 0.
Every (sample, joint) map of a case has its own location and its own maximum value (1 + m / 128 for map m = b J + j), so a
kernel that mixes up joints or samples changes `preds` and `maxval`."""
import functools

import numpy as np
import torch

from oracle import pylib as opl
from tests import inputs

B = 5
NHWC_SPLIT = (1024, 4)          # argmax_nhwc16_kernel: threads per workgroup, loads in flight per thread
NCHW_SPLIT = (256, 8)           # argmax_kernel
NHWC_SIZES = ((16, 16), (32, 32), (48, 48), (64, 64), (80, 80), (96, 96), (48, 64), (64, 48))
NCHW_SIZES = ((5, 7), (8, 8), (16, 16), (48, 64), (64, 48), (96, 96))
REALISTIC_SIZES = (32, 48, 64, 80, 96)      # heat-map sizes of the nets pa_hg_create admits (res = 128 .. 384)


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def nhwc(maps):
    """[B][J][H][W] -> the engine's joint-minor layout [B][H*W][J]"""
    b, j, h, w = maps.shape
    return np.ascontiguousarray(maps.transpose(0, 2, 3, 1).reshape(b, h * w, j))


# ------------------------------------------------------------------------------------------------ people
@functools.lru_cache(maxsize=None)
def people(H, W, J, seed=None):
    """(center [B][2], scale [B], rot [B], image joints [B][J][2], normaliser [B]) as float32 arrays -- what the reference's
    batches carry -- and the joints in heat-map coordinates (float64; the transform's `res` is the map WIDTH, res[0] of
    Evaluation.final_preds).  One heat-map pixel is 200 s / W = 4 .. 14 image pixels at W = 64, so a quarter-pixel step of the
    refinement moves the back-projected integer."""
    c, s, r, gpts, norm = inputs.person_meta(500 + H if seed is None else seed, B, joints=J)
    c, s, r, gpts, norm = (a.astype(np.float32) for a in (c, s, r, gpts, norm))
    tp = np.stack([opl.transform_pts(gpts[i].astype(np.float64), c[i].astype(np.float64), s[i], r[i], W) for i in range(B)])
    tp[gpts[..., 0] <= 0] = 0
    return c, s, r, gpts, norm, tp


def meta_tensors(H, W, J, seed=None):
    """the arguments of oracle.pylib.final_preds / accuracy_origin_res / per_person_pckh: (center, scale [B][1], res, rot [B][1])
    and (grnd_pts, normalizers)"""
    c, s, r, gpts, norm, _ = people(H, W, J, seed)
    return (t(c), t(s).view(B, 1), [W, H], t(r).view(B, 1)), (t(gpts), t(norm))


def targets(tp, H, W):
    out = np.zeros((tp.shape[0], tp.shape[1], H, W), dtype=np.float32)
    for i in range(tp.shape[0]):
        out[i] = opl.pts2heatmap(tp[i], [H, W], sigma=1)[0].astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ realistic maps
@functools.lru_cache(maxsize=None)
def realistic(H, W=None, J=16, variant=0):
    """(maps [B][J][H][W], target maps, joints in heat-map coordinates).  variant != 0: other people and other noise (the maps a
    second forward pass is given)."""
    W = W or H
    seed = None if variant == 0 else 500 + H + 1000 * variant
    tp = people(H, W, J, seed)[5]
    tgt = targets(tp, H, W)
    maps = inputs.noisy_heatmaps(501 + H + 1000 * variant, tgt, noise=0.35)
    return maps, tgt, tp


# ------------------------------------------------------------------------------------------------ adversarial maps
def _background(HW):
    """small distinct negative values: no tie outside the planted maxima, and nothing but them is positive"""
    return -(np.arange(HW, dtype=np.float32) + 1) / np.float32(16384)


def _pix(T, U, t_, u, k):
    return t_ + T * u + T * U * k


def _tie_pixels(name, T, U, HW, m, M):
    """pixel indices of the equal maxima of map m (of M) in case `name`, the expected one FIRST; None or a pixel outside the map:
    the map is too small for the case"""
    nw = max(1, min(T, HW) // 64)               # waves that hold a pixel at u = 0
    if name == 'one_thread_two_u':              # thread m: slot u = 0 and the last slot the map fills in the first trip
        u1 = min(U - 1, (HW - 1 - m) // T)
        return [_pix(T, U, m, 0, 0), _pix(T, U, m, u1, 0)] if u1 >= 1 else None
    if name == 'one_thread_two_trips':          # thread m: its last slot of trip 0 and its first of trip 1
        return [_pix(T, U, m, U - 1, 0), _pix(T, U, m, 0, 1)]
    if name == 'one_wave_earlier_in_lower_lane':
        w, i = m % nw, (m // nw) % 32
        return [64 * w + i, 64 * w + 63 - i]
    if name == 'one_wave_earlier_in_higher_lane':       # the higher lane's pixel at u = 0, the lower lane's at u = 1
        w, i = m % nw, (m // nw) % 32
        return [64 * w + 63 - i, _pix(T, U, 64 * w + i, 1, 0)]
    if name == 'two_waves_earlier_in_lower_wave':       # both at u = 0
        if nw < 2:
            return None
        w, i = m % (nw - 1), (m // (nw - 1)) % 32
        return [64 * w + i, 64 * (w + 1 + i % (nw - 1 - w)) + 63 - i]
    if name == 'two_waves_earlier_in_higher_wave':      # one of the two last waves at u = 0 against a lower wave at u = 1
        if nw < 3 or m >= 128:
            return None
        return [64 * (nw - 1 - m // 64) + m % 64, _pix(T, U, 64 * (m % (nw - 2)) + (m // 2) % 64, 1, 0)]
    if name == 'earlier_in_higher_thread':      # T = 1024, last map: p = 900 (thread 900) against p = 1030 (thread 6 at u = 1)
        return [T - 124 + (M - 1 - m), T + 6 + (M - 1 - m)]
    if name == 'first_pixel':                   # p = 0 and a later equal maximum of the map's own
        return [0, 1 + (7 * m) % (HW - 1)]
    if name == 'last_pixel':
        return [HW - 1]
    if name == 'tail_of_a_partial_u':           # the last slot is partly filled: a maximum of the map's own inside that tail
        tail = HW % T
        return [HW - 1 - m % min(tail, M)] if tail else None
    raise KeyError(name)


TIE_CASES = ('one_thread_two_u', 'one_thread_two_trips', 'one_wave_earlier_in_lower_lane', 'one_wave_earlier_in_higher_lane',
             'two_waves_earlier_in_lower_wave', 'two_waves_earlier_in_higher_wave', 'earlier_in_higher_thread', 'first_pixel',
             'last_pixel', 'tail_of_a_partial_u')
DEGENERATE_CASES = ('plateau', 'plateau_but_first_pixel', 'all_zero', 'all_negative', 'all_neg_inf')


@functools.lru_cache(maxsize=4)
def adversarial(H, W, J, split):
    """dict case name -> (maps [B][J][H][W], expected pixel index [B][J], -1 where the expected prediction is (0, 0)).  The tie
    cases are laid out for the kernel with the given (T, U); a case a map of this size cannot hold is left out (which sizes
    hold which case: tests/test_metrics_cases_cpu.py)."""
    T, U = split
    HW, M = H * W, B * J
    out = {}
    for name in TIE_CASES:
        px = [_tie_pixels(name, T, U, HW, m, M) for m in range(M)]
        if any(p is None or max(p) >= HW or min(p) < 0 or len(set(p)) != len(p) for p in px):
            continue
        maps = np.tile(_background(HW), (M, 1))
        for m, p in enumerate(px):
            maps[m, p] = np.float32(1 + m / 128)
        out[name] = (maps.reshape(B, J, H, W), np.array([p[0] for p in px]).reshape(B, J))
    val = (1 + np.arange(M, dtype=np.float32) / 128)[:, None]
    plateau = np.tile(val, (1, HW))
    out['plateau'] = (plateau.reshape(B, J, H, W), np.zeros((B, J), dtype=np.int64))
    but_first = plateau.copy()
    but_first[:, 0] = -1
    out['plateau_but_first_pixel'] = (but_first.reshape(B, J, H, W), np.ones((B, J), dtype=np.int64))
    none = -np.ones((B, J), dtype=np.int64)
    out['all_zero'] = (np.zeros((B, J, H, W), dtype=np.float32), none)
    out['all_negative'] = ((np.tile(_background(HW), (M, 1)) * val).reshape(B, J, H, W), none)
    out['all_neg_inf'] = (np.full((B, J, H, W), -np.inf, dtype=np.float32), none)
    return out


def expected_preds(pixel, H, W):
    """1-based (x, y) of a pixel index the way Evaluation.get_preds counts: x = p mod W + 1, y = floor(p / H) + 1 -- the
    reference divides by size(2), the map HEIGHT, so y is the row only on a square map; (0, 0) for pixel -1"""
    p = np.asarray(pixel)
    xy = np.stack([p % W + 1, p // H + 1], -1).astype(np.float32)
    xy[p < 0] = 0
    return xy


# ------------------------------------------------------------------------------------------------ refinement cases
REFINE_COMBOS = 16 * 9      # peak position (px, py) in {1, 2, W-1, W} x {1, 2, H-1, H}, sign of the x and of the y difference


def refine_combo(H, W, J, start, m):
    """(px, py, sx, sy) of map m: 1-based peak and the signs of hm[py-1][px] - hm[py-1][px-2], hm[py][px-1] - hm[py-2][px-1]"""
    c = 11 * (start + m) % REFINE_COMBOS        # 11 and 144 are coprime: 144 consecutive maps visit every combination once
    pos, sg = c % 16, c // 16
    return (1, 2, W - 1, W)[pos % 4], (1, 2, H - 1, H)[pos // 4], sg % 3 - 1, sg // 3 - 1


@functools.lru_cache(maxsize=4)
def refinement(H, W, J, start=0):
    """maps [B][J][H][W]: one peak per map on or next to the border, its four neighbours set so that the two differences of
    Evaluation.final_preds (:179) have the signs of refine_combo; everything else is the distinct negative background, so a
    difference read where the guard `1 < px < W and 1 < py < H` forbids it is not zero either."""
    M = B * J
    maps = np.tile(_background(H * W), (M, 1)).reshape(M, H, W)
    for m in range(M):
        px, py, sx, sy = refine_combo(H, W, J, start, m)
        x, y = px - 1, py - 1
        for dx, dy, v in ((-1, 0, 0.5), (1, 0, 0.5 + 0.125 * sx), (0, -1, 0.5), (0, 1, 0.5 + 0.125 * sy)):
            if 0 <= x + dx < W and 0 <= y + dy < H:
                maps[m, y + dy, x + dx] = v
        maps[m, y, x] = 1 + m / 128
    return maps.reshape(B, J, H, W)


# ------------------------------------------------------------------------------------------------ expected values
@functools.lru_cache(maxsize=2)
def case_sets(H, W, J, split):
    """dict name -> maps [B][J][H][W]: every case of the three sets at one size"""
    sets = {'realistic': realistic(H, W, J)[0]}
    sets.update(('adversarial:' + k, v[0]) for k, v in adversarial(H, W, J, split).items())
    sets.update(('refinement:%d' % s, refinement(H, W, J, s)) for s in ((0, B * J) if B * J < REFINE_COMBOS else (0,)))
    return sets


@functools.lru_cache(maxsize=None)
def oracle_points(H, W, J, split, name):
    """(get_preds, maximum values, final_preds) of oracle.pylib on one case, computed once and shared by the tests that need it"""
    o = t(case_sets(H, W, J, split)[name])
    (c, s, res, r), _ = meta_tensors(H, W, J)
    return opl.get_preds(o).numpy(), torch.max(o.reshape(B, J, -1), 2)[0].numpy(), opl.final_preds(o, c, s, res, r).numpy()

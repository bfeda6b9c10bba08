"""CPU checks of tests/pylib_exact.py (the references, bounds and cases of the stand-alone pose-library operators): the float64 references
against the oracle on small shapes, the conditions of every case, the checkers against planted errors, and the argument refusals of the
entry points, which are decided on the host before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pylib_exact as X
from tests import warp_grad_exact as W

_CACHE = {}


def _warp(name):
    if name not in _CACHE:
        cs = X.warp_case(name)
        tinv = W.tinv64(cs['params'], cs['res'])
        _CACHE[name] = (cs, tinv) + X.warp64(cs['frames'], cs['sizes'], tinv, cs['params'], cs['res'])
    return _CACHE[name]


def _lib():
    import os
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


# ------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize('name', X.WARP_CASES)
def test_warp_case_meets_its_conditions(name):
    """every d below 2^-30 (from the reference alone), the saturated share, the window outside its frame, the stride case past the grid
    cap, the padding bytes of the sized case"""
    cs, tinv, ref, d = _warp(name)
    assert X.warp_conditions(cs, ref, d) == []
    assert ref.min() >= 0.0 and ref.max() <= 1.0
    B, res = cs['params'].shape[0], cs['res']
    if name == 'stride':
        assert B * res * res > X.GRID_WARP == 8192 * 256 and B * res * res == 2359296
        assert cs['sizes'] is not None and len({tuple(s) for s in cs['sizes']}) == 3
    if name == 'sat':
        assert cs['frames'].min() >= 180 and np.all(cs['params'][:, 5:8] == 1.4) and (ref == 1.0).mean() > 0.1
    if name == 'int':
        assert np.array_equal(cs['params'][:, 0:2], [[60.0, 45.0], [50.0, 40.0], [70.0, 30.0]])
        sx = tinv[0, 0] * 32 + tinv[0, 1] * 32 + tinv[0, 2]                     # the centre pixel: an integer up to rounding
        assert abs(sx - 60.0) < 1e-12
    if name == 'out':
        cs1 = X.warp_case('out')
        u, v, sx, sy = W._sample(cs1['frames'][1], 40, 30, tinv[1], cs1['params'][1], res)[:4]
        assert sx.min() < -1 and sy.min() < -1 and sx.max() > 0 and sy.max() > 0      # negative source coordinates, and some inside
    if name.startswith('tiny'):
        assert B == 1 and res in (1, 3) and cs['frames'].shape[1:3] in ((1, 1), (2, 3))


@pytest.mark.parametrize('name', ('b', 'out', 'tiny_r1_1x1', 'tiny_r3_1x1', 'tiny_r1_2x3', 'tiny_r3_2x3'))
def test_warp_reference_is_the_oracle_sampler(name):
    from oracle import pylib as opl
    cs, tinv, ref, d = _warp(name)
    p = cs['params']
    for i in range(p.shape[0]):
        w, h = (cs['sizes'][i] if cs['sizes'] is not None else (cs['frames'].shape[2], cs['frames'].shape[1]))
        want = opl.warp_bilinear(cs['frames'][i, :h, :w], p[i, 0:2], p[i, 2], p[i, 3], cs['res'], flip=bool(p[i, 4]), gain=p[i, 5:8])
        assert want.dtype == np.float32
        assert X.ratio(want, ref[i], X.warp_bound(ref[i], d[i])) <= 1.0


def test_warp_checkers_catch_planted_errors():
    cs, tinv, ref, d = _warp('a')
    bound = X.warp_bound(ref, d)
    got = ref.astype(np.float32)
    assert X.ratio(got, ref, bound) <= 1.0
    i = np.unravel_index(np.argmax(ref * (ref < 1)), ref.shape)
    moved = got.copy()
    moved[i] = np.float32(ref[i] + 2.0 * bound[i] + np.spacing(np.float32(ref[i])))           # one element moved by (at least) twice its bound
    assert X.ratio(moved, ref, bound) > 1.0
    assert X.ratio(np.roll(got, 1, axis=3), ref, bound) > 1e3                                 # every pixel one column off
    outf = torch.from_numpy(got)
    for dt in (torch.bfloat16, torch.float16):
        out4 = torch.zeros(got.shape[0], got.shape[2], got.shape[3], 4, dtype=dt)
        out4[..., :3] = outf.permute(0, 2, 3, 1).to(dt)
        assert X.out4_mismatches(out4, outf, dt) == 0
        bits = out4.view(torch.int16).clone()
        bits[1, 7, 9, 2] += 1                                                                 # one storage ulp
        assert X.out4_mismatches(bits.view(dt), outf, dt) == 1
        neg0 = out4.clone()
        neg0[0, 0, 0, 3] = -0.0
        assert X.out4_mismatches(neg0, outf, dt) == 1
    trunc = torch.zeros(got.shape[0], got.shape[2], got.shape[3], 4, dtype=torch.bfloat16)  # a truncating cast: the upper 16 bits
    trunc.view(torch.int16)[..., :3] = (outf.permute(0, 2, 3, 1).contiguous().view(torch.int32) >> 16).to(torch.int16)
    assert X.out4_mismatches(trunc, outf, torch.bfloat16) > 100


# ------------------------------------------------------------------------------------------------------------------- transforms
@pytest.mark.parametrize('res_in,res_out', X.AFFINE_RES)
def test_affine_reference_is_the_oracle_transform_and_its_inverse(res_in, res_out):
    from oracle import pylib as opl
    p = X.affine_case()
    assert p.shape[0] == 65 and p[:, 2].min() == 0.05 and p[:, 2].max() == 10.0
    assert {repr(float(r)) for r in p[:, 3]} == {repr(r) for r in X.AFFINE_ROTS}
    t, bt, ti, bi = X.affine_reference(p, res_in, res_out)
    for b, q in enumerate(p):
        te = X.transform_E(q[0], q[1], q[2], q[3], float(res_out))
        assert X.ratio(np.array([x.v for x in te]), t[b], bt[b]) <= 1.0                       # the restatement the bound walks IS the oracle's transform
        inv = np.linalg.inv(opl.get_transform(q[0:2], q[2], q[3], res_in))[:2].reshape(6)
        assert X.ratio(inv, ti[b], bi[b]) <= 1.0                                              # numpy's inverse: inside the same bound
        q1, qb, qi, qbi = X.affine_reference(p[b:b + 1], res_in, res_in)
        assert X.ratio(X.compose_exact(q1[0], qi[0]), np.zeros(6), X.compose_bound(q1[0], qb[0], qi[0], qbi[0])) <= 1.0
    # the bound is relative (a few tens of u64) wherever no sine or cosine is near a zero
    plain = np.isin(p[:, 3], (0.0, 37.5, -37.5))
    lin = [0, 1, 3, 4]                                             # (the translations are sums of terms that cancel: no relative bound)
    assert np.all(bt[plain][:, lin] <= 64 * X.U64 * np.abs(t[plain][:, lin])) and np.all(bi[plain][:, lin] <= 64 * X.U64 * np.abs(ti[plain][:, lin]))
    # and tells a single-precision coefficient from a double one
    assert X.ratio(t.astype(np.float32), t, bt) > 1e3 and X.ratio(ti.astype(np.float32), ti, bi) > 1e3


@pytest.mark.parametrize('J,sized', ((16, False), (16, True), (5, False), (5, True)))
def test_points_reference_is_the_oracle_and_the_planted_joints_are_the_invalid_ones(J, sized):
    from oracle import pylib as opl
    cs = X.pts_case(J, sized)
    p = cs['params']
    assert cs['B'] * J == 65 * J and set(p[:, 4]) == {0.0, 1.0}
    t = X.affine_reference(p, 256, 64)[0]
    out, bound, img, invalid = X.pts_reference(cs, t)
    assert X.pts_planted_ok(cs, invalid)
    assert np.all(out[invalid] == 0) and np.all(bound[invalid] == 0)
    for b in range(cs['B']):
        w = np.float32(cs['sizes'][b, 0] if sized else cs['width'])
        q = cs['pts'][b]
        if p[b, 4]:
            q = opl.shufflelr(q, w) if J == 16 else np.stack([w - q[:, 0], q[:, 1]], axis=1)            # J != 16: mirror, no swap
        assert q.dtype == np.float32 and np.array_equal(q.view(np.int32), img[b].view(np.int32))
        want = opl.transform_pts(q.astype(np.float64), p[b, 0:2], p[b, 2], p[b, 3], 64)
        ok = ~invalid[b]
        assert X.ratio(want[ok], out[b][ok], bound[b][ok]) <= 1.0
    if sized:
        assert len(set(cs['sizes'][:, 0].tolist())) > 30
    # the checker: a joint moved by twice its bound, an unswapped pair, a mirror about the wrong width
    moved = out.copy()
    moved[5, 3, 0] += 2.5 * bound[5, 3, 0]
    assert X.ratio(moved, out, bound) > 1.0
    if J == 16:
        unswapped = dict(cs, J=15, pts=cs['pts'][:, :15])
        assert X.ratio(X.pts_reference(unswapped, t)[0], out[:, :15], bound[:, :15]) > 1e3
    if sized:
        assert X.ratio(X.pts_reference(dict(cs, sizes=None), t)[0], out, bound) > 1e3


# ------------------------------------------------------------------------------------------------------------------- heat maps
@pytest.mark.parametrize('H,Wd', X.HEAT_SHAPES)
def test_heat_cases_hold_every_edge_and_a_swapped_map_is_caught(H, Wd):
    P = X.heat_points(H, Wd)
    x, y = P[:, 0], P[:, 1]
    valid = ~((x <= 0) | (y <= 0) | (x > Wd) | (y > H))
    assert np.any(valid & (x == Wd) & (y == H)) and np.any(valid & (x == Wd) & (y < H)) and np.any(valid & (y == H) & (x < Wd))
    assert np.any(x == np.nextafter(float(Wd), np.inf)) and np.any(y == np.nextafter(float(H), np.inf))
    if min(H, Wd) >= 3:                     # (a valid point with pt - 3 in (-1, 0) has pt in (2, 3): no such point on the 1 x 1 map)
        assert np.any(valid & (x - 3 > -1) & (x - 3 < 0)) and np.any(valid & (y - 3 > -1) & (y - 3 < 0))
    assert np.any((x > 0) & (x <= Wd) & (y > H)) and np.any((y > 0) & (y <= H) & (x > Wd))
    for cx, cy in ((0.5, 0.5), (Wd - 0.5, 0.5), (0.5, H - 0.5), (Wd - 0.5, H - 0.5)):
        assert np.any((x == cx) & (y == cy))
    differs = 0
    for J in X.HEAT_JOINTS:
        batches = X.heat_batches(H, Wd, J)
        assert sum(b.shape[0] * b.shape[1] for b in batches) >= len(P) and all(b.shape == (3, J, 2) for b in batches)
        held = np.concatenate([b.reshape(-1, 2) for b in batches])[:len(P)]
        assert np.array_equal(held, P)
        for pb in batches:
            model = X.heat_model(pb, H, Wd)
            assert X.heat_mismatches(model, pb, H, Wd) == 0                   # the kernel's rule, restated, IS the oracle on these points
            differs += X.heat_mismatches(X.heat_model(pb, H, Wd, swap=True), pb, H, Wd)
            one_off = model.copy()
            one_off[0, 0, 0, 0] = np.nextafter(one_off[0, 0, 0, 0], np.float32(2))
            assert X.heat_mismatches(one_off, pb, H, Wd) == 1
    assert (differs > 0) == (H != Wd)                                         # only a non-square map tells H from W


# ------------------------------------------------------------------------------------------------------------------- loss
def test_l2_reference_bound_and_sentinels():
    from oracle import pylib as opl
    assert X.L2_SIZES == (1, 63, 64, 255, 256, 257, 1000, 262144, 262145, 600001)
    for n in (1, 63, 257, 1000):
        for weighted in (False, True):
            pred, gt, w = X.l2_case(n, weighted)
            ref, bound = X.l2_reference(pred, gt, w)
            want = opl.weighted_l2(torch.from_numpy(pred).double(), torch.from_numpy(gt).double(), torch.from_numpy(w).double() if weighted else 1)
            assert abs(float(want) - ref) <= bound and abs(float(want) - ref) <= 1e-14 * ref
            assert X.l2_reference(pred, gt, w, 1.5)[0] == 1.5 + ref
            assert abs(float(X.l2_model(pred, gt, w)) - ref) <= bound                 # an fp32 sum in another order
    # D of the largest case: 3 + 3 + 6 + 3 + 1 + 1024
    pred, gt, w = X.l2_case(600001, False)
    d = pred.astype(np.float64) - gt.astype(np.float64)
    ref, bound = X.l2_reference(pred, gt, None)
    assert X.l2_blocks(600001) == 1024 and abs(bound / (X.U32 * float(np.sum(d * d)) / 600001) - 1040) < 1e-6
    assert X.l2_sentinels(600001) == [0, 255, 256, 262143, 262144, 600000]
    assert X.l2_sentinels(1) == [0] and X.l2_sentinels(257) == [0, 255, 256]
    # the sentinel checker: a kernel without the grid-stride increment drops every element behind the first pass
    n = 600001
    for e in X.l2_sentinels(n):
        pred, w = np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32)
        pred[e], w[e] = 1.0, 3.0
        gt = np.zeros(n, dtype=np.float32)
        assert X.l2_sentinel_ok(X.l2_model(pred, gt, w), n)
        assert X.l2_sentinel_ok(X.l2_model(pred, gt, w, passes=1), n) == (e < 262144)
        doubled = np.float32(2) * X.l2_model(pred, gt, w)
        assert not X.l2_sentinel_ok(doubled, n)
    # ... while the bound leg alone would let a dropped element pass
    pred, gt, w = X.l2_case(n, True)
    ref, bound = X.l2_reference(pred, gt, w)
    assert abs(float(X.l2_model(pred[:-1], gt[:-1], w[:-1])) * (n - 1) / n - ref) <= bound


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_an_error_and_launch_nothing():
    """every refusal is decided on the host before any device call: it answers on a machine without a GPU.  The pointers are host
    addresses that are never dereferenced: every call below is refused."""
    L = _lib()
    buf = np.zeros(64, dtype=np.float64)
    p = C.c_void_p(buf.ctypes.data)

    def refused(fn, args, bad, word):
        a = list(args)
        for k, v in bad.items():
            a[k] = v
        assert getattr(L, fn)(*a) != 0, (fn, bad)
        msg = L.pa_last_error()
        assert fn.encode() + b':' in msg and word in msg, (fn, bad, msg)

    def sweep(fn, args, ptrs, dims):
        """ptrs: {position: name} of required pointers, dims: {position: name} of extents that must be >= 1"""
        for k, nm in ptrs.items():
            refused(fn, args, {k: None}, nm.encode() + b' is NULL')
        for k, nm in dims.items():
            for v in (0, -3):
                refused(fn, args, {k: v}, nm.encode() + b' must be >= 1')

    sweep('pa_gaussian_heatmap', (p, p, 2, 16, 64, 64, None), {0: 'pts', 1: 'out'}, {2: 'B', 3: 'J', 4: 'H', 5: 'W'})
    sweep('pa_weighted_l2', (p, p, None, 100, p, None), {0: 'pred', 1: 'gt', 4: 'loss'}, {})
    refused('pa_weighted_l2', (p, p, p, 0, p, None), {}, b'n must be >= 1')
    sweep('pa_affine_params', (p, 2, 256, 64, p, p, None), {0: 'params', 4: 't_out', 5: 'tinv_in'}, {1: 'B', 2: 'res_in', 3: 'res_out'})
    sweep('pa_transform_pts', (p, p, p, 2, 16, 1280.0, p, None, None), {0: 'pts', 1: 'params', 2: 't', 6: 'out'}, {3: 'B', 4: 'J'})
    sweep('pa_transform_pts_sized', (p, p, p, 2, 16, p, p, None, None), {0: 'pts', 1: 'params', 2: 't', 5: 'sizes', 6: 'out'}, {3: 'B', 4: 'J'})
    for outs in ((p, p), (p, None), (None, p)):
        sweep('pa_affine_warp_bilinear', (p, 90, 120, p, p, 2, 64) + outs + (None,), {0: 'src', 3: 'tinv', 4: 'params'},
              {1: 'Hs', 2: 'Ws', 5: 'B', 6: 'res'})
        sweep('pa_affine_warp_bilinear_sized', (p, 90, 120, p, p, p, 2, 64) + outs + (None,), {0: 'src', 3: 'sizes', 4: 'tinv', 5: 'params'},
              {1: 'Hs', 2: 'Ws', 6: 'B', 7: 'res'})
    refused('pa_affine_warp_bilinear', (p, 90, 120, p, p, 2, 64, None, None, None), {}, b'out4 and outf are both NULL')
    refused('pa_affine_warp_bilinear_sized', (p, 90, 120, p, p, p, 2, 64, None, None, None), {}, b'out4 and outf are both NULL')
    sweep('pa_flip_lr_nhwc4', (p, p, 2, 64, 64, None), {0: 'src', 1: 'dst'}, {2: 'B', 3: 'H', 4: 'W'})
    sweep('pa_flip_tta_merge', (p, p, p, 2, 16, 64, 64, None), {0: 'out', 1: 'out_flipped', 2: 'merged'}, {3: 'B', 5: 'H', 6: 'W'})
    for J in (0, 5, 15, 17):
        refused('pa_flip_tta_merge', (p, p, p, 2, J, 64, 64, None), {}, b'J must be 16')
    sweep('pa_nchw_to_nhwc', (p, p, 2, 64, 5, 7, None), {0: 'src', 1: 'dst'}, {2: 'B', 3: 'C', 4: 'H', 5: 'W'})
    sweep('pa_nhwc_to_nchw', (p, p, 2, 64, 5, 7, None), {0: 'src', 1: 'dst'}, {2: 'B', 3: 'C', 4: 'H', 5: 'W'})
    assert not buf.any()


def test_header_lists_the_errors_and_the_unswapped_mirror():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'poseadv.h')).read()
    assert 'mirrored but NOT swapped' in hdr
    assert hdr.count('Errors (non-zero, pa_last_error set, nothing launched)') >= 8

"""CPU checks of the warp's backward pass (tests/warp_grad_exact.py holds the reference, the bound and the cases): the float64 reference
against torch autograd of an independent restatement of the sampler, the chain rule of the library (pure host code) against autograd
through the oracle's transform, the case conditions, the workspace query, the exported symbols and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import warp_grad_exact as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pa_affine_warp_bwd_workspace_bytes', 'pa_affine_warp_bilinear_bwd', 'pa_affine_params_bwd_host')
_CACHE = {}


def _ref(name):
    if name not in _CACHE:
        cs = W.case(name)
        tinv = W.tinv64(cs['params'], cs['res'])
        _CACHE[name] = (cs, tinv, W.warp_grad64(cs['frames'], cs['sizes'], tinv, cs['params'], cs['dimg']))
    return _CACHE[name]


def _lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


def _dp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize('name', W.CASES)
def test_case_conditions_hold(name):
    """no coordinate within 1e-9 of an integer (the integer leg: every one exactly an integer), no pre-clamp value other than an exact 0
    within 1e-9 of 0 or 1, the gain leg clamps, the sized leg has taps outside its frame"""
    cs, tinv, ref = _ref(name)
    assert W.conditions(cs, ref) == []
    if name == 'c':
        assert np.array_equal(tinv, np.array([[1.0, 0.0, 4.0, 0.0, 1.0, 4.0]]))
    if name == 'b':                # one window reaches outside the frame, and the narrow sample is the flipped one
        assert cs['params'][1, 4] == 1 and tuple(cs['sizes'][1]) == (40, 48) and ref['outside'] > 0.01


@pytest.mark.parametrize('name', W.CASES)
def test_reference_is_the_autograd_gradient_of_the_sampler(name):
    cs, tinv, ref = _ref(name)
    t = torch.from_numpy(tinv).clone().requires_grad_()
    g = torch.from_numpy(cs['params'][:, 5:8]).clone().requires_grad_()
    out = W.sampler_torch(cs['frames'], cs['sizes'], t, g, cs['params'][:, 4] != 0, cs['res'])
    (out * torch.from_numpy(cs['dimg']).double()).sum().backward()
    bt, bg = W.bounds(ref, cs['res'])
    assert W._ratio(t.grad.numpy(), ref['dtinv'], bt) <= 1.0
    assert W._ratio(g.grad.numpy(), ref['dgain'], bg) <= 1.0
    assert np.abs(ref['dtinv']).min() > 0 and np.abs(ref['dgain']).min() > 0


@pytest.mark.parametrize('name', ('a', 'b'))
def test_bound_tells_a_wrong_tap_a_lost_mirror_and_a_single_precision_coordinate(name):
    cs, tinv, ref = _ref(name)
    bt, bg = W.bounds(ref, cs['res'])

    def worst(frames=cs['frames'], tinv=tinv, params=cs['params']):
        o = W.warp_grad64(frames, cs['sizes'], tinv, params, cs['dimg'])
        return min(W._ratio(o['dtinv'], ref['dtinv'], bt), W._ratio(o['dgain'], ref['dgain'], bg))

    assert worst() == 0.0
    assert worst(frames=np.roll(cs['frames'], 1, axis=2)) > 1e3               # every tap one column off
    unflipped = cs['params'].copy()
    unflipped[:, 4] = 0
    assert worst(params=unflipped) > 1e3
    # coordinates formed from single-precision coefficients: they move by up to 2^-24 Mx where the bound grants 10 x 2^-53 Mx beside
    # the sum's (N + c) u64 mag, N <= 12288 here -- three orders of magnitude are the least that leaves (measured: 2.6e4 and 2e5)
    assert worst(tinv=tinv.astype(np.float32).astype(np.float64)) > 1e3


def test_sampler_restatement_is_the_oracle_sampler():
    """the torch restatement the reference is held against computes the oracle's warp_bilinear (the forward specification)"""
    from oracle import pylib as opl
    cs, tinv, _ = _ref('a')
    p = cs['params']
    out = W.sampler_torch(cs['frames'], None, torch.from_numpy(tinv), torch.from_numpy(p[:, 5:8]), p[:, 4] != 0, cs['res']).numpy()
    for i in (1, 2):
        want = opl.warp_bilinear(cs['frames'][i], p[i, 0:2], p[i, 2], p[i, 3], cs['res'], flip=bool(p[i, 4]), gain=p[i, 5:8])
        assert np.allclose(out[i], want, atol=1e-6)


def test_integer_leg_takes_the_right_hand_cell():
    """at ax = 0 the derivative is p01 - p00 of the cell the forward sampled: a perturbed copy of the case moved a hair to the RIGHT
    (inside that cell) has the same gradient up to the perturbation; moved to the left it has another"""
    cs, tinv, ref = _ref('c')
    right = W.warp_grad64(cs['frames'], None, tinv + np.array([0, 0, 1e-7, 0, 0, 1e-7]), cs['params'], cs['dimg'])
    left = W.warp_grad64(cs['frames'], None, tinv - np.array([0, 0, 1e-7, 0, 0, 1e-7]), cs['params'], cs['dimg'])
    scale = np.abs(ref['dtinv']).max()
    assert np.abs(right['dtinv'] - ref['dtinv']).max() < 1e-5 * scale
    assert np.abs(left['dtinv'] - ref['dtinv']).max() > 1e-2 * scale


def _transform_torch(cx, cy, s, rot, res):
    """oracle.pylib.get_transform in torch float64 with the rotation always applied (rot = 0: the same numbers, the limit's derivative)"""
    h = 200.0 * s
    t = torch.zeros(3, 3, dtype=torch.float64)
    t[0, 0] = res / h
    t[1, 1] = res / h
    t[0, 2] = res * (-cx / h + .5)
    t[1, 2] = res * (-cy / h + .5)
    t[2, 2] = 1
    r = -rot * np.pi / 180
    sn, cs = torch.sin(r), torch.cos(r)
    rm = torch.zeros(3, 3, dtype=torch.float64)
    rm[0, 0], rm[0, 1], rm[1, 0], rm[1, 1], rm[2, 2] = cs, -sn, sn, cs, 1.0
    tm = torch.eye(3, dtype=torch.float64); tm[0, 2] = -res / 2; tm[1, 2] = -res / 2
    ti = tm.clone(); ti[:2, 2] *= -1
    return ti.mm(rm.mm(tm.mm(t)))


def test_chain_rule_of_the_library_is_the_autograd_gradient_through_the_oracle_transform():
    from oracle import pylib as opl
    L = _lib()
    rows = [(60.3, 45.2, 0.35, 0.0), (50.0, 40.0, 0.5, 40.0), (70.0, 30.0, 0.28, -40.0), (655.3, 371.8, 2.013, 25.0), (20.0, 20.0, 0.16, 0.0)]
    gen = np.random.Generator(np.random.PCG64(7))
    for res in (64, 256, 20):
        B = len(rows)
        params = np.zeros((B, 8))
        params[:, :4] = rows
        params[:, 4] = [0, 1, 0, 1, 0]
        params[:, 5:8] = gen.uniform(0.6, 1.4, size=(B, 3))
        dtinv, dgain = gen.standard_normal((B, 6)), gen.standard_normal((B, 3))
        want = np.zeros((B, 8))
        for b in range(B):
            q = torch.tensor(params[b, :4], dtype=torch.float64, requires_grad=True)
            T = _transform_torch(q[0], q[1], q[2], q[3], res)
            ref_t = opl.get_transform(params[b, 0:2], params[b, 2], params[b, 3], res)
            assert np.allclose(T.detach().numpy(), ref_t, rtol=1e-13, atol=1e-11)          # the restatement IS the oracle's transform
            (torch.linalg.inv(T)[:2].reshape(6) * torch.from_numpy(dtinv[b])).sum().backward()
            want[b, :4], want[b, 5:8] = q.grad.numpy(), dgain[b]
        got = np.full((B, 8), np.nan)
        assert L.pa_affine_params_bwd_host(_dp(params), _dp(dtinv), _dp(dgain), B, res, _dp(got)) == 0
        scale = np.stack([np.abs(W.jacobian(params[b], res)).dot(np.abs(np.concatenate([dtinv[b], dgain[b]]))) for b in range(B)])
        assert np.all(np.abs(got - want) <= 1e-12 * scale + 1e-300), (res, np.abs(got - want) / (scale + 1e-300))
        assert np.all(got[:, 4] == 0) and np.all(scale[:, :4] > 0)
        # the module's own Jacobian (the reference of the GPU legs' dparams) is the same chain
        assert np.all(np.abs(W.chain64(params, dtinv, dgain, res) - want) <= 1e-12 * scale)
        # dgain NULL: zeros
        got0 = np.full((B, 8), np.nan)
        assert L.pa_affine_params_bwd_host(_dp(params), _dp(dtinv), None, B, res, _dp(got0)) == 0
        assert np.array_equal(got0[:, :5], got[:, :5]) and np.all(got0[:, 5:] == 0)
    assert L.pa_affine_params_bwd_host(None, _dp(dtinv), None, B, 64, _dp(got)) != 0 and b'NULL' in L.pa_last_error()
    assert L.pa_affine_params_bwd_host(_dp(params), _dp(dtinv), None, 0, 64, _dp(got)) != 0
    assert L.pa_affine_params_bwd_host(_dp(params), _dp(dtinv), None, B, 0, _dp(got)) != 0


def test_workspace_query_needs_no_gpu():
    L = _lib()
    f = L.pa_affine_warp_bwd_workspace_bytes
    assert f(0, 256) == 0 and f(2, 0) == 0 and f(-1, 64) == 0 and f(1, -3) == 0
    for B, res in ((1, 1), (3, 20), (2, 64), (24, 256), (2, 257)):
        n = f(B, res)
        assert n > 0 and n % (B * 9 * 8) == 0                    # nine doubles per strip and sample
        strips = n // (B * 9 * 8)
        assert strips * (res // strips + (res % strips > 0)) >= res and strips <= res
    assert f(24, 256) // (24 * 72) == f(1, 256) // 72            # the strip count does not depend on B


def test_both_libraries_export_the_symbols_and_the_header_declares_them():
    import pose_adv_aug_amd as P
    _lib()
    here = os.path.dirname(P.LIB_PATH)
    for name in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        l = C.CDLL(os.path.join(here, name))
        assert [s for s in SYMBOLS if not hasattr(l, s)] == [], name
    hdr = open(os.path.join(ROOT, 'include', 'poseadv.h')).read()
    assert set(SYMBOLS) <= set(re.findall(r'\b(pa_[a-z0-9_]+)\s*\(', hdr))
    assert set(SYMBOLS) <= set(P.EXPORTS)


def test_refusals_return_an_error_and_launch_nothing():
    """every refusal is decided on the host before any device call: it answers on a machine without a GPU"""
    L = _lib()
    buf = np.zeros(4096, dtype=np.float64)
    a = buf.ctypes.data
    assert a % 16 == 0 or (a + 8) % 16 == 0
    a += a % 16                                   # a 16-byte aligned host address (never dereferenced: every call below is refused)
    p = C.c_void_p(a)

    def call(src=p, tinv=p, params=p, B=2, res=64, dimg=p, layout=0, ws=p, dt=p, dg=p, dp=p):
        return L.pa_affine_warp_bilinear_bwd(src, 90, 120, None, tinv, params, B, res, dimg, layout, ws, dt, dg, dp, None)

    for kw, word in ((dict(src=None), b'NULL'), (dict(tinv=None), b'NULL'), (dict(params=None), b'NULL'), (dict(dimg=None), b'NULL'),
                     (dict(ws=None), b'NULL'), (dict(layout=2), b'layout'), (dict(layout=-1), b'layout'),
                     (dict(dimg=C.c_void_p(a + 4)), b'aligned'), (dict(dimg=C.c_void_p(a + 8)), b'aligned'), (dict(B=0), b'B >= 1'),
                     (dict(res=0), b'res >= 1'), (dict(res=-5), b'res >= 1'), (dict(dt=None, dg=None, dp=None), b'all NULL')):
        assert call(**kw) != 0, kw
        assert word in L.pa_last_error(), (kw, L.pa_last_error())


def test_python_argument_errors_come_before_any_launch():
    from pose_adv_aug_amd.pylib import HumanAug
    B, res = 2, 16
    frames = torch.zeros(B, 30, 40, 3, dtype=torch.uint8)
    tinv, params = torch.zeros(B, 6, dtype=torch.float64), torch.zeros(B, 8, dtype=torch.float64)
    dimg = torch.zeros(B, 3, res, res)
    with pytest.raises(ValueError):
        HumanAug.warp_batch_backward(frames, tinv, params, dimg, layout='nhwc')
    with pytest.raises(ValueError):                                   # CPU tensors: the device is wrong
        HumanAug.warp_batch_backward(frames, tinv, params, dimg)
    for bad in (dict(frames=frames.float()), dict(tinv=tinv.float()), dict(tinv=torch.zeros(B, 5, dtype=torch.float64)),
                dict(params=torch.zeros(B + 1, 8, dtype=torch.float64)), dict(dimg=dimg.double()), dict(dimg=torch.zeros(B, 3, res, res + 1)),
                dict(dimg=torch.zeros(B, res, res, 4)), dict(sizes=torch.zeros(B, 2, dtype=torch.int64))):
        kw = dict(frames=frames, tinv=tinv, params=params, dimg=dimg, sizes=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            HumanAug.warp_batch_backward(kw['frames'], kw['tinv'], kw['params'], kw['dimg'], 'nchw', sizes=kw['sizes'])

"""The bound of tests/optim_exact.py is not vacuous: a numpy fp32 emulation of the RMSprop kernel (csrc/elementwise.hip rmsprop_kernel, through rmsprop_v / rmsprop_p:
gr = g * gscale; v = alpha * v + (1.f - alpha) * gr * gr; p = p - lr * (gr / (sqrtf(v) + eps)), each operation rounded on its own, and the
same with the update of v contracted into one fma) stays inside it for p and for square_avg over 200 003 elements at every gscale of the
GPU cases, and each of these defects is reported at every gscale at which it is one:
  * eps inside the square root, or no eps at all;
  * gscale dropped, or applied twice (at gscale != 1);
  * four elements left untouched, or updated twice (a vector chunk lost or revisited by the grid-stride loop or its tail).
Inputs as the GPU cases draw them (optim_exact.make_inputs): |g s| log-uniform in 1e-12 .. 1e3 with exact zeros, v zero or log-uniform
in 1e-24 .. 1e6."""
import numpy as np
import pytest
import torch

from tests import optim_exact as X

N = 200003
f = np.float32


def _emulate(p, g, v, gscale, defect=None, fma=False):
    lr, alpha, eps, s = f(X.LR), f(X.ALPHA), f(X.EPS), f(gscale)
    gr = g if defect == 'gscale dropped' else g * s
    if defect == 'gscale twice':
        gr = gr * s
    t = (f(1) - alpha) * gr * gr
    if fma:         # fmaf(alpha, v, t): one rounding (float64 holds the product and the sum of these values far beyond fp32's precision)
        vv = (alpha.astype(np.float64) * v.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    else:
        vv = alpha * v + t
    if defect == 'eps inside the root':
        pp = p - lr * (gr / np.sqrt(vv + eps))
    elif defect == 'no eps':
        with np.errstate(divide='ignore', invalid='ignore'):
            pp = p - lr * (gr / np.sqrt(vv))
    else:
        pp = p - lr * (gr / (np.sqrt(vv) + eps))
    assert pp.dtype == np.float32 and vv.dtype == np.float32
    return pp, vv


def _apply(p, g, v, gscale, defect=None, fma=False):
    pp, vv = _emulate(p, g, v, gscale, defect, fma)
    k = N - 7           # a chunk that ends in the tail region of an n with n % 4 == 3
    if defect == 'four untouched':
        pp[k:k + 4], vv[k:k + 4] = p[k:k + 4], v[k:k + 4]
    if defect == 'four twice':
        p2, v2 = _emulate(pp, g, vv, gscale)
        pp[k:k + 4], vv[k:k + 4] = p2[k:k + 4], v2[k:k + 4]
    return pp, vv


def _ratios(gscale, v_zero, defect=None, fma=False):
    p, g, v = X.make_inputs(N, 7, gscale, v_zero)
    pp, vv = _apply(p, g, v, gscale, defect, fma)
    t = torch.from_numpy
    return X.check(t(p), t(g), t(v), t(pp), t(vv), gscale)


@pytest.mark.parametrize('gscale', X.GSCALES)
@pytest.mark.parametrize('v_zero', (True, False))
@pytest.mark.parametrize('fma', (False, True))
def test_the_emulated_kernel_is_inside_the_bound(gscale, v_zero, fma):
    rp, rv = _ratios(gscale, v_zero, fma=fma)
    print('gscale %g v0 %s fma %s: worst error / bound p %.3f square_avg %.3f' % (gscale, 'zero' if v_zero else 'nonzero', fma, rp, rv))
    assert rp <= 1.0 and rv <= 1.0, (rp, rv)
    # the bound is tight: the emulation uses a good part of it
    assert rp > 0.2 and rv > 0.2, (rp, rv)


DEFECTS = ('eps inside the root', 'no eps', 'gscale dropped', 'gscale twice', 'four untouched', 'four twice')


@pytest.mark.parametrize('v_zero', (True, False))
@pytest.mark.parametrize('defect,gscale', [(d, s) for d in DEFECTS for s in X.GSCALES if not (d.startswith('gscale') and s == 1.0)])
def test_each_defect_is_outside_the_bound(defect, gscale, v_zero):
    rp, rv = _ratios(gscale, v_zero, defect)
    print('%s, gscale %g v0 %s: error / bound p %.3g square_avg %.3g' % (defect, gscale, 'zero' if v_zero else 'nonzero', rp, rv))
    assert not (rp <= 1.0 and rv <= 1.0), (rp, rv)      # (NaN -- no eps at g = 0, v = 0 -- counts as a failure, as in the GPU check)
    # far outside, not marginally: >= 1e5 times the bound in p or in square_avg (the four-element chunks: 2e4 in p, 3e6 in square_avg)
    assert not (rp <= 1e5 and rv <= 1e5), (rp, rv)


def test_a_nan_is_a_failure():
    p, g, v = X.make_inputs(64, 8, 1.0, True)
    pp, vv = _emulate(p, g, v, 1.0)
    pp[5] = np.nan
    t = torch.from_numpy
    rp, rv = X.check(t(p), t(g), t(v), t(pp), t(vv), 1.0)
    assert not (rp <= 1.0) and rv <= 1.0

"""CPU side of the backward pass from given heat-map gradients: the two new C entry points are declared, exported by both builds and
bound; there is no CPU fallback; and the per-element bound of tests/heat_grads_exact.py admits the two fp32 evaluations a compiler may
emit (multiply then add; one fma), rejects the same data one storage ulp off, and is not degenerate on the test's data."""
import ctypes
import os
import re

import pytest
import torch

from tests import heat_grads_exact as hx
from tests.conv_exact import DEGENERATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pa_hg_set_heat_grads', 'pa_weighted_l2_grad')


def test_header_libraries_and_binding_hold_the_new_entry_points():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    hdr = open(os.path.join(ROOT, 'include', 'poseadv.h')).read()
    declared = set(re.findall(r'\b(pa_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW:
        assert name in declared, name
        assert name in P.EXPORTS, name
        for so in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
            assert hasattr(ctypes.CDLL(os.path.join(os.path.dirname(P.LIB_PATH), so)), name), (so, name)


def test_backward_has_no_cpu_fallback():
    import pose_adv_aug_amd as P
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.pylib import Criterion
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    net = create_hg(2, 1, 16, 128, res=128, default_batch=2)
    with pytest.raises(P.PoseAdvError):
        net.backward([torch.zeros(2, 16, 32, 32), None])
    with pytest.raises(P.PoseAdvError):
        net.forward_autograd(torch.zeros(2, 3, 128, 128))
    with pytest.raises(P.PoseAdvError):
        Criterion.weighted_L2(torch.zeros(2, 16, 32, 32, requires_grad=True), torch.zeros(2, 16, 32, 32), 1)


@pytest.mark.parametrize('dtype,scale', [(torch.bfloat16, 1.0), (torch.float16, 32768.0)])
@pytest.mark.parametrize('with_add', [False, True])
def test_injected_gradient_bound(dtype, scale, with_add):
    G, add = hx.cpu_data(11, 1 << 16, scale, dtype)
    add = add if with_add else None
    for emul in (hx.emul_mul_add, hx.emul_fma):
        got = emul(G, scale, add, dtype)
        r, deg = hx.inject_check(got, G, scale, add, dtype)
        assert r <= 1.0, (emul.__name__, r)
        assert deg <= DEGENERATE, (emul.__name__, deg)          # (the emulation alone: the bound still says something on this data)
        assert hx.outside(got, G, scale, add, dtype) == 0.0
        # one storage ulp off, either way: an element passes only if the rounding error it had was within 2u of half an ulp
        for up in (True, False):
            moved = hx.move_one_ulp(got, dtype, up)
            assert bool((moved != got).all())
            assert hx.inject_check(moved, G, scale, add, dtype)[0] > 1.0
            assert hx.outside(moved, G, scale, add, dtype) > 0.99, (emul.__name__, up)


def test_the_two_emulations_differ_somewhere_and_the_bound_holds_both():
    """(so that the test above is about two evaluations, not one: with an addend in fp16 and scale 32768 the product is exact and both
    agree; bf16's scale 1 likewise -- the difference shows with a scale that is not a power of two, which the bound must admit too)"""
    G, add = hx.cpu_data(12, 1 << 16, 3.0, torch.bfloat16)
    a, b = hx.emul_mul_add(G, 3.0, add, torch.float32), hx.emul_fma(G, 3.0, add, torch.float32)
    assert bool((a != b).any())
    for got in (a.to(torch.bfloat16).float(), b.to(torch.bfloat16).float()):
        assert hx.inject_check(got, G, 3.0, add, torch.bfloat16)[0] <= 1.0

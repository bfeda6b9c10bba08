"""CPU checks of the image-gradient feature (tests/image_grad_exact.py holds the reference and the bound): the float64 reference against
torch autograd, the kernel's GEMM formulation against the reference, that the bound can be held by an fp32 evaluation and still tells a
dropped or transposed tap, the exported symbols of both libraries, and the Python argument errors."""
import ctypes
import multiprocessing as mp
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_exact as X
from tests import image_grad_exact as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = [(5, 7), (16, 16), (17, 33)]          # images 10 x 14, 32 x 32 and 34 x 66
SYMBOLS = ('pa_hg_set_image_grad', 'pa_stem_dgrad_workspace_bytes', 'pa_stem_dgrad')


def _operands(Hm, Wm, B=2, seed=0, dtype=None):
    gen = torch.Generator().manual_seed(1000 * Hm + Wm + seed)
    g = torch.randn(B, 64, Hm, Wm, generator=gen, dtype=torch.float64)
    w = torch.randn(64, 3, 7, 7, generator=gen, dtype=torch.float64) / 147 ** 0.5
    if dtype is not None:
        g, w = X.rnd(g, dtype), X.rnd(w, dtype)
    return g, w


@pytest.mark.parametrize('Hm,Wm', MAPS)
def test_reference_is_the_autograd_gradient_of_the_stem_conv(Hm, Wm):
    g, w = _operands(Hm, Wm)
    x = torch.randn(2, 3, 2 * Hm, 2 * Wm, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, stride=2, padding=3).backward(g)
    ref = G.stem_dgrad64(g, w)
    assert ref.shape == x.shape
    assert float((ref - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


@pytest.mark.parametrize('Hm,Wm', MAPS + [(1, 1)])
def test_block_gemm_formulation_is_the_reference(Hm, Wm):
    """the kernel's weight tile and 4 x 4 window (2 x 2 pixel blocks, taps ky = py + 5 - 2 wy) give the transposed convolution; 4th channel 0"""
    g, w = _operands(Hm, Wm)
    o = G.block_gemm64(g, w)
    ref = G.stem_dgrad64(g, w)
    assert float((o[:, :3] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((o[:, 3] == 0).all())


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
@pytest.mark.parametrize('Hm,Wm', MAPS)
def test_bound_holds_for_fp32_and_tells_a_wrong_tap(Hm, Wm, dtype):
    g, w = _operands(Hm, Wm, dtype=dtype)
    ev = lambda ww: F.conv_transpose2d(g.float(), ww.float(), stride=2, padding=3, output_padding=1)
    r, deg = G.bound_check(ev(w), g, w)
    assert r <= 1.0 and deg <= X.DEGENERATE, (r, deg)
    dropped = w.clone()
    dropped[:, :, 2, 4] = 0                                   # one tap of 49
    r, _ = G.bound_check(ev(dropped), g, w)
    assert r > 1.0, r
    r, _ = G.bound_check(ev(w.transpose(2, 3)), g, w)               # ky / kx swapped
    assert r > 1.0, r
    # the half-precision build's scale: value, bound and magnitude scale together
    r, deg = G.bound_check(ev(w) * 2.0 ** -15, g, w, scale=2.0 ** -15)
    assert r <= 1.0 and deg <= X.DEGENERATE, (r, deg)


def test_poisoned_check_is_the_plain_check_for_finite_operands_and_tells_a_lost_nan():
    Hm, Wm = 16, 16
    g, w = _operands(Hm, Wm, dtype=torch.float16)
    ev = lambda gg: F.conv_transpose2d(gg.float(), w.float(), stride=2, padding=3, output_padding=1)
    assert G.poisoned_check(ev(g), g, w) == G.bound_check(ev(g), g, w) + (0,)
    bad = g.clone()
    bad[1, 5, 7, 9] = float('nan')
    bad[0, 60, 0, 15] = float('inf')
    out = G.block_gemm64(bad, w)[:, :3].float()          # the kernel's formulation: 0 x NaN poisons the whole window
    r, deg, lost = G.poisoned_check(out, bad, w)
    assert r <= 1.0 and lost == 0 and not bool(torch.isfinite(out).all())
    r, deg, lost = G.poisoned_check(ev(bad), bad, w)      # the taps' own footprint
    assert r <= 1.0 and lost == 0
    r, deg, lost = G.poisoned_check(ev(g), bad, w)        # a result that lost the NaN
    assert lost > 0
    dropped = w.clone()
    dropped[:, :, 2, 4] = 0
    r, _, _ = G.poisoned_check(F.conv_transpose2d(bad.float(), dropped.float(), stride=2, padding=3, output_padding=1), bad, w)
    assert r > 1.0                                        # still discriminates outside the poisoned blocks


def test_depth_is_one_chain_of_k_1024():
    assert G.K_CHAIN == 1024 and G.DEPTH == 32 + 32


def test_both_libraries_export_the_symbols_and_the_header_declares_them():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    here = os.path.dirname(P.LIB_PATH)
    for name in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        l = ctypes.CDLL(os.path.join(here, name))
        assert [s for s in SYMBOLS if not hasattr(l, s)] == [], name
    hdr = open(os.path.join(ROOT, 'include', 'poseadv.h')).read()
    declared = set(re.findall(r'\b(pa_[a-z0-9_]+)\s*\(', hdr))
    assert set(SYMBOLS) <= declared
    assert set(SYMBOLS) <= set(P.EXPORTS)
    # bad shapes need no device: 0 bytes
    l = P.lib()
    assert l.pa_stem_dgrad_workspace_bytes(1, 3, 4) == 0 and l.pa_stem_dgrad_workspace_bytes(1, 0, 2) == 0
    assert l.pa_stem_dgrad_workspace_bytes(2, 4, 6) >= 2 * 2 * 3 * 64 * 2 + 64 * 256 * 2


@pytest.mark.parametrize('bad', ('nhwc', 'NCHW', 1, 2, 'yes'))
def test_bad_input_grad_value_raises_without_a_gpu(bad):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(1, 1, 16, 128, res=128, default_batch=2)
    with pytest.raises(ValueError):
        net.backward([None], input_grad=bad)
    with pytest.raises(ValueError):
        net.loss_and_backward(img4=torch.zeros(2, 128, 128, 4), pts=torch.zeros(2, 16, 2), input_grad=bad)
    for good, lay in ((False, None), (None, None), (True, 0), ('nchw', 0), ('nhwc4', 1)):
        assert net._input_grad_layout(good) == lay


def _stub_worker(out):
    from tests import abi_stub
    fake = abi_stub.install(0)
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(2, 1, 16, 256, default_batch=2)
    net._net(2)
    net._last_B = 2
    del fake.log[:]
    g = [torch.zeros(2, 16, 64, 64), None]
    try:
        net.backward(g, input_grad='nhwc')
        out['bad'] = 'no error'
    except ValueError:
        out['bad'] = fake.names()
    del fake.log[:]
    d = net.backward(g, input_grad='nhwc4')
    out['shape'] = tuple(d.shape)
    out['calls'] = [(n, a[2]) for n, a in fake.log if n == 'pa_hg_set_image_grad']
    out['order'] = [n for n in fake.names() if n in ('pa_hg_set_image_grad', 'pa_hg_backward', 'pa_hg_set_heat_grads')]
    del fake.log[:]
    out['off'] = net.backward(g)
    out['off_calls'] = [n for n in fake.names() if n == 'pa_hg_set_image_grad']
    del fake.log[:]
    net.use_graph = True
    net.loss_and_backward(img4=torch.zeros(2, 256, 256, 4), pts=torch.zeros(2, 16, 2), input_grad=True)
    out['graph'] = [n for n in fake.names() if n in ('pa_hg_train_step', 'pa_hg_backward', 'pa_hg_set_image_grad')]
    out['last'] = tuple(net.last_input_grad.shape)
    del fake.log[:]
    net.loss_and_backward(img4=torch.zeros(2, 256, 256, 4), pts=torch.zeros(2, 16, 2))
    out['graph_off'] = [n for n in fake.names() if n in ('pa_hg_train_step', 'pa_hg_backward', 'pa_hg_set_image_grad')]
    out['last_off'] = net.last_input_grad


def test_host_control_flow_on_a_stubbed_library():
    """a bad layout reaches no library call; the door is opened before the backward pass and closed behind it; off by default; with
    use_graph a step that wants the gradient takes the eager path"""
    out = mp.Manager().dict()
    p = mp.get_context('spawn').Process(target=_stub_worker, args=(out,))
    p.start(); p.join(120)
    assert p.exitcode == 0
    assert out['bad'] == []
    assert out['shape'] == (2, 256, 256, 4)
    assert out['calls'] == [('pa_hg_set_image_grad', 1), ('pa_hg_set_image_grad', 0)]
    assert out['order'] == ['pa_hg_set_heat_grads', 'pa_hg_set_image_grad', 'pa_hg_backward', 'pa_hg_set_heat_grads', 'pa_hg_set_image_grad']
    assert out['off'] is None and out['off_calls'] == []
    assert out['graph'] == ['pa_hg_set_image_grad', 'pa_hg_backward', 'pa_hg_set_image_grad'] and out['last'] == (2, 3, 256, 256)
    assert out['graph_off'] == ['pa_hg_train_step'] and out['last_off'] is None

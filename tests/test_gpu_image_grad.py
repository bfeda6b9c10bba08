"""d loss / d image on the device: the stem's data-gradient kernel (csrc/stem_dgrad.hip) through pa_stem_dgrad, pa_hg_set_image_grad,
HourglassNet.backward / loss_and_backward(input_grad=...) and forward_autograd.  Reference, bound and legs: tests/image_grad_exact.py.
Small nets throughout (chan 128, B <= 3): each case takes a few seconds."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from tests import image_grad_exact as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('layout', (0, 1))
@pytest.mark.parametrize('B,H,W', G.OP_SHAPES)
def test_operator_element_by_element(B, H, W, layout):
    """pa_stem_dgrad, dy ~ N(0, 1), w ~ N(0, 1 / 147): every element within e + u |ref| (D = 64); the 4th float of layout 1 exactly 0;
    the floats in front of and behind the output untouched"""
    fails = G.operator_leg(B, H, W, layout)
    assert not fails, fails


@pytest.mark.parametrize('stacks,res,B,seed', G.NET_LEGS)
def test_gradient_inside_the_net(stacks, res, B, seed):
    """last_input_grad of a training step from img4 against stem_dgrad64(rnd(view 3 of "stem"), rnd(stem weight)); 'nhwc4' holds the same
    bits; then through pa_hg_set_heat_grads with the MSE's own gradient, in eval mode, and from the NCHW fp32 input"""
    fails = G.net_leg(stacks, res, B, seed)
    assert not fails, fails


def test_nothing_else_moves():
    """door on / off on twin nets: flat_grads, the per-stack losses and the BatchNorm buffers bit for bit; the conv launch log of a
    door-off step equals that of a second one, and a door-on step adds no row"""
    fails = G.same_leg()
    assert not fails, fails


def test_autograd_returns_the_input_gradient():
    from pose_adv_aug_amd.pylib import Criterion, HumanPts
    from tests.heat_grads_exact import make_net
    B, res, seed = 2, 128, 91
    img, img4, pts = G.net_inputs(B, res, seed)
    T = HumanPts.pts2heatmap_batch(pts, res // 4, res // 4)
    net, twin = make_net(2, B, res, seed), make_net(2, B, res, seed)
    x = img.clone().requires_grad_()
    loss = sum(Criterion.weighted_L2(o, T, 1) for o in net.forward_autograd(x=x))
    loss.backward(retain_graph=True)
    assert x.grad is not None and tuple(x.grad.shape) == (B, 3, res, res) and x.grad.dtype == torch.float32
    # the same pass on the twin: the gradients autograd delivered, through backward(input_grad=True)
    o2 = [o.detach().requires_grad_() for o in twin(img)]
    gs = torch.autograd.grad(sum(Criterion.weighted_L2(o, T, 1) for o in o2), o2)
    d = twin.backward(list(gs), input_grad=True)
    torch.cuda.synchronize()
    assert float(d.abs().max()) > 0 and torch.equal(x.grad, d)
    assert torch.equal(net.flat_grads, twin.flat_grads)
    with pytest.raises(RuntimeError):                   # a second backward of one forward pass
        loss.backward()
    # img4: the NHWC4 gradient in img4's dtype
    i4 = img4.clone().requires_grad_()
    sum(Criterion.weighted_L2(o, T, 1) for o in net.forward_autograd(img4=i4)).backward()
    twin(img4=img4)
    o2 = [o.detach().requires_grad_() for o in twin.heatmaps()]
    gs = torch.autograd.grad(sum(Criterion.weighted_L2(o, T, 1) for o in o2), o2)
    d4 = twin.backward(list(gs), input_grad='nhwc4')
    torch.cuda.synchronize()
    assert i4.grad.dtype == img4.dtype and tuple(i4.grad.shape) == (B, res, res, 4)
    assert torch.equal(i4.grad, d4.to(img4.dtype)) and bool((i4.grad[..., 3] == 0).all())
    # without requires_grad nothing is produced: the door is never opened
    opened = []
    orig = net._open_image_grad
    net._open_image_grad = lambda h, B_, lay: opened.append(lay) or orig(h, B_, lay)
    x2 = img.clone()
    sum(Criterion.weighted_L2(o, T, 1) for o in net.forward_autograd(x=x2)).backward()
    torch.cuda.synchronize()
    assert x2.grad is None and opened == [None]
    assert torch.equal(net.flat_grads, twin.flat_grads)          # (the parameter gradients land all the same)


def test_refusals():
    from pose_adv_aug_amd._lib import lib, ptr
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    from tests.heat_grads_exact import make_net
    B, res = 2, 128
    net = make_net(1, B, res, 92)
    img, img4, pts = G.net_inputs(B, res, 92)
    net.loss_and_backward(img4=img4, pts=pts)
    torch.cuda.synchronize()
    before = net.flat_grads.clone()
    L, h = lib(), net._net(B)
    buf = torch.zeros(B * res * res * 4 + 4, dtype=torch.float32, device='cuda')
    assert L.pa_hg_set_image_grad(h, ptr(buf), 2) != 0 and b'layout' in L.pa_last_error()
    assert L.pa_hg_set_image_grad(h, C.c_void_p(buf.data_ptr() + 4), 1) != 0 and b'aligned' in L.pa_last_error()
    agent = create_asn(128, 128, 7, 7, is_aug=True, res=256, default_batch=B)
    assert L.pa_hg_set_image_grad(agent._net(B), ptr(buf), 0) != 0 and b'pose net' in L.pa_last_error()
    # a refused call set nothing: the step writes no image gradient
    net.loss_and_backward(img4=img4, pts=pts)
    torch.cuda.synchronize()
    assert torch.equal(net.flat_grads, before) and float(buf.abs().max()) == 0.0
    with pytest.raises(ValueError):
        net.backward([torch.zeros(B, 16, res // 4, res // 4, device='cuda')], input_grad='nhwc')
    # no captured graph while the door is set; it works again after NULL
    p64 = pts.to(torch.float64).contiguous()
    assert L.pa_hg_set_image_grad(h, ptr(buf), 1) == 0
    try:
        assert L.pa_hg_train_step(h, ptr(img4), ptr(p64), 1, 1, None) != 0 and b'pa_hg_set_image_grad' in L.pa_last_error()
        torch.cuda.synchronize()
        assert torch.equal(net.flat_grads, before) and float(buf.abs().max()) == 0.0
    finally:
        assert L.pa_hg_set_image_grad(h, None, 0) == 0
    assert L.pa_hg_train_step(h, ptr(img4), ptr(p64), 1, 1, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(net.flat_grads).all()) and float(buf.abs().max()) == 0.0


def test_half_precision_build():
    """the operator, net and door on / off legs in the IEEE-half build (the reference divided by grad_scale()): one child process, the
    storage type is per process"""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'image_grad_exact.py')], env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and 'FP16 IMAGE GRAD PASSED' in r.stdout, tail

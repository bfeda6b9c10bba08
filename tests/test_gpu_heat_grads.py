"""The backward pass from the caller's heat-map gradients (pa_hg_set_heat_grads, HourglassNet.backward / forward_autograd,
Criterion.weighted_L2's gradient) on the device.  The legs and bounds: tests/heat_grads_exact.py.  Small nets throughout (chan 128,
B <= 3): each case takes a few seconds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import heat_grads_exact as hx
from tests import inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


# stacks, B, res, seed, the stack whose gradient is None, consumers checked
@pytest.mark.parametrize('stacks,B,res,seed,none_stack,cons', [(2, 2, 128, 41, 0, True), (2, 3, 128, 42, 1, True), (1, 1, 192, 43, None, False)])
def test_injected_gradient_element_by_element_in_both_layouts(stacks, B, res, seed, none_stack, cons):
    """view 1 of heat<i>: channels 0..15 within the bound of G_i * grad_scale (+ heat<i>.in), 16..63 exactly 0, one stack None; both
    layouts give equal buffers and parameter gradients; on the 2-stack legs out_conv's weight / bias gradients and lin's data gradient
    in float64 from the injected tensor (192: 48 x 48 maps, not a power of two)."""
    fails = hx.inject_leg(stacks, B, res, seed, none_stack=none_stack, check_consumers=cons)
    assert not fails, fails


def test_mse_gradient_given_by_the_caller_leaves_the_bits_of_the_built_in_loss():
    """1 stack, B 2, res 128 (numel = 2^15): backward([2 (out - T) / numel]) == loss_and_backward, twice, phased, and the built-in
    path afterwards"""
    fails = hx.same_bits(128, 44)
    assert not fails, fails


def test_the_same_with_occlusion_masks():
    """(the 4 x 4 cell mask needs the neck map of a 256 input: B 2, res 256, numel = 2^17)"""
    fails = hx.same_bits(256, 45, masked=True)
    assert not fails, fails


def test_per_joint_weighted_loss_through_autograd_against_the_oracle():
    """a loss the engine does not have: sum_i ((o_i - T)^2 w).sum() / numel with per-joint weights in [0, 2], three of them 0 per
    sample; forward_autograd + Criterion.weighted_L2 + loss.backward() against autograd of the oracle.  Tolerances: those of
    test_gpu_net.py::test_hourglass_forward_backward_vs_oracle for the built-in loss on this very net."""
    from pose_adv_aug_amd.pylib import Criterion
    from tests.test_gpu_net import _hg_pair, cosine, rel_rms, t
    torch.set_num_threads(8)
    B, res, chan = 2, 128, 128
    ref, net = _hg_pair(2, chan, B, res, seed=7)
    img = t(inputs.images(8, B, res))
    pts = inputs.heat_pts(9, B, res=res // 4)
    T = t(inputs.heatmaps_from_pts(pts, res=res // 4))
    w = t(inputs.rng(10, 4).uniform(0.0, 2.0, size=(B, 16)).astype(np.float32))
    w[0, [2, 5, 11]] = 0
    w[1, [5, 7, 13]] = 0                    # joint 5: no weight in either sample
    wf = w.view(B, 16, 1, 1).expand_as(T).contiguous()
    ref.train(); net.train()
    ref.zero_grad()
    loss_ref = sum(((o - T) ** 2 * wf).sum() / T.numel() for o in ref(img))
    loss_ref.backward()
    outs = net.forward_autograd(img.cuda())
    assert len(outs) == 2 and all(o.grad_fn is not None and tuple(o.shape) == (B, 16, res // 4, res // 4) for o in outs)
    Td, wd = T.cuda(), wf.cuda()
    loss = sum(Criterion.weighted_L2(o, Td, wd) for o in outs)
    net.flat_grads.zero_()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(loss_ref.detach())) / float(loss_ref.detach()) < 1e-2
    gref = dict(ref.named_parameters())
    seen = 0
    for name, g in net.named_grads():
        if name.startswith('out_conv.1.') or name.startswith('linear.1.1.'):
            assert rel_rms(g.cpu(), gref[name].grad) < 5e-2 and cosine(g.cpu(), gref[name].grad) > 0.998, name
            seen += 1
    assert seen == 4
    grads = dict(net.named_grads())
    assert float(grads['out_conv.1.weight'].abs().max()) > 0
    assert bool((grads['out_conv.1.weight'][5] == 0).all()) and float(grads['out_conv.1.bias'][5]) == 0.0
    assert bool((grads['out_conv.1.weight'][2] != 0).any())          # (a joint with weight in one sample)


@pytest.mark.parametrize('n', [5, 4096, 2 * 16 * 32 * 32 + 3])
@pytest.mark.parametrize('weighted', [False, True])
def test_weighted_l2_grad_element_by_element(n, weighted):
    """dpred = 2 w (pred - gt) gout / n: a subtraction and three multiplications in fp32 -> within 4 u |ref| of float64"""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    g = inputs.rng(21, n, int(weighted))
    pred = torch.from_numpy(g.standard_normal(n).astype(np.float32)).cuda()
    gt = torch.from_numpy(g.random(n).astype(np.float32)).cuda()
    w = torch.from_numpy(g.uniform(0.0, 2.0, n).astype(np.float32)).cuda() if weighted else None
    gout = torch.tensor([0.37], dtype=torch.float32, device='cuda')
    dpred = torch.full((n + 8,), 7.0, dtype=torch.float32, device='cuda')
    check(lib().pa_weighted_l2_grad(ptr(pred), ptr(gt), ptr(w), n, ptr(gout), ptr(dpred), stream()), 'pa_weighted_l2_grad')
    torch.cuda.synchronize()
    ref = 2.0 * (w.double() if weighted else 1.0) * (pred.double() - gt.double()) * gout.double() / n
    err = (dpred[:n].double() - ref).abs()
    worst = float((err / (4 * U * ref.abs()).clamp_min(1e-300)).max())
    print('pa_weighted_l2_grad n %d weighted %d: worst error / (4 u |ref|) = %.3f' % (n, weighted, worst))
    assert bool((err <= 4 * U * ref.abs()).all()), worst
    assert bool((dpred[n:] == 7.0).all()), 'wrote past n'
    # buffers that are not 16-byte aligned (one float in) take the scalar loop: the same arithmetic, the same bound
    d1 = torch.full((n + 8,), 7.0, dtype=torch.float32, device='cuda')
    check(lib().pa_weighted_l2_grad(C.c_void_p(pred.data_ptr() + 4), C.c_void_p(gt.data_ptr() + 4), C.c_void_p(w.data_ptr() + 4) if weighted else None,
                                    n - 1, ptr(gout), ptr(d1), stream()), 'pa_weighted_l2_grad')
    torch.cuda.synchronize()
    ref1 = 2.0 * (w.double()[1:] if weighted else 1.0) * (pred.double()[1:] - gt.double()[1:]) * gout.double() / (n - 1)
    assert bool(((d1[:n - 1].double() - ref1).abs() <= 4 * U * ref1.abs()).all())
    assert bool((d1[n - 1:] == 7.0).all()), 'wrote past n'
    # through autograd: Criterion.weighted_L2 of a tensor that requires grad, times a factor so that the arriving gradient is not 1
    from pose_adv_aug_amd.pylib import Criterion
    p = pred.clone().requires_grad_(True)
    loss = Criterion.weighted_L2(p, gt, w if weighted else 1)
    assert loss.grad_fn is not None
    (loss * 0.37).backward()
    assert torch.equal(p.grad, dpred[:n])
    assert Criterion.weighted_L2(pred, gt, w if weighted else 1).grad_fn is None
    for bad in ((None, gt, gout, dpred), (pred, None, gout, dpred), (pred, gt, None, dpred), (pred, gt, gout, None)):
        assert lib().pa_weighted_l2_grad(ptr(bad[0]), ptr(bad[1]), None, n, ptr(bad[2]), ptr(bad[3]), stream()) != 0
        assert b'pa_weighted_l2_grad' in lib().pa_last_error()


def _net_and_input(stacks=2, B=2, res=128, seed=51):
    net = hx.make_net(stacks, B, res, seed)
    img = torch.from_numpy(inputs.images(seed + 100, B, res)).cuda()
    pts = torch.from_numpy(inputs.heat_pts(seed + 101, B, res=res // 4)).cuda()
    return net, img, pts


def test_autograd_semantics():
    net, img, pts = _net_and_input()
    outs = net.forward_autograd(img, pts=pts)
    assert net._last_losses is not None and net.accuracy([0, 1, 2]).numel() == 4          # pts feeds the meters as in forward()
    loss = sum((o ** 2).mean() for o in outs)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError):                   # a second backward of one forward pass
        loss.backward()
    outs = net.forward_autograd(img)
    net(img)                                            # a later forward pass: the stored activations are gone
    with pytest.raises(RuntimeError):
        outs[1].sum().backward()
    # a stack the loss does not use arrives as None = zero: nothing of the last stack gets a gradient when only stack 0 is in the loss
    outs = net.forward_autograd(img)
    net.flat_grads.fill_(1.0)
    outs[0].mean().backward()
    torch.cuda.synchronize()
    g = dict(net.named_grads())
    assert float(g['out_conv.0.weight'].abs().max()) > 0 and float(g['conv1.weight'].abs().max()) > 0
    assert all(float(v.abs().max()) == 0.0 for k, v in g.items() if k.startswith(('out_conv.1.', 'linear.1.', 'hg.1.')))
    with torch.no_grad():
        assert all(o.grad_fn is None for o in net.forward_autograd(img))


def test_train_step_with_a_criterion():
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.pylib import Criterion, HumanPts
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import RMSprop
    torch.cuda.set_device(0)
    B, res = 2, 128
    net = hx.make_net(1, B, res, 52)
    opt = RMSprop(net, lr=2.5e-4)
    aug = Augmenter(seed=3, inp_res=res, out_res=res // 4)
    batch = DeviceBatch.synthetic(B, seed=7)
    data = aug.regular(batch)
    p0 = net.flat_params.clone()

    def criterion(outs, d):
        T = HumanPts.pts2heatmap_batch(d['pts'], res // 4, res // 4)
        return sum(Criterion.weighted_L2(o, T, 1) for o in outs)
    loss, pckh, pckh_o = train_step(net, opt, aug, batch, data=data, criterion=criterion)
    torch.cuda.synchronize()
    step_custom = net.flat_params.clone()
    assert loss.grad_fn is None and np.isfinite(float(loss)) and pckh is not None and pckh_o is not None
    # the same step with the built-in loss from the same weights: numel = 2^15, so the gradients -- and the update -- have the same bits
    net.flat_params.copy_(p0); net.weights_changed()
    opt2 = RMSprop(net, lr=2.5e-4)
    loss2, _, _ = train_step(net, opt2, aug, batch, data=data)
    torch.cuda.synchronize()
    assert not torch.equal(step_custom, p0)
    assert torch.equal(net.flat_params, step_custom)
    assert abs(float(loss) - float(loss2)) <= 1e-5 * abs(float(loss2))


def test_refusals():
    from pose_adv_aug_amd._lib import lib, ptr
    net, img, pts = _net_and_input()
    B, Hh = 2, 32
    net(img)
    net.loss_and_backward(img, pts)
    before = net.flat_grads.clone()
    ok = torch.zeros(B, 16, Hh, Hh, device='cuda')
    for bad in ([ok], [ok, ok, ok],                                     # count
                [ok, torch.zeros(B, 16, Hh, Hh + 1, device='cuda')],      # shape
                [ok.permute(0, 2, 3, 1).contiguous(), None],               # shape (the other layout's)
                [ok.double(), None],                                      # dtype
                [ok.cpu(), ok],                                           # device
                [None, None]):
        with pytest.raises(ValueError):
            net.backward(bad)
    with pytest.raises(ValueError):
        net.backward([ok, ok], layout='chw')
    torch.cuda.synchronize()
    assert torch.equal(net.flat_grads, before), 'a refused call launched something'
    # the C call
    L = lib()
    h = net._net(B)
    buf = torch.zeros(B * 16 * Hh * Hh + 4, device='cuda')
    two = lambda a, b: (C.c_void_p * 2)(a, b)
    assert L.pa_hg_set_heat_grads(h, two(buf.data_ptr(), None), 2) != 0 and b'layout' in L.pa_last_error()
    assert L.pa_hg_set_heat_grads(h, two(None, None), 0) != 0 and b'NULL' in L.pa_last_error()
    assert L.pa_hg_set_heat_grads(h, two(None, buf.data_ptr() + 4), 1) != 0 and b'aligned' in L.pa_last_error()
    # a refused call set nothing: the built-in loss still runs
    net.loss_and_backward(img, pts)
    torch.cuda.synchronize()
    assert torch.equal(net.flat_grads, before)
    # no captured graph while gradients are set
    assert L.pa_hg_set_heat_grads(h, two(buf.data_ptr(), None), 0) == 0
    try:
        img4 = torch.zeros(B, 128, 128, 4, dtype=torch.bfloat16, device='cuda')
        p64 = pts.to(torch.float64).contiguous()
        assert L.pa_hg_train_step(h, ptr(img4), ptr(p64), 1, 1, None) != 0 and b'pa_hg_set_heat_grads' in L.pa_last_error()
        torch.cuda.synchronize()
        assert torch.equal(net.flat_grads, before)
    finally:
        assert L.pa_hg_set_heat_grads(h, None, 0) == 0
    # an agent is not a pose net
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    agent = create_asn(128, 128, 7, 7, is_aug=True, res=256, default_batch=B)
    assert L.pa_hg_set_heat_grads(agent._net(B), two(buf.data_ptr(), None), 0) != 0 and b'pose net' in L.pa_last_error()


def test_half_precision_build():
    """the injection legs and the same-bits legs in the IEEE-half build (gradients travel times 32768): one child process, the storage
    type is per process"""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'heat_grads_exact.py')], env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and 'FP16 HEAT GRADS PASSED' in r.stdout, tail

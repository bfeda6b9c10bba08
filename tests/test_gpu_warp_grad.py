"""d loss / d {scale, rotation, centre, gain} on the device: the backward kernels of the bilinear warp (csrc/warp_bwd.hip) through
pa_affine_warp_bilinear_bwd, HumanAug.warp_batch_backward / warp_autograd and Augmenter.bilinear.  Reference, bound, cases and legs:
tests/warp_grad_exact.py.  Small shapes throughout: each case takes a few seconds."""
import os
import subprocess
import sys

import pytest
import torch

from tests import warp_grad_exact as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('layout', (0, 1))
@pytest.mark.parametrize('name', W.CASES)
def test_operator_element_by_element(name, layout):
    """every element of dtinv, dgain and dparams within u64 (N + c) mag + u64 c_xy mag_xy + u64 |ref| of the float64 reference evaluated on the device's own
    tinv; guard doubles around the outputs and guard bytes around the workspace untouched; two calls give the same bits; the Python
    operator gives the bits of the C call.  (a) the forward test's case, (b) sized frames, a mirrored narrow one, res 20, (c) the
    integer leg, (d) res 256"""
    fails = W.operator_leg(name, layout)
    assert not fails, fails


def test_the_two_layouts_give_the_same_bits():
    from pose_adv_aug_amd.pylib import HumanAug
    cs, frames, sizes, params, tinv = W.device_case('b')
    dimg = torch.from_numpy(cs['dimg']).cuda()
    a = HumanAug.warp_batch_backward(frames, tinv, params, W.dimg_layout(dimg, 0), 'nchw', sizes=sizes)
    b = HumanAug.warp_batch_backward(frames, tinv, params, W.dimg_layout(dimg, 1), 'nhwc4', sizes=sizes)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_optional_outputs_and_refusals_on_the_device():
    """each output alone gives the bits of the full call; a refused call writes nothing"""
    import ctypes as C
    from pose_adv_aug_amd._lib import lib, ptr, stream
    L = lib()
    cs, frames, sizes, params, tinv = W.device_case('b')
    B, res = 3, cs['res']
    dimg = torch.from_numpy(cs['dimg']).cuda()
    ws = torch.empty(int(L.pa_affine_warp_bwd_workspace_bytes(B, res)), dtype=torch.uint8, device='cuda')
    outs = [torch.full((B, n), -1.0, dtype=torch.float64, device='cuda') for n in (6, 3, 8)]
    call = lambda d, lay, o: L.pa_affine_warp_bilinear_bwd(ptr(frames), 48, 64, ptr(sizes), ptr(tinv), ptr(params), B, res, d, lay, ptr(ws),
                                                           ptr(o[0]), ptr(o[1]), ptr(o[2]), stream())
    assert call(ptr(dimg), 0, outs) == 0
    for i in range(3):
        only = [None, None, None]
        only[i] = torch.full_like(outs[i], -1.0)
        assert call(ptr(dimg), 0, only) == 0
        torch.cuda.synchronize()
        assert torch.equal(only[i], outs[i])
    kept = [torch.full_like(o, -1.0) for o in outs]
    assert call(ptr(dimg), 2, kept) != 0 and b'layout' in L.pa_last_error()
    assert call(C.c_void_p(dimg.data_ptr() + 4), 0, kept) != 0 and b'aligned' in L.pa_last_error()
    assert call(ptr(dimg), 0, [None, None, None]) != 0
    torch.cuda.synchronize()
    assert all(bool((k == -1.0).all()) for k in kept)


def test_chain_to_params_grad_through_the_net():
    """loss.backward() through forward_autograd and warp_autograd == the twin net's backward(input_grad=True) fed to warp_batch_backward,
    bit for bit; flat_grads equal; the flip column 0; without requires_grad no backward launch"""
    fails = W.chain_leg()
    assert not fails, fails


def test_augmenter_bilinear():
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.pylib import HumanAug
    B, res = 2, 64
    g0 = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (B, 90, 120, 3), generator=g0, dtype=torch.uint8)
    joints = torch.rand(B, 16, 2, generator=g0) * torch.tensor([100.0, 70.0]) + 10.0
    batch = DeviceBatch(frames, [[60.3, 45.2], [55.1, 40.7]], [0.4, 0.33], joints, [30.0, 40.0])
    aug = Augmenter(seed=1, inp_res=res, out_res=res // 4)
    want = aug.standard(batch, want_nchw=True)                 # (the keys of _finish; fills batch.params with centre, scale, gain 1)
    params = batch.params.clone()
    params[:, 3] = torch.tensor([17.0, -8.0], dtype=torch.float64)
    params[:, 5:8] = torch.tensor([[0.8, 1.0, 1.2], [1.1, 0.9, 1.0]], dtype=torch.float64)
    step = aug.step
    p = params.clone().requires_grad_()
    data = aug.bilinear(batch, p)
    assert sorted(data) == sorted(want) and aug.step == step
    _, tinv = HumanAug.affine_params(params, res, res)
    out4, outf = HumanAug.warp_batch(batch.frames, tinv, params, res=res, want_nchw=True, sizes=batch.sizes)
    assert data['img'].grad_fn is not None and torch.equal(data['img'].detach(), outf)
    assert data['img4'].grad_fn is None and torch.equal(data['img4'], out4)
    for k in ('pts', 'grnd_pts', 'c', 's', 'r'):
        assert not data[k].requires_grad
    t_out, _ = HumanAug.affine_params(params, res, res // 4)
    pts_heat, _ = HumanAug.transform_pts_batch(batch.joints, params, t_out, batch.Ws, sizes=batch.sizes)
    assert torch.equal(data['pts'], pts_heat) and torch.equal(data['s'], params[:, 2].float())
    g = torch.randn(B, 3, res, res, generator=torch.Generator().manual_seed(5)).cuda()
    (data['img'] * g).sum().backward()
    _, _, dp = HumanAug.warp_batch_backward(batch.frames, tinv, params, g, 'nchw', sizes=batch.sizes)
    torch.cuda.synchronize()
    assert torch.equal(p.grad, dp) and bool((p.grad[:, 4] == 0).all()) and float(p.grad[:, :4].abs().min()) > 0
    # no grad asked for: the same pixels, no graph
    plain = aug.bilinear(batch, params)
    assert plain['img'].grad_fn is None and torch.equal(plain['img'], outf) and torch.equal(plain['img4'], out4)
    with pytest.raises(ValueError):
        aug.bilinear(batch, params.float())


def test_params_changed_in_place_before_backward_is_an_error():
    """the node saves params through autograd: a gradient for other parameters than the forward used cannot come out silently"""
    from pose_adv_aug_amd.pylib import HumanAug
    cs, frames, sizes, params, _ = W.device_case('b')
    p = params.clone().requires_grad_()
    img, img4 = HumanAug.warp_autograd(frames, p, res=cs['res'], sizes=sizes, want_nhwc4=True)
    assert img.grad_fn is not None and not img4.requires_grad and tuple(img4.shape) == (3, cs['res'], cs['res'], 4)
    with torch.no_grad():
        p[:, 2] *= 1.5
    with pytest.raises(RuntimeError):
        img.sum().backward()


def test_python_argument_errors_on_the_device():
    from pose_adv_aug_amd.pylib import HumanAug
    cs, frames, sizes, params, tinv = W.device_case('b')
    dimg = torch.from_numpy(cs['dimg']).cuda()
    for kw in (dict(dimg=dimg.cpu()), dict(dimg=dimg.permute(0, 1, 3, 2)), dict(dimg=torch.zeros(dimg.numel() + 1, device='cuda')[1:].view(dimg.shape)),
               dict(params=params[:2]), dict(sizes=sizes.long()), dict(layout='nhwc4')):
        a = dict(frames=frames, tinv=tinv, params=params, dimg=dimg, layout='nchw', sizes=sizes)
        a.update(kw)
        with pytest.raises(ValueError):
            HumanAug.warp_batch_backward(a['frames'], a['tinv'], a['params'], a['dimg'], a['layout'], sizes=a['sizes'])


def test_half_precision_build():
    """leg (a) in both layouts and the chain in the IEEE-half build (the kernels are the same code; dimg is unscaled in both): one child
    process, the storage type is per process"""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'warp_grad_exact.py')], env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and 'FP16 WARP GRAD PASSED' in r.stdout, tail

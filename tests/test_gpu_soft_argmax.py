"""The soft-arg-max on the device: pa_soft_argmax / pa_soft_argmax_bwd (csrc/soft_argmax.hip) element by element against float64,
pylib.Evaluation.soft_argmax, the joint-minor outputs of HourglassNet.forward_autograd and the coordinate loss in train_step.  Reference,
bound, cases and legs: tests/soft_argmax_exact.py.  Small shapes throughout: each test takes a few seconds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import soft_argmax_exact as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', S.CASES)
def test_operator_element_by_element(name):
    """every element of coords, state and dmaps within its bound (forward u32 |ref| + d, backward the same + 2^-126; d counted from the
    kernel's operations), sum_p dmaps within the summed bound of 0, outputs pre-filled with NaN fully overwritten, guard regions around
    maps, coords, state and dmaps untouched, two runs bit-identical.  fast_*: J 16 joint-minor at 1 x 1, 16 x 16, 64 x 64, 96 x 96 and
    8 x 24, B 1 and 3, the maxima on each side of every boundary of the kernels' split, rising and falling ramps; range_*: magnitude 3e4
    at beta 1 and +-3e38 at beta 1e-3; generic_*: J 1, 5, 17 in both layouts, and J 16 from a pointer moved by 4 bytes"""
    fails, worst = S.operator_leg(name)
    print(name, worst)
    assert not fails, (fails, worst)


def _run(maps, H, W, beta=1.0, dco=None, layout=1):
    """ad-hoc maps [B][J][HW] through the guarded device call -> coords, state, dmaps (numpy), findings"""
    B, J, _ = maps.shape
    cs = dict(maps=maps.astype(np.float32), dco=np.ones((B, J, 2), dtype=np.float32) if dco is None else dco, B=B, J=J, H=H, W=W, beta=beta, layout=layout, offset=0)
    coords, state, dmaps, _, fails = S.device_call(cs)
    return coords, state, dmaps, fails


def test_exact_expectations():
    """== : a uniform map gives ((W + 1) / 2, (H + 1) / 2); one peak 1.0 over values <= 0 at beta 1000 gives pa_get_preds_nhwc's
    coordinates (every other term is exp(< -745) = 0), two such peaks their midpoint; a 1 x 1 map gives (1, 1) and a zero gradient; a joint
    with dcoords == 0 has dmaps all zero"""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    for H, W in ((16, 16), (8, 24), (96, 96)):
        coords, state, _, fails = _run(np.full((2, 16, H * W), 0.37), H, W, beta=3.0)
        assert not fails and np.all(coords[..., 0] == (W + 1) / 2) and np.all(coords[..., 1] == (H + 1) / 2) and np.all(state[..., 1] == H * W)
    H = W = 64
    gen = np.random.Generator(np.random.PCG64(5))
    maps = -gen.uniform(0.0, 1.0, (3, 16, H * W))
    peaks = gen.integers(0, H * W, (3, 16))
    peaks[0, :4] = (0, H * W - 1, 1023, 1024)
    np.put_along_axis(maps, peaks[..., None], 1.0, axis=-1)
    dco = gen.standard_normal((3, 16, 2)).astype(np.float32)
    dco[1, 5] = 0.0
    coords, state, dmaps, fails = _run(maps, H, W, beta=1000.0, dco=dco)
    assert not fails and np.all(state[..., 1] == 1.0)
    hard = torch.empty(3, 16, 2, device='cuda')
    nhwc = torch.from_numpy(np.ascontiguousarray(maps.astype(np.float32).transpose(0, 2, 1))).cuda()
    check(lib().pa_get_preds_nhwc(ptr(nhwc), 3, 16, H, W, ptr(hard), None, stream()), 'pa_get_preds_nhwc')
    assert np.array_equal(coords, hard.cpu().numpy())
    assert np.array_equal(coords[..., 0], peaks % W + 1) and np.array_equal(coords[..., 1], peaks // W + 1)
    assert np.all(dmaps[1, 5] == 0) and np.all(dmaps == 0)            # a delta: every pixel either has e_p = 0 or sits on the expectation
    second = (peaks + 1 + 2 * W) % (H * W)
    np.put_along_axis(maps, second[..., None], 1.0, axis=-1)
    coords, state, _, fails = _run(maps, H, W, beta=1000.0)
    assert not fails and np.all(state[..., 1] == 2.0)
    assert np.array_equal(coords[..., 0], ((peaks % W + 1) + (second % W + 1)) / 2) and np.array_equal(coords[..., 1], ((peaks // W + 1) + (second // W + 1)) / 2)
    for J, layout in ((16, 1), (3, 0)):
        coords, state, dmaps, fails = _run(gen.standard_normal((2, J, 1)), 1, 1, beta=2.0, layout=layout)
        assert not fails and np.all(coords == 1.0) and np.all(dmaps == 0) and np.all(state[..., 1:] == 1.0)


def test_refusals_launch_nothing_on_the_device():
    from pose_adv_aug_amd._lib import lib, ptr, stream
    L = lib()
    B, H, W = 2, 8, 8
    maps = torch.randn(B, H * W, 16, device='cuda')
    coords, state = torch.full((B, 16, 2), -1.0, device='cuda'), torch.full((B, 16, 4), -1.0, dtype=torch.float64, device='cuda')
    dmaps, dco = torch.full_like(maps, -1.0), torch.ones(B, 16, 2, device='cuda')
    fwd = lambda **k: L.pa_soft_argmax(k.get('maps', ptr(maps)), k.get('layout', 1), k.get('B', B), 16, H, W, k.get('beta', 1.0), ptr(coords), ptr(state), stream())
    bwd = lambda **k: L.pa_soft_argmax_bwd(ptr(maps), k.get('layout', 1), k.get('B', B), 16, H, W, k.get('beta', 1.0), ptr(state), ptr(dco), k.get('dmaps', ptr(dmaps)), stream())
    for kw, word in ((dict(maps=None), b'NULL'), (dict(layout=2), b'layout'), (dict(B=0), b'>= 1'), (dict(beta=0.0), b'beta'), (dict(beta=float('nan')), b'beta')):
        assert fwd(**kw) != 0 and word in L.pa_last_error(), kw
    for kw, word in ((dict(dmaps=None), b'NULL'), (dict(dmaps=ptr(maps)), b'alias'), (dict(layout=-1), b'layout'), (dict(beta=float('inf')), b'beta')):
        assert bwd(**kw) != 0 and word in L.pa_last_error(), kw
    torch.cuda.synchronize()
    assert bool((coords == -1).all()) and bool((state == -1).all()) and bool((dmaps == -1).all())


@pytest.mark.parametrize('layout', ('nchw', 'nhwc'))
def test_python_operator_gives_the_bits_of_the_c_calls(layout):
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    from pose_adv_aug_amd.pylib import Evaluation
    B, J, H, W, beta = 3, 16, 8, 24, 0.8
    g = torch.Generator().manual_seed(4)
    heat = (torch.randn((B, J, H, W) if layout == 'nchw' else (B, H, W, J), generator=g) * 2).cuda()
    dco = torch.randn(B, J, 2, generator=g).cuda()
    h = heat.clone().requires_grad_()
    out = Evaluation.soft_argmax(h, beta, layout)
    assert out.grad_fn is not None and tuple(out.shape) == (B, J, 2) and out.dtype == torch.float32
    (out * dco).sum().backward()
    lay = 0 if layout == 'nchw' else 1
    coords, state = torch.empty(B, J, 2, device='cuda'), torch.empty(B, J, 4, dtype=torch.float64, device='cuda')
    dmaps = torch.full_like(heat, float('nan'))
    check(lib().pa_soft_argmax(ptr(heat), lay, B, J, H, W, beta, ptr(coords), ptr(state), stream()))
    check(lib().pa_soft_argmax_bwd(ptr(heat), lay, B, J, H, W, beta, ptr(state), ptr(dco), ptr(dmaps), stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), coords) and torch.equal(h.grad, dmaps) and bool(torch.isfinite(dmaps).all()) and float(dmaps.abs().max()) > 0
    plain = Evaluation.soft_argmax(heat, beta, layout)
    assert plain.grad_fn is None and torch.equal(plain, coords)
    for bad in (heat.cpu(), heat.double(), heat[0]):
        with pytest.raises(ValueError):
            Evaluation.soft_argmax(bad, beta, layout)


def test_coordinate_loss_through_the_net():
    """chan 128, B 2, 128 x 128, 1 stack: forward_autograd(layout='nhwc') -> coord_L1(soft_argmax(.)) -> backward() leaves flat_grads
    bit-identical to a twin's backward([dmaps], layout='nhwc') fed from the direct calls; the 'nhwc' outputs are the 'nchw' outputs
    permuted; a second backward raises as it does today"""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    from pose_adv_aug_amd.pylib import Criterion, Evaluation
    from tests import inputs
    from tests.heat_grads_exact import make_net
    B, res, beta = 2, 128, 0.5
    Hh = res // 4
    img = torch.from_numpy(inputs.images(6, B, res)).cuda()
    pts = torch.from_numpy(inputs.heat_pts(7, B, res=Hh)).cuda()
    net, twin = make_net(1, B, res, 31), make_net(1, B, res, 31)
    outs = net.forward_autograd(x=img, pts=pts, layout='nhwc')
    assert len(outs) == 1 and tuple(outs[0].shape) == (B, Hh, Hh, 16) and outs[0].grad_fn is not None
    ref_nchw = net.heatmaps(B)[0]
    assert torch.equal(outs[0].detach().permute(0, 3, 1, 2), ref_nchw)
    assert outs[0].data_ptr() == lib().pa_hg_heatmap_nhwc(net._nets[B][0], 0)               # a view of the engine's buffer, not a copy
    xy = Evaluation.soft_argmax(outs[0], beta, 'nhwc')
    loss = Criterion.coord_L1(xy, pts, size=(Hh, Hh))
    loss.backward()
    # the twin by hand: default-layout forward, the operator pair called directly, backward(layout='nhwc')
    t_nchw = twin.forward(x=img, pts=pts)[0]
    assert torch.equal(t_nchw, ref_nchw)
    maps = twin.heatmaps(B, layout='nhwc')[0]
    coords, state = torch.empty(B, 16, 2, device='cuda'), torch.empty(B, 16, 4, dtype=torch.float64, device='cuda')
    check(lib().pa_soft_argmax(ptr(maps), 1, B, 16, Hh, Hh, beta, ptr(coords), ptr(state), stream()))
    c = coords.clone().requires_grad_()
    Criterion.coord_L1(c, pts, size=(Hh, Hh)).backward()
    dmaps = torch.empty_like(maps)
    check(lib().pa_soft_argmax_bwd(ptr(maps), 1, B, 16, Hh, Hh, beta, ptr(state), ptr(c.grad.contiguous()), ptr(dmaps), stream()))
    twin.backward([dmaps], layout='nhwc')
    torch.cuda.synchronize()
    assert torch.equal(xy.detach(), coords) and float(c.grad.abs().sum()) > 0
    assert torch.equal(net.flat_grads, twin.flat_grads) and float(net.flat_grads.abs().max()) > 0 and bool(torch.isfinite(net.flat_grads).all())
    with pytest.raises(RuntimeError):
        Criterion.coord_L1(Evaluation.soft_argmax(outs[0], beta, 'nhwc'), pts).backward()


def test_two_train_steps_with_the_coordinate_loss(tmp_path):
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.stack_hg import coord_criterion, train_step
    from pose_adv_aug_amd.utils.optim import make_optimizer
    opt = TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'c', '--coord_loss', '0.1', '--bs', '2'])
    torch.cuda.set_device(0)
    net = create_hg(1, 1, 16, 128, res=128, default_batch=2)
    net.reset_parameters(seed=3)
    net.train()
    optimizer = make_optimizer(opt, net, opt.lr)
    aug = Augmenter(seed=9, inp_res=128, out_res=32)
    crit = coord_criterion(opt.coord_loss, opt.coord_beta)
    start = net.flat_params.clone()
    losses = []
    for k in range(2):
        loss, pckh, _ = train_step(net, optimizer, aug, DeviceBatch.synthetic(2, seed=40 + k), criterion=crit, heat_layout='nhwc')
        losses.append(float(loss))
        mse = float(net._last_losses.sum())
        assert np.isfinite(losses[-1]) and losses[-1] > mse > 0          # the coordinate term is on top of the engine's own MSE of the same maps
    assert not torch.equal(net.flat_params, start) and bool(torch.isfinite(net.flat_params).all())


def test_half_precision_build():
    """a subset of the cases in the IEEE-half build (the operator is fp32 in both): one child process, the storage type is per process"""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'soft_argmax_exact.py')], env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and 'FP16 SOFT ARGMAX PASSED' in r.stdout, tail

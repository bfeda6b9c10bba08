"""Pool routing (pa_net_set_pool_route, csrc/net.hip Hourglass::bwd): the forward max pools of an hourglass store a one-byte arg-max map, and
the first block of the skip branch beside a pool reads the pool's gradient through that map in the epilogue of its conv1 data gradient
(PA_LD_POOL, csrc/conv_epilogue.h) instead of from a full-resolution tensor a pool backward launch wrote.  The map holds exactly what the
pool backward kernels recompute (first maximum in scan order, strict >, on the same fp32 values), and the epilogue redoes the one bf16
rounding of the stored tensor, so the two forms must agree BIT FOR BIT: every comparison here is on the raw bits (NaN-safe), no tolerance.

Chan 256, so that the instances of the benchmark run: the one-shot 1x1 kernel below 12288 pixels (every case but the last), the
row-tile 1x1 kernel from 12288 pixels (B = 3 at 64 x 64: 192 tiles of 64 rows).  One case at chan 512, where only the stem's pool can be
routed and the hourglass pools fall back to a launch each."""
import ctypes as C

import pytest
import torch

from tests import inputs

pytestmark = pytest.mark.gpu

STEPS = 3


def _bits(x):
    x = x.detach().contiguous()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dbg(h, name, grad):
    from pose_adv_aug_amd._lib import lib, check, ptr
    fn = lib().pa_hg_debug_tensor
    shp = (C.c_int * 4)()
    check(fn(h, name.encode(), grad, None, shp))
    out = torch.empty(tuple(shp), device='cuda')
    check(fn(h, name.encode(), grad, ptr(out), shp))
    return out.cpu()


def _images(kind, seed, B, res):
    if kind == 'zero':                    # every 2x2 window a tie (after the ReLU too): position 0 by the first-maximum rule
        return torch.zeros(B, 3, res, res)
    img = torch.from_numpy(inputs.images(seed, B, res))
    if kind == 'blocks':                  # constant per 2x2 window
        img = img[:, :, ::2, ::2].repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    return img


def _train(route, B, res, stacks, modules=1, masks=None, kind='random', want=(), chan=256):
    """STEPS training steps from one seed; returns the final state, the last step's gradients and heat maps, and the debug views `want`
    ((name, view) pairs, each read TWICE) of the last step"""
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.utils.optim import RMSprop
    net = create_hg(stacks, modules, 16, chan, res=res, default_batch=B); net.reset_parameters(seed=7); net.train()
    h = net._net(B)
    _lib.check(_lib.lib().pa_net_set_pool_route(h, 1 if route else 0), 'pa_net_set_pool_route')
    opt = RMSprop(net, lr=2.5e-4)
    pts = torch.from_numpy(inputs.heat_pts(17, B, res=res // 4)).cuda()
    from tests import conv_plan_query as Q
    # (the engine's launch log: tests/test_conv_plan_cpu.py counts the routed launches of these steps as covered)
    with Q.launches('pool_route route %d B %d res %d stacks %d modules %d chan %d masks %s' % (route, B, res, stacks, modules, chan, masks is not None)):
        for i in range(STEPS):
            img = _images(kind, 30 + i, B, res).cuda()
            loss, outs = net.loss_and_backward(img, pts, want_outputs=True, dropout_masks=masks)
            if i + 1 < STEPS:
                opt.step()
    design = (C.c_double * 2)()
    _lib.check(_lib.lib().pa_net_design_bytes(h, design), 'pa_net_design_bytes')
    views = [(_dbg(h, n, v), _dbg(h, n, v)) for n, v in want]
    opt.step()
    torch.cuda.synchronize()
    got = {'params': net.flat_params.clone(), 'grads': net.flat_grads.clone(), 'buffers': net.flat_buffers.clone(),
           'loss': loss.clone(), 'views': views, 'design': (design[0], design[1])}
    for i, o in enumerate(outs):
        got['heat%d' % i] = o.clone()
    return got


def _compare(off, on, finite=True):
    for k in off:
        if k == 'views':
            continue
        if k == 'design':                 # the routed step really is another launch plan: it reads and writes fewer bytes (pa_net_design_bytes)
            assert on[k][0] < off[k][0] and on[k][1] < off[k][1], (off[k], on[k])
            continue
        if k == 'loss':                   # (the reported loss is summed with one float atomic per workgroup: not a bitwise quantity)
            assert abs(float(off[k]) - float(on[k])) <= 1e-6 * abs(float(off[k])) or not finite
            continue
        assert _same(off[k], on[k]), '%s differs between pool routing off and on (%d of %d elements)' % (
            k, int((_bits(off[k]) != _bits(on[k])).sum()), off[k].numel())
    assert not finite or bool(torch.isfinite(off['grads']).all())


def _drop_masks(B):
    m = torch.ones(B, 1, 4, 4)
    g = inputs.rng(91)
    for b in range(B):
        for cell in g.choice(16, 2, replace=False):
            m[b, 0, cell // 4, cell % 4] = 0
    return m.cuda()


CASES = {
    # 64 x 64 ... 8 x 8 levels, the addend of the inner stack (d xin1 into level 1 of stack 0), the plain-epilogue input of stack 1
    'two_stacks_b2_res256': dict(B=2, res=256, stacks=2),
    'one_stack_b1_res128': dict(B=1, res=128, stacks=1),
    'one_stack_b1_res192': dict(B=1, res=192, stacks=1),               # map widths 24 / 12 / 6 / 3 pooled pixels: no power of two
    'two_modules_b1_res128': dict(B=1, res=128, stacks=1, modules=2),
    # the occlusion branch (4 x 4 cell masks on the skip / neck tensors); the engine takes cell masks at res 256 only (4 x 4 neck map)
    'occlusion_b2_res256': dict(B=2, res=256, stacks=1, masks=True),
    # 12288 pixels at 64 x 64: the row-tile kernel's instances (BatchNorm-backward epilogue in stack 0, plain epilogue in stack 1)
    'row_tile_b3_res256': dict(B=3, res=256, stacks=2),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_pool_routing_on_and_off_give_the_same_bits(case):
    c = dict(CASES[case])
    if c.pop('masks', False):
        c['masks'] = _drop_masks(c['B'])
    _compare(_train(False, **c), _train(True, **c))


@pytest.mark.parametrize('kind', ['zero', 'blocks'])
def test_ties_go_to_the_first_maximum_in_both_forms(kind):
    """All-zero images: every pooled window is a tie; images constant per 2x2 window: the stem's windows are.  Both forms send the
    gradient of a tie to scan position 0."""
    c = dict(B=2, res=128, stacks=2, kind=kind)
    _compare(_train(False, **c), _train(True, **c), finite=False)      # (a constant image: BatchNorm over zero variance)


@pytest.mark.parametrize('res,stacks', [(128, 2), (256, 1)])
def test_requested_tensors_are_what_the_unrouted_step_stored(res, stacks):
    """hg0.poolgrad1..4 (no step with routing stores them: asking runs the pool backward launch) and the gradient views of res1 (stored dz and
    the gradient of the raw tensor) of a routed step equal, bit for bit, what the step without routing stored; a second request returns the
    same array.  At res 256 the stem's pool is routed too (32768 pixels: residual1's conv3 data gradient is a row-tile launch), at 128 not."""
    want = [('hg0.poolgrad%d' % k, 2) for k in (1, 2, 3, 4)] + [('hg%d.poolgrad1' % (stacks - 1), 2), ('res1', 1), ('res1', 3)]
    if res == 256:
        want.append(('res1', 4))          # dz3 as conv3's data gradient stored it (the row-tile launches store it)
    c = dict(B=2, res=res, stacks=stacks, want=want)
    off, on = _train(False, **c), _train(True, **c)
    _compare(off, on)
    for (name, view), (o1, o2), (r1, r2) in zip(want, off['views'], on['views']):
        assert _same(o1, o2) and _same(r1, r2), '%s: a second request returned something else' % name
        assert _same(o1, r1), '%s differs (%d of %d elements)' % (name, int((_bits(o1) != _bits(r1)).sum()), o1.numel())
        assert float(o1.abs().max()) > 0, name
    # the routed gradient is three quarters zero at least: at most one position of a window takes it (level 2: no addend)
    g = on['views'][1][0]
    assert float((g != 0).float().mean()) <= 0.25


def test_chan_512_routes_the_stem_pool_only_and_gives_the_same_bits():
    """The mixed state: 1 stack, chan 512, B 2, 256 x 256.  The hourglass pools cannot be routed -- the skip block's conv1 data gradient has
    256 gradient channels and the plan's pool_route needs 128 (Hourglass::route_ok; asserted below) -- so each level falls back to a pool backward
    launch into poolgrad<k>, although the forward pools still store their arg-max maps; the stem's pool is routed as at every chan
    (residual1 is 64 -> 128).  Every compared tensor is bit-identical, and hg0.poolgrad1..4, which the routed step stored itself here,
    equal what the unrouted step stored."""
    want = [('hg0.poolgrad%d' % k, 2) for k in (1, 2, 3, 4)] + [('res1', 1), ('res1', 3), ('res1', 4)]
    c = dict(B=2, res=256, stacks=1, chan=512, want=want)
    from tests.conv_plan_query import plan, PLAIN, LIN2, POOL, OUT_BWD, DZ, IN_MAP, IN_Q, EP2_AFFINE, ADD2_MAP
    assert not any(plan(2, H, H, 256, 512, 1, in_=LIN2, a1=PLAIN, a2=POOL, ep=OUT_BWD, flags=ADD2_MAP)['pool_route'] for H in (64, 32, 16, 8))
    assert plan(2, 128, 128, 128, 64, 1, in_=POOL, ep=OUT_BWD, flags=DZ | IN_MAP | IN_Q | EP2_AFFINE)['pool_in']
    off, on = _train(False, **c), _train(True, **c)
    # pa_net_design_bytes: Net::stem_route_ok holds at this size whatever the chan -- residual1's conv3 data gradient (128 gradient channels,
    # 64 outputs, 2 * 128 * 128 pixels) is a launch whose plan says pool_in (asserted above), and the pool's statistics
    # launch is planned over 128 channels -- so the routed step skips the write and the re-read of residual1's full-resolution gradient and
    # _compare's STRICT assertion applies (read and written bytes both smaller), as for the cases above; 'not greater' would be the
    # assertion of a size whose stem pool is not routed either (res 128).
    _compare(off, on)
    for (name, view), (o1, o2), (r1, r2) in zip(want, off['views'], on['views']):
        assert _same(o1, o2) and _same(r1, r2), '%s: a second request returned something else' % name
        assert _same(o1, r1), '%s differs (%d of %d elements)' % (name, int((_bits(o1) != _bits(r1)).sum()), o1.numel())
        assert float(o1.abs().max()) > 0, name
    assert float((on['views'][1][0] != 0).float().mean()) <= 0.25          # level 2: no addend, one position of a window at the most


def test_routed_step_stays_inside_its_workspace():
    """The arg-max maps (and the stem pool's arg-max values) live in the workspace pa_net_workspace_bytes sizes: 64 MB guard regions around the workspace of a 2-stack
    pose net (chan 256, 256 x 256, B = 2: every pool routed, the stem's with its arg-max values) stay untouched over a routed forward + backward pass and a request for a routed pool gradient."""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    L = lib()
    B, res, chan = 2, 256, 256
    SL = 64 << 20
    hp = L.pa_hg_create(2, 16, chan, B, res)
    assert hp, L.pa_last_error()
    nws = L.pa_net_workspace_bytes(hp)
    big = torch.zeros(nws + 2 * SL, dtype=torch.uint8, device='cuda')
    big[:SL] = 0x5A; big[SL + nws:] = 0x5A
    P = torch.rand(L.pa_net_param_floats(hp), device='cuda') * 0.1
    G = torch.zeros_like(P)
    Bf = torch.ones(max(1, L.pa_net_buffer_floats(hp)), device='cuda')
    check(L.pa_net_bind(hp, ptr(P), ptr(G), ptr(Bf), C.c_void_p(big.data_ptr() + SL), stream()), 'pa_net_bind')
    check(L.pa_net_set_pool_route(hp, 1), 'pa_net_set_pool_route')
    img = torch.rand(B, 3, res, res, device='cuda')
    pts = (torch.rand(B, 16, 2, device='cuda', dtype=torch.float64) * 60 + 2)
    loss = torch.empty(2, device='cuda')
    check(L.pa_hg_forward(hp, ptr(img), None, ptr(pts), 1, ptr(loss)), 'pa_hg_forward')
    check(L.pa_hg_backward(hp), 'pa_hg_backward')
    shp = (C.c_int * 4)()
    out = torch.empty(B, chan, res // 4, res // 4, device='cuda')
    check(L.pa_hg_debug_tensor(hp, b'hg1.poolgrad1', 2, ptr(out), shp), 'pa_hg_debug_tensor')
    torch.cuda.synchronize()
    assert bool((big[:SL] == 0x5A).all()) and bool((big[SL + nws:] == 0x5A).all())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(G).all()) and bool(torch.isfinite(out).all())
    L.pa_net_destroy(hp)

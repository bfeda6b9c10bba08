"""The convolution instances that run four workgroups per CU (csrc/conv1x1_tile.hip pa_conv1_occ, csrc/conv3x3_tile.hip pa_conv3_occ): the
row-tile 1x1 instances with 64 input channels (64 -> 64 in 128-row tiles, 64 -> 128 in 64-row tiles with 32-channel weight slices) and with
128 -> 64 channels, and the 16 x 8 halo tiles of the 64 -> 64 channel 3x3.  Every load variant of these shapes was fitted into 128 registers
and the variants that paid in the benchmark's kernel trace run at four (DESIGN.md "Four workgroups per CU"; tests/test_kernel_resources_cpu.py
holds their registers); the shared epilogue forms and the 32-channel weight slices were written for that.  Here they compute.

Standalone launches (pa_conv2d, as tests/test_gpu_conv.py drives it: forward with bias, data gradient) against conv2d in float64 on the
rounded operands, at that file's single-layer bound: rel-rms < 4e-3 (one rounding to the storage type, half an ulp 2^-9 ~ 2e-3, plus
accumulation order).  Every case asserts the tiling the planner names for it, so a case cannot drift to another kernel unseen.  The shapes
are the smallest that reach each instance, plus ragged ones (a last row tile that is partly empty: 65 x 63 maps; 72 x 64 at B 3 is a
whole number of tiles).

pa_conv2d loads its operands plain and has the plain epilogue.  The other forms these instances carry in the net -- BatchNorm+ReLU and
BatchNorm-backward (LIN2) loads, the statistics and BatchNorm-backward epilogues, the stored dz, one and two addends, the pool-routed
input -- are reached through one training step of a 1-stack net at B 2, 256 x 256 (residual1's 128 x 128 maps: 256 row tiles of 128, 512
of 64, 256 halo tiles): tests/conv_exact.py recomputes every convolution of that step in float64 from the engine's own operands, element
by element, and the launch log must show each four-workgroup tiling with each of those forms.

Determinism: every standalone launch twice, and the step twice from the same seed -- outputs, gradients and running statistics (which
are sums of the kernels' partial rows) bitwise equal."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_plan_query as Q
from tests import inputs
from tests.test_gpu_conv import rel_rms, run_conv

pytestmark = pytest.mark.gpu

FOUR = ('R64_128_64', 'R64_64_128', 'R128_64_64', 'R128_64_64_PIN', 'T16x8_64_64')

# B, Cin, Cout, H, W, k, tiling of the forward launch, tiling of the data-gradient launch (a GEMM Cout -> Cin)
CASES = [
    (2, 64, 64, 128, 128, 1, 'R64_128_64', 'R64_128_64'),       # 256 row tiles of 128
    (2, 64, 128, 128, 128, 1, 'R64_64_128', 'R128_64_64'),      # 512 row tiles of 64, both ways
    (6, 64, 64, 64, 64, 1, 'R64_128_64', 'R64_128_64'),         # 192 row tiles of 128: the fewest the planner gives these instances
    (6, 64, 128, 64, 64, 1, 'R64_64_128', 'R128_64_64'),
    (1, 128, 64, 128, 128, 1, 'R128_64_64', 'G64x128_1'),       # 256 row tiles of 64 (the data gradient has 64 input channels and too few tiles)
    # 72 x 64 at B 3 is 13824 pixels = 216 full tiles of 64: it reaches the 128 -> 64 instance, unragged; with 64 input channels it is
    # 108 tiles of 128, below the row-tile kernel's 192
    (3, 128, 64, 72, 64, 1, 'R128_64_64', 'G64x64_1'),
    (3, 64, 128, 72, 64, 1, 'G64x64_1', 'R128_64_64'),
    # ragged: 65 x 63 maps.  B 3: 12285 pixels = 191 tiles of 64 and 61 rows; B 6: 24570 = 191 tiles of 128 and 122 rows, 383 of 64 and 58
    (3, 128, 64, 65, 63, 1, 'R128_64_64', 'G64x64_1'),
    (6, 64, 64, 65, 63, 1, 'R64_128_64', 'R64_128_64'),
    (6, 64, 128, 65, 63, 1, 'R64_64_128', 'R128_64_64'),
    (2, 64, 64, 32, 32, 3, 'T16x8_64_64', 'T16x8_64_64'),       # 16 halo tiles: every tile touches the border
    (1, 64, 64, 128, 128, 3, 'T16x8_64_64', 'T16x8_64_64'),     # 128 halo tiles, interior ones too
]
IDS = ['B%d_%dto%d_%dx%d_k%d' % c[:6] for c in CASES]


def _operands(B, Cin, Cout, H, W, k):
    g = inputs.rng(440, B, Cin, Cout, H, W, k)
    x = torch.from_numpy(g.standard_normal((B, Cin, H, W)).astype(np.float32))
    dy = torch.from_numpy(g.standard_normal((B, Cout, H, W)).astype(np.float32))
    w = torch.from_numpy((g.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32))
    bias = torch.from_numpy(g.standard_normal(Cout).astype(np.float32))
    return x, dy, w, bias


def _r(t):
    from pose_adv_aug_amd._lib import act_dtype
    return t.to(act_dtype()).double()


@pytest.mark.parametrize('B,Cin,Cout,H,W,k,fwd,bwd', CASES, ids=IDS)
def test_standalone_launches_match_float64_and_repeat_bitwise(B, Cin, Cout, H, W, k, fwd, bwd):
    assert Q.plan(B, H, W, Cin, Cout, k * k, flags=Q.BIAS)['tiling'] == fwd
    assert Q.plan(B, H, W, Cout, Cin, k * k)['tiling'] == bwd
    x, dy, w, bias = _operands(B, Cin, Cout, H, W, k)
    y, _ = run_conv(0, x, None, w, bias, B, Cin, Cout, H, W, k)
    ref = F.conv2d(_r(x), _r(w), bias.double(), padding=k // 2)
    e = rel_rms(y, ref)
    print('forward rel-rms %.3e' % e)
    assert e < 4e-3
    y2, _ = run_conv(0, x, None, w, bias, B, Cin, Cout, H, W, k)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), 'forward: a second launch gave other bits'
    dx, _ = run_conv(1, dy, None, w, None, B, Cin, Cout, H, W, k)
    ref = F.conv_transpose2d(_r(dy), _r(w), padding=k // 2)
    e = rel_rms(dx, ref)
    print('data gradient rel-rms %.3e' % e)
    assert e < 4e-3
    dx2, _ = run_conv(1, dy, None, w, None, B, Cin, Cout, H, W, k)
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32)), 'data gradient: a second launch gave other bits'


def _logged(body):
    """the distinct convolution launches `body` makes, as pa_conv_plan_describe arguments"""
    L = Q.lib()
    L.pa_conv_launch_log(None, 0)
    try:
        out = body()
    finally:
        buf = (C.c_int * (14 * 1024))()
        n = L.pa_conv_launch_log(buf, 1024)
    return out, [tuple(buf[14 * i:14 * i + 14]) for i in range(n)]


def test_every_form_of_the_four_workgroup_instances_is_exact_in_a_step():
    """1 stack, chan 256, B 2, 256 x 256: every convolution against float64 (tests/conv_exact.py), and the forms that ran."""
    from tests import conv_exact as X
    (worst, fails), launches = _logged(lambda: X.run_leg(1, 256, 2, 256, 47))
    assert not fails, '%d checks outside their bound, first: %s (worst per kind: %s)' % (len(fails), fails[:12], worst)
    cus = Q.device_cus()
    seen = set()
    for a in launches:
        B, H, W, Cin, Cout, taps, in_, a1, a2, ep, ep2, fin, flags, _ = a
        d = Q.describe(Q.lib(), B, H, W, Cin, Cout, taps, in_=in_, a1=a1, a2=a2, ep=ep, ep2=ep2, fin=fin, flags=flags, cus=cus)
        if d['tiling'] in FOUR:
            seen.add((d['tiling'], in_, ep, bool(d['stores_dz']), (a1 != Q.NONE) + (a2 != Q.NONE)))
    print(sorted(seen))
    tilings = {s[0] for s in seen}
    assert tilings == set(FOUR), tilings
    loads = {(s[0], s[1]) for s in seen}
    # residual1 at 128 x 128 (64 -> 128 channels behind the stem's BatchNorm and pool): conv1 64 -> 64 and its data gradient with the adapter's as
    # addend; conv2; conv3 64 -> 128 with the adapter's output as addend, and the adapter itself (plain epilogue); conv3's data gradient with
    # the pool-routed input and the stored dz, the adapter's with plain load and epilogue.  (The unrouted form of conv3's data gradient,
    # <128,64,64,LIN2>, is held bit for bit against the routed one by tests/test_gpu_pool_route.py at this size.)
    for want in (('R64_128_64', Q.BNRELU), ('R64_128_64', Q.LIN2), ('R64_64_128', Q.BNRELU), ('T16x8_64_64', Q.BNRELU), ('T16x8_64_64', Q.LIN2),
                 ('R128_64_64', Q.PLAIN), ('R128_64_64_PIN', Q.POOL)):
        assert want in loads, (want, sorted(loads))
    assert {s[2] for s in seen} >= {Q.OUT_STATS, Q.OUT_BWD}                           # statistics and BatchNorm-backward epilogues
    assert {s[3] for s in seen} == {False, True}                                      # with and without the stored dz
    assert {s[4] for s in seen} >= {0, 1}                                             # with and without an addend


def _step(seed):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    B, res = 2, 256
    net = create_hg(1, 1, 16, 256, res=res, default_batch=B); net.reset_parameters(seed=seed); net.train()
    img = torch.from_numpy(inputs.images(seed + 1, B, res)).cuda()
    pts = torch.from_numpy(inputs.heat_pts(seed + 2, B, res=res // 4)).cuda()
    loss, outs = net.loss_and_backward(img, pts, want_outputs=True)
    torch.cuda.synchronize()
    return [net.flat_grads.clone(), net.flat_buffers.clone()] + [o.clone() for o in outs]


def test_a_step_repeats_bitwise():
    a, b = _step(9), _step(9)
    assert bool(torch.isfinite(a[0]).all()) and float(a[0].abs().max()) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), 'array %d: %d of %d elements differ' % (
            i, int((x.view(torch.int32) != y.view(torch.int32)).sum()), x.numel())

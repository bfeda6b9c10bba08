"""Pose nets with num_modules > 1 on the GPU: every site of an hourglass and post_res is a chain of residual blocks
(pa_hg_create_modules).  The exact legs (tests/modules_exact.py: every conv, BatchNorm, pool, merge and mask of one training step in
float64, block by block), the engine against the reference's own 2-module golden, bitwise reproducibility across runs, stream modes,
the HIP-graph replay and the phased backward pass, the workspace bound, the agent on a 2-module pose net and the state_dict /
checkpoint round trip.

Leg sizes: each is the smallest that reaches what it names (tests/test_gpu_conv_exact.py has the same geometry at one block per site)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as om
from oracle import pylib as opl
from tests import inputs
from tests import modules_exact as MX
from tests.test_gpu_net import cosine, rel_rms, t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leg(*a, **kw):
    worst, fails = MX.run_leg(*a, **kw)
    assert not fails, '%d checks outside their bound, first: %s (worst per kind: %s)' % (len(fails), fails[:12], worst)


def test_two_module_chains_are_exact_on_tiny_maps():
    """2 stacks, 2 modules, chan 128, B 2, 128 x 128: the generic kernels, the 2 x 2 neck, the inner head."""
    _leg(2, 2, 128, 2, 128, 81, stored_expected=('.x2',))


@pytest.mark.parametrize('history', ('fresh', 'warm'))
def test_three_module_chains_are_exact_at_256(history):
    """1 stack, 3 modules, chan 128, B 2, 256 x 256, the first step and the one behind two optimizer steps: the tile kernels, the
    grouped weight gradients, a MIDDLE block of every chain (both neighbours are blocks of the chain)."""
    _leg(1, 3, 128, 2, 256, 82, expect=('group',), history=history)


def test_two_module_chains_are_exact_with_the_fused_upsample_add_backward():
    """1 stack, 2 modules, chan 256, B 12, 256 x 256: the 1 x 1 data gradient with the upsample-add epilogue takes Cin 128 and
    M / 64 >= 192 workgroups (B >= 3 at 64 x 64, B >= 12 at 32 x 32) -- it sits on the FIRST block of up<k> / post and writes the
    gradient of the LAST block of up<k+1>; the split upsample-add backward; the skip chains on the side stream."""
    _leg(1, 2, 256, 12, 256, 83, expect=('group',))


def test_two_module_chains_are_exact_in_a_masked_step():
    """2 stacks, 2 modules, chan 128, B 2, 256 x 256 with occlusion masks: the first block of up4 reads maskedneck, the cell masks read
    and write the last blocks of the skip chains and of the neck."""
    _leg(2, 2, 128, 2, 256, 84, expect=('group',), masks=840)


def test_two_module_chains_are_exact_at_chan_512():
    """1 stack, 2 modules, chan 512, B 2, 128 x 128: block 1 of every chain reads a 512-channel tensor with a pending BatchNorm that has
    two readers and no consumer prologue (PaConvPlan::takes_fin: not above 256 input channels) -- a finalize launch of its own; the generic
    <64,64> kernel at K = 512 / 2304.  Only the stem's 3 x 3 tile launches store a gradient at this size (dz2)."""
    from tests import conv_plan_query as Q
    d = Q.plan(2, 32, 32, 512, 256, 1, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)
    assert not d['takes_fin'] and d['tiling'] == 'G64x64_1' and Q.plan(2, 32, 32, 256, 256, 9, in_=Q.BNRELU, ep=Q.OUT_STATS, flags=Q.BIAS)['tiling'] == 'G64x64_9'
    _leg(1, 2, 512, 2, 128, 90, expect=('group',), stored_expected=('.x2',))


def test_three_module_chains_are_exact_in_the_fp16_build():
    """the 256 x 256 leg in the IEEE-half library, in a child process (one storage type per process)"""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'modules_exact.py'), '1', '3', '128', '2', '256', '85', 'fresh', 'group'],
                       env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 MODULES EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
def _emul_net(net, img):
    """tests/bf16_emul.py emul_hourglass_net for chains: the oracle's modules with the engine's bf16 storage points, emul_residual
    applied per block of every site"""
    from tests import bf16_emul as E

    def chain(seq, a):
        for blk in seq:
            a = E.emul_residual(blk, a)
        return a
    a = torch.relu(E._bn(net.bn1, E.R(E._conv(net.conv1, img))))
    a = E.emul_residual(net.residual1, a)
    a = E.R(F.max_pool2d(a, 2, 2))
    a = E.emul_residual(net.residual3, E.emul_residual(net.residual2, a))
    outs = []
    for i in range(net.num_stacks):
        hg, x, skips = net.hg[i], a, []
        for lvl in (1, 2, 3, 4):
            skips.append(chain(getattr(hg, 'skip%d' % lvl), x))
            x = chain(getattr(hg, 'down%d' % lvl), E.R(F.max_pool2d(x, 2, 2)))
        x = chain(hg.neck, x)
        for lvl in (4, 3, 2, 1):
            x = E.R(F.interpolate(chain(getattr(hg, 'up%d' % lvl), x), scale_factor=2, mode='nearest') + skips[lvl - 1])
        y = chain(net.post_res[i], x)
        l = torch.relu(E._bn(net.linear[i][1], E.R(E._conv(net.linear[i][0], y))))
        heat = E._conv(net.out_conv[i], l)
        outs.append(heat)
        if i < net.num_stacks - 1:
            a = E.R(E._conv(net.in_conv[i], heat) + E.R(E._conv(net.forth_conv[i], l) + a))
    return outs


def test_engine_against_the_reference_two_module_golden_directly():
    """tests/golden/hg_s1m2c128.npz: the REFERENCE's own create_hg(1, 2, 16, 128) (make_modules_goldens.py), B 2, 128 x 128.  Loss 1 %, the
    output layers' gradients 5 % / cosine .998, heat-map PCK equal to the oracle's metric on the engine's maps at 1e-4 -- the bars of
    tests/test_gpu_net.py::test_engine_against_the_reference_golden_directly.  The heat maps of an untrained net amplify every storage
    rounding through twice as many blocks: the bf16-storage emulation of the oracle itself (per block, _emul_net) sits 0.148 rel-rms
    from the fp32 reference for this seed (0.15 - 0.19 for seeds 71 - 73, measured on the CPU), so the 15 % bar of the one-block net does
    not carry over.  The emulation's distance d is computed here and the engine must stay within 1.75 d, the ratio the one-block test
    grants over its own emulation distance (0.15 over 0.080 - 0.085)."""
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'hg_s1m2c128.npz'))
    ref = om.create_hg(1, 2, 16, 128)
    om.deterministic_fill_(ref, seed=72)
    net = create_hg(1, 2, 16, 128, res=128, default_batch=2)
    net.load_state_dict(ref.state_dict())
    assert net.num_params() == int(g['nparams'])
    img = t(inputs.images(172, 2, 128)); pts = inputs.heat_pts(272, 2, res=32)
    heat = t(inputs.heatmaps_from_pts(pts, res=32))
    net.train()
    loss, outs = net.loss_and_backward(img.cuda(), t(pts).cuda(), want_outputs=True)
    ref.train()
    with torch.no_grad():
        d = rel_rms(_emul_net(ref, img)[0], t(g['out'][0]))
    mine = rel_rms(outs[0].cpu(), t(g['out'][0]))
    print('heat maps against the reference golden: bf16-storage emulation %.4f, engine %.4f (bound %.4f)' % (d, mine, 1.75 * d))
    assert abs(float(loss) - float(g['loss'])) / float(g['loss']) < 1e-2
    assert mine <= 1.75 * d, (mine, d)
    idx = [0, 1, 2, 3, 4, 5, 10, 11, 14, 15]
    assert np.allclose(net.accuracy(idx).cpu().numpy(), opl.accuracy(outs[0].cpu(), heat, idx).numpy(), atol=1e-4)
    grads = dict(net.named_grads())
    hg_ = torch.cat([grads[str(n)].flatten().cpu() for n in g['head_names']])
    assert rel_rms(hg_, t(g['head_grads'])) < 5e-2 and cosine(hg_, t(g['head_grads'])) > 0.998


# ---------------------------------------------------------------------------------------------------------------------------------
def _train4(multi=True, graph=False, phased=False, B=3):
    """4 training steps of a 1-stack, 2-module, chan 256 net on two alternating synthetic batches"""
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import RMSprop
    net = create_hg(1, 2, 16, 256, res=256, default_batch=B); net.reset_parameters(seed=4)
    opt = RMSprop(net, lr=2.5e-4); aug = Augmenter(seed=2)
    batches = [DeviceBatch.synthetic(B, seed=60 + k) for k in range(2)]
    net.train()
    _lib.check(_lib.lib().pa_net_set_multi_stream(net._net(B), 1 if multi else 0))
    net.use_graph = graph
    if phased:
        net.on_stack_done = lambda stack: None          # the backward pass goes through pa_hg_backward_phase, phase by phase
    for i in range(4):
        train_step(net, opt, aug, batches[i % 2])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(net.flat_params).all())
    return net.flat_params.clone(), net.flat_buffers.clone(), net.flat_grads.clone()


def test_two_module_training_is_bitwise_the_same_in_every_mode():
    """Every reduction of the engine is order-deterministic, so 4 steps from the same state give the same bits run to run, with the side
    streams on or off (a skip chain's blocks n-1 .. 1 run their whole backward pass on the side stream: a missing event shows here),
    replayed from the captured HIP graph, and with the backward pass enqueued in phases."""
    a = _train4()
    for what, b in (('run to run', _train4()), ('single stream', _train4(multi=False)), ('graph replay', _train4(graph=True)),
                    ('phased backward', _train4(phased=True))):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what


def test_two_module_step_stays_inside_its_workspace():
    """64 MB guard regions around the workspace of a 2-stack, 2-module net (chan 128, B 2, 256 x 256) stay untouched through forward,
    backward and the half forward; hg.<i> stays one contiguous bucket."""
    from pose_adv_aug_amd._lib import lib, check, ptr, stream
    L = lib()
    B, res, chan = 2, 256, 128
    SL = 64 << 20
    h = L.pa_hg_create_modules(2, 2, 16, chan, B, res)
    assert h, L.pa_last_error()
    nws = L.pa_net_workspace_bytes(h)
    big = torch.zeros(nws + 2 * SL, dtype=torch.uint8, device='cuda')
    big[:SL] = 0x5A; big[SL + nws:] = 0x5A
    P = torch.rand(L.pa_net_param_floats(h), device='cuda') * 0.1
    G = torch.zeros_like(P)
    Bf = torch.ones(max(1, L.pa_net_buffer_floats(h)), device='cuda')
    check(L.pa_net_bind(h, ptr(P), ptr(G), ptr(Bf), C.c_void_p(big.data_ptr() + SL), stream()), 'pa_net_bind')
    img = torch.rand(B, 3, res, res, device='cuda')
    pts = (torch.rand(B, 16, 2, device='cuda', dtype=torch.float64) * 60 + 2)
    loss = torch.empty(2, device='cuda')
    check(L.pa_hg_forward(h, ptr(img), None, ptr(pts), 1, ptr(loss)), 'pa_hg_forward')
    check(L.pa_hg_backward(h), 'pa_hg_backward')
    check(L.pa_hg_forward_half(h, ptr(img), None, 1), 'pa_hg_forward_half')
    torch.cuda.synchronize()
    assert bool((big[:SL] == 0x5A).all()) and bool((big[SL + nws:] == 0x5A).all())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(G).all()) and float(G.abs().max()) > 0
    lo, hi = C.c_size_t(), C.c_size_t()
    for i in range(2):
        check(L.pa_hg_bucket_range(h, i, C.byref(lo), C.byref(hi)), 'pa_hg_bucket_range')
        assert lo.value < hi.value <= L.pa_net_param_floats(h)
    assert L.pa_net_num_modules(h) == 2
    L.pa_net_destroy(h)


def test_agent_reads_the_last_blocks_of_a_two_module_pose_net():
    """pa_hg_forward_half + pa_asn_forward + pa_asn_backward over a 2-module pose net: the agent's five input blocks read the pose
    net's skip / neck OUTPUTS (the last block of each chain) -- their convs are exact against those tensors -- and nothing reaches the
    pose net's gradients."""
    from pose_adv_aug_amd._lib import act_dtype
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    from tests import asn_exact as AX
    from tests import bn_exact as BN
    from tests import conv_exact as X
    B, res, chan = 2, 256, 128
    _, net = MX.hg_pair(1, 2, chan, B, res, seed=86)
    agent = create_asn(chan, chan, 7, 7, is_aug=True, res=res, default_batch=B)
    agent.reset_parameters(seed=87)
    net.train(); agent.train()
    net.zero_grad(); agent.zero_grad()
    sd0 = {k: v.clone() for k, v in agent.state_dict().items()}
    ls, lr = net(t(inputs.images(186, B, res)).cuda(), asn=agent, is_half_hg=True, is_aug=True)
    gs, gr = AX._targets(88, ls, lr, B)
    agent.loss_and_backward(gs, gr)
    torch.cuda.synchronize()
    assert float(net.flat_grads.abs().max()) == 0.0
    grads = {n: g.clone() for n, g in agent.named_grads()}
    ck = X.Checker(sd0, grads, act_dtype(), B)
    Pa, Pp = BN.AsnProbe(agent), BN.Probe(net)
    for k in range(5):
        feat = 'hg0.skip%d' % (k + 1) if k < 4 else 'hg0.neck'
        assert torch.equal(Pp.get(feat, 2), Pp.get(feat + '.m1', 2)) and not torch.equal(Pp.get(feat, 2), Pp.get(feat + '.m0', 2))
        ck.block(AX.IN_PREFIX[k], 'in%d' % k, Pa, Pp, feat, input_grad=False)
    assert not ck.fails, (ck.fails[:12], ck.worst)


def test_state_dict_and_checkpoint_round_trip(tmp_path):
    """load_state_dict(oracle.state_dict()) then state_dict() returns every tensor unchanged; a Checkpoint save / load into a fresh
    2-module net reproduces it."""
    import types
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.utils.checkpoint import Checkpoint
    from pose_adv_aug_amd.utils.util import PoseTrainHistory
    ref, net = MX.hg_pair(2, 2, 128, 2, 128, seed=89)
    rsd = ref.state_dict()
    sd = net.state_dict()
    assert list(sd.keys()) == list(rsd.keys())
    for k, v in sd.items():
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(v.cpu(), rsd[k].float()), k
    opt = types.SimpleNamespace(state_dict=lambda: {'state': {}, 'param_groups': [{'lr': 2.5e-4}]}, load_state_dict=lambda sd: None)
    h = PoseTrainHistory()
    h.update({'epoch': 3}, {'lr': 2.5e-4}, {'train_loss': 1., 'val_loss': 1.}, {'train_pckh': .1, 'val_pckh': .2})
    ck = Checkpoint(); ck.save_prefix = str(tmp_path) + '/'
    path = ck.save_checkpoint(net, opt, h, torch.zeros(3, 16, 2))
    net2 = create_hg(2, 2, 16, 128, res=128, default_batch=2)
    net2.reset_parameters(seed=1)
    ck2 = Checkpoint(); ck2.load_prefix = path[:-len('.pth.tar')]
    assert ck2.load_checkpoint(net2)
    sd2 = net2.state_dict()
    assert list(sd2.keys()) == list(sd.keys())
    for k, v in sd.items():
        assert torch.equal(v, sd2[k]), k

"""The engine's two ledgers of a step, pinned number for number (csrc/work_model.h): the design bytes of pa_net_design_bytes (every operand a
launch reads or writes) and the per-class event profile of pa_net_profile_report (launches, algorithmic bytes, flops per PA_PROF_* class) with
its class sequence (pa_net_profile_classes).  tests/golden/work_ledger.json holds what the commit named in it counted, before the formulas
moved out of the launch code; every case here must count the same.  Every term is an integer-valued double far below 2^53, so the sums do not
depend on their order: the comparison is exact equality.

The plans (stored dz, the fused low-resolution half of the upsample-add backward) depend on the device's compute-unit count: the fixture records
it, and a device with another count skips.  POSEADV_WRITE_WORK_LEDGER=<file> makes the cases write a new fixture instead, with the commit
hash given in POSEADV_WORK_LEDGER_COMMIT (not after a change of the launch code: the fixture is the statement of what that change must keep)."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import inputs

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'work_ledger.json')
NCLS = 12                                    # PA_PROF_CLASSES (include/poseadv.h)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


class _Ledger:
    """around ONE pass on handle h: the profile of its launches and the design bytes behind it"""

    def __init__(self, h, profile=True):
        self.h, self.profile = h, profile

    def __enter__(self):
        from pose_adv_aug_amd import _lib
        if self.profile:
            _lib.check(_lib.lib().pa_net_profile_begin(self.h), 'pa_net_profile_begin')
        return self

    def __exit__(self, et, ev, tb):
        from pose_adv_aug_amd import _lib
        L = _lib.lib()
        if et is not None:
            if self.profile:
                L.pa_net_profile_report(self.h, (C.c_double * (4 * 16))(), 16, None)
            return False
        torch.cuda.synchronize()
        d = (C.c_double * 2)()
        _lib.check(L.pa_net_design_bytes(self.h, d), 'pa_net_design_bytes')
        self.got = {'design': [d[0], d[1]]}
        if self.profile:
            rep, n = (C.c_double * (4 * 16))(), C.c_int(0)
            _lib.check(L.pa_net_profile_report(self.h, rep, 16, C.byref(n)), 'pa_net_profile_report')
            assert n.value == NCLS
            # (column 0, the milliseconds, is a measurement: not recorded)
            self.got['classes'] = [[rep[4 * c + 1], rep[4 * c + 2], rep[4 * c + 3]] for c in range(NCLS)]
            k = L.pa_net_profile_classes(self.h, None, 0)
            seq = (C.c_int32 * max(k, 1))()
            L.pa_net_profile_classes(self.h, seq, k)
            self.got['sequence'] = list(seq)[:k]
        return False


def _drop_masks(B):
    m = torch.ones(B, 1, 4, 4)
    g = inputs.rng(91)
    for b in range(B):
        for cell in g.choice(16, 2, replace=False):
            m[b, 0, cell // 4, cell % 4] = 0
    return m.cuda()


def _pose(B, res, chan, stacks, modules=1, route=None, multi=None):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(stacks, modules, 16, chan, res=res, default_batch=B); net.reset_parameters(seed=7); net.train()
    h = net._net(B)
    if route is not None:
        _lib.check(_lib.lib().pa_net_set_pool_route(h, route), 'pa_net_set_pool_route')
    if multi is not None:
        _lib.check(_lib.lib().pa_net_set_multi_stream(h, multi), 'pa_net_set_multi_stream')
    return net, h


def _train(B, res, chan, stacks, modules=1, route=None, multi=None, masks=False, own_grads=False):
    """two eager training steps (no graph: the profiler refuses it), the ledger of the second"""
    from pose_adv_aug_amd.utils.optim import RMSprop
    net, h = _pose(B, res, chan, stacks, modules, route, multi)
    opt = RMSprop(net, lr=2.5e-4)
    pts = torch.from_numpy(inputs.heat_pts(17, B, res=res // 4)).cuda()
    m = _drop_masks(B) if masks else None
    for i in range(2):
        img = torch.from_numpy(inputs.images(30 + i, B, res)).cuda()
        with _Ledger(h, profile=i == 1) as led:
            if own_grads:           # the caller's heat-map gradients (the injection launch) and d loss / d image (the stem's data gradient)
                outs = net(img, pts=pts)
                dimg = net.backward([o * (1.0 / o.numel()) for o in outs], input_grad=True)
                assert dimg is not None and bool(torch.isfinite(dimg).all())
            else:
                net.loss_and_backward(img, pts, dropout_masks=m)
        opt.step()
    return led.got


def _forward_only(B, res, chan, stacks):
    net, h = _pose(B, res, chan, stacks)
    net.eval()
    img = torch.from_numpy(inputs.images(30, B, res)).cuda()
    with _Ledger(h, profile=False) as led:
        net(img)
    return led.got


def _agent(B, res, chan, occlusion):
    """one step of the scale / rotation agent (or of the occlusion agent) on the pose net's detached features: the ledger of the AGENT's handle,
    whose passes reset (Net::begin_step in its forward trunk) and fill the same counters"""
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    net, _ = _pose(B, res, chan, 1)
    net.eval()
    agent = create_asn(chan, chan, 7, 7, is_aug=not occlusion, is_dropout=occlusion, res=res, default_batch=B)
    agent.reset_parameters(seed=8); agent.train()
    img = torch.from_numpy(inputs.images(30, B, res)).cuda()
    with _Ledger(agent._net(B)) as led:
        if occlusion:
            logits = net(img, asn=agent, is_half_hg=True, is_dropout=True)
            agent.backward_masks(torch.softmax(logits.reshape(B, 16), 1).reshape(B, 1, 4, 4) - 1.0 / 16)
        else:
            net(img, asn=agent, is_half_hg=True, is_aug=True)
            t = torch.full((B, 7), 1.0 / 7, device='cuda')
            agent.loss_and_backward(t, t)
    return led.got


CASES = {
    # every convolution in the low classes; hourglass and stem pool routing on
    'b1_res128_chan128_s1': lambda: _train(1, 128, 128, 1),
    # 4 x 64 x 64 = 16384 pixels = PA_PROF_LOW_M: the boundary of the class split; the row-tile data gradient with the fused low-resolution half,
    # stored dz2 / dz3, the inner-stack layers (forth_conv, in_conv, the dheat_in addend)
    'b4_res256_chan256_s2': lambda: _train(4, 256, 256, 2),
    'b4_res256_chan256_s2_route_off': lambda: _train(4, 256, 256, 2, route=0),            # pool backward launches instead of routed loads
    # group launches on the caller's stream, finish_grad2's pair launch, reduce_grads' one reduction, the both-halves upsample-add backward
    'b4_res256_chan256_s2_single_stream': lambda: _train(4, 256, 256, 2, multi=0),
    'b2_res256_chan128_s1_occlusion': lambda: _train(2, 256, 128, 1, masks=True),         # drop_mask: no fused half, no pending x3 finalize
    'b1_res128_chan128_s1_modules2': lambda: _train(1, 128, 128, 1, modules=2),           # chains
    'b1_res128_chan128_s1_own_grads': lambda: _train(1, 128, 128, 1, own_grads=True),     # the stem's data gradient, the injection launch
    'b1_res128_chan128_s1_forward_eval': lambda: _forward_only(1, 128, 128, 1),           # train = 0: design bytes only
    'agent_sr_b2_res256_chan128': lambda: _agent(2, 256, 128, False),
    'agent_occlusion_b2_res256_chan128': lambda: _agent(2, 256, 128, True),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_the_step_counts_what_the_recorded_step_counted(case):
    got = CASES[case]()
    out = os.environ.get('POSEADV_WRITE_WORK_LEDGER')
    if out:
        d = json.load(open(out)) if os.path.isfile(out) else {}
        d.setdefault('commit', os.environ.get('POSEADV_WORK_LEDGER_COMMIT', ''))
        d.setdefault('compute_units', _cus())
        assert d['compute_units'] == _cus()
        d.setdefault('cases', {})[case] = got
        json.dump(d, open(out, 'w'), indent=0, sort_keys=True)
        return
    fx = json.load(open(FIXTURE))
    if fx['compute_units'] != _cus():
        pytest.skip('the fixture was recorded on a device with %d compute units, this one has %d: the convolution plans (stored dz, the fused '
                    'low-resolution half) and with them the ledger differ' % (fx['compute_units'], _cus()))
    want = fx['cases'][case]
    assert sorted(got) == sorted(want)
    assert got['design'] == want['design'], (case, 'design bytes (read, written)', got['design'], want['design'])
    if 'classes' in want:
        for c in range(NCLS):
            assert got['classes'][c] == want['classes'][c], (case, 'class %d (launches, bytes, flops)' % c, got['classes'][c], want['classes'][c])
        assert got['sequence'] == want['sequence'], (case, 'class sequence', len(got['sequence']), len(want['sequence']))

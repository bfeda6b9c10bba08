"""The fused Adam / AdamW step (pa_adam_step: adam_prologue_kernel and adam_kernel), its device-side step count and utils.optim.Adam /
AdamW, against float64, element by element (reference and the derivation of the bounds: tests/adam_exact.py; tests/test_adam_cpu.py
shows which defects the bound excludes and that the reference is torch's formula).

Cases: the sizes of tests/optim_exact.py (tail only, the first vector chunk, 1023, 100 003, 2048 * 256 * 4 + {0, 1, 3, 5}); no / coupled /
decoupled decay x amsgrad, each with and without the clip coefficient; gscale 1, 1/3, 1/32768; three consecutive steps from zero and
from non-zero state; guard elements around every array; the step count and the four constants of the state after every step.  The
constants after pa_adam_set_steps.  Every argument error.  The optimizer classes on the real flat arrays of a pose net and its agent
(padding stays exactly 0), their state_dict against torch.optim.Adam's / AdamW's in both directions, save / load / continue, an RMSprop
file.  The IEEE-half build runs the exact cases, and the skip of a step whose gradient holds inf / NaN (the step count must not
advance), in a child process."""
import copy
import os
import subprocess
import sys
import types
import warnings

import pytest
import torch

from tests import optim_exact as X
from tests import adam_exact as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n', X.SIZES)
def test_adam_step_is_exact(n):
    fails = A.run_case(n)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


def test_set_steps_moves_the_bias_correction():
    fails = A.run_set_steps()
    assert not fails, fails


def test_argument_errors_launch_nothing():
    fails = A.run_error_cases()
    assert not fails, fails


def test_adam_and_adamw_are_exact_on_a_real_flat_array():
    """Adam(amsgrad, weight_decay, max_grad_norm = half the norm) and AdamW on the 2-stack chan-128 pose net and its agent
    (adam_exact.run_flat_array)"""
    fails = A.run_flat_array()
    assert not fails, fails[:12]


def _toy_net(seed=3):
    """the optimizer's view of a net (flat arrays, parameter table) over three small tensors with alignment padding between them"""
    table = [('a.weight', (2, 3, 5), 0, 30, 0), ('a.bias', (3,), 32, 3, 0), ('b.weight', (7, 9), 36, 63, 0), ('bn.running_mean', (3,), 0, 3, 1)]
    g = torch.Generator().manual_seed(seed)
    net = types.SimpleNamespace(flat_params=torch.zeros(100, device='cuda'), flat_grads=torch.zeros(100, device='cuda'), _table=table, _last_B=1,
                                default_batch=1, _ensure_table=lambda: None, weights_changed=lambda: None, _net=lambda B: None)
    for _, shape, off, numel, kind in table[:3]:
        net.flat_params[off:off + numel] = torch.randn(numel, generator=g).cuda()
        net.flat_grads[off:off + numel] = torch.randn(numel, generator=g).cuda()
    return net


def _rows(net):
    return [r for r in net._table if r[4] == 0]


def _torch_twin(net, cls, **kw):
    """torch's optimizer over CPU clones of the toy net's tensors, gradients set"""
    ps = [torch.nn.Parameter(net.flat_params[off:off + numel].view(shape).cpu().clone()) for _, shape, off, numel, _ in _rows(net)]
    _set_grads(net, ps)
    return getattr(torch.optim, cls)(ps, **kw), ps


def _set_grads(net, ps):
    for q, (_, shape, off, numel, _) in zip(ps, _rows(net)):
        q.grad = net.flat_grads[off:off + numel].view(shape).cpu().clone()


def _params_close(net, ps):
    return all(torch.allclose(net.flat_params[off:off + numel].view(shape).cpu(), q.detach(), rtol=1e-5, atol=1e-7)
               for q, (_, shape, off, numel, _) in zip(ps, _rows(net)))


# The C ABI carries the betas as fp32 (pa_adam_opts), and the kernel forms 1.f - beta2 from that: with the literal 0.999 it is
# 0.00099998713 where torch, which rounds the float64 1 - 0.999 instead, multiplies by 0.001 (1.3e-5 apart, relative; beta itself agrees to
# 2^-24).  Both sides get the fp32 values of 0.9 and 0.999 as their betas, the numbers the engine actually works with, as
# tests/test_adam_cpu.py hands the reference's fp32 constants to torch: then the two compute the same formula and 1e-5 is about rounding.
B32 = (X._f32(0.9), X._f32(0.999))
KINDS = (('Adam', dict()), ('Adam', dict(amsgrad=True, weight_decay=1e-4)), ('AdamW', dict()), ('AdamW', dict(amsgrad=True, weight_decay=0.05)))
GROUP_KEYS = ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'decoupled_weight_decay')


@pytest.mark.parametrize('cls,kw', KINDS)
def test_state_dict_is_torchs_in_both_directions(cls, kw):
    """after one step, against torch.optim.Adam / AdamW over CPU clones of the same tensors with the same options (values to fp32
    accuracy: the exact comparison is run_case's); then each file loaded by the other side, and one more step"""
    from pose_adv_aug_amd.utils import optim
    net = _toy_net()
    topt, ps = _torch_twin(net, cls, lr=1e-3, betas=B32, **kw)
    topt.step()
    o = getattr(optim, cls)(net, lr=1e-3, betas=B32, **kw)
    o.step()
    sd, tsd = o.state_dict(), copy.deepcopy(topt.state_dict())            # (torch hands out its live tensors)
    assert sorted(sd) == sorted(tsd) and sorted(sd['state']) == sorted(tsd['state'])
    assert sd['param_groups'][0]['params'] == tsd['param_groups'][0]['params']
    assert set(sd['param_groups'][0]) <= set(tsd['param_groups'][0]) and set(GROUP_KEYS) <= set(sd['param_groups'][0])
    for k in GROUP_KEYS:
        assert sd['param_groups'][0][k] == tsd['param_groups'][0][k], k
    assert type(sd['param_groups'][0]['betas']) is tuple
    defaults, tdefaults = getattr(optim, cls)(_toy_net()).param_groups[0], _torch_twin(net, cls)[0].param_groups[0]
    assert all(defaults[k] == tdefaults[k] for k in GROUP_KEYS), (defaults, tdefaults)
    for i in tsd['state']:
        assert sorted(sd['state'][i]) == sorted(tsd['state'][i]), (sd['state'][i].keys(), tsd['state'][i].keys())
        a, b = sd['state'][i]['step'], tsd['state'][i]['step']
        assert float(a) == float(b) == 1 and a.dtype == b.dtype == torch.float32 and a.shape == b.shape == () and a.device.type == 'cpu'
        for k in tsd['state'][i]:
            if k != 'step':
                a, b = sd['state'][i][k].cpu(), tsd['state'][i][k]
                assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-12), (i, k)
    assert _params_close(net, ps)
    # our file into torch's optimizer, the torch file into ours: the next step of each pair agrees
    t2, ps2 = _torch_twin(net, cls, lr=1e-3, betas=B32, **kw)
    t2.load_state_dict(sd)
    net_b = _toy_net()
    net_b.flat_params.copy_(net.flat_params)
    o2 = getattr(optim, cls)(net_b)                          # the options come from the file's param group
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o2.load_state_dict(tsd)
    assert not w, [str(x.message) for x in w]
    assert o2.steps_taken() == 1 and all(o2.param_groups[0][k] == tsd['param_groups'][0][k] for k in GROUP_KEYS)
    for n_ in (net, net_b):
        n_.flat_grads.mul_(-0.75)
    _set_grads(net, ps)
    _set_grads(net, ps2)
    topt.step(); t2.step(); o.step(); o2.step()
    torch.cuda.synchronize()
    assert _params_close(net, ps) and _params_close(net, ps2) and _params_close(net_b, ps)
    assert float(t2.state_dict()['state'][0]['step']) == 2 and o2.steps_taken() == 2
    # an arbitrary-id keyed file (the reference's torch 0.3 used object ids)
    ids = [1000 + 7 * i for i in range(len(ps))]
    keyed = {'state': dict((ids[i], st) for i, st in tsd['state'].items()), 'param_groups': [dict(tsd['param_groups'][0], params=ids)]}
    o3 = getattr(optim, cls)(_toy_net())
    o3.load_state_dict(keyed)
    assert torch.equal(o3.exp_avg, _flat_of(tsd, net, 'exp_avg')) and o3.steps_taken() == 1


def _flat_of(tsd, net, key):
    """the flat array a torch file's `key` entries give (zeros in the padding)"""
    flat = torch.zeros(100, device='cuda')
    for i, (_, shape, off, numel, _) in enumerate(_rows(net)):
        flat[off:off + numel] = tsd['state'][i][key].reshape(-1).cuda()
    return flat


def test_save_load_continue_gives_the_same_bits(tmp_path):
    from pose_adv_aug_amd.utils.optim import Adam, AdamW, RMSprop
    kw = dict(amsgrad=True, weight_decay=1e-4, max_grad_norm=0.5)
    a_net, b_net = _toy_net(), _toy_net()
    a = Adam(a_net, **kw)
    a.step(); a.step()
    torch.save(a.state_dict(), str(tmp_path / 'opt.pth'))
    b_net.flat_params.copy_(a_net.flat_params)
    b = AdamW(b_net, max_grad_norm=0.5)                       # the options, coupled decay among them, come from the file's param group
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        b.load_state_dict(torch.load(str(tmp_path / 'opt.pth')))
    assert not [x for x in w if 'optimizer state' in str(x.message)], [str(x.message) for x in w]
    assert b.steps_taken() == 2 and b.param_groups[0] == a.param_groups[0] and b.param_groups[0]['decoupled_weight_decay'] is False
    for net in (a_net, b_net):
        net.flat_grads.mul_(-0.75)
    a.step(); b.step()
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int32)
    for x, y in ((a_net.flat_params, b_net.flat_params), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (a.max_exp_avg_sq, b.max_exp_avg_sq)):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(a._state[2:], b._state[2:]) and a.steps_taken() == 3          # the step count and the constants of t = 3
    assert float(a.last_grad_norm()) == float(b.last_grad_norm()) > 0
    # an RMSprop file: exactly one warning, zero moments, step 0, this optimizer's own options
    r = RMSprop(_toy_net(), momentum=0.9)
    r.step()
    c = Adam(_toy_net(), amsgrad=True)
    c.step()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        c.load_state_dict(r.state_dict())
    assert len(w) == 1 and 'square_avg' in str(w[0].message) and 'no exp_avg' in str(w[0].message), [str(x.message) for x in w]
    assert not bool(c.exp_avg.any()) and not bool(c.exp_avg_sq.any()) and not bool(c.max_exp_avg_sq.any()) and c.steps_taken() == 0
    assert c.param_groups[0]['lr'] == 1e-3 and 'alpha' not in c.param_groups[0]


def test_a_changed_param_group_is_applied_at_the_next_step():
    """lr changed and amsgrad switched on between two steps: max_exp_avg_sq appears, the constants follow the new lr, and a third step
    with a much smaller gradient (the maximum is kept) passes the check with amsgrad and fails it without"""
    from pose_adv_aug_amd._lib import grad_scale
    from pose_adv_aug_amd.utils.optim import Adam
    net = _toy_net()
    gscale = 1.0 / grad_scale()
    o = Adam(net, lr=1e-3)
    o.step()
    assert o.max_exp_avg_sq is None
    o.param_groups[0]['lr'] = 4e-4
    o.param_groups[0]['amsgrad'] = True
    o.step()
    torch.cuda.synchronize()
    assert o.max_exp_avg_sq is not None and torch.equal(o.max_exp_avg_sq, o.exp_avg_sq)
    net.flat_grads.mul_(0.01)
    before = {'p': net.flat_params.clone(), 'exp_avg': o.exp_avg.clone(), 'exp_avg_sq': o.exp_avg_sq.clone(), 'max_exp_avg_sq': o.max_exp_avg_sq.clone()}
    o.step()
    torch.cuda.synchronize()
    c = A.read_state(o._state)
    new, old = A.check_consts(c, 3, lr=4e-4), A.check_consts(c, 3, lr=1e-3)
    assert all(x <= 1.0 for x in new.values()), new
    assert not all(x <= 1.0 for x in old.values()), old
    after = {'p': net.flat_params, 'exp_avg': o.exp_avg, 'exp_avg_sq': o.exp_avg_sq, 'max_exp_avg_sq': o.max_exp_avg_sq}
    r, (took, kept) = A.check(before, net.flat_grads, after, gscale, None, c, amsgrad=True, lr=4e-4)
    assert all(x <= 1.0 for x in r.values()) and kept > 0, (r, took, kept)
    no_max = lambda d: dict(d, max_exp_avg_sq=None)
    r0, _ = A.check(no_max(before), net.flat_grads, no_max(after), gscale, None, c, amsgrad=False, lr=4e-4)
    assert not all(x <= 1.0 for x in r0.values()), r0


def test_adam_is_exact_and_skips_in_the_fp16_build():
    """The IEEE-half library: the exact cases above, the flat arrays and the skipped steps (adam_exact.run_skip_case), in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'adam_exact.py')], env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 ADAM EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]

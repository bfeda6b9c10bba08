"""The RMSprop step with momentum, weight decay, centered and a clip coefficient (pa_rmsprop_step_opts), the gradient norm in front of it
(pa_grad_norm) and utils.optim.RMSprop with those options, against float64, element by element (reference and the derivation of the
bounds: tests/optim_opts_exact.py; tests/test_optim_opts_cpu.py shows which defects the bound excludes and that the reference is torch's
formula).

Cases: the sizes of tests/optim_exact.py (tail only, the first vector chunk, 1023, 100 003, 2048 * 256 * 4 + {0, 1, 3, 5}); the eight
option combinations, each with and without the clip coefficient; gscale 1, 1/3, 1/32768; three consecutive steps from zero and from
non-zero state; guard elements around every array.  All options off: the bits of pa_rmsprop_step_state.  The norm: bounds, determinism,
reads and scratch inside their arrays.  Every argument error.  The optimizer class on the real flat arrays of a pose net and its agent
(padding stays exactly 0), its state_dict against torch.optim.RMSprop's, save / load / continue.  The IEEE-half build runs the exact
cases, and the skip of a step whose gradient holds inf / NaN, in a child process."""
import os
import subprocess
import sys
import types
import warnings

import pytest
import torch

from tests import optim_exact as X
from tests import optim_opts_exact as Y

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n', X.SIZES)
def test_rmsprop_step_opts_is_exact(n):
    fails = Y.run_case(n)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


@pytest.mark.parametrize('n', Y.IDENTITY_SIZES)
def test_all_options_off_gives_the_bits_of_the_plain_step(n):
    fails = Y.run_identity(n)
    assert not fails, fails[:12]


@pytest.mark.parametrize('gscale', Y.NORM_GSCALES)
@pytest.mark.parametrize('n', Y.NORM_SIZES)
def test_grad_norm_and_clip_coefficient(n, gscale):
    fails = Y.run_norm_case(n, gscale)
    assert not fails, fails[:12]


def test_argument_errors_launch_nothing():
    fails = Y.run_error_cases()
    assert not fails, fails


def test_optimizer_with_all_options_is_exact_on_a_real_flat_array():
    """RMSprop(net, momentum=0.9, weight_decay=1e-4, centered=True, max_grad_norm=half the norm) on the 2-stack chan-128 pose net and
    its agent (optim_opts_exact.run_flat_array)"""
    fails = Y.run_flat_array()
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


def test_momentum_constructs():
    from pose_adv_aug_amd.utils.optim import RMSprop
    o = RMSprop(_toy_net(), momentum=0.9)
    assert o.param_groups[0]['momentum'] == 0.9 and o.momentum_buffer is not None and o.grad_avg is None and o.last_grad_norm() is None
    with pytest.raises(ValueError):
        RMSprop(_toy_net(), momentum=-0.1)
    with pytest.raises(ValueError):
        RMSprop(_toy_net(), max_grad_norm=0.0)


OPTION_SETS = (dict(momentum=0.9), dict(centered=True), dict(momentum=0.9, weight_decay=1e-4, centered=True))


@pytest.mark.parametrize('kw', OPTION_SETS)
def test_state_dict_has_torchs_keys_and_shapes(kw):
    """after one step, against torch.optim.RMSprop over CPU clones of the same tensors with the same options (values to fp32 accuracy:
    the exact comparison is run_case's)"""
    from pose_adv_aug_amd.utils.optim import RMSprop
    net = _toy_net()
    rows = [r for r in net._table if r[4] == 0]
    ps = [torch.nn.Parameter(net.flat_params[off:off + numel].view(shape).cpu().clone()) for _, shape, off, numel, _ in rows]
    for q, (_, shape, off, numel, _) in zip(ps, rows):
        q.grad = net.flat_grads[off:off + numel].view(shape).cpu().clone()
    topt = torch.optim.RMSprop(ps, lr=2.5e-4, alpha=0.99, eps=1e-8, **kw)
    topt.step()
    o = RMSprop(net, lr=2.5e-4, alpha=0.99, eps=1e-8, **kw)
    o.step()
    sd, tsd = o.state_dict(), topt.state_dict()
    assert sorted(sd) == sorted(tsd) and sorted(sd['state']) == sorted(tsd['state'])
    assert sd['param_groups'][0]['params'] == tsd['param_groups'][0]['params']
    assert set(sd['param_groups'][0]) <= set(tsd['param_groups'][0])
    for k in ('lr', 'alpha', 'eps', 'momentum', 'weight_decay', 'centered'):
        assert sd['param_groups'][0][k] == tsd['param_groups'][0][k], k
    for i in tsd['state']:
        assert sorted(sd['state'][i]) == sorted(tsd['state'][i]), (sd['state'][i].keys(), tsd['state'][i].keys())
        assert int(sd['state'][i]['step']) == int(tsd['state'][i]['step']) == 1
        for k in tsd['state'][i]:
            if k != 'step':
                a, b = sd['state'][i][k].cpu(), tsd['state'][i][k]
                assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-12), (i, k)
    for q, (_, shape, off, numel, _) in zip(ps, rows):
        assert torch.allclose(net.flat_params[off:off + numel].view(shape).cpu(), q.detach(), rtol=1e-5, atol=1e-7)


def test_save_load_continue_gives_the_same_bits(tmp_path):
    from pose_adv_aug_amd.utils.optim import RMSprop
    kw = dict(momentum=0.9, weight_decay=1e-4, centered=True, max_grad_norm=0.5)
    a_net, b_net = _toy_net(), _toy_net()
    a = RMSprop(a_net, **kw)
    a.step(); a.step()
    torch.save(a.state_dict(), str(tmp_path / 'opt.pth'))
    b_net.flat_params.copy_(a_net.flat_params)
    b = RMSprop(b_net, max_grad_norm=0.5)                     # the options come from the file's param group
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        b.load_state_dict(torch.load(str(tmp_path / 'opt.pth')))
    assert not [x for x in w if 'optimizer state' in str(x.message)], [str(x.message) for x in w]
    assert b.steps == 2 and b.param_groups[0]['momentum'] == 0.9 and b.param_groups[0]['centered'] is True
    for net in (a_net, b_net):
        net.flat_grads.mul_(-0.75)
    a.step(); b.step()
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int32)
    for x, y in ((a_net.flat_params, b_net.flat_params), (a.square_avg, b.square_avg), (a.momentum_buffer, b.momentum_buffer), (a.grad_avg, b.grad_avg)):
        assert torch.equal(bits(x), bits(y))
    assert float(a.last_grad_norm()) == float(b.last_grad_norm()) > 0
    # a file written with the options off: loads with a warning, the new state zero
    plain = RMSprop(_toy_net())
    plain.step()
    sd = plain.state_dict()
    sd['param_groups'][0].update(momentum=0.9, centered=True)
    c = RMSprop(_toy_net(), momentum=0.9, centered=True)
    c.momentum_buffer.fill_(1.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        c.load_state_dict(sd)
    assert any('no momentum_buffer' in str(x.message) for x in w) and any('no grad_avg' in str(x.message) for x in w)
    assert not bool(c.momentum_buffer.any()) and not bool(c.grad_avg.any()) and torch.equal(c.square_avg, plain.square_avg)


def test_a_changed_param_group_is_applied_at_the_next_step():
    """weight_decay switched on between two steps: the second step is pa_rmsprop_step_opts with the new value"""
    from pose_adv_aug_amd.utils.optim import RMSprop
    net = _toy_net()
    o = RMSprop(net)
    o.step()
    o.param_groups[0]['weight_decay'] = 1e-4
    before = {'p': net.flat_params.clone(), 'square_avg': o.square_avg.clone(), 'momentum_buffer': None, 'grad_avg': None}
    o.step()
    torch.cuda.synchronize()
    after = {'p': net.flat_params, 'square_avg': o.square_avg, 'momentum_buffer': None, 'grad_avg': None}
    r, _ = Y.check(before, net.flat_grads, after, 1.0 / __import__('pose_adv_aug_amd')._lib.grad_scale(), None, 0.0, 1e-4, False)
    assert all(x <= 1.0 for x in r.values()), r
    r0, _ = Y.check(before, net.flat_grads, after, 1.0 / __import__('pose_adv_aug_amd')._lib.grad_scale(), None, 0.0, 0.0, False)
    assert not all(x <= 1.0 for x in r0.values()), r0


def test_the_options_are_exact_and_skip_in_the_fp16_build():
    """The IEEE-half library: the exact cases above and the skipped steps (optim_opts_exact.run_skip_case), in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'optim_opts_exact.py')], env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 OPTIM OPTS EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]

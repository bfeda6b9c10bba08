"""Parameter groups in the fused optimizer steps, on the device (pa_rmsprop_step_groups, pa_adam_step_groups, pa_grad_norm_groups and
utils.optim's `groups`): cases, references and bounds in tests/groups_exact.py; tests/test_groups_cpu.py shows which defects the
per-group check excludes.

Sizes: those of tests/optim_exact.py (the tail only, the first vector chunk, 1023, 100 003, 2048 * 256 * 4 + {0, 1, 3, 5}).  Layouts: one
group (bit for bit the ungrouped call), chunk c in group c % 16, contiguous runs with boundaries at the wave and workgroup edges and
the tail.  Three consecutive steps from zero and from non-zero state, gscale 1, 1/3, 1/32768, with and without the clip coefficient;
frozen chunks bit-identical with inf / NaN in their gradient; Adam's per-group constants; the norm over the live groups.  Then the
optimizer classes: against torch.optim with the same param_groups on a toy net, files in both directions; and on a real pose net and
its agent with the command line's groups, the weight EMA behind the step and an accumulated group.  The IEEE-half build runs the
exact cases, and the skip of a whole step for a non-finite value in a FROZEN chunk, in child processes.  Two ranks (the launcher and
records of tests/dist_optim_exact.py): groups with an EMA and with accumulation, against one process accumulating both shards; the
overlapped exchange with groups against the single all-reduce."""
import copy
import os
import subprocess
import sys
import types
import warnings

import pytest
import torch

from tests import optim_exact as X
from tests import optim_opts_exact as Y
from tests import groups_exact as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n', X.SIZES)
@pytest.mark.parametrize('kind', ('rmsprop', 'adam'))
def test_one_group_is_the_ungrouped_call_bit_for_bit(kind, n):
    fails = G.run_one_group(kind, n)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:8])


@pytest.mark.parametrize('n', X.SIZES)
@pytest.mark.parametrize('name', ('mod16', 'runs'))
@pytest.mark.parametrize('kind', ('rmsprop', 'adam'))
def test_every_group_is_exact_and_frozen_chunks_are_untouched(kind, name, n):
    fails = G.run_groups(kind, n, name)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:8])


@pytest.mark.parametrize('n', Y.NORM_SIZES)
@pytest.mark.parametrize('name', G.LAYOUTS)
def test_the_norm_over_the_live_groups_is_the_norm_of_the_zeroed_gradient(name, n):
    fails = G.run_norm(n, name)
    assert not fails, fails[:8]


def test_set_steps_moves_every_groups_constant():
    fails = G.run_set_steps()
    assert not fails, fails


FP16_RUNS = [(kind,) + tuple(str(n) for n in sizes) for kind in ('rmsprop', 'adam') for sizes in (X.SIZES[:8],) + tuple((n,) for n in X.SIZES[8:])] + [('rest',)]


@pytest.mark.parametrize('args', FP16_RUNS, ids=lambda a: '-'.join(a[:2]) + ('..' if len(a) > 2 else ''))
def test_groups_are_exact_and_a_frozen_overflow_skips_the_step_in_the_fp16_build(args):
    """The IEEE-half library in child processes (one storage type per process), a few seconds each: the exact cases above for one
    optimizer at the sizes below one grid pass, at each size beyond it, and ('rest') a non-finite value in a frozen chunk
    (run_frozen_skip), the norm and set_steps."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'groups_exact.py')] + list(args), env=env, capture_output=True, text=True, timeout=300)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 GROUPS EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# against torch.optim with the same param_groups (the toy net of tests/test_gpu_adam.py, rebuilt here with a fourth tensor)
TABLE = [('a.weight', (2, 3, 5), 0, 30, 0), ('a.bias', (3,), 32, 3, 0), ('b.weight', (7, 9), 36, 63, 0), ('b.bias', (7,), 100, 7, 0),
         ('bn.running_mean', (3,), 0, 3, 1)]
B32 = (X._f32(0.9), X._f32(0.999))          # fp32 betas on both sides, as in tests/test_gpu_adam.py
SPECS = lambda: [dict(params=r'^a\.', frozen=True), dict(params=r'bias$', lr=3e-4, weight_decay=0.0)]
OWNERS = [[2], [0, 1], [3]]                 # default group, the frozen one, the biases that are left
TWINS = (('RMSprop', dict(lr=1e-3, alpha=0.99, eps=1e-8, momentum=0.9, centered=True, weight_decay=1e-4)),
         ('Adam', dict(lr=1e-3, betas=B32, weight_decay=1e-4, amsgrad=True)), ('AdamW', dict(lr=1e-3, betas=B32, weight_decay=0.05)))


def _toy_net(seed=3):
    g = torch.Generator().manual_seed(seed)
    net = types.SimpleNamespace(flat_params=torch.zeros(108, device='cuda'), flat_grads=torch.zeros(108, device='cuda'), _table=TABLE, _last_B=1,
                                default_batch=1, _ensure_table=lambda: None, weights_changed=lambda: None, _net=lambda B: None)
    for _, shape, off, numel, kind in TABLE[:4]:
        net.flat_params[off:off + numel] = torch.randn(numel, generator=g).cuda()
        net.flat_grads[off:off + numel] = torch.randn(numel, generator=g).cuda()
    return net


def _torch_twin(net, cls, kw):
    ps = [torch.nn.Parameter(net.flat_params[off:off + numel].view(shape).cpu().clone()) for _, shape, off, numel, _ in TABLE[:4]]
    for i in OWNERS[1]:
        ps[i].requires_grad_(False)
    groups = [dict(params=[ps[i] for i in OWNERS[0]]), dict(params=[ps[i] for i in OWNERS[1]]),
              dict(params=[ps[i] for i in OWNERS[2]], lr=3e-4, weight_decay=0.0)]
    return getattr(torch.optim, cls)(groups, **kw), ps


def _set_grads(net, ps):
    for q, (_, shape, off, numel, _) in zip(ps, TABLE[:4]):
        q.grad = net.flat_grads[off:off + numel].view(shape).cpu().clone() if q.requires_grad else None


def _close(net, ps):
    return all(torch.allclose(net.flat_params[off:off + numel].view(shape).cpu(), q.detach(), rtol=1e-5, atol=1e-7)
               for q, (_, shape, off, numel, _) in zip(ps, TABLE[:4]))


@pytest.mark.parametrize('cls,kw', TWINS)
def test_three_groups_one_frozen_against_torch(cls, kw):
    from pose_adv_aug_amd.utils import optim
    net = _toy_net()
    p0 = net.flat_params.clone()
    topt, ps = _torch_twin(net, cls, kw)
    o = getattr(optim, cls)(net, groups=SPECS(), **kw)
    assert [g['params'] for g in o.param_groups] == OWNERS
    for k in range(3):
        _set_grads(net, ps)
        topt.step()
        o.step()
        torch.cuda.synchronize()
        assert _close(net, ps), k
        net.flat_grads.mul_(-0.75)
    frozen = torch.zeros(108, dtype=torch.bool, device='cuda')
    frozen[:36] = True
    assert torch.equal(net.flat_params[frozen].view(torch.int32), p0[frozen].view(torch.int32))
    assert not bool((net.flat_params[36:99] == p0[36:99]).any()) and not bool(net.flat_params[99:100].any())          # padding
    sd, tsd = o.state_dict(), copy.deepcopy(topt.state_dict())
    assert [g['params'] for g in sd['param_groups']] == OWNERS and sorted(sd['state']) == [0, 1, 2, 3]
    assert [g['params'] for g in tsd['param_groups']] == [[0], [1, 2], [3]]          # torch numbers in chained group order
    for g, tg in zip(sd['param_groups'], tsd['param_groups']):
        assert g['lr'] == tg['lr'] and g['weight_decay'] == tg['weight_decay']
    # our file into torch's optimizer and torch's into ours, then one more step of each pair
    t2, ps2 = _torch_twin(net, cls, kw)
    for q, src in zip(ps2, ps):
        q.data.copy_(src.data)
    ours_for_torch = {'state': dict((j, sd['state'][i]) for j, i in enumerate(i for own in OWNERS for i in own) if i not in OWNERS[1]),
                      'param_groups': [dict((k, v) for k, v in g.items() if k not in ('names', 'frozen', 'lr_mult')) for g in sd['param_groups']]}
    pos = dict((i, j) for j, i in enumerate(i for own in OWNERS for i in own))
    for g in ours_for_torch['param_groups']:
        g['params'] = [pos[i] for i in g['params']]
    t2.load_state_dict(ours_for_torch)
    net_b = _toy_net()
    net_b.flat_params.copy_(net.flat_params)
    net_b.flat_grads.copy_(net.flat_grads)
    o2 = getattr(optim, cls)(net_b, groups=SPECS(), **dict(kw, lr=7.0))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o2.load_state_dict(tsd)
    assert not w, [str(x.message) for x in w]
    assert [g['lr'] for g in o2.param_groups] == [1e-3, 1e-3, 3e-4] and [g['frozen'] for g in o2.param_groups] == [False, True, False]
    _set_grads(net, ps)
    _set_grads(net, ps2)
    topt.step(); t2.step(); o.step(); o2.step()
    torch.cuda.synchronize()
    assert _close(net, ps) and _close(net, ps2) and _close(net_b, ps)
    assert torch.equal(net_b.flat_params[frozen].view(torch.int32), p0[frozen].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# a real net: the smallest the engine builds (2 stacks, chan 128, res 64, B 1) with the command line's groups, the EMA behind the step and
# an accumulated group; then the agent, which the engine builds for 256 <= res only, on a pose net of that size
def _real_nets(res, with_agent):
    """the 2-stack chan-128 pose net at B 1 (res 64: the smallest the engine builds), and on request the scale / rotation agent on it,
    which the engine builds for 256 <= res only"""
    from pose_adv_aug_amd.models.asn_stacked_hg import create_asn
    from tests.test_gpu_net import _hg_pair
    chan, B = 128, 1
    ref, net = _hg_pair(2, chan, B, res, seed=71)
    del ref
    agent = None
    if with_agent:
        agent = create_asn(chan, chan, 7, 7, is_aug=True, res=res, default_batch=B)
        agent.reset_parameters(seed=72)
    return net, agent, B


def _backward(net, agent, B, res, seed):
    from tests import inputs
    from tests.asn_exact import _targets
    from tests.test_gpu_net import t
    img = t(inputs.images(seed, B, res)).cuda()
    net.train()
    if agent is not None:
        agent.train()
        ls, lr = net(img, asn=agent, is_half_hg=True, is_aug=True)
        gs_t, gr_t = _targets(seed + 2, ls, lr, B)
        agent.zero_grad()
        agent.loss_and_backward(gs_t, gr_t)
    net.loss_and_backward(img, t(inputs.heat_pts(seed + 1, B, res=res // 4)).cuda())


def _check_real_step(o, before, g, gscale, coef, fails, what):
    """every group of optimizer o against float64 from the engine's own flat arrays before and after; padding 0; frozen bit-identical"""
    from tests import adam_exact as A
    mod = o.net
    n = mod.flat_params.numel()
    groups = [(float(g_['lr']), float(g_['weight_decay']), bool(g_['frozen'])) for g_ in o.param_groups]
    eg = G.elem_groups(o._map, n).long()
    used = torch.zeros(n, dtype=torch.bool, device='cuda')
    for _, _, off, numel, kind in mod._table:
        if kind == 0:
            used[off:off + numel] = True
    after = {'p': mod.flat_params, 'exp_avg': o.exp_avg, 'exp_avg_sq': o.exp_avg_sq, 'max_exp_avg_sq': None}
    c, gc = A.read_state(o._state), o._group_consts[:len(groups)].cpu()
    for key, x in G.check_group_consts(c, gc, groups, c['step']).items():
        if not (x <= 1.0):
            fails.append(('%s: %s of the constants' % (what, key), x))
    gs = g.double() * X._f32(gscale) * (1.0 if coef is None else coef)
    dom = used & ((gs == 0) | (gs.abs() >= X.DOMAIN)) & ((g == 0) | ((g.double() * X._f32(gscale)).abs() >= X.DOMAIN))
    # and the moments are normal numbers or 0, before and after: the bound's rounding model is relative (tests/optim_exact.py, DOMAIN).  An
    # element whose earlier gradient lay below the domain carries moments of a few units of 2^-149, where 0.9 m rounds to m itself
    dom = dom & G.normal_or_zero(before['exp_avg'], before['exp_avg_sq'], o.exp_avg, o.exp_avg_sq)
    frozen_e = torch.tensor([g_[2] for g_ in groups], device='cuda')[eg]
    dom = dom | (frozen_e & used)                       # a frozen element is compared bit for bit whatever its gradient
    if float(dom[used].float().mean()) < 0.9:
        fails.append(('%s: less than 90 %% of the real gradient is in the bound\'s domain' % what, float(dom[used].float().mean())))
    sel = lambda d: dict((k, None if a is None else a[dom]) for k, a in d.items())
    r = G.check_groups('adam', sel(before), g[dom], sel(after), gscale, coef, (True, False), eg[dom], groups, c, gc)
    for key, x in r.items():
        if not (x <= 1.0):
            fails.append(('%s: group %d %s' % (what, key[0], key[1]), x))
    if set(k for k, _ in r) != set(range(len(groups))):
        fails.append(('%s: groups checked' % what, sorted(set(k for k, _ in r))))
    for name, a in after.items():
        if a is not None and bool((a[~used] != 0).any()):
            fails.append(('%s: padding of %s not zero' % (what, name), 0))
        if a is not None and not bool(torch.isfinite(a).all()):
            fails.append(('%s: non-finite value in %s' % (what, name), 0))


def test_a_real_net_with_the_command_lines_groups_ema_and_accumulation(tmp_path):
    """Two real loss_and_backward() + step() + ModelEma.update() and one accumulated group of two, AdamW with --no_decay_1d, --freeze and
    --lr_group; every group against float64 from the engine's own arrays, frozen tensors of the net and of the EMA twin bit-identical,
    padding 0, last_grad_norm() over the trainable groups; then the agent's optimizer (--no_decay_1d only).
    The domain of the bound (_check_real_step): the gradient as in adam_exact._check_flat, and moments that are normal numbers or 0.  On
    this small net a few hundred elements have a first-step gradient around 1e-44 (below the domain, so not checked at that step) and
    from then on carry exp_avg of 1 to 4 units of 2^-149 with exp_avg_sq 0.  At the next step their gradient is exactly 0, 0.9 m rounds to
    m itself in subnormal arithmetic, and the relative rounding model of the bound (u |m|) calls that an error of 0.1 / (1.1 u) =
    1.5e6 bounds; the kernel's result is the correctly rounded one.  Measured: 280 such elements at step 2, 278 of them with gradient 0,
    of 27 797 elements with gradient 0 and non-zero exp_avg, all others moved."""
    from pose_adv_aug_amd._lib import grad_scale
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils import optim
    res = 64
    net, _, B = _real_nets(res, False)
    opt = TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'e', '--optimizer', 'adamw', '--weight_decay', '0.01', '--no_decay_1d', '1',
                                '--freeze', r'^(conv1|bn1|residual[123])\.', '--lr_group', r'hg\.1\.:0.1', '--clip_grad_norm', '0.05'])
    o = optim.make_optimizer(opt, net, 1e-3)
    assert [g['frozen'] for g in o.param_groups] == [False, True, False, False, False]
    assert [g['weight_decay'] for g in o.param_groups] == [0.01, 0.01, 0.0, 0.01, 0.0] and [g['lr_mult'] for g in o.param_groups] == [1.0, 1.0, 0.1, 0.1, 1.0]
    shapes = dict((t[0], t[1]) for t in net._table)
    assert all(len(shapes[n]) <= 1 for k in (2, 4) for n in o.param_groups[k]['names']) and all(len(shapes[n]) > 1 for k in (0, 3) for n in o.param_groups[k]['names'])
    assert all(g['names'] for g in o.param_groups)
    ema = optim.ModelEma(net, decay=0.9)
    loaded = net.flat_params.clone()
    n = net.flat_params.numel()
    eg = G.elem_groups(o._map, n).long()
    frozen_e = eg == 1
    assert bool(frozen_e.any())
    fails = []
    gscale = 1.0 / grad_scale()

    def stepped(opt_, tag, what, micro, backward):
        """`micro` backward passes (all but the last accumulated), then opt_.step(), checked per group; returns the gradient it applied"""
        for k in range(micro):
            backward(171 + 10 * k + len(what))
            if k < micro - 1:
                opt_.accumulate()
        mod = opt_.net
        g = mod.flat_grads.clone() if micro == 1 else opt_._acc + mod.flat_grads
        before = {'p': mod.flat_params.clone(), 'exp_avg': opt_.exp_avg.clone(), 'exp_avg_sq': opt_.exp_avg_sq.clone(), 'max_exp_avg_sq': None}
        opt_.step()
        torch.cuda.synchronize()
        _check_real_step(opt_, before, g, gscale / micro, float(opt_._norm_out[1]), fails, '%s, %s' % (tag, what))
        return g

    def step(what, micro=1):
        g = stepped(o, 'the pose net', what, micro, lambda seed: _backward(net, None, B, res, seed))
        live = torch.where(frozen_e, torch.zeros_like(g), g)            # last_grad_norm(): the norm over the trainable groups
        norm = float(((live.double() * X._f32(gscale / micro)) ** 2).sum().sqrt())
        if abs(float(o.last_grad_norm()) - norm) > 4 * 2.0 ** -24 * norm:
            fails.append(('last_grad_norm() %s' % what, (float(o.last_grad_norm()), norm)))
        ema.update(o)
        torch.cuda.synchronize()
        bits = lambda a: a[frozen_e].view(torch.int32)
        if not torch.equal(bits(net.flat_params), bits(loaded)):
            fails.append(('frozen tensors of the net moved: ' + what, 0))
        if not torch.equal(bits(ema.module.flat_params), bits(loaded)):
            fails.append(('frozen tensors of the EMA twin moved: ' + what, 0))
        if bool((ema.module.flat_params[~frozen_e] == net.flat_params[~frozen_e]).all()):
            fails.append(('the EMA twin did not average: ' + what, 0))

    step('step 1')
    step('step 2')
    step('an accumulated group of two', micro=2)
    assert o.steps_taken() == 3 and ema.updates() == 3
    assert not fails, fails[:12]
    # the agent (--no_decay_1d only; its flat array has alignment padding), on a pose net of the smallest size the agent is built for
    res_a = 256
    net_a, agent, B = _real_nets(res_a, True)
    oa = optim.make_optimizer(opt, agent, 1e-3)
    assert [g['frozen'] for g in oa.param_groups] == [False, False] and [g['weight_decay'] for g in oa.param_groups] == [0.01, 0.0]
    assert all(len(t[1]) <= 1 for t in agent._table if t[0] in oa.param_groups[1]['names']) and oa.param_groups[1]['names']
    for what, micro in (('agent step 1', 1), ('agent step 2', 1), ('an accumulated agent group of two', 2)):
        stepped(oa, 'the agent', what, micro, lambda seed: _backward(net_a, agent, B, res_a, seed))
    assert oa.steps_taken() == 3
    assert not fails, fails[:12]


# ---------------------------------------------------------------------------------------------------------------------------------
# two ranks (the launcher, the records and the skip condition of tests/test_gpu_dist_optim.py; tests/dist_optim_exact.py)
two_ranks = pytest.mark.skipif(os.environ.get('POSEADV_TEST_DIST_BACKEND') == 'nccl' and torch.cuda.device_count() < 2,
                               reason='two ranks over RCCL need two GPUs (a GPU holds one RCCL rank)')


def _dist_specs():
    from pose_adv_aug_amd.utils.optim import no_decay_1d
    return [dict(params=r'^(conv1|bn1)\.', frozen=True), dict(params=no_decay_1d, weight_decay=0.0), dict(params=r'^hg\.0\.', lr_mult=0.1)]


def _check_dist_groups(c, recs):
    """What groups add to a two-rank record: every group of every step against float64 with gscale = 1 / (2 N) from the EXCHANGED gradient
    (check_groups; Adam's step sizes are fp32(lr_k) / the engine's bc1, one correctly rounded division on either side), the frozen
    tensors of the net and of the EMA twin bit-identical to the start weights although their summed gradient is not zero."""
    import numpy as np
    from tests import dist_optim_exact as D
    net = D.make_net(c, 0)
    o = D.make_opt(c, net)
    n = net.flat_params.numel()
    groups = [(float(g['lr']), float(g['weight_decay']), bool(g['frozen'])) for g in o.param_groups]
    eg = G.elem_groups(o._map, n).long().cpu()
    frozen_e = torch.tensor([g[2] for g in groups])[eg]
    adam = hasattr(o, 'exp_avg')
    names = ({'p': 'flat_params', 'exp_avg': 'exp_avg', 'exp_avg_sq': 'exp_avg_sq', 'max_exp_avg_sq': 'max_exp_avg_sq'} if adam else
             {'p': 'flat_params', 'square_avg': 'square_avg', 'momentum_buffer': 'momentum_buffer', 'grad_avg': 'grad_avg'})
    opts = (bool(o.param_groups[0]['decoupled_weight_decay']), bool(o.param_groups[0]['amsgrad'])) if adam else \
        (float(o.param_groups[0]['momentum']), bool(o.param_groups[0]['centered']))
    del net, o
    fails = []
    rec = recs[0]                                      # (rank 1 holds the same bits: check_replicas)
    bits = lambda a: a[frozen_e].contiguous().view(torch.int32)
    for t, st in enumerate(rec['steps']):
        what = '%s step %d' % (c['name'], t)
        g, gscale = D._g_of(st), D.expected_gscale(rec, st)
        b, a = st['before'], st['after']
        if not torch.equal(bits(a['flat_params']), bits(rec['start'])):
            fails.append((what + ': frozen tensors moved', 0))
        if not bool((g[frozen_e] != 0).any()):
            fails.append((what + ': the frozen tensors received no gradient', 0))
        if st['ema'] is not None and not torch.equal(bits(st['ema']['p1']), bits(rec['start'])):
            fails.append((what + ': frozen tensors of the EMA twin moved', 0))
        sel = lambda d, dom: dict((k, d[nm][dom] if nm in d else None) for k, nm in names.items())
        gs = g.double() * X._f32(gscale)
        every = [d[nm] for d in (b, a) for k, nm in names.items() if nm in d and k != 'p']
        dom = (((gs == 0) | (gs.abs() >= X.DOMAIN)) & G.normal_or_zero(*every)) | frozen_e
        if float(dom.float().mean()) < 0.9:
            fails.append((what + ': less than 90 % of the gradient is in the bound\'s domain', float(dom.float().mean())))
        consts = gc = None
        if adam:
            consts = st['adam']
            gc = torch.tensor([float(np.float32(lr) / np.float32(consts['bc1'])) for lr, _, _ in groups])
            for key, x in G.check_group_consts(consts, gc, groups, t + 1).items():
                if not (x <= 1.0):
                    fails.append(('%s: %s of the constants' % (what, key), x))
        r = G.check_groups('adam' if adam else 'rmsprop', sel(b, dom), g[dom], sel(a, dom), gscale, None, opts, eg[dom], groups, consts, gc)
        if set(k for k, _ in r) != set(range(len(groups))):
            fails.append((what + ': groups checked', sorted(set(k for k, _ in r))))
        for key, x in r.items():
            if not (x <= 1.0):
                fails.append(('%s: group %d %s' % (what, key[0], key[1]), x))
    return fails


@two_ranks
def test_groups_on_two_ranks_are_one_process_accumulating_both_shards():
    """AdamW with a frozen, a no-decay and a 0.1 x group and an EMA, and RMSprop(momentum) with the same groups over N = 2 micro-batches:
    replicas identical, ONE exchange of the whole flat gradient per step (frozen tensors included), every group in float64 from the
    exchanged gradient, frozen tensors of the net and of the twin untouched; the first case bit for bit one process that accumulates
    the two shards."""
    from tests import dist_optim_exact as D
    cases = [D.case('adamw_groups_ema', 'AdamW', kw=dict(groups=_dist_specs()), ema=dict(decay=0.9)),
             D.case('rmsprop_groups_accum2', kw=dict(momentum=0.9, weight_decay=1e-4, groups=_dist_specs()), N=2)]
    seen = []
    for c, recs in D.run_ranks(list(cases)):
        out = [('replicas', D.check_replicas(recs)), ('exchange', D.check_exchange(recs)), ('accumulation', [f for r in recs for f in D.check_accum(r)]),
               ('skipped steps', D.check_skips(recs)), ('groups', _check_dist_groups(c, recs))]
        if c['N'] == 1:
            out.append(('one process accumulating both shards', D.check_same_run(recs[0], D.run_single(c), 'two ranks against one process')))
        bad = [(c['name'], name, fails[:6]) for name, fails in out if fails]
        assert not bad, bad
        assert recs[0]['final']['skipped'] == 0
        seen.append(c['name'])
    assert seen == [c['name'] for c in cases]


@two_ranks
def test_the_overlapped_exchange_with_groups_is_the_single_all_reduce():
    """Adam(overlap=True) and RMSprop(overlap=True, momentum) with the groups above on the 2-stack net: parameters, buffers and state bit
    for bit those of overlap=False on both ranks, 2 asynchronous buckets per step, every gradient exchanged once, frozen tensors untouched."""
    from tests import dist_optim_exact as D
    big = dict(stacks=2, res=256)
    kinds = (('adam', dict(opt='Adam', kw=dict(groups=_dist_specs()))), ('rmsprop', dict(kw=dict(momentum=0.9, groups=_dist_specs()))))
    cases = [D.case('%s_groups_%s' % (kind, how), overlap=how == 'overlap', **dict(kw, **big)) for kind, kw in kinds for how in ('plain', 'overlap')]
    seen = {}
    for c, recs in D.run_ranks(list(cases)):
        out = [('replicas', D.check_replicas(recs)), ('skipped steps', D.check_skips(recs))]
        out.append(('buckets', [f for r in recs for f in D.check_buckets(r)]) if c['overlap'] else ('exchange', D.check_exchange(recs)))
        bad = [(c['name'], name, fails[:6]) for name, fails in out if fails]
        assert not bad, bad
        seen[c['name']] = [dict(case=r['case'], rank=r['rank'], start=r['start'],
                                steps=[dict(after=st['after'], norm_out=st['norm_out'], adam=st['adam']) for st in r['steps']]) for r in recs]
    for kind, _ in kinds:
        for rank in (0, 1):
            a, b = seen[kind + '_groups_overlap'][rank], seen[kind + '_groups_plain'][rank]
            fails = D.check_same_run(a, b, '%s rank %d: overlap=True against overlap=False' % (kind, rank), buffers=True)
            assert not fails, fails[:8]
            assert D._differ(a['steps'][-1]['after']['flat_params'], a['start']) > 0

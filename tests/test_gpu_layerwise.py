"""SGD, LARS and LAMB on the device (csrc/opt_layerwise.hip: pa_lamb_step, pa_lars_step, pa_tensor_norms; utils.optim.SGD / LARS / LAMB), against
float64 element by element.  The references, the bounds and the synthetic table (tensors of 1 .. 7 S floats with 0 / 4 / 12 floats of
padding, one all-zero tensor, one with a zero gradient) are tests/layerwise_exact.py's; tests/test_layerwise_cpu.py shows that the oracles
are torch.optim.SGD's and torch.optim.AdamW's formulas.

Cases: LAMB over three steps with and without a clip coefficient, gscale 1, 1/3, 1/32768, wd 0 / 0.01, max_trust 0 / 1, from zero and non-zero
state; LARS / SGD with momentum 0 / 0.9, Nesterov, wd 0 / 1e-4, trust_coefficient 0 / 1e-3, and torch.optim.SGD itself on a twin; the norms
and ratios on their own; pa_tensor_norms; 16 interleaved groups; a frozen group with inf / NaN in its gradient; determinism and
independence of the layout; every argument error; the optimizer classes on a real net under the command line's groups with the EMA,
accumulation and state_dict round trips; the IEEE-half build (exact cases and the skipped step) in a child process."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

from tests import layerwise_exact as LW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lamb_is_exact_on_the_synthetic_table():
    fails = LW.run_lamb()
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


def test_lars_and_sgd_are_exact_and_sgd_is_torchs():
    fails = LW.run_lars()
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


def test_tensor_norms_on_the_table_and_on_one_tensor():
    fails = LW.run_tensor_norms()
    assert not fails, fails[:12]


def test_sixteen_interleaved_groups():
    fails = LW.run_groups()
    assert not fails, fails[:12]


def test_a_frozen_group_is_untouched_with_inf_and_nan_in_its_gradient():
    fails = LW.run_frozen(plant=True)
    assert not fails, fails[:12]


def test_the_same_bits_twice_and_in_another_layout():
    fails = LW.run_determinism_and_packing()
    assert not fails, fails[:12]


def test_argument_errors_launch_nothing():
    fails = LW.run_error_cases()
    assert not fails, fails[:12]


# ---------------------------------------------------------------------------------------------------------------------------------
# the optimizer classes on a real net (accum_exact.small_net: 1 stack, chan 128, 64 x 64, B 2: the smallest net the engine builds)
GROUPS = ['--weight_decay', '0.01', '--no_decay_1d', '1', '--freeze', r'^(conv1|bn1)\.', '--lr_group', r'hg\.0\.:0.1', '--clip_grad_norm', '0.05']
KINDS = (('lamb', []), ('lars', ['--momentum', '0.9', '--nesterov', '1']))


def _make(kind, extra, net, tmp_path, lr=1e-3):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils import optim
    opt = TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'e', '--optimizer', kind] + GROUPS + extra)
    return optim.make_optimizer(opt, net, lr)


@pytest.mark.parametrize('kind,extra', KINDS)
def test_a_real_net_under_the_command_lines_groups(kind, extra, tmp_path):
    """one step and one accumulated group of two, each within the bounds per element; last_trust() per parameter, 1 on the tensors
    without decay; the EMA twin moves; frozen tensors bit for bit (check_step)"""
    from pose_adv_aug_amd._lib import grad_scale
    from pose_adv_aug_amd.utils import optim
    from tests.accum_exact import small_batch, small_net
    net = small_net()
    o = _make(kind, extra, net, tmp_path)
    assert [g['frozen'] for g in o.param_groups] == [False, True, False, False, False], o.describe_groups()
    assert [g['weight_decay'] for g in o.param_groups] == [0.01, 0.01, 0.0, 0.01, 0.0] and o.last_trust() is None and o.tensor_norms() is None
    ema = optim.ModelEma(net, decay=0.9)
    gscale = 1.0 / grad_scale()
    fails = []
    net.loss_and_backward(*small_batch(0))
    lay = LW.check_optimizer_step(o, net.flat_grads.clone(), gscale, fails, '%s step 1' % kind)
    trust = o.last_trust()
    assert trust.numel() == len(o._params()) == len(lay.offsets) and o.tensor_norms()[0].numel() == trust.numel()
    no_decay = [i for k in (2, 4) for i in o.param_groups[k]['params']]
    decayed = [i for k in (0, 3) for i in o.param_groups[k]['params']]
    assert no_decay and bool((trust[no_decay] == 1).all()) and bool((trust[o.param_groups[1]['params']] == 1).all())
    assert bool((trust[decayed] != 1).any()) and bool(torch.isfinite(trust).all()) and bool((trust > 0).all())
    twin = ema.module.flat_params.clone()
    ema.update(o)
    torch.cuda.synchronize()
    frozen_e = lay.per_elem([float(g == 1) for g in lay.groups]) != 0
    assert not torch.equal(ema.module.flat_params[~frozen_e], twin[~frozen_e]) and torch.equal(ema.module.flat_params[frozen_e], twin[frozen_e])
    net.loss_and_backward(*small_batch(1))
    o.accumulate()
    net.loss_and_backward(*small_batch(2))
    LW.check_optimizer_step(o, o._acc + net.flat_grads, gscale / 2, fails, '%s accumulated group of two' % kind)
    assert o.pending == 0 and o.skipped_steps() == 0
    assert not fails, fails[:12]


@pytest.mark.parametrize('kind,extra', KINDS + (('sgd', ['--momentum', '0.9']),))
def test_accumulate_then_step_is_a_step_on_the_fold(kind, extra, tmp_path):
    """accumulate() twice then step() against ONE step on (g1 + g2) + g3 with gscale / 3: bit for bit, parameters, state, norms and ratios"""
    from pose_adv_aug_amd._lib import grad_scale
    from tests.accum_exact import small_net
    nets = [small_net(), small_net()]
    opts = [_make(kind, extra, net, tmp_path) for net in nets]
    gen = torch.Generator().manual_seed(5)
    p0 = nets[0].flat_params.clone()
    n = nets[0].flat_params.numel()
    used = LW.NetLayout(opts[0]).used
    gs = [torch.where(used, torch.randn(n, generator=gen).cuda() * 1e-3, torch.zeros(n, device='cuda')) for _ in range(3)]
    for g in gs[:2]:
        nets[0].flat_grads.copy_(g)
        opts[0].accumulate()
    nets[0].flat_grads.copy_(gs[2])
    opts[0].step()
    nets[1].flat_grads.copy_((gs[0] + gs[1]) + gs[2])
    opts[1]._exchanged_gscale = lambda: (1.0 / grad_scale()) / 3           # the mean over the group, as step() takes it after a fold
    opts[1].step()
    torch.cuda.synchronize()
    a, b = LW.optimizer_arrays(opts[0]), LW.optimizer_arrays(opts[1])
    a.update(norms=opts[0]._norms, trust=opts[0]._trust)
    b.update(norms=opts[1]._norms, trust=opts[1]._trust)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert not torch.equal(nets[0].flat_params, p0)


def _bits_equal(x, y):
    return (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize('cls,kw', (('LAMB', dict(max_grad_norm=0.5)), ('LARS', dict(lr=0.1, weight_decay=1e-4, nesterov=True)), ('SGD', dict(lr=0.1, momentum=0.9))))
def test_save_load_continue_gives_the_same_bits(cls, kw, tmp_path):
    from pose_adv_aug_amd.utils import optim
    from tests.test_gpu_adam import _toy_net
    a_net, b_net = _toy_net(), _toy_net()
    a = getattr(optim, cls)(a_net, **kw)
    a.step(); a.step()
    torch.save(a.state_dict(), str(tmp_path / 'opt.pth'))
    b_net.flat_params.copy_(a_net.flat_params)
    b = getattr(optim, cls)(b_net, **dict(kw, lr=0.5))            # the options come from the file's param group
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        b.load_state_dict(torch.load(str(tmp_path / 'opt.pth')))
    assert not [x for x in w if 'optimizer state' in str(x.message)], [str(x.message) for x in w]
    assert b.param_groups[0] == a.param_groups[0]
    for net in (a_net, b_net):
        net.flat_grads.mul_(-0.75)
    a.step(); b.step()
    torch.cuda.synchronize()
    x, y = LW.optimizer_arrays(a), LW.optimizer_arrays(b)
    assert sorted(x) == sorted(y) and all(_bits_equal(x[k], y[k]) for k in x)
    assert _bits_equal(a._trust, b._trust) and _bits_equal(a._norms, b._norms)
    if cls == 'LAMB':
        assert a.steps_taken() == b.steps_taken() == 3 and torch.equal(a._state[2:], b._state[2:])
    # the padding between the toy net's tensors is exactly 0 everywhere
    pad = torch.ones(100, dtype=torch.bool, device='cuda')
    for _, _, off, numel, kind in a_net._table:
        if kind == 0:
            pad[off:off + numel] = False
    assert all(not bool(t[pad].any()) for t in x.values())


def test_an_adam_file_loads_into_lamb_and_torch_sgd_files_go_both_ways():
    from pose_adv_aug_amd.utils import optim
    from tests.optim_exact import _f32
    from tests.test_gpu_adam import _toy_net, _torch_twin, _set_grads, _params_close
    adam = optim.Adam(_toy_net(), weight_decay=0.0)
    adam.step(); adam.step()
    net = _toy_net()
    net.flat_params.copy_(adam.net.flat_params)
    lamb = optim.LAMB(net)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        lamb.load_state_dict(adam.state_dict())
    assert not w, [str(x.message) for x in w]
    assert lamb.steps_taken() == 2 and torch.equal(lamb.exp_avg, adam.exp_avg) and torch.equal(lamb.exp_avg_sq, adam.exp_avg_sq)
    lamb.step()
    torch.cuda.synchronize()
    assert lamb.steps_taken() == 3 and bool(torch.isfinite(net.flat_params).all()) and float(lamb.last_trust().min()) > 0
    back = optim.Adam(_toy_net())
    back.load_state_dict(lamb.state_dict())
    assert back.steps_taken() == 3 and torch.equal(back.exp_avg, lamb.exp_avg)
    # torch.optim.SGD: the same step, each file into the other side, the same next step
    kw = dict(lr=_f32(0.1), momentum=_f32(0.9), weight_decay=_f32(1e-4), nesterov=True)
    net = _toy_net()
    topt, ps = _torch_twin(net, 'SGD', **kw)
    topt.step()
    o = optim.SGD(net, **kw)
    o.step()
    torch.cuda.synchronize()
    sd, tsd = o.state_dict(), topt.state_dict()
    assert sorted(sd['state']) == sorted(tsd['state']) and all(sorted(sd['state'][i]) == sorted(tsd['state'][i]) == ['momentum_buffer'] for i in sd['state'])
    assert all(torch.allclose(sd['state'][i]['momentum_buffer'].cpu(), tsd['state'][i]['momentum_buffer'], rtol=1e-6, atol=1e-9) for i in sd['state'])
    assert _params_close(net, ps)
    t2, ps2 = _torch_twin(net, 'SGD', lr=0.5)
    t2.load_state_dict(sd)
    net_b = _toy_net()
    net_b.flat_params.copy_(net.flat_params)
    o2 = optim.SGD(net_b, lr=0.5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o2.load_state_dict(tsd)
    assert not w, [str(x.message) for x in w]
    assert all(o2.param_groups[0][k] == tsd['param_groups'][0][k] for k in ('lr', 'momentum', 'weight_decay', 'nesterov'))
    for n_ in (net, net_b):
        n_.flat_grads.mul_(-0.75)
    _set_grads(net, ps)
    _set_grads(net, ps2)
    topt.step(); t2.step(); o.step(); o2.step()
    torch.cuda.synchronize()
    assert _params_close(net, ps) and _params_close(net, ps2) and _params_close(net_b, ps)


def test_the_layerwise_optimizers_are_exact_and_skip_in_the_fp16_build():
    """The IEEE-half library: the exact cases above and the skipped step (layerwise_exact.run_skip_case), in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'layerwise_exact.py')], env=env, capture_output=True, text=True, timeout=600)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 LAYERWISE EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(os.environ.get('POSEADV_TEST_DIST_BACKEND') == 'nccl' and torch.cuda.device_count() < 2,
                    reason='two ranks over RCCL need two GPUs (a GPU holds one RCCL rank)')
def test_two_ranks_are_bit_identical_and_one_process_with_both_shards(monkeypatch):
    """three LAMB and three LARS steps on two data-parallel ranks (tests/dist_optim_exact.py: the smallest net, its own batches per rank):
    parameters, state, norms and trust ratios bit-identical on both ranks and bit for bit one process that accumulates both shards;
    exactly one all-reduce of the flat gradient per step"""
    from tests import dist_optim_exact as D
    monkeypatch.setattr(D, 'plain_worker', D.worker, raising=False)
    monkeypatch.setattr(D, 'worker', LW.dist_worker)
    LW.record_trust()
    cases = [D.case('lamb', 'LAMB', kw=dict(weight_decay=0.01)), D.case('lars', 'LARS', kw=dict(lr=1e-3, weight_decay=1e-4, nesterov=True))]
    seen = []
    for c, recs in D.run_ranks(cases):
        fails = D.check_replicas(recs) + D.check_exchange(recs)
        one = D.run_single(c)
        fails += D.check_same_run(recs[0], one, 'two ranks against one process accumulating both shards')
        for r in recs + [one]:
            for st in r['steps']:
                if '_trust' not in st['after'] or not bool((st['after']['_trust'] != 1).any()):
                    fails.append(('no trust ratio was recorded or none differs from 1', c['name']))
        assert not fails, (c['name'], fails[:8])
        assert recs[0]['final']['skipped'] == 0 and not D._differ(recs[0]['steps'][-1]['after']['_trust'], recs[1]['steps'][-1]['after']['_trust'])
        seen.append(c['name'])
    assert seen == ['lamb', 'lars']

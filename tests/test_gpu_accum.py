"""Gradient accumulation on the device (pa_grad_accumulate; utils.optim accumulate() / step(); --accum_steps), bit for bit (reference and
check: tests/accum_exact.py; tests/test_accum_cpu.py shows which defects they exclude).

Kernel: the sizes of tests/optim_exact.py (tail only, the first vector chunk, 1023, 100 003, 2048 * 256 * 4 + {0, 1, 3, 5}); dst distinct,
dst == a, dst == b and the copy form; every pointer in turn one float off the 16-byte boundary; guard elements; +-0, +-inf, inf + -inf,
NaN, denormal operands and sums, an overflowing sum.  Every refusal.

End to end, bf16 build, the smallest net the engine builds: net A accumulates N - 1 micro-batches and steps; its twin B (same seed, the same
forward passes in the same order) clones flat_grads after every backward pass, writes ((g1 + g2) + ...) * (1 / N) with torch's fp32
operators and calls the plain step().  For N = 2 and 4 the factor is a power of two and commutes with every rounding, so after two
optimizer steps the parameters, every state array of the optimizer and the BatchNorm buffers must be the same bits.  For N = 3 B hands the
unscaled sum and gscale = 1/3 to pa_rmsprop_step_state itself.  This rests on the engine being deterministic run to run.

State and wiring; stack_hg.train and the joint loop's pose_step against the same sequence driven by hand; --accum_steps 1 against the
option absent.  The IEEE-half build runs the kernel cases and a group with an inf in its first micro-batch in a child process."""
import os
import subprocess
import sys
import types

import pytest
import torch

from tests import optim_exact as O
from tests import accum_exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda x: x.view(torch.int32)


@pytest.mark.parametrize('n', O.SIZES)
def test_accumulate_is_exact(n):
    fails = X.run_case(n)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


def test_argument_errors_launch_nothing():
    fails = X.run_error_cases()
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
def _img4(k):
    from pose_adv_aug_amd import _lib
    x, pts = X.small_batch(k)
    img4 = torch.zeros(X.B, X.RES, X.RES, 4, dtype=_lib.act_dtype(), device='cuda')
    img4[..., :3] = x.permute(0, 2, 3, 1)
    return img4, pts


def _backward(net, k, autograd=False):
    img4, pts = _img4(k)
    if not autograd:
        net.loss_and_backward(img4=img4, pts=pts)
        return
    from pose_adv_aug_amd.pylib import HumanPts
    outs = net.forward_autograd(img4=img4, pts=pts)
    target = HumanPts.pts2heatmap_batch(pts, outs[0].shape[2], outs[0].shape[3])
    sum(((o - target) ** 2).mean() for o in outs).backward()


def _state(net, opt):
    arrays = [('flat_params', net.flat_params), ('flat_buffers', net.flat_buffers)]
    for k in ('square_avg', 'momentum_buffer', 'grad_avg', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq', '_state'):
        if getattr(opt, k, None) is not None:
            arrays.append((k, getattr(opt, k)))
    return arrays


def _same(net_a, opt_a, net_b, opt_b):
    torch.cuda.synchronize()
    sa, sb = _state(net_a, opt_a), _state(net_b, opt_b)
    assert [k for k, _ in sa] == [k for k, _ in sb]
    diff = [(k, int((bits(x) != bits(y)).sum())) for (k, x), (_, y) in zip(sa, sb) if not torch.equal(bits(x), bits(y))]
    assert not diff, 'arrays that differ (name, elements): %s' % diff


def _seq_sum(gs):
    acc = gs[0]
    for g in gs[1:]:
        acc = acc + g
    return acc


def _pair(make, N, use_graph=False, autograd=False, steps=2, direct_third=False):
    """A: accumulate() N - 1 times, then step().  B: the same backward passes, the sum by torch, the plain step()."""
    from pose_adv_aug_amd._lib import check, lib, ptr, stream
    nets = [X.small_net(), X.small_net()]
    for net in nets:
        net.use_graph = use_graph
    (net_a, net_b), (opt_a, opt_b) = nets, [make(net) for net in nets]
    assert torch.equal(bits(net_a.flat_params), bits(net_b.flat_params))
    start = net_a.flat_params.clone()
    for s in range(steps):
        for j in range(N):
            _backward(net_a, s * N + j, autograd)
            opt_a.accumulate() if j < N - 1 else opt_a.step()
        assert opt_a.pending == 0
        gs = []
        for j in range(N):
            _backward(net_b, s * N + j, autograd)
            gs.append(net_b.flat_grads.clone())
        if direct_third:
            net_b.flat_grads.copy_(_seq_sum(gs))
            g = opt_b.param_groups[0]
            check(lib().pa_rmsprop_step_state(ptr(net_b.flat_params), ptr(net_b.flat_grads), ptr(opt_b.square_avg), net_b.flat_params.numel(),
                                              float(g['lr']), float(g['alpha']), float(g['eps']), float(1 / 3), ptr(opt_b._skip_state), stream()))
            opt_b.steps += 1
            opt_b._weights_stepped()
        else:
            net_b.flat_grads.copy_(_seq_sum(gs) * (1.0 / N))
            opt_b.step()
        assert opt_b._acc is None
    _same(net_a, opt_a, net_b, opt_b)
    assert not torch.equal(bits(net_a.flat_params), bits(start)) and bool(torch.isfinite(net_a.flat_params).all())
    return net_a, opt_a


def _makers():
    from pose_adv_aug_amd.utils.optim import Adam, RMSprop
    return {'rmsprop': lambda net: RMSprop(net),
            'rmsprop_opts': lambda net: RMSprop(net, momentum=0.9, centered=True, max_grad_norm=0.5),
            'adam_clip': lambda net: Adam(net, max_grad_norm=0.5)}


@pytest.mark.parametrize('N', (2, 4))
@pytest.mark.parametrize('kind', ('rmsprop', 'rmsprop_opts', 'adam_clip'))
def test_a_group_is_the_step_on_its_mean_gradient(kind, N):
    net, opt = _pair(_makers()[kind], N)
    if kind == 'adam_clip':
        assert opt.steps_taken() == 2
    if kind != 'rmsprop':
        assert float(opt.last_grad_norm()) > 0


def test_a_group_of_three_is_the_step_with_gscale_one_third():
    _pair(_makers()['rmsprop'], 3, direct_third=True)


def test_a_group_behind_the_graph_replay():
    _pair(_makers()['rmsprop'], 2, use_graph=True)


def test_a_group_through_autograd():
    _pair(_makers()['rmsprop'], 2, autograd=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# state and wiring
def test_pending_counts_up_and_returns_to_zero_and_step_alone_allocates_nothing():
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    net = X.small_net()
    opt = RMSprop(net)
    ema = ModelEma(net, decay=0.9)
    calls = []
    plain = opt.allreduce_grads
    opt.allreduce_grads = lambda: (calls.append(opt.pending), plain())[1]
    _backward(net, 0)
    opt.step(); ema.update(opt)
    assert opt._acc is None and opt.pending == 0 and calls == [0]
    for j in range(3):
        _backward(net, 1 + j)
        opt.accumulate()
        assert opt.pending == j + 1
    acc = opt._acc
    assert acc is not None and acc.shape == net.flat_grads.shape and acc.dtype == torch.float32 and acc.data_ptr() != net.flat_grads.data_ptr()
    _backward(net, 4)
    opt.step(); ema.update(opt)
    assert opt.pending == 0 and opt._acc is acc and calls == [0, 3]          # the exchange ran once for the group of 4
    assert opt.steps == 2 and ema.updates() == 2                              # optimizer steps, not micro-batches


def test_zero_grad_drops_a_group():
    """backward, accumulate(), zero_grad(), backward, step() against the same two backward passes and the step alone (the dropped
    micro-batch still moved the BatchNorm statistics, so the twin runs its forward and backward pass too)"""
    from pose_adv_aug_amd.utils.optim import RMSprop
    done = []
    for drop in (True, False):
        net = X.small_net()
        opt = RMSprop(net)
        _backward(net, 0)
        opt.step()
        _backward(net, 5)
        if drop:
            opt.accumulate()
            assert opt.pending == 1
            opt.zero_grad()
            assert opt.pending == 0 and float(net.flat_grads.abs().max()) == 0
        _backward(net, 6)
        opt.step()
        assert opt.pending == 0
        done.append((net, opt))
    _same(*(done[0] + done[1]))


def test_an_overlapping_optimizer_refuses_to_accumulate():
    from pose_adv_aug_amd.utils.optim import Adam, RMSprop
    for cls in (RMSprop, Adam):
        net = X.small_net()
        opt = cls(net, overlap=True)
        _backward(net, 0)
        with pytest.raises(ValueError, match='overlap=False'):
            opt.accumulate()
        assert opt.pending == 0 and opt._acc is None
        opt.step()


# ---------------------------------------------------------------------------------------------------------------------------------
# loops
RES_LOOP = 256          # the crop size of the augmenter


def _loop_net(seed=4):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(1, 1, 16, 128, res=RES_LOOP, default_batch=2)
    net.reset_parameters(seed=seed)
    net.train()
    return net


def _batches(n):
    from pose_adv_aug_amd.data import DeviceBatch
    return [DeviceBatch.synthetic(2, seed=60 + k) for k in range(n)]


def test_the_loop_of_stack_hg_steps_on_groups_of_2_2_and_1():
    from pose_adv_aug_amd import stack_hg
    from pose_adv_aug_amd.data import Augmenter
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    batches = _batches(5)
    net_a, net_b = _loop_net(), _loop_net()
    opt_a, opt_b = RMSprop(net_a), RMSprop(net_b)
    ema = ModelEma(net_a, decay=0.9)
    groups, step_a, lines = [], opt_a.step, []
    opt_a.step = lambda: (groups.append(opt_a.pending + 1), step_a())[1]
    o = types.SimpleNamespace(print_freq=2, accum_steps=2, bs=2)
    loss, pckh = stack_hg.train(batches, net_a, opt_a, Augmenter(seed=2), 0, o, log=lines.append, ema=ema)
    assert groups == [2, 2, 1] and opt_a.steps == 3 and opt_a.pending == 0 and ema.updates() == 3
    assert sum('effective batch 2 x 2 x 1 rank(s) = 4' in l for l in lines) == 1
    assert sum('iters:' in l for l in lines) == 3                               # iterations 0, 2 and 4: the log stays per iteration
    stack_hg.train(batches[:1], net_a, opt_a, Augmenter(seed=3), 1, o, log=lines.append)
    assert sum('effective batch' in l for l in lines) == 1 and groups == [2, 2, 1, 1]          # said once per run
    # by hand
    aug = Augmenter(seed=2)
    for i, batch in enumerate(batches):
        data = aug.regular(batch)
        net_b.loss_and_backward(img4=data['img4'], pts=data['pts'])
        opt_b.accumulate() if i in (0, 2) else opt_b.step()
    data = Augmenter(seed=3).regular(batches[0])
    net_b.loss_and_backward(img4=data['img4'], pts=data['pts'])
    opt_b.step()
    _same(net_a, opt_a, net_b, opt_b)
    assert bool(torch.isfinite(torch.as_tensor(loss)))


def test_pose_step_of_the_joint_loop_accumulates_and_steps():
    from pose_adv_aug_amd import joint_train_pose_s_r_agent as J
    from pose_adv_aug_amd.data import Augmenter
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    batch = _batches(1)[0]
    net_a, net_b = _loop_net(), _loop_net()
    opt_a, opt_b = RMSprop(net_a), RMSprop(net_b)
    ema = ModelEma(net_a, decay=0.9)
    aug = Augmenter(seed=5)
    loss, pckh = J.pose_step(net_a, opt_a, aug.regular(batch), ema, accumulate=True)
    assert opt_a.pending == 1 and opt_a.steps == 0 and ema.updates() == 0 and 0.0 <= float(pckh) <= 1.0
    J.pose_step(net_a, opt_a, aug.regular(batch), ema, accumulate=False)
    assert opt_a.pending == 0 and opt_a.steps == 1 and ema.updates() == 1
    aug = Augmenter(seed=5)
    for k in range(2):
        data = aug.regular(batch)
        net_b.loss_and_backward(img4=data['img4'], pts=data['pts'])
        opt_b.accumulate() if k == 0 else opt_b.step()
    _same(net_a, opt_a, net_b, opt_b)


def test_accum_steps_1_is_the_loop_without_the_option(tmp_path):
    from pose_adv_aug_amd import stack_hg
    from pose_adv_aug_amd.data import Augmenter
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils.optim import make_optimizer
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e', '--bs', '2']
    batches = _batches(3)
    done = []
    for extra in ([], ['--accum_steps', '1']):
        o = TrainOptions().parse(base + extra)
        net = _loop_net()
        opt = make_optimizer(o, net, o.lr)
        lines = []
        stack_hg.train(batches, net, opt, Augmenter(seed=2), 0, o, log=lines.append)
        assert opt.steps == 3 and opt._acc is None and opt.pending == 0 and not any('effective batch' in l for l in lines)
        done.append((net, opt))
    _same(*(done[0] + done[1]))


def test_accumulation_in_the_fp16_build():
    """The IEEE-half library: the kernel cases at two sizes, the refusals, and a group of 2 whose first micro-batch gradient holds an inf
    (accum_exact.run_skip_group), in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'accum_exact.py')], env=env, capture_output=True, text=True, timeout=600)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 ACCUM EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]

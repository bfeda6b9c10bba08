"""The weight EMA on the device (pa_ema_advance, pa_ema_lerp, pa_ema_counts, pa_ema_set_updates; utils.optim.ModelEma), element by element
against float64 (reference, bound and state model: tests/ema_exact.py; tests/test_ema_cpu.py shows which defects they exclude).

Cases: the sizes of tests/optim_exact.py (tail only, the first vector chunk, 1023, 100 003, 2048 * 256 * 4 + {0, 1, 3, 5}); decay 0, 0.5,
0.999, 0.9999; warm-up off and on (five updates from count 0, one from 9 -> 10 through pa_ema_set_updates); the copying launch; guard
elements; the state exact after every update.  A held step (flag word 1) and the update after it.  Every refusal.  ModelEma behind RMSprop
and Adam on the real flat arrays of a pose net and its agent, buffers averaged and copied, the padding exactly 0.  The twin as a net:
its heat maps against a freshly created net that loaded its state_dict (a stale 16-bit weight copy would show), the training net
untouched by the attachment.  Checkpoint: save, load, continue gives the same bits; a file without the entry.  stack_hg's step function
with --ema_decay.  The IEEE-half build runs the exact cases and the skipped optimizer steps in a child process."""
import os
import subprocess
import sys

import pytest
import torch

from tests import optim_exact as X
from tests import ema_exact as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda x: x.view(torch.int32)


@pytest.mark.parametrize('n', X.SIZES)
def test_ema_update_is_exact(n):
    fails = M.run_case(n)
    assert not fails, '%d checks failed, first: %s' % (len(fails), fails[:12])


def test_a_held_step_moves_nothing_and_the_count_stays():
    fails = M.run_hold_case()
    assert not fails, fails[:12]


def test_argument_errors_launch_nothing():
    fails = M.run_error_cases()
    assert not fails, fails


def test_model_ema_is_exact_on_real_flat_arrays():
    """three optimizer.step() + ema.update() rounds behind RMSprop and Adam on the 2-stack chan-128 pose net and its agent, buffers
    'ema' and 'copy' (ema_exact.run_flat_array)"""
    fails = M.run_flat_array()
    assert not fails, fails[:12]


# 1-stack chan-128 pose net, 64 x 64 input, batch 2: the smallest net the engine builds
STACKS, CHAN, RES, B = 1, 128, 64, 2


def _net(seed=11):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(STACKS, 1, 16, CHAN, res=RES, default_batch=B)
    net.reset_parameters(seed=seed)
    return net


def _batch(k):
    from tests import inputs
    return (torch.from_numpy(inputs.images(300 + k, B, RES)).cuda(), torch.from_numpy(inputs.heat_pts(400 + k, B, res=RES // 4)).cuda())


def _steps(net, opt, ema, ks):
    """training steps on the batches ks; returns the heat maps of every step"""
    outs = []
    net.train()
    for k in ks:
        img, pts = _batch(k)
        _, o = net.loss_and_backward(img, pts, want_outputs=True)
        opt.step()
        if ema is not None:
            ema.update(opt)
        outs.append(o[-1].clone())
    return outs


def test_the_twin_evaluates_its_own_average_and_the_training_net_is_untouched():
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    net, plain = _net(), _net()
    opt, opt_plain = RMSprop(net), RMSprop(plain)
    ema = ModelEma(net, decay=0.5)
    twin = ema.module
    img, _ = _batch(9)
    first = twin(img)[-1].clone()                         # the twin's 16-bit weight copies are packed now: the updates make them stale
    assert not twin.training and type(twin) is type(net)
    outs, outs_plain = _steps(net, opt, ema, (0, 1)), _steps(plain, opt_plain, None, (0, 1))
    torch.cuda.synchronize()
    assert ema.updates() == 2 and ema.held() == 0
    # the training net, with and without an average attached
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, outs_plain))
    assert torch.equal(bits(net.flat_params), bits(plain.flat_params)) and torch.equal(bits(net.flat_buffers), bits(plain.flat_buffers))
    # the twin against a freshly created net that loads its state_dict
    got = twin.eval()(img)[-1].clone()
    fresh = _net(seed=99)
    fresh.load_state_dict(twin.state_dict())
    want = fresh.eval()(img)[-1]
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))
    assert not torch.equal(bits(got), bits(first))                                    # (the average moved, and the heat maps with it)
    assert not torch.equal(bits(twin.flat_params), bits(net.flat_params)) and twin._nbt == net._nbt == 2
    assert int(twin.state_dict()['bn1.num_batches_tracked']) == 2
    raw = net.eval()(img)[-1]
    assert not torch.equal(bits(got), bits(raw))
    # reset(): a copy again, count 0
    ema.reset()
    assert torch.equal(bits(twin.flat_params), bits(net.flat_params)) and torch.equal(bits(twin.flat_buffers), bits(net.flat_buffers))
    assert (ema.updates(), ema.held()) == (0, 0)
    assert torch.equal(bits(twin.eval()(img)[-1]), bits(raw))


def _history(epoch=0):
    from pose_adv_aug_amd.utils.util import PoseTrainHistory
    h = PoseTrainHistory()
    h.update({'epoch': epoch}, {'lr': 2.5e-4}, {'train_loss': 1., 'val_loss': 1.}, {'train_pckh': .1, 'val_pckh': .2})
    return h


def test_save_load_continue_gives_the_same_bits(tmp_path, capsys):
    from pose_adv_aug_amd.utils.checkpoint import Checkpoint
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    net = _net()
    opt = RMSprop(net)
    ema = ModelEma(net, decay=0.999, warmup=True, buffers='ema')
    _steps(net, opt, ema, (0, 1))
    ck = Checkpoint()
    ck.save_prefix = str(tmp_path) + '/'
    path = ck.save_checkpoint(net, opt, _history(), torch.zeros(B, 16, 2), ema=ema)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(saved) == ['ema', 'optimizer', 'state_dict', 'train_history']
    assert sorted(saved['ema']) == ['buffers', 'decay', 'module', 'updates', 'warmup']
    assert (saved['ema']['decay'], saved['ema']['warmup'], saved['ema']['buffers'], saved['ema']['updates']) == (0.999, True, 'ema', 2)
    assert all(not v.is_cuda for v in saved['ema']['module'].values()) and list(saved['ema']['module']) == list(net.state_dict())
    assert torch.equal(saved['state_dict']['module.conv1.weight'], net.state_dict()['conv1.weight'].cpu())        # the raw weights
    assert not torch.equal(saved['ema']['module']['conv1.weight'], saved['state_dict']['module.conv1.weight'])
    # a new pair, other options and other weights until the file is loaded
    net2 = _net(seed=5)
    opt2 = RMSprop(net2)
    ema2 = ModelEma(net2, decay=0.5, warmup=False, buffers='copy')
    ck2 = Checkpoint()
    ck2.load_prefix = path[:-len('.pth.tar')]
    assert ck2.load_checkpoint(net2, opt2, _history(), ema=ema2)
    assert (ema2.decay, ema2.warmup, ema2.buffers, ema2.updates(), ema2.held()) == (0.999, True, 'ema', 2, 0)
    assert torch.equal(bits(ema2.module.flat_params), bits(ema.module.flat_params)) and ema2.module._nbt == ema.module._nbt
    assert "no 'ema' entry" not in capsys.readouterr().out
    _steps(net, opt, ema, (2,))
    _steps(net2, opt2, ema2, (2,))
    torch.cuda.synchronize()
    for a, b in ((net.flat_params, net2.flat_params), (ema.module.flat_params, ema2.module.flat_params), (ema.module.flat_buffers, ema2.module.flat_buffers)):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(ema._state, ema2._state) and ema2.updates() == 3          # the count and the w of the warm-up at count 2
    # load_ema: an average created after the checkpoint load
    ema3 = ModelEma(net2, decay=0.9)
    assert ck2.load_ema(ema3) and ema3.updates() == 2 and ema3.decay == 0.999
    assert torch.equal(ema3.module.state_dict()['conv1.weight'].cpu(), saved['ema']['module']['conv1.weight'])


def test_a_file_without_the_entry_leaves_the_twin_a_copy(tmp_path, capsys):
    from pose_adv_aug_amd.utils.checkpoint import Checkpoint
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    net = _net()
    opt = RMSprop(net)
    _steps(net, opt, None, (0,))
    ck = Checkpoint()
    ck.save_prefix = str(tmp_path) + '/'
    path = ck.save_checkpoint(net, opt, _history(), torch.zeros(B, 16, 2))
    assert 'ema' not in torch.load(path, map_location='cpu', weights_only=False)
    net2 = _net(seed=5)
    opt2 = RMSprop(net2)
    ema2 = ModelEma(net2, decay=0.9)
    _steps(net2, opt2, ema2, (1,))
    ck2 = Checkpoint()
    ck2.load_prefix = path[:-len('.pth.tar')]
    capsys.readouterr()
    assert ck2.load_checkpoint(net2, opt2, _history(), ema=ema2)
    out = capsys.readouterr().out
    assert out.count("no 'ema' entry") == 1
    assert torch.equal(bits(net2.flat_params), bits(net.flat_params))
    assert torch.equal(bits(ema2.module.flat_params), bits(net.flat_params)) and torch.equal(bits(ema2.module.flat_buffers), bits(net.flat_buffers))
    assert (ema2.updates(), ema2.held(), ema2.decay, ema2.module._nbt) == (0, 0, 0.9, net._nbt)


def test_the_step_function_of_stack_hg_updates_the_average(tmp_path):
    from pose_adv_aug_amd.data import Augmenter, DeviceBatch
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.stack_hg import train_step
    from pose_adv_aug_amd.utils.optim import make_ema, make_optimizer
    opt = TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'e', '--ema_decay', '0.9', '--bs', '2'])
    net = create_hg(1, 1, 16, 128, res=256, default_batch=2)
    net.reset_parameters(seed=4)
    optimizer = make_optimizer(opt, net, opt.lr)
    ema = make_ema(opt, net)
    assert ema is not None and (ema.decay, ema.warmup, ema.buffers) == (0.9, False, 'ema')
    aug = Augmenter(seed=2)
    batch = DeviceBatch.synthetic(2, seed=60)
    net.train()
    for _ in range(3):
        loss, pckh, pckh_o = train_step(net, optimizer, aug, batch, ema=ema)
    torch.cuda.synchronize()
    assert ema.updates() == 3 and ema.held() == 0 and bool(torch.isfinite(loss))
    twin = ema.module
    assert bool(torch.isfinite(twin.flat_params).all()) and not torch.equal(bits(twin.flat_params), bits(net.flat_params))
    assert not torch.equal(bits(twin.flat_buffers), bits(net.flat_buffers)) and twin._nbt == net._nbt == 3
    assert make_ema(TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'e']), net) is None


def test_ema_is_exact_and_holds_in_the_fp16_build():
    """The IEEE-half library: the exact cases above, the flat arrays, and the optimizer steps skipped for an inf in the gradient, on
    which the average and its count stay (ema_exact.run_skip_case), in a child process."""
    env = dict(os.environ, POSEADV_DTYPE='fp16')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'ema_exact.py')], env=env, capture_output=True, text=True, timeout=900)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print(r.stdout)
    assert r.returncode == 0 and 'FP16 EMA EXACT PASSED' in r.stdout, (r.stdout + r.stderr)[-3000:]

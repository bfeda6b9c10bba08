"""world_size-2 (gloo, CPU) test of the data-parallel exchange: ONE all-reduce (sum) of the flat gradient,
1/world scaling folded into the optimizer, replicas stay bit-identical, parameters are broadcast once."""
import os
import types

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import step as ostep
from tests._rendezvous import file_init_method, set_env


def _worker(rank, world, init, out):
    dist.init_process_group('gloo', init_method=init, rank=rank, world_size=world)
    from pose_adv_aug_amd.utils.optim import RMSprop
    from pose_adv_aug_amd.stack_hg import broadcast_parameters
    n = 1000
    g = torch.Generator().manual_seed(7)
    net = types.SimpleNamespace(flat_params=torch.randn(n, generator=g) + rank,        # replicas start different
                                flat_grads=torch.zeros(n), flat_buffers=torch.zeros(4) + rank,
                                _table=[('w', (n,), 0, n, 0)], _ensure_table=lambda: None,
                                weights_changed=lambda: None)
    broadcast_parameters(net)                                                           # rank 0's values everywhere
    opt = RMSprop(net)
    local = torch.Generator().manual_seed(100 + rank)
    per_rank = torch.randn(n, generator=local)                                          # this rank's shard gradient
    net.flat_grads.copy_(per_rank)
    gscale = opt.allreduce_grads()
    # emulate the fused device update with the oracle's RMSprop on (sum * gscale)
    v = torch.zeros(n)
    ostep.rmsprop_update(net.flat_params, net.flat_grads * gscale, v, 2.5e-4)
    out[rank] = (net.flat_params.clone(), net.flat_grads.clone(), gscale, net.flat_buffers.clone())
    dist.barrier()
    dist.destroy_process_group()


def test_flat_gradient_allreduce_world2():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, file_init_method(), out), nprocs=2, join=True)
    p0, g0, s0, b0 = out[0]
    p1, g1, s1, b1 = out[1]
    assert s0 == s1 == 0.5
    assert torch.equal(g0, g1) and torch.equal(p0, p1) and torch.equal(b0, b1)         # identical replicas
    ref = sum(torch.randn(1000, generator=torch.Generator().manual_seed(100 + r)) for r in range(2))
    assert torch.allclose(g0, ref)
    # equals the single-process step on the mean gradient of the concatenated batch
    pref = torch.randn(1000, generator=torch.Generator().manual_seed(7))
    ostep.rmsprop_update(pref, ref * 0.5, torch.zeros(1000), 2.5e-4)
    assert torch.allclose(p0, pref)


def test_flat_gradient_allreduce_world4():
    """the same exchange typed for N not in {1, 2} (joint-train-pose-s-r-agent.py:62,90 run on 4 / 8 GPUs): 1/4 scaling, replicas
    identical on every rank, equal to one process stepping on the mean of the four shard gradients"""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(4, file_init_method(), out), nprocs=4, join=True)
    assert all(out[r][2] == 0.25 for r in range(4))
    for r in range(1, 4):
        assert torch.equal(out[0][0], out[r][0]) and torch.equal(out[0][1], out[r][1]) and torch.equal(out[0][3], out[r][3])
    ref = sum(torch.randn(1000, generator=torch.Generator().manual_seed(100 + r)) for r in range(4))
    assert torch.allclose(out[0][1], ref, atol=1e-6)
    assert torch.equal(out[0][3], torch.zeros(4))                                       # rank 0's buffers everywhere
    pref = torch.randn(1000, generator=torch.Generator().manual_seed(7))
    ostep.rmsprop_update(pref, ref * 0.25, torch.zeros(1000), 2.5e-4)
    assert torch.allclose(out[0][0], pref)


KEPT = ('pa_sample_aug', 'pa_rmsprop_step', 'all_reduce', 'pa_net_bind')
KEPT_OPTS = KEPT + ('pa_grad_accumulate', 'pa_grad_norm', 'pa_adam_step', 'pa_rmsprop_step_opts', 'pa_ema_advance', 'pa_ema_lerp')


def _main_worker(rank, world, init, exp_dir, out, extra=(), kept=KEPT):
    """stack_hg.main() -- the REAL host control flow -- on 2 gloo ranks with the engine stubbed at the C ABI.  extra: further command-line
    arguments; kept: the calls whose arguments travel back with the log."""
    # gloo named explicitly: the stub's tensors live on the CPU, and init_distributed picks nccl (RCCL) whenever a GPU is visible
    set_env(rank, world, init, POSEADV_DIST_BACKEND='gloo')
    from tests import abi_stub
    fake = abi_stub.install(rank)
    orig_ar, orig_save = dist.all_reduce, torch.save
    saves = []

    def all_reduce(t, op=dist.ReduceOp.SUM, **kw):
        fake.log.append(('all_reduce', (t.numel(), str(t.dtype))))
        return orig_ar(t, op=op, **kw)

    def save(obj, path, *a, **kw):
        saves.append(os.path.basename(path))
        return orig_save(obj, path, *a, **kw)
    dist.all_reduce, torch.save = all_reduce, save
    from pose_adv_aug_amd import stack_hg
    captured = {}
    orig_create = stack_hg.create_hg

    def create(*a, **kw):
        captured['net'] = orig_create(*a, **kw)
        return captured['net']
    stack_hg.create_hg = create
    stack_hg.main(['--exp_dir', exp_dir, '--exp_id', 'dp', '--bs', '2', '--nEpochs', '1', '--is_train', '1', '--print_freq', '2'] + list(extra))
    net = captured['net']
    out[rank] = dict(log=[(n, a if n in kept else None) for n, a in fake.log],
                     params=net.flat_params.clone(), buffers=net.flat_buffers.clone(), saves=saves, grads_at=net.flat_grads.data_ptr())
    dist.barrier()
    dist.destroy_process_group()


def test_training_main_on_two_ranks_with_the_engine_stubbed_at_the_abi(tmp_path):
    """SURVEY.md section 8e on the real host code (stack_hg.main -> train -> train_step -> RMSprop.step -> validate ->
    checkpoint): per step every rank runs backward, then ONE all-reduce of the whole flat gradient, then the fused RMSprop
    with gscale = 1/world on the stream the net was bound to, then the weight re-pack; ranks draw DIFFERENT augmentations
    (seed + rank, same step counter); replicas stay bit-identical although their shard gradients differ; the logged meters
    are all-reduced (2 x names numbers, at print time only); rank 0 alone writes checkpoints."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_main_worker, args=(2, file_init_method(), str(tmp_path), out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    assert torch.equal(r0['params'], r1['params']) and torch.equal(r0['buffers'], r1['buffers'])
    for r in (r0, r1):
        names = [n for n, _ in r['log']]
        steps = [i for i, n in enumerate(names) if n == 'pa_hg_backward']
        assert len(steps) == 4                                            # 4 synthetic batches, one epoch
        for k, i in enumerate(steps):
            end = steps[k + 1] if k + 1 < len(steps) else len(names)
            seg = names[i:end]
            ar = [j for j, n in enumerate(seg) if n == 'all_reduce' and r['log'][i + j][1][0] == 40]
            rp = seg.index('pa_rmsprop_step')
            assert len(ar) == 1 and 0 < ar[0] < rp < seg.index('pa_net_prepare_weights'), seg[:12]
            # the step's meters (stack-hg.py:176-178) read the forward pass's heat maps only: train_step asks for them between the two passes,
            # on the engine's meter stream (pa_net_meters_async on ... off), so they run beside the backward pass
            fwd = max(j for j in range(i) if names[j] == 'pa_hg_forward')
            between = names[fwd:i]
            on = [j for j, n in enumerate(between) if n == 'pa_net_meters_async']
            assert len(on) == 2, between
            assert on[0] < between.index('pa_hg_accuracy') < between.index('pa_hg_pckh') < on[1], between
        bind_stream = [a for n, a in r['log'] if n == 'pa_net_bind'][0][1]
        for n, a in r['log']:
            if n == 'pa_rmsprop_step':
                assert a[0] == 40 and a[4] == 0.5 and a[5] == bind_stream and abs(a[1] - 2.5e-4) < 1e-12
        meters = [a for n, a in r['log'] if n == 'all_reduce' and a[0] == 6]
        assert len(meters) == 4                                           # prints at i = 0, 2 (print_freq 2) and 3 (last) + the epoch's return value
    s0 = [a for n, a in r0['log'] if n == 'pa_sample_aug']
    s1 = [a for n, a in r1['log'] if n == 'pa_sample_aug']
    assert [a[1] for a in s0[:4]] == [1234] * 4 and [a[1] for a in s1[:4]] == [1235] * 4       # seed + rank
    assert [a[2] for a in s0[:4]] == [0, 1, 2, 3] == [a[2] for a in s1[:4]]
    assert len(r0['saves']) == 1 and r0['saves'][0].endswith('-0.pth.tar') and r1['saves'] == []
    files = os.listdir(os.path.join(str(tmp_path), 'dp'))
    assert any(f.endswith('-0.pth.tar') for f in files) and any(f.endswith('-0-preds.mat') for f in files) and 'train-log.txt' in files


def test_adamw_with_clipping_and_accumulation_on_two_ranks_with_the_engine_stubbed_at_the_abi(tmp_path):
    """--optimizer adamw --clip_grad_norm 1 --accum_steps 2 through the same host code on two ranks: 4 synthetic batches per rank, so two
    groups of 2.  A micro-batch that does not end its group: one pa_grad_accumulate into the optimizer's own sum and NO all-reduce of the
    gradient.  The one that ends it: the fold with dst == flat_grads, then exactly ONE all-reduce of the whole flat gradient, then
    pa_grad_norm with gscale = 1 / (2 ranks x 2 micro-batches), then pa_adam_step with the same gscale and the coefficient's device
    pointer, then the weight re-pack; with --ema_decay 0.9 beside them, the EMA's prologue (with the optimizer's flag word) and its two
    launches behind every optimizer step and none behind a micro-batch that only accumulates.  Replicas bit-identical at the end (the
    stub's Adam depends on every operand)."""
    mgr = mp.Manager()
    out = mgr.dict()
    extra = ['--optimizer', 'adamw', '--clip_grad_norm', '1', '--accum_steps', '2', '--ema_decay', '0.9']
    mp.spawn(_main_worker, args=(2, file_init_method(), str(tmp_path), out, extra, KEPT_OPTS), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    assert torch.equal(r0['params'], r1['params'])
    for r in (r0, r1):
        log = r['log']
        names = [n for n, _ in log]
        assert 'pa_rmsprop_step' not in names and 'pa_rmsprop_step_opts' not in names
        starts = [i for i, n in enumerate(names) if n == 'pa_hg_backward']
        assert len(starts) == 4
        train_end = max(i for i, n in enumerate(names) if n == 'pa_adam_step') + 1
        accs = set()
        for k, i in enumerate(starts):
            end = starts[k + 1] if k + 1 < len(starts) else len(names)
            seg = log[i:end]
            seg_names = [n for n, _ in seg]
            whole = [j for j, (n, a) in enumerate(seg) if n == 'all_reduce' and a[0] == 40]
            folds = [j for j, n in enumerate(seg_names) if n == 'pa_grad_accumulate']
            assert len(folds) == 1, seg_names
            dst, a, b, n, stream = seg[folds[0]][1]
            assert n == 40
            if k % 2 == 0:                                   # does not end its group
                assert whole == [] and 'pa_adam_step' not in seg_names and 'pa_grad_norm' not in seg_names, seg_names
                assert dst != r['grads_at'] and a == r['grads_at'] and b is None          # the first of a group: a copy into the sum
                accs.add(dst)
            else:
                assert len(whole) == 1, seg_names
                norm, step, repack = seg_names.index('pa_grad_norm'), seg_names.index('pa_adam_step'), seg_names.index('pa_net_prepare_weights')
                assert folds[0] < whole[0] < norm < step < repack, seg_names
                assert seg_names.count('pa_grad_norm') == 1 and seg_names.count('pa_adam_step') == 1
                assert dst == r['grads_at'] and a in accs and b == r['grads_at']          # flat_grads = _acc + flat_grads
                g_at, n_norm, gscale, max_norm, _ = seg[norm][1]
                assert g_at == r['grads_at'] and n_norm == 40 and gscale == 0.25 and max_norm == 1.0
                n_step, gscale_step, coef_at, _, (lr, wd, amsgrad, decoupled), g_step = seg[step][1]
                assert n_step == 40 and gscale_step == 0.25 and coef_at is not None and g_step == r['grads_at'] and decoupled == 1 and amsgrad == 0
                # --ema_decay 0.9: behind the step, the prologue with the optimizer's flag word, then parameters and buffers
                ema = [(j, a) for j, (n, a) in enumerate(seg) if n in ('pa_ema_advance', 'pa_ema_lerp')]
                assert [seg_names[j] for j, _ in ema] == ['pa_ema_advance', 'pa_ema_lerp', 'pa_ema_lerp'] and ema[0][0] > step, seg_names
                assert abs(ema[0][1][0] - 0.9) < 1e-12 and ema[0][1][2] is not None and [a[2:4] for _, a in ema[1:]] == [(40, 0), (8, 0)]
            if k % 2 == 0:
                assert 'pa_ema_advance' not in seg_names and 'pa_ema_lerp' not in seg_names          # the weights did not move
        assert len(accs) == 1                                # allocated once
        assert len([1 for n, a in log[:train_end] if n == 'all_reduce' and a[0] == 40]) == 2 and names.count('pa_adam_step') == 2
    assert len(r0['saves']) == 1 and r1['saves'] == []

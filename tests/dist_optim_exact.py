"""Two data-parallel ranks through every optimizer option, gradient accumulation and the weight EMA (utils.optim: _exchanged_gscale ->
_clip_coef -> step, ModelEma.update), checked from what each rank's step actually consumed.

Recording.  `worker` runs a list of cases on one process group (gloo with both ranks on the one GPU, or RCCL with one rank per GPU:
tests/_rendezvous.engine_rank_env).  Per case: the smallest net the engine builds (accum_exact.small_net's shape), seeded 100 + rank and
then broadcast; inputs accum_exact.small_batch's with seed 1000 rank + counter, so the shards differ.  dist.all_reduce is wrapped (Tap):
for every exchange of the whole flat gradient the tensor is cloned before the call (g_local) and after it (g_sum).  flat_grads is cloned
after every backward pass; around every step() flat_params, flat_buffers and every state array of the optimizer; after it _norm_out,
Adam's device state, the optimizer's skip flag; around every ModelEma.update the twin's arrays and its device state.  Everything is kept as
CPU tensors, one file per rank and case (torch.save keeps an array that two places hold once).

Checks, per case and optimizer step t with k micro-batches accumulated before it (each returns the failures [(what, figure)]):
  check_replicas   every array, state word, norm and count the same bits on both ranks; BatchNorm buffers, the twin's too, differ
  check_exchange   exactly one exchange of the whole flat gradient per optimizer step and none in a micro-batch that does not end its
                   group; g_sum the same bits on both ranks and the bits of g_local[0] + g_local[1] (fp32; two operands: no order);
                   g_local the bits of the rank's own fold ((g1 + g2) + ...) of the clones taken after each backward pass
  check_steps      the recorded before, g_sum, after, gscale = 1 / (world (k + 1) grad_scale) and the recorded coefficient handed to
                   optim_exact.check, optim_opts_exact.check / check_norm, adam_exact.check / check_consts, ema_exact.check_arrays /
                   check_state with their own bounds and the domain masks of their own flat-array cases: no tolerance is set here
  check_clip       the coefficient exactly 1 at the first step of a case and wherever max_grad_norm is LARGE (the norm is recorded
                   all the same), below 1 at every later step of a 'half' case, whose max_grad_norm is half the float64 norm of the
                   very gradient the step consumed (_half_the_norm: half the FIRST step's norm does not clip the later steps of this
                   untrained net -- measured norms of three steps: 74, 24, 1070 with RMSprop's options, 1028, 12, 1266 with Adam and
                   N = 2, 1.00, 0.71, 0.33 on the 2-stack net)
  check_accum      pending counts up and is 0 after the step, _acc allocated once
  check_skips      fp16 build, one inf written by rank 1 alone: both ranks leave parameters and state bit-unchanged on that step, flag,
                   skipped_steps, Adam's step count and the EMA's held / update counts; every other step applied
  check_same_run   parameters, state, norm and Adam's words bit for bit those of another record: one process that runs shard 0's backward
                   pass, accumulate(), shard 1's, step() (g0 + g1 and gscale = 1/2: the same operands in the same launches, which is what
                   data parallelism means here), or the same case with overlap=True
  check_buckets    the overlapped exchange: 2 asynchronous buckets per step, every gradient exchanged exactly once

tests/test_dist_optim_cpu.py feeds these functions recorded-shaped data with one defect each.  tests/test_gpu_dist_optim.py runs the
cases; the IEEE-half build runs this file as a child process, which spawns its two ranks itself."""
import os
import shutil
import sys
import tempfile
import time

import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import accum_exact as AX
from tests import adam_exact as A
from tests import ema_exact as M
from tests import optim_exact as O
from tests import optim_opts_exact as Y
from tests.optim_exact import DOMAIN, _f32

LARGE = 1.0e30                   # a max_grad_norm no gradient reaches: the norm is recorded, the coefficient is exactly 1
POISON_AT = 12345                # the element of flat_grads that receives the inf (accum_exact.run_skip_group's)
STATE_ARRAYS = ('square_avg', 'momentum_buffer', 'grad_avg', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')      # test_gpu_accum._state's
WORDS = ('_state', '_skip_state')                                                                             # int32 device words
PER_RANK = ('flat_buffers',)     # BatchNorm running statistics: every rank keeps its own


def case(name, opt='RMSprop', kw=None, clip=None, N=1, steps=3, ema=None, overlap=False, stacks=1, res=AX.RES, poison=None, loop=False):
    """One case as plain data (it travels to the spawned ranks).  opt, kw: the class of utils.optim and its keyword arguments.
    clip: None, 'half' (max_grad_norm = LARGE at the first step, then half the norm of each step's own gradient) or 'large'.  N: micro-batches
    per optimizer step.  ema: ModelEma's keyword arguments.  poison: {'step', 'micro'}, where rank 1 alone writes an inf (fp16 build).
    loop: stack_hg.train over 3 batches with accum_steps 2 instead."""
    return dict(name=name, opt=opt, kw=dict(kw or {}), clip=clip, N=N, steps=steps, ema=None if ema is None else dict(ema),
                overlap=overlap, stacks=stacks, res=res, poison=poison, loop=loop)


def deadline_for(cases):
    """seconds a spawn may take: imports, two library loads and a process group, then per case two nets and their steps"""
    return 120 + 30 * len(cases)


# ---------------------------------------------------------------------------------------------------------------------------------
# recording (GPU)
def _cpu(x):
    return x.detach().cpu()


class _Keep(object):
    """snapshots as CPU tensors; an array that has not changed since its last snapshot is the same object again"""
    def __init__(self):
        self.last = {}

    def __call__(self, name, x):
        new, old = _cpu(x), self.last.get(name)
        if old is not None and _same_bits(old, new):
            return old
        self.last[name] = new
        return new


class Tap(object):
    """dist.all_reduce wrapped: every call on the storage of the current net's flat_grads is recorded, the whole-array ones with a clone
    before and after (clone off for the overlapped exchange, whose buckets run on another stream)"""
    def __init__(self, dist):
        self.dist, self.orig, self.net, self.events, self.clone = dist, dist.all_reduce, None, [], True
        dist.all_reduce = self

    def __call__(self, t, *a, **k):
        net = self.net
        if net is None or t.untyped_storage().data_ptr() != net.flat_grads.untyped_storage().data_ptr():
            return self.orig(t, *a, **k)
        ev = dict(numel=t.numel(), offset=t.storage_offset(), async_op=bool(k.get('async_op', False)), whole=t.numel() == net.flat_grads.numel())
        if ev['whole'] and self.clone:
            ev['g_local'] = _cpu(t)
        r = self.orig(t, *a, **k)
        if ev['whole'] and self.clone:
            ev['g_sum'] = _cpu(t)
        self.events.append(ev)
        return r


def batch(k, res=AX.RES):
    """accum_exact.small_batch(k) at any input size"""
    from tests import inputs
    return (torch.from_numpy(inputs.images(300 + k, AX.B, res)).cuda(), torch.from_numpy(inputs.heat_pts(400 + k, AX.B, res=res // 4)).cuda())


def make_net(c, seed):
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    net = create_hg(c['stacks'], 1, 16, AX.CHAN, res=c['res'], default_batch=AX.B)
    net.reset_parameters(seed=seed)
    net.train()
    return net


def make_opt(c, net):
    from pose_adv_aug_amd.utils import optim
    kw = dict(c['kw'], overlap=True) if c['overlap'] else dict(c['kw'])
    if c['clip']:
        kw['max_grad_norm'] = LARGE
    return getattr(optim, c['opt'])(net, **kw)


def _snapshot(net, opt, keep):
    from tests.test_gpu_accum import _state
    arrays = dict((k, keep(k, x)) for k, x in _state(net, opt))
    if getattr(opt, '_skip_state', None) is not None:
        arrays['_skip_state'] = keep('_skip_state', opt._skip_state)
    return arrays


def _half_the_norm(opt, net, steps):
    """clip = 'half': from the second step on, max_grad_norm becomes half the norm of the very gradient pa_grad_norm is about to read --
    the folded, exchanged one -- formed in float64 by torch just in front of that launch (_clip_coef), so the coefficient is about 0.5
    at every such step.  (Half the FIRST step's norm does not clip the later ones: over its first three steps the norm of this untrained
    net moves between 12 and 1266, see check_clip.)"""
    plain = opt._clip_coef

    def clip(n, gscale):
        if steps['half']:
            opt.max_grad_norm = 0.5 * float((net.flat_grads.double() * _f32(gscale)).pow(2).sum().sqrt())
        return plain(n, gscale)
    opt._clip_coef = clip


def drive(c, net, opt, ema, batches_of, rec, tap=None, poison_here=False, max_norms=None):
    """the optimizer steps of case c: per step the backward passes of batches_of(t), accumulate() after all but the last, step(), the EMA
    update; everything recorded into rec['steps'].  max_norms: the max_grad_norm of every step, from another run's record"""
    keep = _Keep()
    acc_ptrs = []
    auto = dict(half=False)
    if c['clip'] == 'half' and max_norms is None:
        _half_the_norm(opt, net, auto)
    for t in range(c['steps']):
        ids = batches_of(t)
        st = dict(micro=[], pending_seen=[], poisoned=False)
        if tap is not None:
            tap.events = []
        for j, b in enumerate(ids):
            net.loss_and_backward(*batch(b, c['res']))
            if c['poison'] and t == c['poison']['step'] and j == c['poison']['micro']:
                st['poisoned'] = True
                if poison_here:
                    net.flat_grads[POISON_AT] = float('inf')
            if not c['overlap']:
                st['micro'].append(_cpu(net.flat_grads))
            if j < len(ids) - 1:
                opt.accumulate()
                st['pending_seen'].append(opt.pending)
        st['early'] = len(tap.events) if tap is not None else 0          # exchanges in micro-batches that do not end the group
        if c['clip']:
            opt.max_grad_norm = max_norms[t] if max_norms is not None else LARGE          # LARGE: the norm is recorded, the coefficient exactly 1
            auto['half'] = c['clip'] == 'half' and t > 0
        st['before'] = _snapshot(net, opt, keep)
        opt.step()
        torch.cuda.synchronize()
        st['max_norm'] = opt.max_grad_norm
        st['after'] = _snapshot(net, opt, keep)
        st['exchanges'] = list(tap.events) if tap is not None else []
        st['norm_out'] = None if opt._norm_out is None else _cpu(opt._norm_out)
        norm = opt.last_grad_norm()
        st['last_grad_norm'] = None if norm is None else float(norm)
        st['adam'] = A.read_state(opt._state) if hasattr(opt, 'exp_avg') else None
        st['flag'] = st['adam']['flag'] if st['adam'] is not None else int(opt._skip_state[0])
        st['pending'] = opt.pending
        acc_ptrs.append(0 if opt._acc is None else opt._acc.data_ptr())
        if ema is not None:
            tw = ema.module
            e = dict(s0=M.read_state(ema._state), p0=keep('ema_p', tw.flat_params), b0=keep('ema_b', tw.flat_buffers))
            ema.update(opt)
            torch.cuda.synchronize()
            e.update(s1=M.read_state(ema._state), p1=keep('ema_p', tw.flat_params), b1=keep('ema_b', tw.flat_buffers))
            st['ema'] = e
        else:
            st['ema'] = None
        rec['steps'].append(st)
    rec['acc_ptrs'] = acc_ptrs
    rec['final'] = dict(skipped=opt.skipped_steps(), steps_taken=opt.steps_taken() if hasattr(opt, 'steps_taken') else opt.steps,
                        pending=opt.pending, ema_updates=None if ema is None else ema.updates(), ema_held=None if ema is None else ema.held())


def _new_record(c, rank, world, net):
    from pose_adv_aug_amd import _lib
    return dict(case=c, rank=rank, world=world, grad_scale=float(_lib.grad_scale()), dtype=int(_lib.lib().pa_dtype()),
                start=_cpu(net.flat_params), nparams=net.flat_params.numel(), steps=[])


def run_case(c, rank, world, tap):
    """case c on this rank of a process group"""
    from pose_adv_aug_amd.stack_hg import broadcast_parameters
    from pose_adv_aug_amd.utils.optim import ModelEma
    net = make_net(c, 100 + rank)                          # replicas start DIFFERENT: the broadcast must fix that
    broadcast_parameters(net)
    torch.cuda.synchronize()
    opt = make_opt(c, net)
    ema = ModelEma(net, **c['ema']) if c['ema'] else None
    rec = _new_record(c, rank, world, net)
    tap.net, tap.events, tap.clone = net, [], not c['overlap']
    N = c['N']
    drive(c, net, opt, ema, lambda t: [1000 * rank + t * N + j for j in range(N)], rec, tap, poison_here=rank == 1)
    tap.net = None
    return rec


def run_single(c, max_norms=None):
    """case c (N = 1) in ONE process that accumulates the two shards: from rank 0's initialisation (what the broadcast hands every rank),
    per step shard 0's backward pass, accumulate(), shard 1's backward pass, step().  max_norms: the ranks' max_grad_norm per step."""
    from pose_adv_aug_amd.utils.optim import ModelEma
    assert c['N'] == 1 and not c['poison'] and not c['overlap']
    net = make_net(c, 100)
    rec = _new_record(c, 0, 1, net)
    opt = make_opt(c, net)
    ema = ModelEma(net, **c['ema']) if c['ema'] else None
    drive(c, net, opt, ema, lambda t: [t, 1000 + t], rec, max_norms=max_norms if c['clip'] else None)
    return rec


def run_loop(c, rank, world, tap):
    """stack_hg.train over 3 synthetic batches with accum_steps 2 on this rank: groups [2, 1], the trailing short group included"""
    import types
    from pose_adv_aug_amd import stack_hg
    from pose_adv_aug_amd.data import Augmenter
    from pose_adv_aug_amd.utils.optim import ModelEma, RMSprop
    from tests import test_gpu_accum as T
    net = T._loop_net(seed=100 + rank)
    stack_hg.broadcast_parameters(net)
    opt = RMSprop(net)
    ema = ModelEma(net, decay=0.9)
    rec = _new_record(c, rank, world, net)
    groups, lines, step = [], [], opt.step
    opt.step = lambda: (groups.append(opt.pending + 1), step())[1]
    tap.net, tap.events, tap.clone = net, [], False
    o = types.SimpleNamespace(print_freq=2, accum_steps=2, bs=2)
    stack_hg.train(T._batches(3), net, opt, Augmenter(seed=50 + rank), 0, o, log=lines.append if rank == 0 else (lambda m: None), ema=ema)
    torch.cuda.synchronize()
    keep = _Keep()
    rec.update(groups=groups, lines=lines, exchanges=[e['whole'] for e in tap.events], after=_snapshot(net, opt, keep),
               ema_p=_cpu(ema.module.flat_params), ema_b=_cpu(ema.module.flat_buffers), ema_state=M.read_state(ema._state),
               final=dict(skipped=opt.skipped_steps(), steps_taken=opt.steps, pending=opt.pending, ema_updates=ema.updates(), ema_held=ema.held()))
    tap.net = None
    return rec


def worker(rank, world, init, out, cases):
    """one rank: the set-up of tests/test_gpu_dist._worker, then every case on the one process group.  out['dir']: where the records
    go; out[rank]: {case name: file}, extended as the cases finish (the parent's deadline message names them)."""
    from tests._rendezvous import engine_rank_env, set_env
    set_env(rank, world, init, **engine_rank_env(rank))
    import torch.distributed as dist
    from pose_adv_aug_amd.stack_hg import init_distributed
    init_distributed()
    tap = Tap(dist)
    done = {}
    for c in cases:
        rec = (run_loop if c['loop'] else run_case)(c, rank, world, tap)
        path = os.path.join(out['dir'], 'rank%d_%s.pt' % (rank, c['name']))
        torch.save(rec, path)
        del rec
        done[c['name']] = path
        out[rank] = dict(done)
    dist.barrier()
    dist.destroy_process_group()


class RanksLate(AssertionError):
    pass


def run_ranks(cases, world=2, deadline=None):
    """Spawn the ranks, join them with a deadline (a mismatch of collective counts between ranks must end as a failure here, not as
    the process group's own timeout half an hour later: the children are terminated, nothing is tried again).  Returns a generator of
    (case, [record of rank 0, record of rank 1, ...]) that loads one case at a time and removes the files behind it."""
    import torch.multiprocessing as mp
    from tests._rendezvous import file_init_method
    deadline = deadline_for(cases) if deadline is None else deadline
    ctx = mp.get_context('spawn')
    mgr = ctx.Manager()
    out = mgr.dict()
    folder = tempfile.mkdtemp(prefix='poseadv_dist_optim_')
    out['dir'] = folder
    try:
        pc = mp.spawn(worker, args=(world, file_init_method(), out, cases), nprocs=world, join=False)
        end = time.monotonic() + deadline
        while not pc.join(timeout=max(0.05, min(1.0, end - time.monotonic()))):
            if time.monotonic() >= end:
                reported = dict((r, sorted(out.get(r, {}))) for r in range(world))
                for p in pc.processes:
                    if p.is_alive():
                        p.terminate()
                for p in pc.processes:
                    p.join(10)
                    if p.is_alive():
                        p.kill()
                raise RanksLate('the %d ranks were still running after %d s (a collective that one rank never entered?); cases that had '
                                'reported, per rank: %s' % (world, deadline, reported))
        paths = dict((r, dict(out[r])) for r in range(world))
    except BaseException:
        shutil.rmtree(folder, ignore_errors=True)
        raise
    finally:
        mgr.shutdown()

    def records():
        try:
            for c in cases:
                yield c, [torch.load(paths[r][c['name']], weights_only=False) for r in range(world)]
        finally:
            shutil.rmtree(folder, ignore_errors=True)
    return records()


# ---------------------------------------------------------------------------------------------------------------------------------
# checks (CPU tensors only)
def _bits(x):
    return x if x.dtype == torch.int32 else x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def _differ(a, b):
    """elements whose bits differ (all of them for another shape)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return max(a.numel(), b.numel())
    return int((_bits(a) != _bits(b)).sum())


def _fold(gs):
    acc = gs[0]
    for g in gs[1:]:
        acc = acc + g
    return acc


def _whole(st):
    return [e for e in st['exchanges'] if e['whole']]


def _compare_arrays(what, a, b, fails, per_rank=PER_RANK):
    if sorted(a) != sorted(b):
        fails.append(('%s: the arrays are not the same set' % what, (sorted(a), sorted(b))))
        return
    for k in sorted(a):
        d = _differ(a[k], b[k])
        if k in per_rank:
            if d == 0:
                fails.append(('%s: %s is the same on both ranks (BatchNorm statistics are per rank)' % (what, k), 0))
        elif d:
            fails.append(('%s: %s differs between the ranks in this many elements' % (what, k), d))


def check_replicas(recs):
    """bit-identical replicas: everything but the BatchNorm buffers, which must differ"""
    fails = []
    r0 = recs[0]
    for r in recs[1:]:
        what0 = 'rank %d against rank 0' % r['rank']
        if _differ(r0['start'], r['start']):
            fails.append((what0 + ': the start weights differ after the broadcast', _differ(r0['start'], r['start'])))
        if len(r0['steps']) != len(r['steps']):
            fails.append((what0 + ': number of optimizer steps', (len(r0['steps']), len(r['steps']))))
        for t, (a, b) in enumerate(zip(r0['steps'], r['steps'])):
            what = '%s, step %d' % (what0, t)
            _compare_arrays(what + ' before', a['before'], b['before'], fails)
            _compare_arrays(what + ' after', a['after'], b['after'], fails)
            if (a['norm_out'] is None) != (b['norm_out'] is None) or (a['norm_out'] is not None and _differ(a['norm_out'], b['norm_out'])):
                fails.append((what + ': {norm, coefficient}', (a['norm_out'], b['norm_out'])))
            for k in ('adam', 'flag', 'last_grad_norm', 'pending', 'max_norm'):
                if a[k] != b[k]:
                    fails.append((what + ': ' + k, (a[k], b[k])))
            if (a['ema'] is None) != (b['ema'] is None):
                fails.append((what + ': one rank has an EMA', 0))
            elif a['ema'] is not None:
                for k in ('s0', 's1'):
                    if a['ema'][k] != b['ema'][k]:
                        fails.append((what + ': state of the EMA (%s)' % k, (a['ema'][k], b['ema'][k])))
                _compare_arrays(what + ', EMA', dict(p1=a['ema']['p1'], b1=a['ema']['b1']), dict(p1=b['ema']['p1'], b1=b['ema']['b1']), fails,
                                per_rank=('b1',))
        if r0['final'] != r['final']:
            fails.append((what0 + ': the final counts', (r0['final'], r['final'])))
    return fails


def check_exchange(recs):
    fails = []
    for t in range(len(recs[0]['steps'])):
        sts = [r['steps'][t] for r in recs]
        ok = True
        for r, st in zip(recs, sts):
            what = 'rank %d step %d' % (r['rank'], t)
            if len(_whole(st)) != 1 or len(st['exchanges']) != 1:
                fails.append((what + ': exchanges of the flat gradient in one optimizer step (whole, all)', (len(_whole(st)), len(st['exchanges']))))
                ok = False
            if st['early']:
                fails.append((what + ': exchanges in micro-batches that do not end their group', st['early']))
                ok = False
        if not ok:
            continue
        ex = [_whole(st)[0] for st in sts]
        for r, st, e in zip(recs, sts, ex):
            what = 'rank %d step %d' % (r['rank'], t)
            d = _differ(e['g_sum'], ex[0]['g_sum'])
            if d:
                fails.append((what + ': the summed gradient differs from rank 0\'s', d))
            d = AX.mismatches(e['g_local'], _fold(st['micro']))
            if d:
                fails.append((what + ': the exchanged gradient is not the fold ((g1 + g2) + ...) of the %d micro-batch gradients' % len(st['micro']), d))
        d = AX.mismatches(ex[0]['g_sum'], _fold([e['g_local'] for e in ex]))
        if d:
            fails.append(('step %d: the summed gradient is not the fp32 sum of the ranks\' gradients' % t, d))
    return fails


def expected_gscale(rec, st):
    """1 / (world (k + 1) grad_scale) with k micro-batches accumulated before the step's own"""
    return 1.0 / (rec['world'] * len(st['micro']) * rec['grad_scale'])


def _g_of(st):
    return _whole(st)[0]['g_sum'] if st['exchanges'] else _fold(st['micro'])


def _le1(fails, what, x):
    if not (x <= 1.0):
        fails.append((what, x))


def _domain(fails, what, g, dom):
    if float(dom.float().mean()) < 0.9:
        fails.append((what + ': less than 90 % of the gradient is in the bound\'s domain', float(dom.float().mean())))
    if not bool((g != 0).any()):
        fails.append((what + ': the gradient is all zero', 0))


def _check_rmsprop(rec, st, g, gscale, what, fails):
    kw = rec['case']['kw']
    mom, wd, centered = float(kw.get('momentum', 0)), float(kw.get('weight_decay', 0)), bool(kw.get('centered', False))
    b, a = st['before'], st['after']
    gs = g.double() * _f32(gscale)
    if mom == 0 and wd == 0 and not centered and not rec['case']['clip']:
        dom = (gs == 0) | (gs.abs() >= DOMAIN)
        _domain(fails, what, g, dom)
        rp, rv = O.check(b['flat_params'][dom], g[dom], b['square_avg'][dom], a['flat_params'][dom], a['square_avg'][dom], gscale)
        _le1(fails, what + ': p', rp)
        _le1(fails, what + ': square_avg', rv)
        return
    coef = float(st['norm_out'][1]) if rec['case']['clip'] else None
    gr = gs * (1.0 if coef is None else coef) + _f32(wd) * b['flat_params'].double()
    dom = ((gr == 0) | (gr.abs() >= DOMAIN)) & ((g == 0) | (gs.abs() >= DOMAIN))
    _domain(fails, what, g, dom)
    names = {'p': 'flat_params', 'square_avg': 'square_avg', 'momentum_buffer': 'momentum_buffer', 'grad_avg': 'grad_avg'}
    sel = lambda d: dict((k, d[n][dom] if n in d else None) for k, n in names.items())
    r, reach = Y.check(sel(b), g[dom], sel(a), gscale, coef, mom, wd, centered)
    for k, x in r.items():
        _le1(fails, '%s: %s' % (what, k), x)
    if reach:
        fails.append((what + ': intervals of v - ga^2 that reach 0', reach))


def _check_adam(rec, st, g, gscale, t_applied, what, fails):
    kw = rec['case']['kw']
    wd = float(kw.get('weight_decay', 1e-2 if rec['case']['opt'] == 'AdamW' else 0))
    dec = rec['case']['opt'] == 'AdamW' or bool(kw.get('decoupled_weight_decay', False))
    ams = bool(kw.get('amsgrad', False))
    b, a, c = st['before'], st['after'], st['adam']
    for k, x in A.check_consts(c, t_applied).items():
        _le1(fails, '%s: %s of Adam\'s state at t = %d' % (what, k, t_applied), x)
    if c['flag'] != 0:
        fails.append((what + ': Adam\'s skip flag on an applied step', c['flag']))
    coef = float(st['norm_out'][1]) if rec['case']['clip'] else None
    gs = g.double() * _f32(gscale)
    gr = gs * (1.0 if coef is None else coef)
    if wd != 0 and not dec:
        gr = gr + _f32(wd) * b['flat_params'].double()
    dom = ((gr == 0) | (gr.abs() >= DOMAIN)) & ((g == 0) | (gs.abs() >= DOMAIN))
    _domain(fails, what, g, dom)
    names = {'p': 'flat_params', 'exp_avg': 'exp_avg', 'exp_avg_sq': 'exp_avg_sq', 'max_exp_avg_sq': 'max_exp_avg_sq'}
    sel = lambda d: dict((k, d[n][dom] if n in d else None) for k, n in names.items())
    r, _ = A.check(sel(b), g[dom], sel(a), gscale, coef, c, wd, dec, ams)
    for k, x in r.items():
        _le1(fails, '%s: %s' % (what, k), x)


def _check_ema(rec, st, skipped, what, fails):
    kw, e = rec['case']['ema'], st['ema']
    decay, warmup, copy = kw.get('decay', 0.999), bool(kw.get('warmup', False)), kw.get('buffers', 'ema') == 'copy'
    for word in M.check_state(e['s0'], e['s1'], decay, warmup, 1 if skipped else 0):
        fails.append((what + ': state word of the EMA (name, got, expected)', word))
    _le1(fails, what + ': parameters of the average', M.check_arrays(e['p0'], st['after']['flat_params'], e['p1'], e['s1']))
    _le1(fails, what + ': buffers of the average', M.check_arrays(e['b0'], st['after']['flat_buffers'], e['b1'], e['s1'], copy=copy))
    if not skipped and (_differ(e['p0'], e['p1']) == 0 or _differ(e['b0'], e['b1']) == 0):
        fails.append((what + ': the average did not move', 0))


def skipped_steps_of(rec):
    """indices of the optimizer steps the case poisons (the fp16 build skips them on every rank)"""
    return [t for t, st in enumerate(rec['steps']) if st['poisoned']]


def check_steps(rec):
    """every applied step, the norm in front of it and the EMA update behind it in float64, with the existing checks and bounds"""
    fails = []
    c = rec['case']
    applied = 0
    for t, st in enumerate(rec['steps']):
        what = '%s rank %d step %d' % (c['name'], rec['rank'], t)
        skipped = st['poisoned']
        if rec['world'] > 1 and len(_whole(st)) != 1:
            fails.append((what + ': no single exchanged gradient to check the step with', len(_whole(st))))
            continue
        g, gscale = _g_of(st), expected_gscale(rec, st)
        if not skipped:
            applied += 1
            if c['clip']:
                rn, rc = Y.check_norm(g, gscale, st['max_norm'], st['norm_out'])
                _le1(fails, what + ': norm of the exchanged gradient', rn)
                _le1(fails, what + ': clip coefficient', rc)
                if st['last_grad_norm'] != float(st['norm_out'][0]):
                    fails.append((what + ': last_grad_norm() is not the recorded norm', (st['last_grad_norm'], float(st['norm_out'][0]))))
            if c['opt'] == 'RMSprop':
                _check_rmsprop(rec, st, g, gscale, what, fails)
            else:
                _check_adam(rec, st, g, gscale, applied, what, fails)
            if _differ(st['before']['flat_params'], st['after']['flat_params']) == 0:
                fails.append((what + ': the parameters did not move', 0))
        if st['ema'] is not None:
            _check_ema(rec, st, skipped, what, fails)
    return fails


def check_clip(rec):
    fails = []
    c = rec['case']
    norms = [None if st['norm_out'] is None else float(st['norm_out'][0]) for st in rec['steps']]
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        print('dist_optim_exact %s rank %d: norms %s coefficients %s' % (c['name'], rec['rank'], norms,
                                                                        [None if st['norm_out'] is None else float(st['norm_out'][1]) for st in rec['steps']]))
    for t, st in enumerate(rec['steps']):
        if not c['clip'] or st['poisoned']:
            continue
        coef = float(st['norm_out'][1])
        half = c['clip'] == 'half' and t > 0
        if (half and not coef < 1.0) or (not half and coef != 1.0):
            fails.append(('%s rank %d step %d: coefficient with max_grad_norm %g (norms of the steps: %s)' % (c['name'], rec['rank'], t, st['max_norm'], norms), coef))
        if not half and st['max_norm'] != LARGE:
            fails.append(('%s rank %d step %d: max_grad_norm of an unclipped step' % (c['name'], rec['rank'], t), st['max_norm']))
        if half and st['micro']:          # the bound the step ran with is half the float64 norm of the gradient it consumed (1e-9: the order of a double sum)
            want = 0.5 * float((_g_of(st).double() * _f32(expected_gscale(rec, st))).pow(2).sum().sqrt())
            if not abs(st['max_norm'] - want) <= 1e-9 * want:
                fails.append(('%s rank %d step %d: max_grad_norm is not half the norm of the exchanged gradient' % (c['name'], rec['rank'], t), (st['max_norm'], want)))
    return fails


def check_accum(rec):
    fails = []
    c = rec['case']
    for t, st in enumerate(rec['steps']):
        what = '%s rank %d step %d' % (c['name'], rec['rank'], t)
        if len(st['micro']) != c['N'] or st['pending_seen'] != list(range(1, c['N'])):
            fails.append((what + ': micro-batches / pending after each accumulate()', (len(st['micro']), st['pending_seen'])))
        if st['pending'] != 0:
            fails.append((what + ': pending after the step', st['pending']))
    ptrs = set(rec['acc_ptrs'])
    if len(ptrs) != 1 or (0 in ptrs) != (c['N'] == 1):
        fails.append(('%s rank %d: _acc allocated once, and only when accumulating' % (c['name'], rec['rank']), sorted(ptrs)))
    if rec['final']['pending'] != 0:
        fails.append(('%s rank %d: pending at the end' % (c['name'], rec['rank']), rec['final']['pending']))
    return fails


def check_skips(recs):
    """fp16 build: the step whose gradient rank 1 poisoned is skipped on EVERY rank, and only that one"""
    fails = []
    for rec in recs:
        c = rec['case']
        poisoned = skipped_steps_of(rec)
        applied = 0
        for t, st in enumerate(rec['steps']):
            what = '%s rank %d step %d' % (c['name'], rec['rank'], t)
            moved = [(k, _differ(st['before'][k], st['after'][k])) for k in sorted(st['before'])
                     if k not in PER_RANK and k not in WORDS and _differ(st['before'][k], st['after'][k])]
            if st['poisoned']:
                if len(_whole(st)) == 1 and not bool(torch.isinf(_whole(st)[0]['g_sum'][POISON_AT])):
                    fails.append((what + ': the inf did not reach the exchanged gradient', float(_whole(st)[0]['g_sum'][POISON_AT])))
                if moved:
                    fails.append((what + ': arrays changed on the step that must be skipped (name, elements)', moved))
                if st['flag'] != 1:
                    fails.append((what + ': the skip flag after the poisoned step', st['flag']))
                if st['ema'] is not None and (st['ema']['s1']['held'] != st['ema']['s0']['held'] + 1 or _differ(st['ema']['p0'], st['ema']['p1'])):
                    fails.append((what + ': the EMA moved, or did not count a held update', st['ema']['s1']))
            else:
                applied += 1
                if 'flat_params' not in [k for k, _ in moved]:
                    fails.append((what + ': the step was not applied', 0))
                if st['flag'] != 0:
                    fails.append((what + ': the skip flag after a finite step', st['flag']))
            if st['adam'] is not None and (st['adam']['step'], st['adam']['skipped']) != (applied, t + 1 - applied):
                fails.append((what + ': Adam\'s device (step, skipped)', (st['adam']['step'], st['adam']['skipped'])))
            if st['ema'] is not None and (st['ema']['s1']['updates'], st['ema']['s1']['held']) != (applied, t + 1 - applied):
                fails.append((what + ': the EMA\'s (updates, held)', (st['ema']['s1']['updates'], st['ema']['s1']['held'])))
        n, k = len(rec['steps']), len(poisoned)
        want = dict(skipped=k, steps_taken=n - k if c['opt'] != 'RMSprop' else n, pending=0,
                    ema_updates=n - k if c['ema'] else None, ema_held=k if c['ema'] else None)
        if rec['final'] != want:
            fails.append(('%s rank %d: final counts (got, expected)' % (c['name'], rec['rank']), (rec['final'], want)))
    return fails


def check_same_run(rec, other, what, buffers=False):
    """parameters, optimizer state, {norm, coefficient} and Adam's words of `rec` bit for bit those of `other`, step by step"""
    fails = []
    if _differ(rec['start'], other['start']):
        fails.append((what + ': the start weights differ', _differ(rec['start'], other['start'])))
    if len(rec['steps']) != len(other['steps']):
        return fails + [(what + ': number of optimizer steps', (len(rec['steps']), len(other['steps'])))]
    for t, (a, b) in enumerate(zip(rec['steps'], other['steps'])):
        for k in sorted(set(a['after']) | set(b['after'])):
            if k in PER_RANK and not buffers:
                continue
            if k not in a['after'] or k not in b['after']:
                fails.append(('%s step %d: %s exists in one run only' % (what, t, k), 0))
            elif _differ(a['after'][k], b['after'][k]):
                fails.append(('%s step %d: %s differs in this many elements' % (what, t, k), _differ(a['after'][k], b['after'][k])))
        if (a['norm_out'] is None) != (b['norm_out'] is None) or (a['norm_out'] is not None and _differ(a['norm_out'], b['norm_out'])):
            fails.append(('%s step %d: {norm, coefficient}' % (what, t), (a['norm_out'], b['norm_out'])))
        if a['adam'] != b['adam']:
            fails.append(('%s step %d: Adam\'s device state' % (what, t), (a['adam'], b['adam'])))
    return fails


def check_buckets(rec):
    """overlap=True: per step 2 asynchronous buckets (one per stack) and the remaining ranges, every gradient exchanged exactly once"""
    fails = []
    for t, st in enumerate(rec['steps']):
        what = '%s rank %d step %d' % (rec['case']['name'], rec['rank'], t)
        n_async = len([e for e in st['exchanges'] if e['async_op']])
        if n_async != 2:
            fails.append((what + ': asynchronous buckets', n_async))
        if sum(e['numel'] for e in st['exchanges']) != rec['nparams']:
            fails.append((what + ': elements exchanged, of %d' % rec['nparams'], sum(e['numel'] for e in st['exchanges'])))
        spans = sorted((e['offset'], e['offset'] + e['numel']) for e in st['exchanges'])
        if any(a[1] != b[0] for a, b in zip(spans, spans[1:])) or not spans or spans[0][0] != 0 or spans[-1][1] != rec['nparams']:
            fails.append((what + ': the exchanged ranges do not tile the flat gradient', spans))
    return fails


def check_loop(recs):
    """run_loop's records: groups [2, 1] and two exchanges on every rank, two EMA updates, the effective-batch line once on the rank that
    logs, identical replicas"""
    fails = []
    world = recs[0]['world']
    line = 'effective batch 2 x 2 x %d rank(s) = %d' % (world, 4 * world)
    for r in recs:
        what = 'rank %d' % r['rank']
        if r['groups'] != [2, 1]:
            fails.append((what + ': group sizes at the optimizer steps', r['groups']))
        if r['exchanges'] != [True, True]:
            fails.append((what + ': exchanges of the flat gradient (True: the whole array)', r['exchanges']))
        want = dict(skipped=0, steps_taken=2, pending=0, ema_updates=2, ema_held=0)
        if r['final'] != want:
            fails.append((what + ': final counts (got, expected)', (r['final'], want)))
        said = sum(line in l for l in r['lines'])
        if said != (1 if r['rank'] == 0 else 0):
            fails.append((what + ': lines that say "%s"' % line, said))
        if r is not recs[0]:
            _compare_arrays(what + ' against rank 0', recs[0]['after'], r['after'], fails)
            _compare_arrays(what + ' against rank 0, EMA', dict(p=recs[0]['ema_p'], b=recs[0]['ema_b']), dict(p=r['ema_p'], b=r['ema_b']), fails,
                            per_rank=('b',))
            if r['ema_state'] != recs[0]['ema_state']:
                fails.append((what + ': state of the EMA', (r['ema_state'], recs[0]['ema_state'])))
        if _differ(r['start'], recs[0]['start']) or _differ(r['start'], r['after']['flat_params']) == 0:
            fails.append((what + ': start weights differ between the ranks, or the loop did not move them', 0))
    return fails


def check_case(recs, single=None):
    """every check that applies to the records of one case (one per rank): [(check name, failures)]"""
    c = recs[0]['case']
    out = [('replicas', check_replicas(recs))]
    if not c['overlap']:
        out.append(('exchange', check_exchange(recs)))
        out.append(('float64 steps', check_steps(recs[0])))          # (rank 1 holds the same bits: check_replicas)
        out.append(('accumulation', [f for r in recs for f in check_accum(r)]))
    else:
        out.append(('buckets', [f for r in recs for f in check_buckets(r)]))
    if c['clip']:
        out.append(('clip coefficient', [f for r in recs for f in check_clip(r)]))
    out.append(('skipped steps', check_skips(recs)))
    if single is not None:
        out.append(('one process accumulating both shards', check_same_run(recs[0], single, 'two ranks against one process')))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp16 build: rank 1 alone poisons step 2 of 3.
# These cases run the 1-stack chan-128 net at 256 x 256, not at 64 x 64.  The library's gradient scale is a constant (32768) sized for the
# 64 x 64 heat maps of a 256 input; the heat-map gradient carries 1 / (B 16 H H), so at 16 x 16 maps every element is 16 times larger and
# the untrained net overflows IEEE half by itself.  Measured on two ranks without any planted inf: at 64 x 64 step 1 of 3 was skipped on
# both ranks in every case (397952 and 352704 non-finite gradient elements; finite scaled gradients up to 3.5e5 against half's 65504)
# and a later step again with Adam and with N = 2; at 256 x 256 no step was skipped and the largest scaled gradient was 930.  A step that
# skips itself would make "exactly the poisoned step is skipped" meaningless.
EMA = dict(decay=0.9)
FP16_RES = 256
FP16_CASES = (case('fp16_rmsprop', 'RMSprop', ema=EMA, res=FP16_RES, poison=dict(step=1, micro=0)),
              case('fp16_adam', 'Adam', ema=EMA, res=FP16_RES, poison=dict(step=1, micro=0)),
              case('fp16_rmsprop_accum2', 'RMSprop', N=2, ema=EMA, res=FP16_RES, poison=dict(step=1, micro=0)))
FP16_MARKER = 'FP16 DIST OPTIM EXACT '

if __name__ == '__main__':          # tests/test_gpu_dist_optim.py runs this with POSEADV_DTYPE=fp16; this process itself opens no GPU
    assert os.environ.get('POSEADV_DTYPE') == 'fp16', 'run with POSEADV_DTYPE=fp16'
    bad = 0
    for c, recs in run_ranks(list(FP16_CASES)):
        results = check_case(recs)
        results.append(('the ranks ran the IEEE-half library with its gradient scale',
                        [('dtype, grad_scale', (r['dtype'], r['grad_scale'])) for r in recs if r['dtype'] != 1 or not r['grad_scale'] > 1]))
        results.append(('the case poisons exactly one step', [] if skipped_steps_of(recs[0]) == [1] else [('poisoned steps', skipped_steps_of(recs[0]))]))
        for name, fails in results:
            bad += len(fails)
            print('%s %s: %s%s' % ('FAIL' if fails else 'PASS', c['name'], name, ' %s' % (fails[:6],) if fails else ''), flush=True)
    print(FP16_MARKER + ('PASSED' if not bad else 'FAILED'), flush=True)
    sys.exit(1 if bad else 0)

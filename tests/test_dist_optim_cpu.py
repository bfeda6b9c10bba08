"""CPU checks of tests/dist_optim_exact.py: its check functions accept records of the shape the two-rank worker writes, filled by an fp32
emulation of what two data-parallel ranks launch (the fold of accumulate(), the all-reduce, pa_grad_norm, the step kernels as
tests/test_optim_exact_cpu.py, test_optim_opts_cpu.py and test_adam_cpu.py emulate them, ema_exact.emulate), and report each planted
defect: a gscale without 1/world or without 1/(k + 1), the norm of the local gradient, an exchange per micro-batch, the fold behind the
exchange, a step that one rank did not skip, Adam's step count advanced on a skipped step, an EMA that moved on one, one replica's
momentum buffer off by one ulp in four elements."""
import numpy as np
import pytest
import torch

from tests import dist_optim_exact as D
from tests import ema_exact as M
from tests import optim_exact as X
from tests.test_adam_cpu import _consts as adam_consts, _emulate as adam_emulate
from tests.test_optim_exact_cpu import _emulate as rmsprop_emulate
from tests.test_optim_opts_cpu import _emulate as opts_emulate

N_PARAMS, N_BUFFERS, WORLD = 20011, 64, 2
f = np.float32
t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def _add(a, b):
    with np.errstate(all='ignore'):
        return (a + b).astype(np.float32)


def _fold(gs):
    acc = gs[0].copy()
    for g in gs[1:]:
        acc = _add(acc, g)
    return acc


def _norm_out(g, gscale, max_norm):
    """pa_grad_norm on the host: the squares and their sum in double, one rounding; the coefficient in fp32"""
    norm = f(np.sqrt(((g.astype(np.float64) * float(f(gscale))) ** 2).sum()))
    coef = min(f(1), f(max_norm) / (norm + f(1e-6)))
    return np.array([norm, coef], dtype=np.float32)


def _adam_words(flag, skipped, c):
    ints = np.array([flag, skipped, c['step'], 0], dtype=np.int32)
    return np.concatenate([ints, np.array([c['bc1'], c['bc2'], c['step_size'], c['bc2s']], dtype=np.float32).view(np.int32)])


class _Rank(object):
    """the host model of one rank's net, optimizer and EMA"""
    def __init__(self, c, rank):
        r = np.random.Generator(np.random.PCG64([5, N_PARAMS]))
        self.c, self.rank = c, rank
        self.p = r.standard_normal(N_PARAMS).astype(np.float32)               # (the same on every rank: the broadcast)
        self.buffers = np.random.Generator(np.random.PCG64([6, rank])).standard_normal(N_BUFFERS).astype(np.float32)
        z = lambda: np.zeros(N_PARAMS, dtype=np.float32)
        kw = c['kw']
        if c['opt'] == 'RMSprop':
            self.state = {'square_avg': z()}
            if kw.get('momentum', 0) > 0:
                self.state['momentum_buffer'] = z()
            if kw.get('centered'):
                self.state['grad_avg'] = z()
            self.words = ('_skip_state', np.zeros(2, dtype=np.int32))
        else:
            self.state = {'exp_avg': z(), 'exp_avg_sq': z()}
            self.adam = dict(flag=0, skipped=0, step=0, bc1=0.0, bc2=0.0, step_size=0.0, bc2s=0.0)
            self.words = ('_state', _adam_words(0, 0, self.adam))
        self.flag = self.skipped = 0
        if c['ema']:
            self.ema = dict(p=self.p.copy(), b=self.buffers.copy(), s=dict(updates=0, held=0, apply=0, reserved=0, w=0.0, decay_used=0.0))

    def arrays(self):
        d = dict((k, t_(v.copy())) for k, v in self.state.items())
        d.update(flat_params=t_(self.p.copy()), flat_buffers=t_(self.buffers.copy()))
        d[self.words[0]] = t_(self.words[1].copy())
        return d

    def step(self, g, gscale, coef, skip, count_step_on_skip=False):
        c, kw = self.c, self.c['kw']
        self.flag = 1 if skip else 0
        self.skipped += self.flag
        if c['opt'] == 'RMSprop':
            self.words = ('_skip_state', np.array([self.flag, self.skipped], dtype=np.int32))
            if skip:
                return
            mom = float(kw.get('momentum', 0))
            with np.errstate(all='ignore'):
                if mom == 0 and coef is None:
                    self.p, self.state['square_avg'] = rmsprop_emulate(self.p, g, self.state['square_avg'], gscale)
                else:
                    out = opts_emulate(self.p, g, self.state['square_avg'], self.state.get('momentum_buffer'), None, gscale, coef, mom, 0.0, False)
                    self.p = out.pop('p')
                    self.state.update(out)
            return
        if not skip or count_step_on_skip:
            cc = adam_consts(self.adam['step'] + 1)
            cc['step'] = self.adam['step'] + 1
            self.adam.update(cc)
        self.adam.update(flag=self.flag, skipped=self.skipped)
        self.words = ('_state', _adam_words(self.flag, self.skipped, self.adam))
        if skip:
            return
        s = dict(p=self.p, exp_avg=self.state['exp_avg'], exp_avg_sq=self.state['exp_avg_sq'], max_exp_avg_sq=None)
        with np.errstate(all='ignore'):
            out = adam_emulate(s, g, gscale, coef, 0.0, False, False, self.adam)
        self.p = out.pop('p')
        self.state.update(out)

    def ema_update(self, flag):
        kw, e = self.c['ema'], self.ema
        rec = dict(s0=dict(e['s']), p0=t_(e['p'].copy()), b0=t_(e['b'].copy()))
        e['s'] = M.expected_state(e['s'], kw.get('decay', 0.999), kw.get('warmup', False), flag)
        if e['s']['apply']:
            e['p'], e['b'] = M.emulate(e['p'], self.p, e['s']['w']), M.emulate(e['b'], self.buffers, e['s']['w'])
        rec.update(s1=dict(e['s']), p1=t_(e['p'].copy()), b1=t_(e['b'].copy()))
        return rec


def fabricate(c, defect=None):
    """the records of two ranks running case c, with one defect planted"""
    ranks = [_Rank(c, r) for r in range(WORLD)]
    recs = [dict(case=c, rank=r, world=WORLD, grad_scale=1.0, dtype=0, start=t_(ranks[r].p.copy()), nparams=N_PARAMS, steps=[], acc_ptrs=[])
            for r in range(WORLD)]
    N = c['N']
    for t in range(c['steps']):
        poisoned = bool(c['poison']) and t == c['poison']['step']
        micro = [[X.make_inputs(N_PARAMS, 7000 + 100 * r + 10 * t + j, 1.0, True)[1] for j in range(N)] for r in range(WORLD)]
        if poisoned:
            micro[1][c['poison']['micro']][D.POISON_AT] = np.inf
        local = [_fold(m) for m in micro]
        if defect == 'fold after the exchange':                    # the last micro-batch gradient alone goes to the ranks ...
            local = [m[-1].copy() for m in micro]
        g_sum = _fold(local)
        used = g_sum
        if defect == 'fold after the exchange':                    # ... and the rank's own sum of the earlier ones is added behind it
            used = None
        gscale = 1.0 / (WORLD * N)
        if defect == 'gscale without 1/world':
            gscale = 1.0 / N
        if defect == 'gscale without 1/(k+1)':
            gscale = 1.0 / WORLD
        for r, (rk, rec) in enumerate(zip(ranks, recs)):
            rk.buffers = (rk.buffers * f(0.9) + f(0.1) * f(1 + r + t)).astype(np.float32)          # a forward pass moved the statistics
            g = used if used is not None else _add(_fold(micro[r][:-1]), g_sum)
            st = dict(micro=[t_(m.copy()) for m in micro[r]], pending_seen=list(range(1, N)), poisoned=poisoned,
                      early=N - 1 if defect == 'two exchanges in a group' else 0)
            max_norm = coef = norm_out = None
            if c['clip']:
                max_norm = D.LARGE if (c['clip'] == 'large' or t == 0) else \
                    0.5 * float(np.sqrt(((g.astype(np.float64) * float(f(gscale))) ** 2).sum()))          # half the norm of what the step consumes
                norm_out = _norm_out(local[r] if defect == 'norm of the local gradient' else g, gscale, max_norm)
                coef = float(norm_out[1])
            st['max_norm'] = max_norm
            st['before'] = rk.arrays()
            skip = poisoned and not (defect == 'one rank did not skip' and r == 0)
            rk.step(local[r] if (poisoned and not skip) else g, gscale, coef, skip, count_step_on_skip=defect == 'Adam step advanced on a skip')
            if defect == 'momentum off by one ulp' and r == 1 and t == 1:
                buf = rk.state['momentum_buffer']
                buf[1000:1004] = np.nextafter(buf[1000:1004], f(np.inf))
            st['after'] = rk.arrays()
            st['exchanges'] = [dict(numel=N_PARAMS, offset=0, async_op=False, whole=True, g_local=t_(local[r].copy()), g_sum=t_(g_sum.copy()))]
            st['norm_out'] = None if norm_out is None else t_(norm_out)
            st['last_grad_norm'] = None if norm_out is None else float(norm_out[0])
            st['adam'] = dict(rk.adam) if c['opt'] != 'RMSprop' else None
            st['flag'], st['pending'] = rk.flag, 0
            st['ema'] = rk.ema_update(0 if defect == 'EMA moved on a skip' else rk.flag) if c['ema'] else None
            rec['steps'].append(st)
            rec['acc_ptrs'].append(4096 if N > 1 else 0)
    for rk, rec in zip(ranks, recs):
        n = c['steps']
        rec['final'] = dict(skipped=rk.skipped, steps_taken=rk.adam['step'] if c['opt'] != 'RMSprop' else n, pending=0,
                            ema_updates=rk.ema['s']['updates'] if c['ema'] else None, ema_held=rk.ema['s']['held'] if c['ema'] else None)
    return recs


ACCUM = D.case('rmsprop_accum2', N=2)
CLIP = D.case('rmsprop_momentum_clip', kw=dict(momentum=0.9), clip='half')
SKIP = D.case('adam_ema_skip', 'Adam', ema=dict(decay=0.9, warmup=True), poison=dict(step=1, micro=0))
SKIP_RMS = D.case('rmsprop_ema_skip', ema=dict(decay=0.9), poison=dict(step=1, micro=0))


def _failed(recs):
    return dict((name, fails) for name, fails in D.check_case(recs) if fails)


@pytest.mark.parametrize('c', (ACCUM, CLIP, SKIP, SKIP_RMS, D.case('adam_clip_accum3', 'Adam', clip='half', N=3), D.case('adam_large', 'Adam', clip='large')),
                         ids=lambda c: c['name'])
def test_the_emulated_ranks_pass_every_check(c):
    recs = fabricate(c)
    results = D.check_case(recs)
    assert [name for name, _ in results][:2] == ['replicas', 'exchange'] and 'float64 steps' in [name for name, _ in results]
    assert not _failed(recs), _failed(recs)
    assert D.skipped_steps_of(recs[0]) == ([1] if c['poison'] else [])
    if c['clip'] == 'half':
        assert all(float(st['norm_out'][1]) < 1.0 for st in recs[0]['steps'][1:]) and float(recs[0]['steps'][0]['norm_out'][1]) == 1.0
    assert D.expected_gscale(recs[0], recs[0]['steps'][0]) == 1.0 / (WORLD * c['N'])


# defect -> (the case it is planted in, the checks that must report it)
DEFECTS = {'gscale without 1/world': (ACCUM, ('float64 steps',)),
           'gscale without 1/(k+1)': (ACCUM, ('float64 steps',)),
           'norm of the local gradient': (CLIP, ('float64 steps', 'replicas')),
           'two exchanges in a group': (ACCUM, ('exchange',)),
           'fold after the exchange': (ACCUM, ('exchange',)),
           'one rank did not skip': (SKIP, ('skipped steps', 'replicas')),
           'Adam step advanced on a skip': (SKIP, ('skipped steps', 'float64 steps')),
           'EMA moved on a skip': (SKIP_RMS, ('skipped steps', 'float64 steps')),
           'momentum off by one ulp': (CLIP, ('replicas',))}


@pytest.mark.parametrize('defect', sorted(DEFECTS))
def test_each_defect_is_reported(defect):
    c, checks = DEFECTS[defect]
    failed = _failed(fabricate(c, defect))
    print(defect, dict((k, v[:3]) for k, v in failed.items()))
    for name in checks:
        assert failed.get(name), (defect, name, sorted(failed))


def test_what_the_reports_say():
    """the figures behind four of the reports: where, how many elements, which word"""
    failed = _failed(fabricate(CLIP, 'momentum off by one ulp'))
    assert failed['replicas'] == [('rank 1 against rank 0, step 1 after: momentum_buffer differs between the ranks in this many elements', 4),
                                  ('rank 1 against rank 0, step 2 before: momentum_buffer differs between the ranks in this many elements', 4)] \
        or failed['replicas'][0][1] == 4                                   # (the later steps inherit the four elements and spread them to p)
    failed = _failed(fabricate(ACCUM, 'two exchanges in a group'))
    assert all('do not end their group' in what and n == 1 for what, n in failed['exchange']) and len(failed['exchange']) == 2 * ACCUM['steps']
    failed = _failed(fabricate(ACCUM, 'fold after the exchange'))
    assert all('is not the fold' in what and n > N_PARAMS // 2 for what, n in failed['exchange'])
    failed = _failed(fabricate(SKIP, 'Adam step advanced on a skip'))
    assert any('Adam\'s device (step, skipped)' in what and got == (2, 1) for what, got in failed['skipped steps'])
    assert any(what.endswith('step of Adam\'s state at t = 2') for what, _ in failed['float64 steps'])
    # a gscale that lacks a factor of 2 is far outside the bound, not at its edge
    failed = _failed(fabricate(ACCUM, 'gscale without 1/world'))
    assert all(x > 1e3 for what, x in failed['float64 steps'] if what.endswith(': p'))


def test_the_same_run_check_and_the_bucket_check():
    a, b = fabricate(CLIP)[0], fabricate(CLIP)[0]
    assert D.check_same_run(a, b, 'twice') == []
    wrong = fabricate(CLIP, 'gscale without 1/world')[0]
    fails = D.check_same_run(a, wrong, 'against a run with another gscale')
    assert fails and any('flat_params differs' in what for what, _ in fails) and any('{norm, coefficient}' in what for what, _ in fails)
    ok = [dict(numel=8000, offset=6000, async_op=True, whole=False), dict(numel=6011, offset=14000, async_op=True, whole=False),
          dict(numel=6000, offset=0, async_op=False, whole=False)]
    rec = dict(case=D.case('overlap', overlap=True), rank=0, nparams=N_PARAMS, steps=[dict(exchanges=ok)])
    assert D.check_buckets(rec) == []
    rec['steps'][0]['exchanges'] = ok[:2] + [dict(ok[2], numel=6004)]              # four gradients exchanged twice
    assert len(D.check_buckets(rec)) == 2
    rec['steps'][0]['exchanges'] = [dict(ok[0], async_op=False)] + ok[1:]          # a bucket that was not overlapped
    assert len(D.check_buckets(rec)) == 1


def test_the_loop_check():
    z = lambda v: torch.full((8,), float(v))
    def rec(rank, **kw):
        d = dict(rank=rank, world=2, groups=[2, 1], exchanges=[True, True], start=z(0), lines=['gradient accumulation: 2 micro-batches per optimizer '
                 'step; effective batch 2 x 2 x 2 rank(s) = 8 (BatchNorm statistics stay per micro-batch)'] if rank == 0 else [],
                 final=dict(skipped=0, steps_taken=2, pending=0, ema_updates=2, ema_held=0), after=dict(flat_params=z(1), flat_buffers=z(2 + rank), square_avg=z(3)),
                 ema_p=z(4), ema_b=z(5 + rank), ema_state=dict(updates=2, held=0))
        d.update(kw)
        return d
    assert D.check_loop([rec(0), rec(1)]) == []
    assert D.check_loop([rec(0), rec(1, groups=[2, 2])])                      # a rank that did not step on the short trailing group
    assert D.check_loop([rec(0), rec(1, exchanges=[True, True, True])])
    assert D.check_loop([rec(0, lines=[]), rec(1)])
    assert D.check_loop([rec(0), rec(1, ema_b=z(5))])                         # averaged BatchNorm statistics must be per rank
    assert D.check_loop([rec(0), rec(1, ema_p=z(9))])


def test_the_deadline_ends_ranks_that_wait_for_each_other(monkeypatch, tmp_path):
    """run_ranks around two ranks that never finish (no GPU, no process group: both block once rank 0 has reported its first case).  The
    clock run_ranks reads jumps past the deadline at that moment, so nothing waits a deadline out: the children are terminated, and the
    failure names the cases that had reported."""
    import os
    import types
    marker = str(tmp_path / 'rank0_reported')
    monkeypatch.setenv('POSEADV_TEST_STUCK_MARKER', marker)
    monkeypatch.setattr(D, 'worker', _stuck_worker)
    monkeypatch.setattr(D, 'time', types.SimpleNamespace(monotonic=lambda: 1.0e9 if os.path.exists(marker) else 0.0))
    with pytest.raises(D.RanksLate, match=r"still running after 300 s.*\{0: \['first'\], 1: \[\]\}"):
        D.run_ranks([D.case('first'), D.case('second')], deadline=300)


def _stuck_worker(rank, world, init, out, cases):
    import os
    import threading
    if rank == 0:
        out[0] = {'first': 'nowhere'}
        open(os.environ['POSEADV_TEST_STUCK_MARKER'], 'w').close()
    threading.Event().wait()                                              # (ended by the parent's terminate())

"""CPU checks of gradient accumulation: the reference and the check of tests/accum_exact.py accept an fp32 emulation of what
accumulate() ... step() launch and reject each planted defect; accum_plan; the command line; the new symbol in both libraries, the header
and the export table; the refusals, which are decided on the host; the launch sequence of accumulate() and step() and the gscale they
hand to the step kernel, with a recorder in place of the library."""
import ctypes as C
import os
import types
import warnings

import numpy as np
import pytest
import torch

from tests import accum_exact as X

N = 100003
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


@pytest.fixture(scope='module')
def grads():
    return X.make_inputs(N, 7, count=4)


def _add(a, b):
    with np.errstate(all='ignore'):
        return (a + b).astype(np.float32)


def _protocol(groups, acc=None, copy_first=True):
    """what the optimizer launches, on the host: per group accumulate() for all but the last gradient (the first a copy into _acc, the
    later ones _acc = _acc + g), then the fold flat_grads = _acc + g of step().  Returns the folded gradient of every group.
    copy_first False plants the defect of a first micro-batch that is added onto whatever _acc held."""
    out = []
    for gs in groups:
        pending = 0
        for g in gs[:-1]:
            acc = g.copy() if (pending == 0 and (copy_first or acc is None)) else _add(acc, g)
            pending += 1
        out.append(_add(acc, gs[-1]) if pending else gs[-1].copy())
    return out


def test_the_emulated_protocol_is_the_reference_bit_for_bit(grads):
    for k in (1, 2, 3, 4):
        got = _protocol([grads[:k]])[0]
        assert X.mismatches(got, X.reference_sum(grads[:k])) == 0
    two = _protocol([grads[:2], grads[2:]])
    assert X.mismatches(two[1], X.reference_sum(grads[2:])) == 0          # the second group starts from a copy, not from the first's sum
    want = X.reference_sum(grads[:2])
    # the specials do what IEEE says, and the reference holds them
    a, b = grads[0], grads[1]
    assert np.isnan(want[np.isinf(a) & np.isinf(b) & (np.sign(a) != np.sign(b))]).all()
    den = (np.abs(want) > 0) & (np.abs(want) < X._TINY)
    assert den.sum() >= 3 and (np.isinf(want) & np.isfinite(a) & np.isfinite(b)).sum() >= 2          # denormal sums, overflowed sums
    assert (np.signbit(want) & (want == 0)).any()                                                      # -0 + -0 = -0


def test_a_nan_matches_any_nan_and_nothing_else():
    want = np.array([np.nan, 1.0, 0.0, -0.0], dtype=np.float32)
    other_nan = np.array([0x7fc00001], dtype=np.uint32).view(np.float32)[0]
    assert X.mismatches(np.array([other_nan, 1.0, 0.0, -0.0], dtype=np.float32), want) == 0
    assert X.mismatches(np.array([np.inf, 1.0, 0.0, -0.0], dtype=np.float32), want) == 1
    assert X.mismatches(np.array([np.nan, 1.0, -0.0, 0.0], dtype=np.float32), want) == 2             # the sign of a zero is a bit
    assert X.mismatches(np.array([np.nan, np.nan, 0.0, -0.0], dtype=np.float32), want) == 1          # a NaN where a number belongs


def test_each_defect_is_rejected(grads):
    g1, g2, g3, g4 = grads
    want = X.reference_sum(grads)
    # pairwise order (g1 + g2) + (g3 + g4)
    bad = X.mismatches(_add(_add(g1, g2), _add(g3, g4)), want)
    print('pairwise order: %d of %d elements differ' % (bad, N))
    assert bad > N // 100
    # scaled before summing: ((g1 / 4 + g2 / 4) + ...) -- and even that times 4 again is not the sum (denormals lose bits)
    q = np.float32(0.25)
    scaled = X.reference_sum([(g * q).astype(np.float32) for g in grads])
    assert X.mismatches(scaled, want) > N // 2
    with np.errstate(all='ignore'):
        assert X.mismatches((scaled * np.float32(4)).astype(np.float32), want) > 0
    third = np.float32(1.0 / 3.0)
    with np.errstate(all='ignore'):
        assert X.mismatches(X.reference_sum([(g * third).astype(np.float32) for g in grads[:3]]),
                            (X.reference_sum(grads[:3]) * third).astype(np.float32)) > N // 100
    # tail dropped: the last n % 4 elements keep what the destination held
    assert N % 4 == 3
    two = X.reference(g1, g2)
    dropped = two.copy()
    dropped[N - 3:] = np.float32(X.FILL_DST)
    assert X.mismatches(dropped, two) == 3
    # flush to zero: denormal operands or sums replaced by 0
    flushed = two.copy()
    flushed[(np.abs(two) > 0) & (np.abs(two) < X._TINY)] = 0
    assert X.mismatches(flushed, two) >= 3
    # guard elements written: the check looks at the whole buffer
    G = X.GUARD
    buf = np.full(N + 2 * G, np.float32(X.FILL_DST), dtype=np.float32)
    buf[G:G + N] = two
    for pos in (G - 1, G + N, 0, N + 2 * G - 1):
        wrote = buf.copy()
        wrote[pos] = 0.0
        assert X.mismatches(wrote, buf) == 1
    # the copy treated as an add onto the stale sum of the group before
    stale = _protocol([grads[:2], grads[2:]], copy_first=False)
    assert X.mismatches(stale[0], X.reference_sum(grads[:2])) == 0 and X.mismatches(stale[1], X.reference_sum(grads[2:])) > N // 2


@pytest.mark.parametrize('n', (0, 1, 5))
@pytest.mark.parametrize('N_', (1, 2, 3, 8))
def test_accum_plan(n, N_):
    from pose_adv_aug_amd.utils.optim import accum_plan
    plan = accum_plan(n, N_)
    assert len(plan) == n and all(isinstance(s, bool) and 1 <= k <= N_ for s, k in plan)
    assert sum(k for s, k in plan if s) == n                       # the groups cover the epoch
    if n:
        assert plan[-1][0]                                         # an epoch never ends with a gradient pending
    size = 0
    for i, (steps, k) in enumerate(plan):
        size += 1
        assert k == size and steps == (i % N_ == N_ - 1 or i == n - 1)
        if steps:
            size = 0
    if N_ == 1:
        assert plan == [(True, 1)] * n
    if (n, N_) == (5, 2):
        assert plan == [(False, 1), (True, 2), (False, 1), (True, 2), (True, 1)]
    if (n, N_) == (5, 3):
        assert [k for s, k in plan if s] == [3, 2]
    if (n, N_) == (5, 8):
        assert [k for s, k in plan if s] == [5]


def test_accum_plan_refuses_a_group_size_below_one():
    from pose_adv_aug_amd.utils.optim import accum_plan
    for bad in (0, -1):
        with pytest.raises(ValueError):
            accum_plan(5, bad)


def test_the_command_line(tmp_path):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd import pretrain_s_r_agent, stack_hg
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e']
    assert TrainOptions().parse(base).accum_steps == 1
    assert TrainOptions().parse(base + ['--accum_steps', '4']).accum_steps == 4
    for bad in ('0', '-1', '1.5', 'two'):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + ['--accum_steps', bad])
    with pytest.raises(SystemExit) as e:
        pretrain_s_r_agent.main(base + ['--accum_steps', '2'])
    assert '--accum_steps 2 is not supported' in str(e.value)
    # the plan of the loops: None with the option off or absent, and the effective batch said once per optimizer
    lines = []
    o1, o2 = _Opt(), _Opt()
    assert stack_hg.accum_plan_for(types.SimpleNamespace(), 5, o1, lines.append) is None
    assert stack_hg.accum_plan_for(TrainOptions().parse(base), 5, o1, lines.append) is None and lines == []
    opt = TrainOptions().parse(base + ['--accum_steps', '2', '--bs', '16'])
    for _ in range(2):
        assert [s for s, _ in stack_hg.accum_plan_for(opt, 5, o1, lines.append)] == [False, True, False, True, True]
    assert len(lines) == 1 and 'effective batch 16 x 2 x 1 rank(s) = 32' in lines[0]
    stack_hg.accum_plan_for(opt, 5, o2, lines.append)
    assert len(lines) == 2


class _Opt(object):
    """an optimizer as far as the plan of the loops needs one: an object to remember"""


NAME = 'pa_grad_accumulate'


def test_the_symbol_exists_in_both_libraries_the_header_and_the_export_table():
    import pose_adv_aug_amd as P
    _lib()
    here = os.path.dirname(P.LIB_PATH)
    for so in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        assert hasattr(C.CDLL(os.path.join(here, so)), NAME), so
    assert NAME in P.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'poseadv.h')).read()
    assert 'int pa_grad_accumulate(float* dst, const float* a, const float* b, size_t n, void* stream);' in hdr
    from pose_adv_aug_amd import _lib as L
    res, args = L._PROTOS[NAME]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert 'grad_accum' in open(os.path.join(ROOT, 'pose_adv_aug_amd', 'csrc', 'build.sh')).read().split('SRCS="')[1].split('"')[0].split()


def test_refusals_are_decided_on_the_host():
    """The pointers are host addresses that are never dereferenced: every call below is answered before any device call, so it answers
    on a machine without a GPU."""
    L = _lib()
    buf = np.full(4096, 9.0, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    at = lambda k: C.c_void_p(base + 4 * k)
    n = 1024

    def refused(rc, word):
        msg = L.pa_last_error()
        assert rc != 0 and msg.startswith(b'pa_grad_accumulate: ') and word in msg, (rc, msg)

    refused(L.pa_grad_accumulate(None, at(0), at(n), n, None), b'dst is NULL')
    refused(L.pa_grad_accumulate(at(0), None, at(n), n, None), b'a is NULL')
    refused(L.pa_grad_accumulate(at(0), None, None, n, None), b'a is NULL')
    refused(L.pa_grad_accumulate(at(0), at(n), at(2 * n), 0, None), b'n must be >= 1')
    refused(L.pa_grad_accumulate(at(0), at(n), None, 0, None), b'n must be >= 1')
    refused(L.pa_grad_accumulate(at(0), at(n), at(2 * n), 2 ** 63, None), b'n must be >= 1')           # n floats do not fit an address space
    for d, a, b in ((1, 0, 2 * n), (0, n - 1, 2 * n), (0, 2 * n, n - 1), (n - 1, 2 * n, 0), (0, n, n + 1), (0, 8, 0), (8, 0, 0)):
        refused(L.pa_grad_accumulate(at(d), at(a), at(b), n, None), b'overlap in part')
    refused(L.pa_grad_accumulate(at(1), at(0), None, n, None), b'overlap in part')
    assert L.pa_grad_accumulate(at(0), at(0), None, n, None) == 0 and not L.pa_last_error()              # nothing to do, nothing launched
    assert (buf == 9.0).all()


class _Recorder(object):
    """stands in for the library under utils.optim (host control flow only): logs every pa_* call, computes nothing"""
    def __init__(self):
        self.log = []

    def pa_grad_scale(self):
        return 1.0

    def __getattr__(self, name):
        if not name.startswith('pa_'):
            raise AttributeError(name)

        def call(*args):
            if not name.endswith('_workspace_bytes'):
                self.log.append((name, args))
            return 0
        return call


class _HostNet(object):
    def __init__(self):
        self.flat_params, self.flat_grads, self.flat_buffers = torch.arange(12.), torch.ones(12), torch.arange(5.)
        self._table = [('a.weight', (2, 3), 0, 6, 0), ('a.bias', (3,), 8, 3, 0), ('bn.running_mean', (5,), 0, 5, 1)]
        self._nbt, self._last_B, self.default_batch, self.zeroed = 4, 1, 1, 0

    def _ensure_table(self):
        pass

    def _net(self, B):
        return None

    def weights_changed(self):
        pass

    def zero_grad(self):
        self.zeroed += 1


@pytest.fixture
def rec(monkeypatch):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.utils import optim
    r = _Recorder()
    for mod in (optim, _lib):
        monkeypatch.setattr(mod, 'lib', lambda: r)
    monkeypatch.setattr(optim, 'ptr', lambda x: x)
    monkeypatch.setattr(optim, 'stream', lambda: 12345)
    return r


def _gscale_of(call):
    name, args = call
    return args[{'pa_rmsprop_step_state': 7, 'pa_rmsprop_step_opts': 7, 'pa_adam_step': 7, 'pa_grad_norm': 2}[name]]


def test_the_launch_sequence_and_the_gscale(rec):
    from pose_adv_aug_amd.utils import optim
    makes = ((lambda n: optim.RMSprop(n), ['pa_rmsprop_step_state']),
             (lambda n: optim.RMSprop(n, momentum=0.9, max_grad_norm=1.0), ['pa_grad_norm', 'pa_rmsprop_step_opts']),
             (lambda n: optim.Adam(n, max_grad_norm=1.0), ['pa_grad_norm', 'pa_adam_step']),
             (lambda n: optim.AdamW(n), ['pa_adam_step']))
    for make, step_calls in makes:
        net = _HostNet()
        o = make(net)
        g = net.flat_grads
        assert (o.pending, o._acc) == (0, None)
        o.step()                                              # no group pending: the launches of today, and no private array
        assert [n for n, _ in rec.log] == step_calls and all(_gscale_of(c) == 1.0 for c in rec.log) and o._acc is None
        del rec.log[:]
        for k in range(1, 4):                                 # groups of 2, 3 and 4
            for j in range(k):
                o.accumulate()
                assert o.pending == j + 1
            acc = o._acc
            assert acc is not None and acc is not g and acc.shape == g.shape and acc.dtype == torch.float32
            calls = [a for n, a in rec.log if n == 'pa_grad_accumulate']
            assert len(calls) == len(rec.log) == k
            assert calls[0][0] is acc and calls[0][1] is g and calls[0][2:] == (None, 12, 12345)                    # the copy
            assert all(c[0] is acc and c[1] is acc and c[2] is g and c[3:] == (12, 12345) for c in calls[1:])      # _acc = _acc + g
            del rec.log[:]
            o.step()
            assert o.pending == 0 and o._acc is acc                                                                 # allocated once
            assert [n for n, _ in rec.log] == ['pa_grad_accumulate'] + step_calls
            fold = rec.log[0][1]
            assert fold[0] is g and fold[1] is acc and fold[2] is g and fold[3:] == (12, 12345)                     # flat_grads = _acc + flat_grads
            assert all(_gscale_of(c) == 1.0 / (k + 1) for c in rec.log[1:])
            del rec.log[:]
        o.step()
        assert [n for n, _ in rec.log] == step_calls and all(_gscale_of(c) == 1.0 for c in rec.log)
        del rec.log[:]


def test_zero_grad_drops_a_group_and_state_dict_warns(rec):
    from pose_adv_aug_amd.utils import optim
    for cls in (optim.RMSprop, optim.Adam):
        net = _HostNet()
        o = cls(net)
        o.accumulate(); o.accumulate()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            o.state_dict()
        assert len(w) == 1 and '2 accumulated micro-batch gradient(s) are pending and are NOT saved' in str(w[0].message)
        o.zero_grad()
        assert o.pending == 0 and net.zeroed == 1
        del rec.log[:]
        o.accumulate()
        assert rec.log[0][1][1] is net.flat_grads and rec.log[0][1][2] is None          # a new group: a copy again
        o.step()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            o.state_dict()
        assert w == []
        del rec.log[:]


def test_an_overlapping_optimizer_refuses_to_accumulate(rec):
    from pose_adv_aug_amd.utils import optim
    for cls in (optim.RMSprop, optim.Adam, optim.AdamW):
        o = cls(_HostNet(), overlap=True)
        with pytest.raises(ValueError, match='overlap=False'):
            o.accumulate()
        assert o.pending == 0 and o._acc is None and rec.log == []
        o.step()                                              # stepping alone is what it was
        del rec.log[:]


def test_the_exchange_runs_once_per_group_behind_the_fold(rec):
    from pose_adv_aug_amd.utils import optim
    net = _HostNet()
    o = optim.RMSprop(net)
    order = []
    o.allreduce_grads = lambda: (order.append(len(rec.log)), 0.5)[1]          # (a world of 2)
    for _ in range(3):
        o.accumulate()
    assert order == []
    o.step()
    assert order == [4]                                       # behind three accumulate launches and the fold, before the step kernel
    assert rec.log[3][0] == 'pa_grad_accumulate' and rec.log[4][0] == 'pa_rmsprop_step_state' and _gscale_of(rec.log[4]) == 0.5 / 4


def test_the_loops_pass_accumulate_by_the_plan(monkeypatch):
    from pose_adv_aug_amd import joint_train_pose_s_r_agent as J, stack_hg
    seen = []
    ahead = types.SimpleNamespace(start=lambda b: None, take=lambda: 'data')
    z = torch.zeros(())
    meters = lambda names, dev: types.SimpleNamespace(update=lambda d: None, averages=lambda: dict(loss=0.0, pckh=0.0, pckh_origin_res=0.0, loss_hg=0.0))
    monkeypatch.setattr(stack_hg, 'AugmentAhead', lambda aug: ahead)
    monkeypatch.setattr(stack_hg, 'train_step', lambda *a, **k: (seen.append(k), (z, z, z))[1])
    monkeypatch.setattr(stack_hg, 'DeviceMeters', meters)
    monkeypatch.setattr(J, 'train_hg_step', lambda i, *a, **k: (seen.append(k), ('regular', z, z))[1])
    monkeypatch.setattr(J, 'DeviceMeters', meters)
    net = types.SimpleNamespace(train=lambda: None)
    for N_, want in ((2, [True, False, True, False, False]), (3, [True, True, False, True, False]), (8, [True] * 4 + [False]), (1, [False] * 5)):
        opt = types.SimpleNamespace(print_freq=100, accum_steps=N_, bs=2)
        del seen[:]
        stack_hg.train(list('abcde'), net, _Opt(), None, 0, opt, log=lambda m: None)
        assert [k.get('accumulate', False) for k in seen] == want
        assert all(k == (dict(data='data', accumulate=True) if acc else dict(data='data')) for k, acc in zip(seen, want))
        del seen[:]
        J.train_hg(list('abcde'), None, _Opt(), None, None, 0, opt, log=lambda m: None)
        assert [k.get('accumulate', False) for k in seen] == want and all('ema' not in k for k in seen)

"""SGD, LARS and LAMB, everything that needs no GPU: the header and the exports, the segment plan of pa_opt_segments_host through the built
library (coverage, order, every input error), the float64 oracles of tests/layerwise_exact.py against torch.optim.SGD and torch.optim.AdamW
and on the special cases of the trust ratio, the host layer of utils/optim.py on a recording library (which calls, with which arguments;
state_dict in torch's formats; the command line), and the compiler's resource report of csrc/opt_layerwise.hip (no scratch)."""
import ctypes as C
import itertools
import os
import sys
import types
import warnings

import pytest
import torch

from tests import abi_stub
from tests import layerwise_exact as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pa_opt_segments_host', 'pa_opt_layer_workspace_bytes', 'pa_tensor_norms', 'pa_lamb_step', 'pa_lars_step')


def _lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


def test_the_header_declares_and_both_libraries_export_the_entry_points():
    import pose_adv_aug_amd as P
    from pose_adv_aug_amd import _lib as L
    _lib()
    here = os.path.dirname(P.LIB_PATH)
    for so in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        for name in NAMES:
            assert hasattr(C.CDLL(os.path.join(here, so)), name), (so, name)
    assert all(name in P.EXPORTS for name in NAMES)
    hdr = ' '.join(open(os.path.join(ROOT, 'include', 'poseadv.h')).read().split())
    for decl in ('#define PA_OPT_SEGMENT_FLOATS %d' % LW.S,
                 'typedef struct pa_opt_segment { uint32_t chunk0, nfloats; int32_t tensor, group; } pa_opt_segment;',
                 'size_t pa_opt_segments_host(const size_t* offsets_host, const size_t* numels_host, const int32_t* group_host, int ntensors, '
                 'size_t n, pa_opt_segment* segs_host, size_t cap);',
                 'int pa_tensor_norms(const float* x, const pa_opt_segment* segs, size_t nsegs, int ntensors, float scale, void* workspace, '
                 'float* norms, void* stream);',
                 'int pa_lamb_step(const pa_lamb_opts* o,', 'int pa_lars_step(const pa_lars_opts* o,', 'size_t pa_opt_layer_workspace_bytes('):
        assert decl in hdr, decl
    assert C.sizeof(L.OptSegment) == 16 and L.OPT_SEGMENT_FLOATS == LW.S and LW.S % 4 == 0
    assert C.sizeof(L.LambOpts) == 24 and C.sizeof(L.LarsOpts) == 20


# ---------------------------------------------------------------------------------------------------------------------------------
# the segment plan
def test_the_segment_plan_covers_every_tensor_exactly():
    L = _lib()
    offsets, numels, n = LW.table()
    assert n % 4 == 3 and sorted(set((offsets[i + 1] - (offsets[i] + numels[i] + 3) // 4 * 4) for i in range(len(offsets) - 1))) == [0, 4, 12]
    groups = [t % 16 for t in range(len(offsets))]
    count, segs = LW.segments(L, offsets, numels, groups, n)
    expected = sum((k + LW.S - 1) // LW.S for k in numels)
    assert count == expected == len(segs)          # the count-only call and the fill call agree (segments() makes both)
    covered = [0] * n
    end, by_tensor = 0, {}
    for s in segs:
        first = 4 * s.chunk0
        assert first >= end and s.nfloats >= 1                         # ascending and disjoint
        end = first + s.nfloats
        t = s.tensor
        assert offsets[t] <= first and end <= offsets[t] + numels[t]    # inside one tensor: no padding, no boundary crossed
        assert s.group == groups[t] and s.nfloats <= LW.S
        by_tensor.setdefault(t, []).append(s)
        for i in range(first, end):
            covered[i] += 1
    for t, (o, k) in enumerate(zip(offsets, numels)):
        assert all(c == 1 for c in covered[o:o + k]), t                 # the union of a tensor's segments is exactly the tensor
        assert all(s.nfloats % 4 == 0 for s in by_tensor[t][:-1])       # only the last segment of a tensor may be ragged
        assert sum(s.nfloats for s in by_tensor[t]) == k
    assert sum(covered) == sum(numels)
    tensors = [s.tensor for s in segs]
    assert tensors == sorted(tensors)                                   # a tensor's segments are contiguous in the list


def test_every_input_error_of_the_segment_plan_returns_zero_and_writes_nothing():
    from pose_adv_aug_amd._lib import OptSegment
    L = _lib()
    offsets, numels, n = LW.table()
    nt = len(offsets)
    count, _ = LW.segments(L, offsets, numels, [0] * nt, n)
    arr = lambda typ, v: (typ * len(v))(*v)
    good = dict(offsets=arr(C.c_size_t, offsets), numels=arr(C.c_size_t, numels), group=arr(C.c_int32, [0] * nt))
    host = (OptSegment * count)()
    C.memset(host, 0x5a, C.sizeof(host))
    keep = bytes(host)

    def refused(what, offsets=good['offsets'], numels=good['numels'], group=good['group'], ntensors=nt, n_=n, cap=count):
        for out, c in ((None, 0), (host, cap)):
            if out is None and what == 'cap too small':
                continue
            got = L.pa_opt_segments_host(offsets, numels, group, ntensors, n_, out, c)
            assert got == 0 and b'pa_opt_segments_host' in L.pa_last_error(), (what, got, L.pa_last_error())
        assert bytes(host) == keep, what

    refused('NULL offsets', offsets=None)
    refused('NULL numels', numels=None)
    refused('NULL group', group=None)
    refused('ntensors 0', ntensors=0)
    refused('an offset that is not a multiple of 4', offsets=arr(C.c_size_t, [offsets[0], offsets[1] + 1] + offsets[2:]))
    swapped = list(offsets)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    refused('tensors out of order', offsets=arr(C.c_size_t, swapped))
    refused('overlapping tensors', numels=arr(C.c_size_t, [numels[0]] * 10 + [numels[10] + 8] + numels[11:]))
    refused('a tensor that ends past n', n_=offsets[-1] + numels[-1] - 1)
    refused('cap too small', cap=count - 1)
    assert L.pa_opt_segments_host(good['offsets'], good['numels'], good['group'], nt, n, host, count) == count and bytes(host) != keep


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracles
def _toy(seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=dtype) for s in ((5, 7), (7,), (3, 2, 4))]


def _rel(a, b, prev):
    return float(((a - b).abs() / torch.maximum(b.abs(), prev.abs()).clamp_min(1e-300)).max())


@pytest.mark.parametrize('momentum,nesterov,wd', [(m, n, w) for m, n, w in itertools.product((0.0, 0.9), (False, True), (0.0, 1e-4)) if m or not n])
def test_the_lars_oracle_without_trust_is_torch_sgd(momentum, nesterov, wd):
    ps = _toy(1)
    qs = [torch.nn.Parameter(p.clone()) for p in ps]
    topt = torch.optim.SGD(qs, lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    bufs = [torch.zeros_like(p) for p in ps]
    for k in range(5):
        gs = _toy(10 + k)
        prev = [p.clone() for p in ps]
        r = LW.lars_oracle(ps, gs, bufs, 0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov, trust_coefficient=0.0)
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        topt.step()
        assert r == [1.0] * 3
        for p, q, p0, b in zip(ps, qs, prev, bufs):
            assert _rel(p, q.detach(), p0) <= 1e-12
            if momentum:
                assert _rel(b, topt.state[q]['momentum_buffer'], b) <= 1e-12


def test_the_lamb_oracle_with_every_ratio_one_is_torch_adamw():
    """p - lr ((m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd p) against AdamW's p (1 - lr wd) - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps):
    equal in exact arithmetic"""
    lr, betas, eps, wd = 2.0 ** -10, (0.9, 0.999), 1e-6, 0.01
    ps = _toy(2)
    qs = [torch.nn.Parameter(p.clone()) for p in ps]
    topt = torch.optim.AdamW(qs, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for k in range(5):
        gs = _toy(20 + k)
        prev = [p.clone() for p in ps]
        LW.lamb_oracle(ps, gs, ms, vs, k + 1, lr=lr, betas=betas, eps=eps, weight_decay=wd, force_ratio=1.0)
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        topt.step()
        for p, q, p0, m, v in zip(ps, qs, prev, ms, vs):
            assert _rel(p, q.detach(), p0) <= 1e-12
            assert _rel(m, topt.state[q]['exp_avg'], m) <= 1e-12 and _rel(v, topt.state[q]['exp_avg_sq'], v) <= 1e-12


def test_the_special_cases_of_the_trust_ratio():
    z = lambda ps: [torch.zeros_like(p) for p in ps]
    # an all-zero tensor, and a tensor with zero gradient and zero moments: r = 1
    ps, gs = _toy(3), _toy(4)
    ps[0].zero_()
    gs[1].zero_()
    r = LW.lamb_oracle(ps, gs, z(ps), z(ps), 1, weight_decay=0.0, always_adapt=True)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] != 1.0 and bool((ps[1] == _toy(3)[1]).all())
    ps = _toy(3)
    ps[0].zero_()
    r = LW.lars_oracle(ps, gs, z(ps), 0.1, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-3)
    assert r[0] == 1.0 and r[1] == 1.0 and 0 < r[2] < 1.0
    # max_trust caps the ratio
    ps = [100.0 * p for p in _toy(3)]
    free = LW.lamb_oracle([p.clone() for p in ps], gs, z(ps), z(ps), 1, weight_decay=0.01)
    capped = LW.lamb_oracle([p.clone() for p in ps], gs, z(ps), z(ps), 1, weight_decay=0.01, max_trust=2.0)
    assert all(f > 2.0 for f in free) and capped == [2.0] * 3
    # a zero-decay group: r = 1 unless always_adapt
    wds, gs = [0.01, 0.0, 0.01], _toy(4)
    for oracle, kw in ((lambda **k: LW.lamb_oracle(_toy(3), gs, z(ps), z(ps), 1, **k), dict()),
                       (lambda **k: LW.lars_oracle(_toy(3), gs, z(ps), 0.1, trust_coefficient=1e-3, **k), dict())):
        r = oracle(wds=wds, **kw)
        assert r[1] == 1.0 and r[0] != 1.0 and r[2] != 1.0
        r = oracle(wds=wds, always_adapt=True, **kw)
        assert all(x != 1.0 for x in r)
    # the ratio is the definition
    ps = _toy(3)
    r = LW.lars_oracle([p.clone() for p in ps], gs, z(ps), 0.1, weight_decay=1e-4, trust_coefficient=1e-3, eps=1e-8)
    W, G = float(ps[2].norm()), float(gs[2].norm())
    assert abs(r[2] - 1e-3 * W / (G + 1e-4 * W + 1e-8)) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------------------------
# the host layer on a recording library
class _Stub(abi_stub.FakeLib):
    """abi_stub.FakeLib plus what the layer-wise optimizers need answers from: a segment plan (one segment per tensor) and the sizes"""
    def pa_opt_segments_host(self, offsets, numels, group, nt, n, segs, cap):
        self.log.append(('pa_opt_segments_host', (list(offsets), list(numels), list(group), nt, n, segs is not None)))
        if segs is not None:
            for t in range(nt):
                segs[t].chunk0, segs[t].nfloats, segs[t].tensor, segs[t].group = offsets[t] // 4, numels[t], t, group[t]
        return nt

    def pa_opt_layer_workspace_bytes(self, nsegs, nt):
        return 16 * nsegs

    def pa_opt_chunk_map_host(self, *a):
        self.log.append(('pa_opt_chunk_map_host', a[3:6]))
        return 0


def _host_net():
    table = [('a.weight', (2, 3), 0, 6, 0), ('a.bias', (3,), 8, 3, 0), ('bn.running_mean', (3,), 0, 3, 1)]
    return types.SimpleNamespace(flat_params=torch.zeros(12), flat_grads=torch.ones(12), _table=table, _last_B=1, default_batch=1,
                                 _ensure_table=lambda: None, weights_changed=lambda: None, _net=lambda B: None)


@pytest.fixture
def host(monkeypatch):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.utils import optim
    rec = _Stub(0)
    for mod in (optim, _lib):
        monkeypatch.setattr(mod, 'lib', lambda: rec)
    monkeypatch.setattr(optim, 'ptr', lambda x: x)
    monkeypatch.setattr(optim, 'stream', lambda: 12345)
    return optim, rec


def test_sgd_is_one_call_without_norm_arrays(host):
    optim, rec = host
    net = _host_net()
    o = optim.SGD(net, lr=0.1)
    assert [n for n in rec.names()] == ['pa_opt_segments_host'] * 2 and o._nsegs == 2 and o._ntensors == 2
    assert o._segs.dtype == torch.int32 and o._segs.tolist() == [0, 6, 0, 0, 2, 3, 1, 0]
    del rec.log[:]
    o.step()
    assert rec.names() == ['pa_lars_step']
    a = rec.log[0][1]
    opts = a[0]._obj
    assert (opts.momentum, opts.trust_coef, opts.nesterov, opts.always_adapt) == (0.0, 0.0, 0, 0)
    assert a[2] == 1 and abs(a[1][0].lr - 0.1) < 1e-8 and a[1][0].weight_decay == 0 and a[1][0].frozen == 0
    assert a[3] is o._segs and a[4] == 2 and a[5] == 2 and a[6] is net.flat_params and a[7] is net.flat_grads and a[8] is None
    assert a[9] == 12 and a[10] == 1.0 and a[11] is None and a[12] is None and a[13] is None and a[14] is None
    assert a[15] is o._skip_state and a[16] == 12345
    assert o.last_trust() is None and o.tensor_norms() is None and o.momentum_buffer is None
    sd = o.state_dict()
    assert sd['state'] == {} and sd['param_groups'][0]['params'] == [0, 1] and sd['param_groups'][0]['dampening'] == 0
    o.param_groups[0]['momentum'] = 0.9          # read at every step; the buffer appears with it
    o.param_groups[0]['lr'] = 0.05
    o.step()
    a = rec.log[-1][1]
    assert a[8] is o.momentum_buffer and o.momentum_buffer is not None and abs(a[0]._obj.momentum - 0.9) < 1e-7 and abs(a[1][0].lr - 0.05) < 1e-8
    assert sorted(o.state_dict()['state'][1]) == ['momentum_buffer'] and o.state_dict()['state'][1]['momentum_buffer'].shape == (3,)
    for bad in (dict(momentum=-0.1), dict(weight_decay=-1.0), dict(nesterov=True), dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            optim.SGD(_host_net(), lr=0.1, **bad)
    o.param_groups[0].update(momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        o.step()


def test_lars_and_lamb_pass_their_arrays_and_options(host):
    optim, rec = host
    net = _host_net()
    o = optim.LARS(net, lr=0.1, weight_decay=1e-4, max_grad_norm=2.0)
    assert o.param_groups[0]['momentum'] == 0.9 and o.param_groups[0]['trust_coefficient'] == 1e-3 and o.last_trust() is None
    del rec.log[:]
    o.step()
    assert rec.names() == ['pa_grad_norm', 'pa_lars_step']
    a = rec.log[-1][1]
    assert a[8] is o.momentum_buffer and a[12] is o._layer_ws and a[13] is o._norms and a[14] is o._trust
    assert a[11].data_ptr() == o._norm_out.data_ptr() + 4 and abs(a[0]._obj.trust_coef - 1e-3) < 1e-9
    assert o.last_trust() is o._trust and bool((o._trust == 1).all()) and o._norms.numel() == 4
    W, G = o.tensor_norms()
    assert W.numel() == G.numel() == 2
    net = _host_net()
    o = optim.LAMB(net, groups=[{'params': optim.no_decay_1d, 'weight_decay': 0.0}, {'params': r'a\.weight', 'frozen': True}], max_trust=10.0)
    assert o._segs.tolist() == [0, 6, 0, 2, 2, 3, 1, 1]              # the group of every tensor travels in its segments
    del rec.log[:]
    o.step()
    assert rec.names() == ['pa_lamb_step']
    a = rec.log[0][1]
    opts = a[0]._obj
    assert (round(opts.beta1, 6), round(opts.beta2, 6), round(opts.eps, 9), opts.max_trust, opts.always_adapt, opts.amsgrad) == (0.9, 0.999, 1e-6, 10.0, 0, 0)
    assert a[2] == 3 and [a[1][k].frozen for k in range(3)] == [0, 0, 1] and a[1][1].weight_decay == 0 and abs(a[1][0].weight_decay - 0.01) < 1e-9
    assert a[3] is o._segs and a[6] is net.flat_params and a[7] is net.flat_grads and a[8] is o.exp_avg and a[9] is o.exp_avg_sq and a[10] == 12
    assert a[12] is None and a[13] is o._layer_ws and a[14] is o._norms and a[15] is o._trust and a[16] is o._state and o._state.numel() == 8
    assert o.last_trust() is o._trust and len(o.describe_groups()) == 3 and o.skip_flag_ptr() is o._state
    sd = o.state_dict()
    assert sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step']
    o.param_groups[0]['amsgrad'] = True
    with pytest.raises(ValueError):
        o.step()
    for bad in (dict(betas=(1.0, 0.9)), dict(eps=0.0), dict(weight_decay=-1.0), dict(max_trust=-1.0)):
        with pytest.raises(ValueError):
            optim.LAMB(_host_net(), **bad)


def test_files_of_other_kinds_load_with_one_warning_and_adam_files_load_into_lamb(host):
    optim, rec = host
    adam = optim.Adam(_host_net(), amsgrad=True)
    adam.exp_avg.fill_(2.0)
    adam.exp_avg_sq.fill_(3.0)
    lamb = optim.LAMB(_host_net())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        lamb.load_state_dict(adam.state_dict())
    assert not w, [str(x.message) for x in w]
    assert bool((lamb.exp_avg[:6] == 2).all()) and bool((lamb.exp_avg_sq[8:11] == 3).all()) and lamb.max_exp_avg_sq is None
    assert lamb.param_groups[0]['amsgrad'] is False and 'decoupled_weight_decay' not in lamb.param_groups[0] and lamb.param_groups[0]['max_trust'] == 0
    back = optim.Adam(_host_net())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        back.load_state_dict(lamb.state_dict())
    assert not w and bool((back.exp_avg[:6] == 2).all())
    sgd = optim.SGD(_host_net(), lr=0.1, momentum=0.9)
    sgd.momentum_buffer.fill_(4.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        lamb.load_state_dict(sgd.state_dict())
    assert len(w) == 1 and 'momentum_buffer' in str(w[0].message) and not bool(lamb.exp_avg.any())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        sgd.load_state_dict(adam.state_dict())
    assert len(w) == 1 and 'no momentum_buffer' in str(w[0].message) and not bool(sgd.momentum_buffer.any()) and sgd.param_groups[0]['lr'] == 0.1
    # torch.optim.SGD's own file, both ways
    qs = [torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(3))]
    topt = torch.optim.SGD(qs, lr=0.2, momentum=0.8, nesterov=True, weight_decay=1e-3)
    for q in qs:
        q.grad = torch.full_like(q, 5.0)
    topt.step()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        sgd.load_state_dict(topt.state_dict())
    assert not w, [str(x.message) for x in w]
    g0 = sgd.param_groups[0]
    assert (g0['lr'], g0['momentum'], g0['nesterov'], g0['weight_decay']) == (0.2, 0.8, True, 1e-3)
    assert bool((sgd.momentum_buffer[:6] == 5).all()) and bool((sgd.momentum_buffer[8:11] == 5).all()) and not bool(sgd.momentum_buffer[6:8].any())
    t2 = torch.optim.SGD(qs, lr=0.1)
    t2.load_state_dict(sgd.state_dict())
    for q in qs:
        q.grad = torch.ones_like(q)
    p0 = float(qs[0].detach()[0, 0])
    t2.step()
    assert t2.param_groups[0]['momentum'] == 0.8 and t2.param_groups[0]['nesterov'] is True
    assert abs(float(t2.state[qs[0]]['momentum_buffer'][0, 0]) - (0.8 * 5 + 1 + 1e-3 * p0)) < 1e-6


def test_the_command_line_builds_the_three_kinds_and_refuses_the_rest(host, tmp_path):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    optim, rec = host
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e']
    opt = TrainOptions().parse(base)
    assert (opt.nesterov, opt.trust_coef, opt.max_trust, opt.always_adapt) == (0, 1e-3, 0.0, 0)
    o = optim.make_optimizer(TrainOptions().parse(base + ['--optimizer', 'sgd', '--momentum', '0.9', '--nesterov', '1', '--weight_decay', '1e-4']), _host_net(), 0.1)
    assert type(o) is optim.SGD
    g = o.param_groups[0]
    assert (g['lr'], g['momentum'], g['nesterov'], g['weight_decay'], g['trust_coefficient']) == (0.1, 0.9, True, 1e-4, 0.0)
    o = optim.make_optimizer(TrainOptions().parse(base + ['--optimizer', 'lars', '--momentum', '0.9', '--trust_coef', '0.02', '--always_adapt', '1',
                                                          '--clip_grad_norm', '5', '--no_decay_1d', '1']), _host_net(), 0.1)
    assert type(o) is optim.LARS and o.max_grad_norm == 5.0 and len(o.param_groups) == 2 and o.param_groups[1]['weight_decay'] == 0.0
    assert o.param_groups[0]['trust_coefficient'] == 0.02 and o.param_groups[0]['always_adapt'] is True and o.param_groups[1]['names'] == ['a.bias']
    o = optim.make_optimizer(TrainOptions().parse(base + ['--optimizer', 'lamb', '--weight_decay', '0.01', '--max_trust', '10', '--beta2', '0.99',
                                                          '--adam_eps', '1e-6']), _host_net(), 1e-3)
    assert type(o) is optim.LAMB
    g = o.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay'], g['max_trust'], g['always_adapt']) == (1e-3, (0.9, 0.99), 1e-6, 0.01, 10.0, False)
    for kind, extra in (('sgd', ['--centered', '1']), ('lars', ['--amsgrad', '1']), ('lamb', ['--amsgrad', '1']), ('lamb', ['--centered', '1']),
                        ('sgd', ['--nesterov', '1']), ('sgd', []), ('lars', ['--nesterov', '1']), ('lamb', ['--nesterov', '1', '--momentum', '0.9']),
                        ('adam', ['--nesterov', '1']), ('lamb', ['--momentum', '0.9'])):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + ['--optimizer', kind] + extra)
    ns = lambda **kw: types.SimpleNamespace(**kw)
    for bad in (ns(optimizer='sgd', centered=1), ns(optimizer='lamb', amsgrad=1), ns(optimizer='lars', nesterov=1), ns(optimizer='sgd', nesterov=1, momentum=0), ns(optimizer='sgd'),
                ns(optimizer='lamb', momentum=0.9)):
        with pytest.raises(ValueError):
            optim.make_optimizer(bad, _host_net(), 0.1)
    # the kinds that existed make the calls they made
    del rec.log[:]
    optim.make_optimizer(TrainOptions().parse(base), _host_net(), 2.5e-4).step()
    optim.make_optimizer(TrainOptions().parse(base + ['--optimizer', 'adamw']), _host_net(), 1e-3).step()
    assert rec.names() == ['pa_rmsprop_step', 'pa_adam_step']          # (the stub logs pa_rmsprop_step_state under that name)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_no_kernel_of_the_file_uses_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    if KR._tool('hipcc') is None:
        pytest.fail('hipcc not found: the resource check needs the compiler the build uses')
    src = os.path.join(ROOT, 'pose_adv_aug_amd', 'csrc', 'opt_layerwise.hip')
    for flags in ((), ('-DPA_FP16',)):
        res = KR.kernel_resources(src, flags)
        names = ' '.join(res)
        for kernel in ('tensor_sqsum_kernel', 'tensor_finish_kernel<0>', 'tensor_finish_kernel<1>', 'tensor_finish_kernel<2>', 'lamb_moments_kernel',
                       'lamb_apply_kernel', 'lars_sqsum_kernel', 'lars_step_kernel<true,true,true>', 'lars_step_kernel<false,false,false>'):
            assert kernel in names, (kernel, sorted(res))
        for k, r in res.items():
            assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (flags, k, r)

"""Parameter groups, everything that needs no GPU: the header and the exports, pa_opt_chunk_map_host against numpy, every argument error of
the device entry points (refused before any device call), the per-group bound on numpy emulations of the grouped kernels (inside for
the correct kernel, far outside for each defect), and the host layer of utils/optim.py on a recording library: selectors, the calls
with and without groups, adjust_lr, state_dict round trips, the command line."""
import ctypes as C
import os
import types
import warnings

import numpy as np
import pytest
import torch

from tests import abi_stub
from tests import adam_exact as A
from tests import groups_exact as G
from tests import optim_exact as X
from tests import optim_opts_exact as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200003
COEF = float(np.float32(0.37))
NAMES = ('pa_opt_chunk_map_bytes', 'pa_opt_chunk_map_host', 'pa_rmsprop_step_groups', 'pa_adam_step_groups', 'pa_grad_norm_groups')


def _lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_the_header_declares_and_both_libraries_export_the_entry_points():
    import pose_adv_aug_amd as P
    _lib()
    here = os.path.dirname(P.LIB_PATH)
    for so in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        for name in NAMES:
            assert hasattr(C.CDLL(os.path.join(here, so)), name), (so, name)
    assert all(name in P.EXPORTS for name in NAMES)
    hdr = ' '.join(open(os.path.join(ROOT, 'include', 'poseadv.h')).read().split())
    for decl in ('#define PA_OPT_GROUPS_MAX 16',
                 'typedef struct pa_opt_group { float lr, weight_decay; int32_t frozen, reserved; } pa_opt_group;',
                 'size_t pa_opt_chunk_map_bytes(size_t n);',
                 'int pa_opt_chunk_map_host(const size_t* offsets_host, const size_t* numels_host, const int32_t* group_host, int ntensors, '
                 'size_t n, int ngroups, uint8_t* map_host);',
                 'int pa_rmsprop_step_groups(const pa_rmsprop_opts* o, const pa_opt_group* groups_host, int ngroups, const uint8_t* chunk_map, '
                 'float* param, const float* grad, float* square_avg, float* momentum_buf, float* grad_avg, size_t n, float gscale, '
                 'const float* clip_coef, int32_t* state, void* stream);',
                 'int pa_adam_step_groups(const pa_adam_opts* o, const pa_opt_group* groups_host, int ngroups, const uint8_t* chunk_map, '
                 'float* group_consts, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n, '
                 'float gscale, const float* clip_coef, pa_adam_state* state, void* stream);',
                 'int pa_grad_norm_groups(const float* grad, size_t n, const uint8_t* chunk_map, uint32_t excluded_groups, float gscale, '
                 'float max_norm, void* workspace, float* out2, void* stream);'):
        assert decl in hdr, decl
    from pose_adv_aug_amd import _lib as L
    assert C.sizeof(L.OptGroup) == 16 and L.OPT_GROUPS_MAX == 16


def _map(L, table, n, ngroups):
    nt = len(table)
    off = (C.c_size_t * nt)(*[t[0] for t in table])
    num = (C.c_size_t * nt)(*[t[1] for t in table])
    grp = (C.c_int32 * nt)(*[t[2] for t in table])
    out = (C.c_uint8 * int(L.pa_opt_chunk_map_bytes(n)))(*([255] * int(L.pa_opt_chunk_map_bytes(n))))
    rc = L.pa_opt_chunk_map_host(off, num, grp, nt, n, ngroups, out)
    return rc, np.frombuffer(out, dtype=np.uint8).copy()


# a tensor of 1, 3, 4 and 5 floats, a gap of two whole chunks (chunks 6 and 7), the last tensor ending in a partial chunk
ODD_TABLE = [(0, 1, 2), (4, 3, 0), (8, 4, 3), (12, 5, 1), (32, 6, 2)]
ODD_N = 38


def test_the_chunk_map_against_numpy():
    L = _lib()
    assert [int(L.pa_opt_chunk_map_bytes(n)) for n in (0, 1, 4, 5, 38, 40)] == [0, 1, 1, 2, 10, 10]
    params = [t for t in abi_stub.TABLE if t[4] == 0]
    stub = [(t[2], t[3], i % 3) for i, t in enumerate(params)]
    for table, n, ngroups in ((stub, abi_stub.N_PARAMS, 3), (ODD_TABLE, ODD_N, 4)):
        rc, got = _map(L, table, n, ngroups)
        want = G.numpy_chunk_map(table, n)
        assert rc == 0 and got.tolist() == want.tolist(), (got, want)
    assert _map(L, ODD_TABLE, ODD_N, 4)[1].tolist() == [2, 0, 3, 1, 1, 1, 1, 1, 2, 2]
    # in front of the first tensor: group 0
    assert _map(L, [(8, 4, 1)], 12, 2)[1].tolist() == [0, 0, 1]


def test_the_chunk_map_refuses_every_listed_error():
    L = _lib()

    def refused(rc, word):
        msg = L.pa_last_error()
        assert rc != 0 and msg.startswith(b'pa_opt_chunk_map_host: ') and word in msg, (rc, msg, word)

    ok = (C.c_size_t * 2)(0, 8), (C.c_size_t * 2)(5, 4), (C.c_int32 * 2)(0, 1)
    out = (C.c_uint8 * 3)()
    for i in range(3):
        args = list(ok) + [2, 12, 2, out]
        args[i] = None
        refused(L.pa_opt_chunk_map_host(*args), b'NULL')
    refused(L.pa_opt_chunk_map_host(ok[0], ok[1], ok[2], 2, 12, 2, None), b'NULL')
    refused(L.pa_opt_chunk_map_host(ok[0], ok[1], ok[2], 0, 12, 2, out), b'ntensors')
    for ng in (0, 17):
        refused(L.pa_opt_chunk_map_host(ok[0], ok[1], ok[2], 2, 12, ng, out), b'ngroups')
    refused(_map(L, [(0, 4, 0), (6, 2, 1)], 12, 2)[0], b'multiple of 4')
    refused(_map(L, [(8, 4, 0), (0, 4, 1)], 12, 2)[0], b'out of order')
    refused(_map(L, [(0, 5, 0), (4, 4, 1)], 12, 2)[0], b'overlapping')
    refused(_map(L, [(0, 4, 0), (8, 5, 1)], 12, 2)[0], b'past n')
    refused(_map(L, [(0, 4, 0), (16, 0, 1)], 12, 2)[0], b'past n')
    refused(_map(L, [(0, 4, 0), (8, 4, 2)], 12, 2)[0], b'group id')
    refused(_map(L, [(0, 4, -1), (8, 4, 1)], 12, 2)[0], b'group id')
    assert _map(L, [(0, 4, 0), (8, 4, 1)], 12, 2)[0] == 0 and not L.pa_last_error()


def test_the_device_entry_points_refuse_on_the_host():
    """The pointers are host addresses that are never dereferenced: every call is answered before any device call."""
    L = _lib()
    from pose_adv_aug_amd._lib import RmspropOpts, AdamOpts
    buf = np.full(8192, 9.0, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    at = lambda k: C.c_void_p(base + 4 * k)
    n = 1024
    p, g, v, b1, b2, cm, gc, st, ws, out2 = tuple(at(k * n) for k in range(5)) + tuple(at(5 * n + 64 * k) for k in range(5))
    two = G.group_table([(1e-3, 0.0, False), (1e-4, 1e-2, False)])
    one = G.group_table([(1e-3, 0.0, False)])
    one_frozen = G.group_table([(1e-3, 0.0, True)])

    def refused(who, rc, word):
        msg = L.pa_last_error()
        assert rc != 0 and msg.startswith(who + b': ') and word in msg, (who, rc, msg, word)

    def rms(o=RmspropOpts(1.0, 0.99, 1e-8, 0.9, 0.0, 1), tab=two, ng=2, m=cm, p_=p, g_=g, v_=v, buf_=b1, ga_=b2, s_=st):
        return L.pa_rmsprop_step_groups(None if o is None else C.byref(o), tab, ng, m, p_, g_, v_, buf_, ga_, n, 1.0, None, s_, None)

    who = b'pa_rmsprop_step_groups'
    for kw in (dict(o=None), dict(p_=None), dict(g_=None), dict(v_=None), dict(s_=None)):
        refused(who, rms(**kw), b'NULL')
    refused(who, rms(o=RmspropOpts(1.0, 0.99, 1e-8, -0.1, 0.0, 1)), b'momentum')
    refused(who, rms(buf_=None), b'momentum_buf')
    refused(who, rms(o=RmspropOpts(1.0, 0.99, 1e-8, 0.0, 0.0, 1)), b'momentum_buf')
    refused(who, rms(ga_=None), b'grad_avg')
    refused(who, rms(o=RmspropOpts(1.0, 0.99, 1e-8, 0.9, 0.0, 0)), b'grad_avg')

    def adam(o=AdamOpts(1.0, 0.9, 0.999, 1e-8, 0.0, 1, 1), tab=two, ng=2, m=cm, gc_=gc, p_=p, g_=g, m_=v, v_=b1, x_=b2, s_=st):
        return L.pa_adam_step_groups(None if o is None else C.byref(o), tab, ng, m, gc_, p_, g_, m_, v_, x_, n, 1.0, None, s_, None)

    whoa = b'pa_adam_step_groups'
    for kw in (dict(o=None), dict(p_=None), dict(g_=None), dict(m_=None), dict(v_=None), dict(s_=None)):
        refused(whoa, adam(**kw), b'NULL')
    refused(whoa, adam(s_=C.c_void_p(st.value + 4)), b'aligned')
    refused(whoa, adam(x_=None), b'max_exp_avg_sq')
    refused(whoa, adam(o=AdamOpts(1.0, 0.9, 0.999, 1e-8, 0.0, 0, 1)), b'max_exp_avg_sq')
    for kw in (dict(beta1=-0.1), dict(beta1=1.0), dict(beta2=1.0), dict(beta2=float('nan'))):
        refused(whoa, adam(o=A._opts(0.0, True, True, **kw)), b'beta')
    refused(whoa, adam(o=A._opts(0.0, True, True, eps=0.0)), b'eps')
    refused(whoa, adam(gc_=None), b'group_consts')
    # what the groups add, for both steps
    for who_, call in ((who, rms), (whoa, adam)):
        refused(who_, call(tab=None), b'groups_host is NULL')
        for ng in (0, -1, 17):
            refused(who_, call(ng=ng), b'ngroups')
        refused(who_, call(m=None), b'chunk_map')
        refused(who_, call(tab=one_frozen, ng=1, m=None), b'chunk_map')
        for bad in (-1e-3, float('inf'), float('nan')):
            refused(who_, call(tab=G.group_table([(1e-3, 0.0, False), (bad, 0.0, False)])), b'lr of group 1')
            refused(who_, call(tab=G.group_table([(1e-3, bad, False), (1e-3, 0.0, False)])), b'weight_decay of group 0')
    # the norm
    whon = b'pa_grad_norm_groups'
    norm = lambda g_=g, m=cm, ex=1, mx=1.0, w=ws, o=out2: L.pa_grad_norm_groups(g_, n, m, ex, 1.0, mx, w, o, None)
    for kw in (dict(g_=None), dict(w=None), dict(o=None)):
        refused(whon, norm(**kw), b'NULL')
    refused(whon, norm(mx=0.0), b'max_norm')
    refused(whon, norm(w=C.c_void_p(ws.value + 4)), b'8-byte aligned')
    refused(whon, norm(ex=1 << 16), b'at or above 16')
    refused(whon, norm(m=None), b'chunk_map')
    assert (buf == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-group bound is not vacuous.  Five groups: different lr, zero and non-zero decay next to each other, one frozen; the decoupled
# factor 1 - 1e-2 * 0.1 is what a wd == 0 neighbour must not receive
CPU_GROUPS = [(2.5e-4, 0.0, False), (1e-2, 0.1, False), (1e-5, 0.0, False), (1e-3, 1e-2, True), (1e-3, 1e-4, False)]


def _cpu_map():
    return (np.arange(G.n_chunks(N)) % len(CPU_GROUPS)).astype(np.uint8)


def _rms_case(gscale, defect=None):
    p, g, v = X.make_inputs(N, 7, gscale, False)
    buf, ga = Y.make_state(N, 7, v, False)
    s = {'p': p, 'square_avg': v, 'momentum_buffer': buf, 'grad_avg': ga}
    cmap = _cpu_map()
    out = G.emulate_rmsprop(s, g, gscale, COEF, Y.MOM, True, cmap, CPU_GROUPS, defect)
    return G.check_groups('rmsprop', s, g, out, gscale, COEF, (Y.MOM, True), G.elem_groups(cmap, N).astype(np.int64), CPU_GROUPS)


def _adam_case(gscale, decoupled, defect=None):
    p, g, v = X.make_inputs(N, 7, gscale, False)
    m, vmax = A.make_state(N, 7, v, False)
    s = {'p': p, 'exp_avg': m, 'exp_avg_sq': v, 'max_exp_avg_sq': vmax}
    cmap = _cpu_map()
    c, gc_true = G.adam_consts(2, CPU_GROUPS)
    _, gc = G.adam_consts(2, CPU_GROUPS, defect)
    out = G.emulate_adam(s, g, gscale, COEF, decoupled, True, cmap, CPU_GROUPS, c, gc, defect)
    r = G.check_groups('adam', s, g, out, gscale, COEF, (decoupled, True), G.elem_groups(cmap, N).astype(np.int64), CPU_GROUPS, c, gc_true)
    r.update((('consts', k), x) for k, x in G.check_group_consts(c, gc, CPU_GROUPS, 2).items())
    return r


@pytest.mark.parametrize('gscale', G.GSCALES)
def test_the_emulated_grouped_kernels_are_inside_the_bound(gscale):
    for r in (_rms_case(gscale), _adam_case(gscale, True), _adam_case(gscale, False)):
        print('gscale %g: worst error / bound %.3g over %d figures' % (gscale, max(r.values()), len(r)))
        assert all(x <= 1.0 for x in r.values()), dict((k, x) for k, x in r.items() if not x <= 1.0)
        assert set(k for k, _ in r if k != 'consts') == set(range(len(CPU_GROUPS)))
        assert max(r.values()) > 0.2                                    # the bound is tight


@pytest.mark.parametrize('gscale', G.GSCALES)
@pytest.mark.parametrize('defect', G.DEFECTS_BOTH)
def test_each_defect_of_the_grouped_rmsprop_is_far_outside(defect, gscale):
    r = _rms_case(gscale, defect)
    print('%s, gscale %g: worst %.3g' % (defect, gscale, max(x if x == x else float('inf') for x in r.values())))
    assert not all(x <= 1e3 for x in r.values()), r


@pytest.mark.parametrize('gscale', G.GSCALES)
@pytest.mark.parametrize('defect', G.DEFECTS_BOTH + G.DEFECTS_ADAM)
def test_each_defect_of_the_grouped_adam_is_far_outside(defect, gscale):
    r = _adam_case(gscale, True, defect)
    print('%s, gscale %g: worst %.3g' % (defect, gscale, max(x if x == x else float('inf') for x in r.values())))
    assert not all(x <= 1e3 for x in r.values()), r


# ---------------------------------------------------------------------------------------------------------------------------------
# the host layer on a recording library
class _Recorder(object):
    """logs every pa_* call and computes nothing, except the chunk map, which the real library builds (host only)"""
    def __init__(self):
        self.log = []

    def pa_grad_scale(self):
        return 1.0

    def pa_grad_norm_workspace_bytes(self, n):
        return 16

    def pa_opt_chunk_map_host(self, *a):
        self.log.append(('pa_opt_chunk_map_host', a))
        return _lib().pa_opt_chunk_map_host(*a)

    def __getattr__(self, name):
        if not name.startswith('pa_'):
            raise AttributeError(name)

        def call(*args):
            self.log.append((name, args))
            return 0
        return call

    def names(self):
        return [n for n, _ in self.log if n != 'pa_opt_chunk_map_host']


TABLE = [('conv1.weight', (2, 3, 2, 2), 0, 24, 0), ('conv1.bias', (2,), 24, 2, 0), ('bn1.weight', (4,), 28, 4, 0), ('bn1.bias', (4,), 32, 4, 0),
         ('hg.0.conv.weight', (2, 2), 36, 4, 0), ('hg.1.conv.weight', (2, 3), 40, 6, 0), ('hg.1.bn.bias', (3,), 48, 3, 0),
         ('bn1.running_mean', (4,), 0, 4, 1)]
NFLOATS = 52


def _host_net(pose=True):
    net = types.SimpleNamespace(flat_params=torch.zeros(NFLOATS), flat_grads=torch.ones(NFLOATS), _table=TABLE, _last_B=1, default_batch=1,
                                _ensure_table=lambda: None, weights_changed=lambda: None, _net=lambda B: None)
    if pose:
        net.num_stacks = 2
    return net


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


def test_without_groups_the_calls_are_the_ones_there_have_always_been(rec):
    from pose_adv_aug_amd.utils import optim
    for make, want in ((lambda: optim.RMSprop(_host_net()), ['pa_rmsprop_step_state']),
                       (lambda: optim.RMSprop(_host_net(), momentum=0.9, max_grad_norm=1.0), ['pa_grad_norm', 'pa_rmsprop_step_opts']),
                       (lambda: optim.Adam(_host_net(), max_grad_norm=1.0), ['pa_grad_norm', 'pa_adam_step']),
                       (lambda: optim.AdamW(_host_net()), ['pa_adam_step'])):
        del rec.log[:]
        o = make()
        o.step()
        o.step()
        assert [n for n, _ in rec.log] == want * 2, rec.log
        assert len(o.param_groups) == 1 and not set(o.param_groups[0]) & set(['params', 'names', 'frozen', 'lr_mult'])
        assert o._map is None


def test_the_single_group_state_dict_is_todays_key_for_key(rec):
    from pose_adv_aug_amd.utils import optim
    sd = optim.RMSprop(_host_net(), momentum=0.9).state_dict()
    assert list(sd) == ['state', 'param_groups'] and len(sd['param_groups']) == 1
    assert sd['param_groups'][0] == dict(lr=2.5e-4, alpha=0.99, eps=1e-8, momentum=0.9, weight_decay=0, centered=False, params=list(range(7)))
    assert list(sd['param_groups'][0]) == ['lr', 'alpha', 'eps', 'momentum', 'weight_decay', 'centered', 'params']
    assert sorted(sd['state'][6]) == ['momentum_buffer', 'square_avg', 'step'] and sd['state'][0]['square_avg'].shape == (2, 3, 2, 2)
    sd = optim.AdamW(_host_net()).state_dict()
    assert sd['param_groups'] == [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, decoupled_weight_decay=True, params=list(range(7)))]
    assert list(sd['param_groups'][0]) == ['lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'decoupled_weight_decay', 'params']
    assert sorted(sd['state'][3]) == ['exp_avg', 'exp_avg_sq', 'step']


THREE = lambda: [dict(params=r'^(conv1|bn1)\.', frozen=True), dict(params=lambda name, shape: len(shape) <= 1, weight_decay=0.0, lr_mult=0.5)]


def test_selectors_first_match_wins_and_the_group_dicts(rec):
    from pose_adv_aug_amd.utils import optim
    o = optim.AdamW(_host_net(), lr=1e-3, groups=THREE() + [dict(params=['hg.1.conv.weight', 'bn1.bias'], lr=1e-4)])
    g = o.param_groups
    assert [x['params'] for x in g] == [[4], [0, 1, 2, 3], [6], [5]]           # bn1.bias went to the first spec that matched it
    assert g[1]['names'] == ['conv1.weight', 'conv1.bias', 'bn1.weight', 'bn1.bias'] and g[3]['names'] == ['hg.1.conv.weight']
    assert [x['frozen'] for x in g] == [False, True, False, False]
    assert [x['lr'] for x in g] == [1e-3, 1e-3, 5e-4, 1e-4] and [x['weight_decay'] for x in g] == [1e-2, 1e-2, 0.0, 1e-2]
    assert [x['lr_mult'] for x in g] == [1.0, 1.0, 0.5, pytest.approx(0.1)]
    assert all(x['betas'] == (0.9, 0.999) and x['decoupled_weight_decay'] is True and x['eps'] == 1e-8 for x in g)
    assert optim.no_decay_1d('bn1.weight', (4,)) and optim.no_decay_1d('s', ()) and not optim.no_decay_1d('w', (2, 2))
    o = optim.RMSprop(_host_net(), groups=[dict(params=optim.no_decay_1d, weight_decay=0.0)], weight_decay=1e-4)
    assert o.param_groups[1]['names'] == ['conv1.bias', 'bn1.weight', 'bn1.bias', 'hg.1.bn.bias'] and o.param_groups[0]['weight_decay'] == 1e-4
    # the map, built once by the library from the net's table
    assert [n for n, _ in rec.log].count('pa_opt_chunk_map_host') == 2
    want = G.numpy_chunk_map([(t[2], t[3], 1 if len(t[1]) <= 1 else 0) for t in TABLE if t[4] == 0], NFLOATS)
    assert o._map.dtype == torch.uint8 and o._map.tolist() == want.tolist()
    o.step()
    o.step()
    assert [n for n, _ in rec.log].count('pa_opt_chunk_map_host') == 2


def test_group_errors(rec):
    from pose_adv_aug_amd.utils import optim
    with pytest.raises(ValueError, match='bn9'):
        optim.Adam(_host_net(), groups=[dict(params=r'^bn9\.')])
    with pytest.raises(ValueError, match='matches no parameter'):
        optim.RMSprop(_host_net(), groups=[dict(params=lambda n, s: False)])
    with pytest.raises(ValueError, match='conv7.weight'):
        optim.Adam(_host_net(), groups=[dict(params=['conv1.weight', 'conv7.weight'])])
    with pytest.raises(ValueError, match='at most 16'):
        optim.Adam(_host_net(), groups=[dict(params='conv1')] * 16)           # 16 specs and the default group: 17
    optim.Adam(_host_net(), groups=[dict(params='conv1')] * 15)
    with pytest.raises(ValueError):
        optim.Adam(_host_net(), groups=[dict(params='conv1', lr=-1.0)])
    with pytest.raises(ValueError):
        optim.Adam(_host_net(), groups=[dict(params='conv1', betas=(0.5, 0.5))])
    for cls, key, val in ((optim.Adam, 'betas', (0.5, 0.999)), (optim.Adam, 'eps', 1e-6), (optim.Adam, 'amsgrad', True), (optim.RMSprop, 'momentum', 0.5),
                          (optim.RMSprop, 'alpha', 0.9)):
        o = cls(_host_net(), groups=THREE())
        o.step()
        o.param_groups[2][key] = val
        with pytest.raises(ValueError, match=key):
            o.step()
        o.param_groups[0][key] = o.param_groups[1][key] = val          # the same everywhere: a shared option, changed
        o.step()


def _table_of(args_tab, ngroups):
    return [(round(args_tab[k].lr, 7), round(args_tab[k].weight_decay, 7), args_tab[k].frozen) for k in range(ngroups)]          # (fp32 fields)


def test_with_groups_the_steps_go_through_the_groups_entry_points(rec):
    from pose_adv_aug_amd.utils import optim
    net = _host_net()
    o = optim.AdamW(net, lr=1e-3, max_grad_norm=2.0, groups=[dict(params=optim.no_decay_1d, weight_decay=0.0), dict(params=r'hg\.1\.', lr_mult=0.1)])
    o.step()
    assert rec.names() == ['pa_grad_norm', 'pa_adam_step_groups']          # no frozen group: the plain norm
    a = rec.log[-1][1]
    assert a[2] == 3 and _table_of(a[1], 3) == [(1e-3, 1e-2, 0), (1e-3, 0.0, 0), (1e-4, 1e-2, 0)]
    assert a[3] is o._map and a[4] is o._group_consts and o._group_consts.numel() == 16 and a[5] is net.flat_params and a[6] is net.flat_grads
    assert a[7] is o.exp_avg and a[8] is o.exp_avg_sq and a[9] is None and a[10] == NFLOATS and a[13] is o._state and a[14] == 12345
    assert a[12].data_ptr() == o._norm_out.data_ptr() + 4 and a[0]._obj.decoupled == 1
    o.param_groups[2]['lr'], o.param_groups[1]['frozen'], o.param_groups[0]['weight_decay'] = 7e-4, True, 0.5        # read at every step
    del rec.log[:]
    o.step()
    assert rec.names() == ['pa_grad_norm_groups', 'pa_adam_step_groups']
    nargs, a = rec.log[0][1], rec.log[1][1]
    assert nargs[0] is net.flat_grads and nargs[1] == NFLOATS and nargs[2] is o._map and nargs[3] == 0b010 and nargs[5] == 2.0 and nargs[7] is o._norm_out
    assert _table_of(a[1], 3) == [(1e-3, 0.5, 0), (1e-3, 0.0, 1), (7e-4, 1e-2, 0)]
    # RMSprop: the reference's recipe with groups still goes through the groups call (no clip: no norm)
    del rec.log[:]
    r = optim.RMSprop(net, momentum=0.9, groups=[dict(params='^bn1', frozen=True)])
    r.step()
    assert rec.names() == ['pa_rmsprop_step_groups']
    a = rec.log[-1][1]
    assert a[2] == 2 and _table_of(a[1], 2) == [(2.5e-4, 0.0, 0), (2.5e-4, 0.0, 1)] and a[3] is r._map and a[4] is net.flat_params
    assert a[6] is r.square_avg and a[7] is r.momentum_buffer and a[8] is None and a[9] == NFLOATS and a[11] is None and a[12] is r._skip_state
    assert a[0]._obj.momentum == pytest.approx(0.9) and a[0]._obj.weight_decay == 0.0
    # accumulate() and the EMA hook are untouched by groups: the fold, then the grouped step
    del rec.log[:]
    r.accumulate()
    r.step()
    assert rec.names() == ['pa_grad_accumulate', 'pa_grad_accumulate', 'pa_rmsprop_step_groups'] and rec.log[-1][1][10] == 0.5
    assert len(r.describe_groups()) == 2 and 'frozen 1' in r.describe_groups()[1] and '2 tensors, 8 floats' in r.describe_groups()[1]


def test_adjust_lr_keeps_the_multiples(rec):
    from pose_adv_aug_amd.utils import optim
    from pose_adv_aug_amd.utils.util import adjust_lr
    o = optim.RMSprop(_host_net(), lr=2.5e-4, groups=[dict(params='^hg', lr_mult=0.1), dict(params='^bn1', lr=1e-3)])
    single = optim.RMSprop(_host_net(), lr=2.5e-4)
    opt, opt1 = types.SimpleNamespace(lr=2.5e-4), types.SimpleNamespace(lr=2.5e-4)
    lrs = lambda: [g['lr'] for g in o.param_groups]
    adjust_lr(opt, o, 99), adjust_lr(opt1, single, 99)
    assert lrs() == [2.5e-4, 2.5e-4 * 0.1, 1e-3] and single.param_groups[0]['lr'] == 2.5e-4
    adjust_lr(opt, o, 100), adjust_lr(opt1, single, 100)
    assert opt.lr == 2.5e-4 * 0.2 and lrs() == [opt.lr, opt.lr * 0.1, pytest.approx(opt.lr * 4.0)] and single.param_groups[0]['lr'] == 2.5e-4 * 0.2
    adjust_lr(opt, o, 120)
    assert lrs()[0] == 2.5e-4 * 0.2
    adjust_lr(opt, o, 140), adjust_lr(opt1, single, 140)
    assert opt.lr == 2.5e-4 * 0.2 * 0.5 and lrs() == [opt.lr, opt.lr * 0.1, pytest.approx(opt.lr * 4.0)]
    assert single.param_groups[0]['lr'] == opt.lr and 'lr_mult' not in single.param_groups[0]


def test_state_dict_round_trips(rec):
    from pose_adv_aug_amd.utils import optim
    specs = lambda: [dict(params='^bn1', frozen=True, weight_decay=0.0), dict(params='^hg', lr_mult=0.1)]
    o = optim.AdamW(_host_net(), lr=1e-3, amsgrad=True, groups=specs())
    o.exp_avg.copy_(torch.arange(NFLOATS))
    sd = o.state_dict()
    assert [g['params'] for g in sd['param_groups']] == [[0, 1], [2, 3], [4, 5, 6]] and sorted(sd['state']) == list(range(7))
    assert sd['param_groups'][1]['frozen'] is True and sd['param_groups'][2]['lr_mult'] == 0.1 and sd['param_groups'][2]['names'][0] == 'hg.0.conv.weight'
    assert sd['state'][5]['exp_avg'].flatten().tolist() == list(range(40, 46))
    # its own file: every per-group value and the shared options come back, no warning
    for g, lr in zip(sd['param_groups'], (3e-3, 2e-3, 1e-3)):
        g['lr'], g['eps'] = lr, 1e-6
    sd['param_groups'][1]['frozen'], sd['param_groups'][2]['lr_mult'], sd['param_groups'][0]['weight_decay'] = False, 0.25, 0.3
    o2 = optim.AdamW(_host_net(), lr=1e-3, amsgrad=True, groups=specs())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o2.load_state_dict(sd)
    assert not w, [str(x.message) for x in w]
    g = o2.param_groups
    assert [x['lr'] for x in g] == [3e-3, 2e-3, 1e-3] and [x['frozen'] for x in g] == [False, False, False] and g[2]['lr_mult'] == 0.25
    assert g[0]['weight_decay'] == 0.3 and all(x['eps'] == 1e-6 for x in g) and all(torch.equal(o2.exp_avg[t[2]:t[2] + t[3]], o.exp_avg[t[2]:t[2] + t[3]]) for t in TABLE[:7])
    assert [x['params'] for x in g] == [[0, 1], [2, 3], [4, 5, 6]]
    o2.step()                                                               # the shared options agree in every group
    # a single-group file into the three-group optimizer: the state by position, the shared options, ONE warning, own per-group values
    one = optim.AdamW(_host_net(), lr=5e-2, eps=1e-5, weight_decay=0.7, amsgrad=True)
    one.exp_avg_sq.copy_(torch.arange(NFLOATS) * 2.0)
    o3 = optim.AdamW(_host_net(), lr=1e-3, amsgrad=True, groups=specs())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o3.load_state_dict(one.state_dict())
    assert len(w) == 1 and 'keeps its own lr' in str(w[0].message), [str(x.message) for x in w]
    g = o3.param_groups
    assert [x['lr'] for x in g] == [1e-3, 1e-3, 1e-4] and [x['weight_decay'] for x in g] == [1e-2, 0.0, 1e-2] and [x['frozen'] for x in g] == [False, True, False]
    assert all(x['eps'] == 1e-5 for x in g) and all(torch.equal(o3.exp_avg_sq[t[2]:t[2] + t[3]], one.exp_avg_sq[t[2]:t[2] + t[3]]) for t in TABLE[:7])
    # and RMSprop, three groups, through a file in torch's numbering (ids in chained group order)
    r = optim.RMSprop(_host_net(), momentum=0.9, groups=[dict(params='^hg', lr=1e-5), dict(params='^bn1', frozen=True)])
    assert [x['params'] for x in r.param_groups] == [[0, 1], [4, 5, 6], [2, 3]]
    r.square_avg.copy_(torch.arange(NFLOATS))
    sd = r.state_dict()
    order = [0, 1, 4, 5, 6, 2, 3]
    torch_sd = {'state': dict((j, sd['state'][i]) for j, i in enumerate(order)),
                'param_groups': [dict(((k, v) for k, v in g.items() if k != 'names'), params=[order.index(i) for i in g['params']])
                                 for g in sd['param_groups']]}
    torch_sd['param_groups'][1]['lr'] = 3e-5
    r2 = optim.RMSprop(_host_net(), momentum=0.9, groups=[dict(params='^hg', lr=1e-5), dict(params='^bn1', frozen=True)])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        r2.load_state_dict(torch_sd)
    assert not w and r2.param_groups[1]['lr'] == 3e-5 and r2.param_groups[2]['frozen'] is True
    for t in TABLE[:7]:
        assert torch.equal(r2.square_avg[t[2]:t[2] + t[3]], r.square_avg[t[2]:t[2] + t[3]]), t[0]


def test_a_file_with_the_same_group_sizes_and_other_members_is_not_this_partition(rec):
    """this class's own file names its members: equal sizes are not enough.  The state goes to the parameter each id names, the per-group
    values stay this optimizer's, one warning"""
    from pose_adv_aug_amd.utils import optim
    a = optim.Adam(_host_net(), lr=1e-3, groups=[dict(params=['bn1.weight', 'bn1.bias'], lr=5e-3, frozen=True)])
    b = optim.Adam(_host_net(), lr=1e-3, groups=[dict(params=['conv1.bias', 'hg.1.bn.bias'], lr=7e-4)])
    assert [len(g['params']) for g in a.param_groups] == [len(g['params']) for g in b.param_groups] == [5, 2]
    a.exp_avg.copy_(torch.arange(NFLOATS))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        b.load_state_dict(a.state_dict())
    assert len(w) == 1 and 'keeps its own lr' in str(w[0].message), [str(x.message) for x in w]
    assert [g['lr'] for g in b.param_groups] == [1e-3, 7e-4] and [g['frozen'] for g in b.param_groups] == [False, False]
    for t in TABLE[:7]:
        assert torch.equal(b.exp_avg[t[2]:t[2] + t[3]], a.exp_avg[t[2]:t[2] + t[3]]), t[0]


def test_the_command_line(tmp_path, rec):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils import optim
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e']
    opt = TrainOptions().parse(base)
    assert (opt.no_decay_1d, opt.freeze, opt.lr_group) == (0, '', []) and optim.group_specs(opt, _host_net()) is None
    assert len(optim.make_optimizer(opt, _host_net(), 2.5e-4).param_groups) == 1
    args = base + ['--optimizer', 'adamw', '--weight_decay', '0.01', '--no_decay_1d', '1', '--freeze', r'^(conv1|bn1)\.', '--lr_group', r'hg\.1\.:0.1']
    opt = TrainOptions().parse(args)
    o = optim.make_optimizer(opt, _host_net(), 1e-3)
    g = o.param_groups
    assert type(o) is optim.AdamW and [x['names'] for x in g] == [['hg.0.conv.weight'], ['conv1.weight', 'conv1.bias', 'bn1.weight', 'bn1.bias'],
                                                                  ['hg.1.bn.bias'], ['hg.1.conv.weight']]
    assert [x['frozen'] for x in g] == [False, True, False, False] and [x['weight_decay'] for x in g] == [0.01, 0.01, 0.0, 0.01]
    assert [x['lr'] for x in g] == [1e-3, 1e-3, pytest.approx(1e-4), pytest.approx(1e-4)] and [x['lr_mult'] for x in g] == [1.0, 1.0, 0.1, 0.1]
    # the agent: --no_decay_1d only
    a = optim.make_optimizer(opt, _host_net(pose=False), 5e-5)
    assert [x['frozen'] for x in a.param_groups] == [False, False] and a.param_groups[1]['names'] == ['conv1.bias', 'bn1.weight', 'bn1.bias', 'hg.1.bn.bias']
    assert a.param_groups[1]['weight_decay'] == 0.0 and a.param_groups[1]['lr'] == 5e-5
    r = optim.make_optimizer(TrainOptions().parse(base + ['--lr_group', '^hg:0.5', '--lr_group', r'^bn1\.:2']), _host_net(), 2.5e-4)
    assert type(r) is optim.RMSprop and [x['lr'] for x in r.param_groups] == [2.5e-4, 1.25e-4, 5e-4]
    for bad in (['--freeze', '^nothing'], ['--lr_group', '^nothing:0.1'], ['--lr_group', '^hg'], ['--lr_group', '^hg:fast'], ['--lr_group', '^hg:-1']):
        with pytest.raises(ValueError):
            optim.make_optimizer(TrainOptions().parse(base + bad), _host_net(), 1e-3)


def _stub_worker(out):
    fake = abi_stub.install(0)
    from pose_adv_aug_amd.models.asn_stacked_hg import create_hg
    from pose_adv_aug_amd.utils import optim
    net = create_hg(2, 1, 16, 256, default_batch=2)
    net._net(2)
    optimizer_calls = lambda: [n for n in fake.names() if n.startswith(('pa_rmsprop', 'pa_adam', 'pa_grad_norm', 'pa_opt'))]
    for key, make in (('rmsprop', lambda: optim.RMSprop(net)), ('rmsprop opts', lambda: optim.RMSprop(net, momentum=0.9, centered=True, max_grad_norm=1.0)),
                      ('adam', lambda: optim.Adam(net)), ('adamw', lambda: optim.AdamW(net, max_grad_norm=1.0))):
        o = make()
        del fake.log[:]
        o.step()
        out[key] = optimizer_calls()
    del fake.log[:]
    o = optim.AdamW(net, groups=[dict(params=optim.no_decay_1d, weight_decay=0.0), dict(params='^conv1', frozen=True)], max_grad_norm=1.0)
    out['names'] = [g['names'] for g in o.param_groups]
    out['map built'] = optimizer_calls()
    del fake.log[:]
    o.step()
    o.step()
    out['grouped'] = optimizer_calls()
    norm, step = [[a for n, a in fake.log if n == name][-1] for name in ('pa_grad_norm_groups', 'pa_adam_step_groups')]
    out['mask, ngroups, table'] = (norm[3], step[2], [(round(step[1][k].lr, 7), round(step[1][k].weight_decay, 7), step[1][k].frozen) for k in range(3)])


def test_the_stub_library_sees_todays_calls_without_groups_and_the_groups_calls_with_them():
    """tests/abi_stub.py's recording library under the real net and optimizer classes, in a process of its own (it patches the package)"""
    import multiprocessing as mp
    out = mp.Manager().dict()
    p = mp.get_context('spawn').Process(target=_stub_worker, args=(out,))
    p.start(); p.join(120)
    assert p.exitcode == 0
    # (the stub logs pa_rmsprop_step_state under the name of the stateless call it forwards to, and answers the workspace size unlogged)
    assert out['rmsprop'] == ['pa_rmsprop_step'] and out['rmsprop opts'] == ['pa_grad_norm', 'pa_rmsprop_step_opts']
    assert out['adam'] == ['pa_adam_step'] and out['adamw'] == ['pa_grad_norm', 'pa_adam_step']
    assert out['names'] == [[], ['conv1.bias', 'bn1.weight', 'bn1.bias'], ['conv1.weight']]
    assert out['map built'] == ['pa_opt_chunk_map_host']
    assert out['grouped'] == ['pa_grad_norm_groups', 'pa_adam_step_groups'] * 2
    assert out['mask, ngroups, table'] == (0b100, 3, [(1e-3, 1e-2, 0), (1e-3, 0.0, 0), (1e-3, 1e-2, 1)])

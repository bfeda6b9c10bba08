"""The bound of tests/adam_exact.py is not vacuous, its reference is torch's formula, and the host side of utils.optim.Adam.

A numpy fp32 emulation of adam_kernel (csrc/elementwise.hip), each operation rounded on its own -- and the same with the update of v
contracted into one fma -- stays inside the bound for p, exp_avg, exp_avg_sq and max_exp_avg_sq over 200 003 elements under every
decay mode, with and without amsgrad (with a clip coefficient), at every gscale of optim_exact.GSCALES.  Each of these defects is at
least 1e3 times the bound in some output (amsgrad on, at t = 2 from non-zero state):
  * bias correction dropped, or taken at t - 1 (these sit in the constants of the state: check_consts);
  * eps inside the root; eps added before the division by bc2s;
  * coupled decay applied after the moments; decoupled decay without lr;
  * beta1 and 1 - beta1 swapped; vmax not used in the denominator;
  * the clip coefficient dropped, or applied twice;
  * four elements left untouched, or updated twice.
Semantic anchor: five steps of the float64 reference equal torch.optim.Adam / AdamW on float64 CPU tensors for every decay mode, with
and without amsgrad.  Host control flow of the optimizer class against a recording stand-in for the library; the command line."""
import types

import numpy as np
import pytest
import torch

from tests import optim_exact as X
from tests import adam_exact as A

N = 200003
f = np.float32
COEF = float(f(0.37))
T = 2
t = torch.from_numpy


def _consts(step, defect=None):
    """the four constants as adam_prologue_kernel forms them (pow in double, one rounding; then fp32)"""
    if defect == 'bias correction at t - 1':
        step -= 1
    bc1 = f(1.0 - float(f(A.BETA1)) ** step)
    bc2 = f(1.0 - float(f(A.BETA2)) ** step)
    if defect == 'bias correction dropped':
        bc1 = bc2 = f(1)
    return {'step': T, 'bc1': float(bc1), 'bc2': float(bc2), 'step_size': float(f(A.LR) / bc1), 'bc2s': float(np.sqrt(bc2))}


def _emulate(s, g, gscale, coef, wd, decoupled, amsgrad, c, defect=None, fma=False):
    lr, b1, b2, eps, sc, w = f(A.LR), f(A.BETA1), f(A.BETA2), f(A.EPS), f(gscale), f(wd)
    o1, o2 = f(1) - b1, f(1) - b2
    bc2s, step_size = f(c['bc2s']), f(c['step_size'])
    p, m, v, vmax = s['p'], s['exp_avg'], s['exp_avg_sq'], s['max_exp_avg_sq']
    gr = g * sc
    if coef is not None and defect != 'coef dropped':
        gr = gr * f(coef)
        if defect == 'coef twice':
            gr = gr * f(coef)
    g0 = gr
    if wd != 0:
        if decoupled:
            p = p * (f(1) - w if defect == 'decoupled decay without lr' else f(A.c_dec(A.LR, wd)))
        else:
            gr = gr + w * p
    gm = g0 if defect == 'coupled decay after the moments' else gr
    mm = m + (gm - m) * (b1 if defect == 'beta1 swapped' else o1)
    tt = (o2 * gm) * gm
    if fma:         # fmaf(beta2, v, tt): one rounding (float64 holds the product and the sum far beyond fp32's precision)
        vv = (b2.astype(np.float64) * v.astype(np.float64) + tt.astype(np.float64)).astype(np.float32)
    else:
        vv = b2 * v + tt
    out = {'exp_avg': mm, 'exp_avg_sq': vv}
    vhat = vv
    if amsgrad:
        out['max_exp_avg_sq'] = np.maximum(vmax, vv)
        if defect != 'vmax not in the denominator':
            vhat = out['max_exp_avg_sq']
    if defect == 'eps inside the root':
        den = np.sqrt(vhat + eps) / bc2s
    elif defect == 'eps before the division':
        den = (np.sqrt(vhat) + eps) / bc2s
    else:
        den = np.sqrt(vhat) / bc2s + eps
    upd = mm / den
    if defect == 'coupled decay after the moments':
        upd = upd + w * p
    out['p'] = p - step_size * upd
    assert all(a.dtype == np.float32 for a in out.values())
    return out


def _inputs(gscale, zero, seed=7):
    p, g, v = X.make_inputs(N, seed, gscale, zero)
    m, vmax = A.make_state(N, seed, v, zero)
    return {'p': p, 'exp_avg': m, 'exp_avg_sq': v, 'max_exp_avg_sq': vmax}, g


def _step(state, g, gscale, coef, wd, decoupled, amsgrad, c, defect=None, fma=False):
    out = _emulate(state, g, gscale, coef, wd, decoupled, amsgrad, c, defect, fma)
    k = N - 7           # a chunk that ends in the tail region of an n with n % 4 == 3
    if defect == 'four untouched':
        for name in out:
            out[name][k:k + 4] = state[name][k:k + 4]
    if defect == 'four twice':
        again = _emulate(dict(state, **out), g, gscale, coef, wd, decoupled, amsgrad, c)
        for name in out:
            out[name][k:k + 4] = again[name][k:k + 4]
    return out


def _check(state, g, out, gscale, coef, wd, decoupled, amsgrad, c):
    tt = lambda d: dict((k, None if a is None else t(a)) for k, a in d.items())
    before = dict(state, max_exp_avg_sq=state['max_exp_avg_sq'] if amsgrad else None)
    after = dict((k, out.get(k)) for k in A.OUTPUTS)
    return A.check(tt(before), t(g), tt(after), gscale, coef, c, wd, decoupled, amsgrad)


@pytest.mark.parametrize('gscale', X.GSCALES)
@pytest.mark.parametrize('decay,amsgrad', A.COMBOS)
@pytest.mark.parametrize('fma', (False, True))
def test_the_emulated_kernel_is_inside_the_bound(gscale, decay, amsgrad, fma):
    wd, decoupled = decay
    c = _consts(T)
    assert all(x <= 1.0 for x in A.check_consts(c, T).values()), A.check_consts(c, T)
    worst = {}
    for zero in (True, False):
        state, g = _inputs(gscale, zero)
        out = _step(state, g, gscale, COEF, wd, decoupled, amsgrad, c, fma=fma)
        r, (took, kept) = _check(state, g, out, gscale, COEF, wd, decoupled, amsgrad, c)
        print('gscale %g wd %g decoupled %d amsgrad %d state %s fma %s: worst error / bound %s' % (gscale, wd, decoupled, amsgrad, 'zero' if zero else 'nonzero', fma, r))
        assert sorted(r) == sorted(['p', 'exp_avg', 'exp_avg_sq'] + (['max_exp_avg_sq'] if amsgrad else []))
        assert all(x <= 1.0 for x in r.values()), r
        if amsgrad and not zero:
            assert took > 1000 and kept > 1000, (took, kept)            # both branches of the maximum
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
    # the bound is tight: the emulation uses a good part of it, in every output
    assert all(x > 0.2 for x in worst.values()), worst


CONST_DEFECTS = ('bias correction dropped', 'bias correction at t - 1')
DEFECTS = ('eps inside the root', 'eps before the division', 'coupled decay after the moments', 'decoupled decay without lr', 'beta1 swapped',
           'vmax not in the denominator', 'coef dropped', 'coef twice', 'four untouched', 'four twice')


@pytest.mark.parametrize('defect', CONST_DEFECTS)
def test_a_wrong_bias_correction_is_far_outside_the_bounds_of_the_constants(defect):
    r = A.check_consts(_consts(T, defect), T)
    print('%s: error / bound %s' % (defect, r))
    assert not all(x <= 1e3 for x in r.values()), r
    # and a step count that is one off is refused whatever the constants are
    assert A.check_consts(dict(_consts(T), step=T + 1), T)['step'] > 1e3


@pytest.mark.parametrize('gscale', X.GSCALES)
@pytest.mark.parametrize('defect', DEFECTS)
def test_each_defect_is_far_outside_the_bound(defect, gscale):
    wd, decoupled = (1e-2, True) if defect == 'decoupled decay without lr' else (1e-4, False)
    c = _consts(T)
    state, g = _inputs(gscale, False)
    out = _step(state, g, gscale, COEF, wd, decoupled, True, c, defect)
    r, _ = _check(state, g, out, gscale, COEF, wd, decoupled, True, c)
    print('%s, gscale %g: error / bound %s' % (defect, gscale, r))
    assert not all(x <= 1e3 for x in r.values()), r          # (a NaN counts as outside, as in the GPU check)


# lr = 2^-10 and weight decay 2^-6 for the decoupled mode: 1 - lr wd = 1 - 2^-16 is an fp32 number, so the factor the C ABI rounds to
# fp32 (adam_exact.c_dec) is the float64 factor torch multiplies by, and the comparison below can ask for 1e-12 there too
@pytest.mark.parametrize('decay,amsgrad', tuple((d, a) for d in ((0.0, False), (1e-4, False), (2.0 ** -6, True)) for a in (False, True)))
def test_the_reference_is_torch_adam(decay, amsgrad):
    """five steps in float64: the reference's values (its fp32 constants handed to torch as they are) against torch.optim.Adam / AdamW"""
    wd, decoupled = decay
    n = 4099
    lr = 2.0 ** -10
    p, _, v = X.make_inputs(n, 31, 1.0, True)
    lr32, b1, b2, eps32, w32 = (X._f32(x) for x in (lr, A.BETA1, A.BETA2, A.EPS, wd))
    assert not decoupled or A.c_dec(lr, wd) == 1.0 - lr32 * w32
    q = torch.nn.Parameter(t(p).double())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    topt = cls([q], lr=lr32, betas=(b1, b2), eps=eps32, weight_decay=w32, amsgrad=amsgrad)
    z = lambda: torch.zeros(n, dtype=torch.float64)
    cur = {'p': t(p).double(), 'exp_avg': z(), 'exp_avg_sq': z(), 'max_exp_avg_sq': z()}
    for k in range(5):
        g = t(X.make_inputs(n, 40 + k, 1.0, True)[1]).double()
        bc1, bc2 = 1.0 - b1 ** (k + 1), 1.0 - b2 ** (k + 1)
        ref, _ = A.reference(cur['p'], g, cur['exp_avg'], cur['exp_avg_sq'], cur['max_exp_avg_sq'], 1.0, None, bc2 ** 0.5, lr32 / bc1,
                             wd, decoupled, amsgrad, lr=lr)
        prev = dict(cur)
        for name, e in ref.items():
            cur[name] = e.v
        q.grad = g.clone()
        topt.step()
        st = topt.state[q]
        assert float(st['step']) == k + 1
        # relative to the larger of the value and the value it was updated from: m' and p' are sums whose terms can cancel
        rel = lambda name, b: float(((cur[name] - b).abs() / torch.maximum(b.abs(), prev[name].abs()).clamp_min(1e-300)).max())
        assert rel('p', q.detach()) <= 1e-12 and rel('exp_avg', st['exp_avg']) <= 1e-12 and rel('exp_avg_sq', st['exp_avg_sq']) <= 1e-12
        if amsgrad:
            assert rel('max_exp_avg_sq', st['max_exp_avg_sq']) <= 1e-12
        else:
            assert 'max_exp_avg_sq' not in ref and 'max_exp_avg_sq' not in st


class _Recorder(object):
    """stands in for the library under utils.optim (host control flow only): logs every pa_* call, computes nothing"""
    def __init__(self):
        self.log = []

    def pa_grad_scale(self):
        return 1.0

    def pa_grad_norm_workspace_bytes(self, n):
        return 16

    def __getattr__(self, name):
        if not name.startswith('pa_'):
            raise AttributeError(name)

        def call(*args):
            self.log.append((name, args))
            return 0
        return call


def _host_net():
    table = [('a.weight', (2, 3), 0, 6, 0), ('a.bias', (3,), 8, 3, 0)]
    return types.SimpleNamespace(flat_params=torch.zeros(12), flat_grads=torch.ones(12), _table=table, _last_B=1, default_batch=1,
                                 _ensure_table=lambda: None, weights_changed=lambda: None, _net=lambda B: None)


def _host_optimizer(monkeypatch, cls='Adam', **kw):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.utils import optim
    rec = _Recorder()
    for mod in (optim, _lib):
        monkeypatch.setattr(mod, 'lib', lambda: rec)
    monkeypatch.setattr(optim, 'ptr', lambda x: x)
    monkeypatch.setattr(optim, 'stream', lambda: 12345)
    net = _host_net()
    return getattr(optim, cls)(net, **kw), rec, net


def test_default_step_is_the_one_adam_call(monkeypatch):
    o, rec, net = _host_optimizer(monkeypatch)
    o.step()
    assert [n for n, _ in rec.log] == ['pa_adam_step']
    args = rec.log[0][1]
    opts = args[0]._obj
    assert (round(opts.lr, 9), round(opts.beta1, 6), round(opts.beta2, 6), round(opts.eps, 12), opts.weight_decay, opts.amsgrad, opts.decoupled) == (1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    assert args[1] is net.flat_params and args[2] is net.flat_grads and args[3] is o.exp_avg and args[4] is o.exp_avg_sq and args[5] is None
    assert args[6] == 12 and args[7] == 1.0 and args[8] is None and args[9] is o._state and args[10] == 12345
    assert o._state.dtype == torch.int32 and o._state.numel() == 8 and not bool(o._state.any())
    assert o.max_exp_avg_sq is None and o._norm_out is None and o.last_grad_norm() is None
    sd = o.state_dict()
    assert sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step'] and sd['state'][1]['exp_avg'].shape == (3,)
    assert sd['state'][0]['step'].dtype == torch.float32 and sd['state'][0]['step'].dim() == 0
    assert sd['param_groups'][0] == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, decoupled_weight_decay=False, params=[0, 1])


def test_clipping_goes_through_the_norm_then_the_adam_step(monkeypatch):
    o, rec, net = _host_optimizer(monkeypatch, amsgrad=True, weight_decay=1e-4, max_grad_norm=2.0)
    o.step()
    o.param_groups[0]['lr'] = 5e-4          # read at every step
    o.step()
    assert [n for n, _ in rec.log] == ['pa_grad_norm', 'pa_adam_step'] * 2
    (_, norm_args), (_, step_args) = rec.log[2], rec.log[3]
    assert norm_args[0] is net.flat_grads and norm_args[1] == 12 and norm_args[3] == 2.0 and norm_args[5] is o._norm_out
    opts = step_args[0]._obj
    assert (round(opts.lr, 9), round(opts.weight_decay, 9), opts.amsgrad, opts.decoupled) == (5e-4, 1e-4, 1, 0)
    assert step_args[5] is o.max_exp_avg_sq and o.max_exp_avg_sq is not None
    assert step_args[8].data_ptr() == o._norm_out.data_ptr() + 4 and step_args[9] is o._state
    assert sorted(o.state_dict()['state'][1]) == ['exp_avg', 'exp_avg_sq', 'max_exp_avg_sq', 'step']


def test_max_exp_avg_sq_exists_exactly_with_amsgrad(monkeypatch):
    o, rec, _ = _host_optimizer(monkeypatch, cls='AdamW')
    assert o.max_exp_avg_sq is None and o.param_groups[0]['weight_decay'] == 1e-2 and o.param_groups[0]['decoupled_weight_decay'] is True
    o.step()
    assert o.max_exp_avg_sq is None and rec.log[-1][1][5] is None and rec.log[-1][1][0]._obj.decoupled == 1
    o.param_groups[0]['amsgrad'] = True         # allocated when amsgrad is first on
    o.step()
    assert o.max_exp_avg_sq is not None and rec.log[-1][1][5] is o.max_exp_avg_sq and not bool(o.max_exp_avg_sq.any())
    o2, _, _ = _host_optimizer(monkeypatch, amsgrad=True)
    assert o2.max_exp_avg_sq is not None
    from pose_adv_aug_amd.utils import optim
    for bad in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(weight_decay=-1.0), dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            optim.Adam(_host_net(), **bad)


def test_an_rmsprop_file_loads_with_one_warning(monkeypatch):
    import warnings
    o, rec, net = _host_optimizer(monkeypatch, amsgrad=True)
    from pose_adv_aug_amd.utils import optim
    r = optim.RMSprop(_host_net(), momentum=0.9)
    o.exp_avg.fill_(1.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o.load_state_dict(r.state_dict())
    assert len(w) == 1 and 'square_avg' in str(w[0].message) and 'exp_avg' in str(w[0].message)
    assert not bool(o.exp_avg.any()) and o.param_groups[0]['lr'] == 1e-3 and 'alpha' not in o.param_groups[0]
    assert rec.log[-1][0] == 'pa_adam_set_steps' and rec.log[-1][1][1] == 0
    # its own file: no warning, the step count goes to the device, a list of betas comes back as a tuple
    sd = o.state_dict()
    for st in sd['state'].values():
        st['step'] = torch.tensor(7.0)
    sd['param_groups'][0]['betas'] = [0.8, 0.99]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o.load_state_dict(sd)
    assert not w and rec.log[-1][0] == 'pa_adam_set_steps' and rec.log[-1][1][1] == 7 and o.param_groups[0]['betas'] == (0.8, 0.99)
    # a missing and a mis-shaped entry are reported
    del sd['state'][0]['exp_avg_sq']
    sd['state'][1]['exp_avg'] = torch.zeros(5)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        o.load_state_dict(sd)
    text = ' | '.join(str(x.message) for x in w)
    assert 'a.bias: exp_avg has 5 elements, expected 3' in text and '1 of 2 parameters had no exp_avg_sq' in text and '1 of 2 parameters had no exp_avg entry' in text


def test_the_command_line_picks_the_optimizer(tmp_path, monkeypatch):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils import optim
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e']
    opt = TrainOptions().parse(base)
    assert opt.optimizer == 'rmsprop' and (opt.beta1, opt.beta2, opt.adam_eps, opt.amsgrad) == (0.9, 0.999, 1e-8, 0)
    o = optim.make_optimizer(opt, _host_net(), 2.5e-4)
    assert type(o) is optim.RMSprop and o.max_grad_norm is None
    assert o.param_groups[0] == optim.RMSprop(_host_net(), lr=2.5e-4, alpha=0.99, eps=1e-8, **optim.optim_options(opt)).param_groups[0]
    assert o.param_groups[0] == dict(lr=2.5e-4, alpha=0.99, eps=1e-8, momentum=0.0, weight_decay=0.0, centered=False)
    opt = TrainOptions().parse(base + ['--optimizer', 'adamw', '--weight_decay', '0.05', '--amsgrad', '1', '--clip_grad_norm', '10', '--beta2', '0.99'])
    o = optim.make_optimizer(opt, _host_net(), 5e-5)
    assert type(o) is optim.AdamW and o.max_grad_norm == 10.0 and o.max_exp_avg_sq is not None
    assert o.param_groups[0] == dict(lr=5e-5, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05, amsgrad=True, decoupled_weight_decay=True)
    o = optim.make_optimizer(TrainOptions().parse(base + ['--optimizer', 'adam']), _host_net(), 1e-3)
    assert type(o) is optim.Adam and o.param_groups[0]['decoupled_weight_decay'] is False and o.max_exp_avg_sq is None
    for extra in (['--momentum', '0.9'], ['--centered', '1']):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + ['--optimizer', 'adam'] + extra)
    with pytest.raises(SystemExit):
        TrainOptions().parse(base + ['--optimizer', 'sgd'])
    for name in ('pa_adam_step', 'pa_adam_steps', 'pa_adam_set_steps'):
        assert name in _lib.EXPORTS

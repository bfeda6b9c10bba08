"""The bound of tests/optim_opts_exact.py is not vacuous, and its reference is torch's formula.

A numpy fp32 emulation of rmsprop_opts_kernel (csrc/elementwise.hip), each operation rounded on its own -- and the same with the update
of v contracted into one fma -- stays inside the bound for p, square_avg, momentum_buffer and grad_avg over 200 003 elements under
all eight option combinations (with a clip coefficient) at every gscale of optim_exact.GSCALES, and uses a good part of it.  Each of
these defects is at least 1e3 times the bound in some output (all options on):
  * weight decay added after the update of v instead of before it; weight decay scaled by lr;
  * grad_avg updated with alpha and 1 - alpha swapped; ga'^2 not subtracted; eps inside the root;
  * the momentum buffer not multiplied by the momentum; lr applied inside the buffer;
  * the clip coefficient dropped, or applied twice;
  * four elements left untouched, or updated twice.
Semantic anchor: five steps of the float64 reference equal torch.optim.RMSprop on float64 CPU tensors with the same options, and the
clip reference equals torch.nn.utils.clip_grad_norm_.  The clamp max(0, v' - ga'^2) is never what makes a case pass: no E interval of
v' - ga'^2 reaches 0, on the first step or over three consecutive emulated steps with fresh gradients."""
import numpy as np
import pytest
import torch

from tests import optim_exact as X
from tests import optim_opts_exact as Y

N = 200003
f = np.float32
COEF = float(f(0.37))
t = torch.from_numpy


def _emulate(p, g, v, buf, ga, gscale, coef, mom, wd, centered, defect=None, fma=False):
    lr, alpha, eps, s, m, w = f(X.LR), f(X.ALPHA), f(X.EPS), f(gscale), f(mom), f(wd)
    c = f(1) - alpha
    gr = g * s
    if coef is not None and defect != 'coef dropped':
        gr = gr * f(coef)
        if defect == 'coef twice':
            gr = gr * f(coef)
    g0 = gr
    if wd != 0:
        gr = gr + (lr * w if defect == 'decay scaled by lr' else w) * p
    gv = g0 if defect == 'decay after v' else gr
    tt = c * gv * gv
    if fma:         # fmaf(alpha, v, tt): one rounding (float64 holds the product and the sum far beyond fp32's precision)
        vv = (alpha.astype(np.float64) * v.astype(np.float64) + tt.astype(np.float64)).astype(np.float32)
    else:
        vv = alpha * v + tt
    out = {'square_avg': vv}
    var = vv
    if centered:
        aa = (c * ga + alpha * gr) if defect == 'ga weights swapped' else (alpha * ga + c * gr)
        out['grad_avg'] = aa
        if defect != 'ga^2 not subtracted':
            var = np.maximum(f(0), vv - aa * aa)
    den = np.sqrt(var + eps) if defect == 'eps inside the root' else np.sqrt(var) + eps
    q = gr / den
    if mom > 0:
        if defect == 'lr inside buf':
            bb = m * buf + lr * q
            pp = p - bb
        else:
            bb = (buf if defect == 'buf not times mom' else m * buf) + q
            pp = p - lr * bb
        out['momentum_buffer'] = bb
    else:
        pp = p - lr * q
    out['p'] = pp
    assert all(a.dtype == np.float32 for a in out.values())
    return out


def _inputs(gscale, zero, seed=7):
    p, g, v = X.make_inputs(N, seed, gscale, zero)
    buf, ga = Y.make_state(N, seed, v, zero)
    return {'p': p, 'square_avg': v, 'momentum_buffer': buf, 'grad_avg': ga}, g


def _step(state, g, gscale, coef, mom, wd, centered, defect=None, fma=False):
    out = _emulate(state['p'], g, state['square_avg'], state['momentum_buffer'], state['grad_avg'], gscale, coef, mom, wd, centered, defect, fma)
    k = N - 7           # a chunk that ends in the tail region of an n with n % 4 == 3
    if defect == 'four untouched':
        for name in out:
            out[name][k:k + 4] = state[name][k:k + 4]
    if defect == 'four twice':
        nxt = dict(state, **out)
        again = _emulate(nxt['p'], g, nxt['square_avg'], nxt['momentum_buffer'], nxt['grad_avg'], gscale, coef, mom, wd, centered)
        for name in out:
            out[name][k:k + 4] = again[name][k:k + 4]
    return out


def _check(state, g, out, gscale, coef, mom, wd, centered):
    tt = lambda d: dict((k, None if a is None else t(a)) for k, a in d.items())
    after = dict((k, out.get(k)) for k in Y.OUTPUTS)
    return Y.check(tt(state), t(g), tt(after), gscale, coef, mom, wd, centered)


@pytest.mark.parametrize('gscale', X.GSCALES)
@pytest.mark.parametrize('mom,wd,centered', Y.COMBOS)
@pytest.mark.parametrize('fma', (False, True))
def test_the_emulated_kernel_is_inside_the_bound(gscale, mom, wd, centered, fma):
    worst = {}
    for zero in (True, False):
        state, g = _inputs(gscale, zero)
        out = _step(state, g, gscale, COEF, mom, wd, centered, fma=fma)
        r, reach = _check(state, g, out, gscale, COEF, mom, wd, centered)
        print('gscale %g mom %g wd %g centered %d state %s fma %s: worst error / bound %s' % (gscale, mom, wd, centered, 'zero' if zero else 'nonzero', fma, r))
        assert reach == 0
        assert sorted(r) == sorted(['p', 'square_avg'] + (['momentum_buffer'] if mom > 0 else []) + (['grad_avg'] if centered else []))
        assert all(x <= 1.0 for x in r.values()), r
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
    # the bound is tight: the emulation uses a good part of it, in every output
    assert all(x > 0.2 for x in worst.values()), worst


def test_without_a_coefficient_and_options_the_reference_is_the_plain_one():
    """all off, coef None: the E terms of optim_exact.reference, value and bound"""
    state, g = _inputs(1.0 / 3.0, False)
    ref, reach = Y.reference(t(state['p']).double(), t(g).double(), t(state['square_avg']).double(), None, None, 1.0 / 3.0)
    rp, rv = X.reference(t(state['p']).double(), t(g).double(), t(state['square_avg']).double(), gscale=1.0 / 3.0)
    assert reach == 0 and sorted(ref) == ['p', 'square_avg']
    assert torch.equal(ref['p'].v, rp.v) and torch.equal(ref['p'].e, rp.e) and torch.equal(ref['square_avg'].v, rv.v) and torch.equal(ref['square_avg'].e, rv.e)


DEFECTS = ('decay after v', 'decay scaled by lr', 'ga weights swapped', 'ga^2 not subtracted', 'eps inside the root', 'buf not times mom',
           'lr inside buf', 'coef dropped', 'coef twice', 'four untouched', 'four twice')


@pytest.mark.parametrize('gscale', X.GSCALES)
@pytest.mark.parametrize('defect', DEFECTS)
def test_each_defect_is_far_outside_the_bound(defect, gscale):
    state, g = _inputs(gscale, False)
    out = _step(state, g, gscale, COEF, Y.MOM, Y.WD, True, defect)
    r, _ = _check(state, g, out, gscale, COEF, Y.MOM, Y.WD, True)
    print('%s, gscale %g: error / bound %s' % (defect, gscale, r))
    assert not all(x <= 1e3 for x in r.values()), r          # (a NaN counts as outside, as in the GPU check)


@pytest.mark.parametrize('mom,wd,centered', Y.COMBOS)
def test_the_reference_is_torch_rmsprop(mom, wd, centered):
    """five steps in float64: the reference's values (its fp32 constants handed to torch as they are) against torch.optim.RMSprop"""
    n = 4099
    p, _, v = X.make_inputs(n, 31, 1.0, True)
    a32, lr32, eps32, m32, w32 = (X._f32(x) for x in (X.ALPHA, X.LR, X.EPS, mom, wd))
    q = torch.nn.Parameter(t(p).double())
    topt = torch.optim.RMSprop([q], lr=lr32, alpha=a32, eps=eps32, momentum=m32, weight_decay=w32, centered=centered)
    cur = {'p': t(p).double(), 'square_avg': t(v).double(), 'momentum_buffer': torch.zeros(n, dtype=torch.float64), 'grad_avg': torch.zeros(n, dtype=torch.float64)}
    for k in range(5):
        g = t(X.make_inputs(n, 40 + k, 1.0, True)[1]).double()
        ref, reach = Y.reference(cur['p'], g, cur['square_avg'], cur['momentum_buffer'], cur['grad_avg'], 1.0, None, mom, wd, centered)
        assert reach == 0            # the clamp is not hit: torch's unclamped root is the same number
        prev = dict(cur)
        for name, e in ref.items():
            cur[name] = e.v
        q.grad = g.clone()
        topt.step()
        st = topt.state[q]
        # relative to the larger of the value and the value it was updated from: buf' = mom buf + gr / den, ga' and p' are sums whose
        # terms can cancel, and torch rounds ga' differently (lerp), so no arithmetic gives the cancelled sum itself to 1e-12
        rel = lambda name, b: float(((cur[name] - b).abs() / torch.maximum(b.abs(), prev[name].abs()).clamp_min(1e-300)).max())
        assert rel('p', q.detach()) <= 1e-12 and rel('square_avg', st['square_avg']) <= 1e-12
        if mom > 0:
            assert rel('momentum_buffer', st['momentum_buffer']) <= 1e-12
        if centered:
            assert rel('grad_avg', st['grad_avg']) <= 1e-12


@pytest.mark.parametrize('factor', (0.5, 2.0))
def test_the_clip_reference_is_torch_clip_grad_norm(factor):
    g = X.make_inputs(100003, 51, 1.0, True)[1]
    q = torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64))
    q.grad = t(g).double()
    total = float(q.grad.norm())
    max_norm = X._f32(factor * total)
    norm, bound, c = Y.norm_reference(t(g), 1.0, max_norm, total)
    got = torch.nn.utils.clip_grad_norm_([q], max_norm)
    assert abs(float(got) - norm) <= 1e-12 * norm and bound == 2 * Y.U * norm
    coef = min(1.0, float(c.v))
    assert float(((q.grad - t(g).double() * coef).abs() / (t(g).double().abs() * coef).clamp_min(1e-300)).max()) <= 1e-12
    # the check itself: the fp32 evaluation of the coefficient from the fp32 norm passes; a norm 1e-5 off does not, nor does a
    # coefficient 1e-5 off the one that follows from the norm beside it
    n32 = f(total)
    c32 = min(f(1), f(max_norm) / (n32 + f(1e-6)))
    rn, rc = Y.check_norm(t(g), 1.0, max_norm, torch.tensor([n32, c32]))
    assert rn <= 1.0 and rc <= 1.0, (rn, rc)
    assert (c32 == 1.0) == (factor > 1)
    rn, rc = Y.check_norm(t(g), 1.0, max_norm, torch.tensor([n32 * f(1 + 1e-5), c32 * f(1 + 1e-5)]))
    assert rn > 1.0 and rc > 1.0, (rn, rc)


@pytest.mark.parametrize('gscale', X.GSCALES)
@pytest.mark.parametrize('zero', (True, False))
def test_three_steps_keep_the_centered_variance_positive(gscale, zero):
    state, _ = _inputs(gscale, zero, seed=11)
    for k in range(3):
        g = X.make_inputs(N, 60 + k, gscale, True)[1]
        out = _step(state, g, gscale, COEF, Y.MOM, Y.WD, True)
        r, reach = _check(state, g, out, gscale, COEF, Y.MOM, Y.WD, True)
        assert reach == 0 and all(x <= 1.0 for x in r.values()), (k, reach, r)
        var = out['square_avg'].astype(np.float64) - out['grad_avg'].astype(np.float64) ** 2
        assert (var[out['square_avg'] > 0] > 0).all()
        state = dict(state, **out)


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


def _host_optimizer(monkeypatch, **kw):
    import types
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.utils import optim
    rec = _Recorder()
    for mod in (optim, _lib):
        monkeypatch.setattr(mod, 'lib', lambda: rec)
    monkeypatch.setattr(optim, 'ptr', lambda x: x)
    monkeypatch.setattr(optim, 'stream', lambda: 12345)
    table = [('a.weight', (2, 3), 0, 6, 0), ('a.bias', (3,), 8, 3, 0)]
    net = types.SimpleNamespace(flat_params=torch.zeros(12), flat_grads=torch.ones(12), _table=table, _last_B=1, default_batch=1,
                                _ensure_table=lambda: None, weights_changed=lambda: None, _net=lambda B: None)
    return optim.RMSprop(net, **kw), rec, net


def test_default_step_is_the_one_plain_call(monkeypatch):
    o, rec, net = _host_optimizer(monkeypatch)
    o.step()
    assert [n for n, _ in rec.log] == ['pa_rmsprop_step_state']
    assert o.momentum_buffer is None and o.grad_avg is None and o._norm_out is None and o.last_grad_norm() is None
    assert sorted(o.state_dict()['state'][0]) == ['square_avg', 'step']


def test_options_go_through_the_norm_then_the_opts_step(monkeypatch):
    o, rec, net = _host_optimizer(monkeypatch, momentum=0.9, centered=True, max_grad_norm=2.0)
    o.step()
    o.param_groups[0]['weight_decay'] = 1e-4          # read at every step, like lr
    o.step()
    assert [n for n, _ in rec.log] == ['pa_grad_norm', 'pa_rmsprop_step_opts'] * 2
    (_, norm_args), (_, step_args) = rec.log[2], rec.log[3]
    assert norm_args[0] is net.flat_grads and norm_args[1] == 12 and norm_args[3] == 2.0 and norm_args[5] is o._norm_out
    opts = step_args[0]._obj
    assert (round(opts.momentum, 6), round(opts.weight_decay, 9), opts.centered) == (0.9, 1e-4, 1)
    assert step_args[4] is o.momentum_buffer and step_args[5] is o.grad_avg and step_args[6] == 12
    assert step_args[8].data_ptr() == o._norm_out.data_ptr() + 4 and step_args[9] is o._skip_state
    assert sorted(o.state_dict()['state'][1]) == ['grad_avg', 'momentum_buffer', 'square_avg', 'step']
    # weight decay alone: no norm launch, no momentum_buf / grad_avg pointer
    o2, rec2, _ = _host_optimizer(monkeypatch, weight_decay=1e-4)
    o2.step()
    assert [n for n, _ in rec2.log] == ['pa_rmsprop_step_opts'] and rec2.log[0][1][4] is None and rec2.log[0][1][5] is None and rec2.log[0][1][8] is None


def test_the_command_line_options_reach_the_optimizer(tmp_path):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils.optim import optim_options
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e']
    assert optim_options(TrainOptions().parse(base)) == dict(momentum=0.0, weight_decay=0.0, centered=False, max_grad_norm=None)
    opt = TrainOptions().parse(base + ['--momentum', '0.9', '--weight_decay', '1e-4', '--centered', '1', '--clip_grad_norm', '10'])
    assert optim_options(opt) == dict(momentum=0.9, weight_decay=1e-4, centered=True, max_grad_norm=10.0)

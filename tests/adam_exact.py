"""Exact check of the fused Adam / AdamW step (adam_prologue_kernel and adam_kernel, csrc/elementwise.hip; pa_adam_step): every element of
p, exp_avg, exp_avg_sq and max_exp_avg_sq after a step, against a float64 evaluation of

    gr  = (g s) coef                                (the product with coef only with a clip pointer)
    coupled decay:    gr = gr + wd32 p              decoupled decay:  p = p c_dec,  c_dec = (float)(1.0 - (double)lr32 (double)wd32)
    m'  = m + (gr - m) (1.f - beta1_32)
    v'  = beta2_32 v + ((1.f - beta2_32) gr) gr
    vmax' = max(vmax, v')                           amsgrad; vhat = amsgrad ? vmax' : v'
    den = sqrt(vhat) / bc2s + eps32,   p' = p - step_size (m' / den)

from the (p, g, m, v, vmax) the engine itself held before that step, with the engine's own fp32 constants and the engine's own coef
(out2[1] of pa_grad_norm), bc2s and step_size (read from its pa_adam_state): every step is a local check.  The formula is torch 2.10's
_single_tensor_adam, non-capturable branch (tests/test_adam_cpu.py compares five float64 steps with torch.optim.Adam / AdamW).

Bound.  Class E of tests/bn_exact.py as in tests/optim_exact.py: every fp32 operation above charged on its own (which admits any FMA
contraction), sqrtf within 2u over the exact interval of its argument, both divisions correctly rounded.  fmaxf is exact: the maximum
of an exact vmax and a v' known to within e is known to within e, and exactly where vmax lies above the whole interval of v'.

The four constants of the state are checked on their own (check_consts): bc1 = (float)(1 - beta1_32^t) and bc2 within 2u relative of the
float64 value (pow in double and one rounding to fp32 is u; the second u is slack for the device's double pow); bc2s as one sqrtf
(E.sqrt) and step_size as one division (E.div) on the engine's own bc2 and bc1.

tests/test_gpu_adam.py runs the cases below; the IEEE-half build (whose step first scans the gradient for inf / NaN, and whose prologue
then counts a skipped step instead of advancing the step count) runs this file as a child process, one storage type per process."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.bn_exact import E, U, _ratio
from tests import optim_exact as X
from tests.optim_exact import DOMAIN, Guarded, make_inputs, _f32, _t

LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8
# (weight_decay, decoupled): none, coupled, decoupled
DECAYS = ((0.0, False), (1e-4, False), (1e-2, True))
COMBOS = tuple(itertools.product(DECAYS, (False, True)))          # ((wd, decoupled), amsgrad)
GSCALES = (1.0, 1.0 / 3.0, 1.0 / 32768.0)
OUTPUTS = ('p', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def c_dec(lr, wd):
    """the factor of the decoupled decay as the C ABI forms it"""
    return _f32(1.0 - _f32(lr) * _f32(wd))


def one_minus(beta):
    return float(np.float32(1.0) - np.float32(beta))


def host_consts(t, beta1=BETA1, beta2=BETA2):
    """float64 {bc1, bc2} at step t from the fp32 betas the engine receives"""
    return {'bc1': 1.0 - _f32(beta1) ** t, 'bc2': 1.0 - _f32(beta2) ** t}


def reference(p, g, m, v, vmax, gscale, coef, bc2s, step_size, wd=0.0, decoupled=False, amsgrad=False, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """({name: E term} for p', m', v' and vmax' (amsgrad), (elements where v' took the max, elements where vmax kept it)) from float64
    tensors that hold fp32 values; coef: None or the float the engine wrote; bc2s, step_size: the floats the engine wrote."""
    gr = E(g) * E(_f32(gscale))
    if coef is not None:
        gr = gr * E(float(coef))
    P = E(p)
    if wd != 0:
        if decoupled:
            P = P * E(c_dec(lr, wd))
        else:
            gr = gr + E(_f32(wd)) * P
    m1 = E(m) + (gr - E(m)) * E(one_minus(beta1))
    v1 = E(_f32(beta2)) * E(v) + (E(one_minus(beta2)) * gr) * gr
    out, branches = {'exp_avg': m1, 'exp_avg_sq': v1}, (0, 0)
    vhat = v1
    if amsgrad:
        keep = vmax >= v1.v + v1.e                         # vmax lies above the whole interval of v': the result is vmax itself
        vhat = E(torch.maximum(vmax, v1.v), torch.where(keep, torch.zeros_like(v1.e), v1.e))
        out['max_exp_avg_sq'] = vhat
        branches = (int((v1.v > vmax).sum()), int((vmax > v1.v).sum()))
    den = vhat.sqrt().div(E(float(bc2s))) + E(_f32(eps))
    out['p'] = P - E(float(step_size)) * m1.div(den)
    return out, branches


def check(before, g, after, gscale, coef, consts, wd=0.0, decoupled=False, amsgrad=False, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """before / after: {name: tensor} of the four arrays (max_exp_avg_sq None without amsgrad); consts: the engine's {bc2s, step_size}.
    Returns ({name: worst error / bound, NaN if the step produced one}, the branch counts of `reference`)."""
    d = lambda t: None if t is None else t.double()
    ref, branches = reference(d(before['p']), g.double(), d(before['exp_avg']), d(before['exp_avg_sq']), d(before['max_exp_avg_sq']),
                              gscale, coef, consts['bc2s'], consts['step_size'], wd, decoupled, amsgrad, lr, beta1, beta2, eps)
    return dict((k, _ratio(after[k], r.v, r.e)) for k, r in ref.items()), branches


def check_consts(c, t, lr=LR, beta1=BETA1, beta2=BETA2):
    """c: the engine's {step, bc1, bc2, step_size, bc2s}.  Returns {name: error / bound}; step must equal t (inf otherwise)."""
    ref = host_consts(t, beta1, beta2)
    r = {'step': 0.0 if c['step'] == t else float('inf')}
    for k in ('bc1', 'bc2'):
        r[k] = abs(c[k] - ref[k]) / (2 * U * ref[k])
    s = E(c['bc2']).sqrt()
    r['bc2s'] = abs(c['bc2s'] - float(s.v)) / max(float(s.e), 1e-300)
    q = E(_f32(lr)).div(E(c['bc1']))
    r['step_size'] = abs(c['step_size'] - float(q.v)) / max(float(q.e), 1e-300)
    for k in r:
        if not r[k] == r[k]:
            r[k] = float('nan')
    return r


def make_state(n, seed, v, zero):
    """numpy fp32 (m0, vmax0): zeros, or m0 log-uniform in 1e-6 .. 1e3 with random signs (optim_opts_exact.make_state's buf) and
    vmax0 = v0 * U(1, 4), so that the maximum is kept at some elements and replaced at others (where v0 = 0, vmax0 = 0)."""
    if zero:
        return np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    r = np.random.Generator(np.random.PCG64([seed, n, 78]))
    m = (10.0 ** r.uniform(-6, 3, n) * np.where(r.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    vmax = (v.astype(np.float64) * r.uniform(1.0, 4.0, n)).astype(np.float32)
    return m, vmax


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU cases
def _opts(wd, decoupled, amsgrad, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    from pose_adv_aug_amd._lib import AdamOpts
    return AdamOpts(lr, beta1, beta2, eps, wd, int(amsgrad), int(decoupled))


def read_state(state):
    """the engine's pa_adam_state (an 8-element int32 device tensor) as a dict"""
    h = state.cpu()
    f = h.view(torch.float32)
    return {'flag': int(h[0]), 'skipped': int(h[1]), 'step': int(h[2]), 'bc1': float(f[4]), 'bc2': float(f[5]), 'step_size': float(f[6]),
            'bc2s': float(f[7])}


class AdamStepper(object):
    """one optimizer state (p, m, v, vmax, its pa_adam_state) behind pa_adam_step; vmax exists only with amsgrad"""
    def __init__(self, wd, decoupled, amsgrad, p, m, v, vmax):
        from pose_adv_aug_amd._lib import lib
        self.L, self.wd, self.decoupled, self.amsgrad = lib(), wd, decoupled, amsgrad
        self.a = {'p': Guarded(p, 3.0), 'exp_avg': Guarded(m, 5.0), 'exp_avg_sq': Guarded(v, 7.0),
                  'max_exp_avg_sq': Guarded(vmax, 9.0) if amsgrad else None}
        self.state = torch.zeros(8, dtype=torch.int32, device='cuda')

    def arrays(self):
        return dict((k, None if a is None else a.x.clone()) for k, a in self.a.items())

    def step(self, g, gscale, coef=None):
        """g: a Guarded gradient; coef: None or a 1-element device tensor"""
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        x = lambda k: None if self.a[k] is None else ptr(self.a[k].x)
        o = _opts(self.wd, self.decoupled, self.amsgrad)
        ok(self.L.pa_adam_step(C.byref(o), x('p'), ptr(g.x), x('exp_avg'), x('exp_avg_sq'), x('max_exp_avg_sq'), g.x.numel(), float(gscale),
                               None if coef is None else ptr(coef), ptr(self.state), stream()), 'pa_adam_step')

    def counts(self):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        s, k = C.c_longlong(-1), C.c_longlong(-1)
        ok(self.L.pa_adam_steps(ptr(self.state), C.byref(s), C.byref(k), stream()), 'pa_adam_steps')
        return int(s.value), int(k.value)

    def set_steps(self, steps):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        ok(self.L.pa_adam_set_steps(ptr(self.state), steps, stream()), 'pa_adam_set_steps')

    def guards_intact(self):
        return all(a.guards_intact() for a in self.a.values() if a is not None)


def grad_norm(g, n, gscale, max_norm):
    from tests.optim_opts_exact import grad_norm as norm
    return norm(g, n, gscale, max_norm)


def run_case(n, log=print, steps=3):
    """Every decay mode x amsgrad, with and without a clip coefficient (pa_grad_norm with max_norm = half the norm), every gscale, from
    zero state and from non-zero state: `steps` consecutive steps with fresh gradients, each checked from the engine's own state
    before it; all outputs within the bound, state.step == k and the constants within their bounds at t = k, guards bit-identical,
    the skip counter unmoved; from non-zero state both branches of the maximum occur (n >= 1023).  Returns the failures [(what, figure)]."""
    fails = []
    worst = dict((k, 0.0) for k in OUTPUTS)
    for gi, gscale in enumerate(GSCALES):
        grads = []
        for k in range(steps):
            G = Guarded(_t(make_inputs(n, 3000 + 10 * gi + k, gscale, True)[1]), float('nan'))
            norm = float(((G.x.double() * _f32(gscale)) ** 2).sum().sqrt())
            grads.append((G, grad_norm(G.x, n, gscale, 0.5 * norm if norm > 0 else 1.0)))
        for zero in (True, False):
            p, _, v = make_inputs(n, 2900 + gi, gscale, zero)
            m, vmax = make_state(n, 2900 + gi, v, zero)
            p, v, m, vmax = _t(p), _t(v), _t(m), _t(vmax)
            for ((wd, decoupled), amsgrad), clip in itertools.product(COMBOS, (False, True)):
                S = AdamStepper(wd, decoupled, amsgrad, p, m, v, vmax)
                what0 = 'n %d wd %g decoupled %d amsgrad %d clip %d gscale %g state %s' % (n, wd, decoupled, amsgrad, clip, gscale, 'zero' if zero else 'nonzero')
                for k, (G, out2) in enumerate(grads):
                    before = S.arrays()
                    S.step(G, gscale, out2[1:] if clip else None)
                    torch.cuda.synchronize()
                    c = read_state(S.state)
                    for name, x in check_consts(c, k + 1).items():
                        if not (x <= 1.0):
                            fails.append(('%s of the state %s step %d' % (name, what0, k), x))
                    r, (took, kept) = check(before, G.x, S.arrays(), gscale, float(out2[1]) if clip else None, c, wd, decoupled, amsgrad)
                    for name, x in r.items():
                        worst[name] = max(worst[name], x) if x == x else x
                        if not (x <= 1.0):
                            fails.append(('%s %s step %d' % (name, what0, k), x))
                    if amsgrad and not zero and k == 0 and n >= 1023 and not (took > 0 and kept > 0):
                        fails.append(('one branch of the maximum never occurred ' + what0, (took, kept)))
                    if not (S.guards_intact() and G.guards_intact()):
                        fails.append(('guard elements changed %s step %d' % (what0, k), 0))
                if S.counts() != (steps, 0):
                    fails.append(('step / skip counters after finite gradients ' + what0, S.counts()))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('adam_exact n %d: worst error / bound %s' % (n, ', '.join('%s %.3g' % (k, worst[k]) for k in OUTPUTS)))
    return fails


def run_set_steps():
    """from pa_adam_set_steps(1000) the next step uses the constants of t = 1001 (bc1 exactly 1 with beta1 = 0.9) and is within the bound"""
    n, gscale = 1023, 1.0
    fails = []
    p, g, v = make_inputs(n, 3100, gscale, False)
    m, vmax = make_state(n, 3100, v, False)
    S = AdamStepper(1e-4, False, True, _t(p), _t(m), _t(v), _t(vmax))
    G = Guarded(_t(g), float('nan'))
    S.set_steps(1000)
    torch.cuda.synchronize()
    if S.counts() != (1000, 0):
        fails.append(('counts after pa_adam_set_steps(1000)', S.counts()))
    before = S.arrays()
    S.step(G, gscale)
    torch.cuda.synchronize()
    c = read_state(S.state)
    rc = check_consts(c, 1001)
    if not all(x <= 1.0 for x in rc.values()):
        fails.append(('constants at t = 1001', rc))
    if c['bc1'] != 1.0 or c['step_size'] != _f32(LR):
        fails.append(('bc1 / step_size at t = 1001', (c['bc1'], c['step_size'])))
    if all(x <= 1.0 for x in check_consts(c, 1).values()):
        fails.append(('the constants of t = 1 pass as well: the check says nothing', c))
    r, _ = check(before, G.x, S.arrays(), gscale, None, c, 1e-4, False, True)
    if not all(x <= 1.0 for x in r.values()):
        fails.append(('the step from t = 1000', r))
    if not S.guards_intact():
        fails.append(('guard elements changed', 0))
    return fails


def run_error_cases():
    """every listed argument error: non-zero, a message, nothing written"""
    from pose_adv_aug_amd._lib import lib, ptr, stream
    L = lib()
    n = 1023
    p, g, v = make_inputs(n, 3200, 1.0, False)
    m, vmax = make_state(n, 3200, v, False)
    state = torch.zeros(12, dtype=torch.int32, device='cuda')          # [0:8] aligned, [1:9] not 16-byte aligned
    state[:] = torch.arange(12, dtype=torch.int32)
    arrays = dict(p=_t(p), g=_t(g), m=_t(m), v=_t(v), vmax=_t(vmax), state=state)
    keep = dict((k, a.clone()) for k, a in arrays.items())
    a = dict((k, ptr(t)) for k, t in arrays.items())
    odd = ptr(state[1:9])
    fails = []

    def step(what, o, p_, g_, m_, v_, x_, s_):
        rc = L.pa_adam_step(None if o is None else C.byref(o), p_, g_, m_, v_, x_, n, 1.0, None, s_, stream())
        if rc == 0 or not L.pa_last_error():
            fails.append(('pa_adam_step accepted ' + what, rc))

    full, plain = _opts(1e-4, False, True), _opts(1e-4, False, False)
    step('NULL opts', None, a['p'], a['g'], a['m'], a['v'], a['vmax'], a['state'])
    step('NULL param', full, None, a['g'], a['m'], a['v'], a['vmax'], a['state'])
    step('NULL grad', full, a['p'], None, a['m'], a['v'], a['vmax'], a['state'])
    step('NULL exp_avg', full, a['p'], a['g'], None, a['v'], a['vmax'], a['state'])
    step('NULL exp_avg_sq', full, a['p'], a['g'], a['m'], None, a['vmax'], a['state'])
    step('NULL state', full, a['p'], a['g'], a['m'], a['v'], a['vmax'], None)
    step('a missing max_exp_avg_sq', full, a['p'], a['g'], a['m'], a['v'], None, a['state'])
    step('a superfluous max_exp_avg_sq', plain, a['p'], a['g'], a['m'], a['v'], a['vmax'], a['state'])
    for what, kw in (('beta1 < 0', dict(beta1=-0.1)), ('beta1 = 1', dict(beta1=1.0)), ('beta2 < 0', dict(beta2=-0.1)), ('beta2 = 1', dict(beta2=1.0)),
                     ('beta1 NaN', dict(beta1=float('nan'))), ('eps 0', dict(eps=0.0)), ('eps < 0', dict(eps=-1e-8))):
        step(what, _opts(1e-4, False, True, **kw), a['p'], a['g'], a['m'], a['v'], a['vmax'], a['state'])
    step('weight_decay < 0', _opts(-1e-4, False, True), a['p'], a['g'], a['m'], a['v'], a['vmax'], a['state'])
    step('a misaligned state', full, a['p'], a['g'], a['m'], a['v'], a['vmax'], odd)
    s, k = C.c_longlong(-7), C.c_longlong(-7)
    for what, rc in (('pa_adam_steps accepted a NULL state', L.pa_adam_steps(None, C.byref(s), C.byref(k), stream())),
                     ('pa_adam_steps accepted a misaligned state', L.pa_adam_steps(odd, C.byref(s), C.byref(k), stream())),
                     ('pa_adam_set_steps accepted a NULL state', L.pa_adam_set_steps(None, 3, stream())),
                     ('pa_adam_set_steps accepted a misaligned state', L.pa_adam_set_steps(odd, 3, stream())),
                     ('pa_adam_set_steps accepted steps < 0', L.pa_adam_set_steps(a['state'], -1, stream()))):
        if rc == 0 or not L.pa_last_error():
            fails.append((what, rc))
    if (s.value, k.value) != (-7, -7):
        fails.append(('a refused pa_adam_steps wrote its outputs', (s.value, k.value)))
    torch.cuda.synchronize()
    for k_, t in arrays.items():
        if not torch.equal(t.view(torch.int32), keep[k_].view(torch.int32)):
            fails.append(('a refused call changed ' + k_, 0))
    return fails


def _check_flat(module, make_opt, what, fails, log):
    """make_opt(module, max_grad_norm) -> an utils.optim.Adam on the whole flat array, over two steps: every element in the bound's
    domain within the bound, at least 90 % of the real gradient in the domain, last_grad_norm() against float64, the padding exactly 0
    before and after in all arrays.  Returns the number of padding elements."""
    from pose_adv_aug_amd._lib import grad_scale
    from tests.optim_opts_exact import check_norm
    n = module.flat_params.numel()
    used = torch.zeros(n, dtype=torch.bool, device='cuda')
    for _, _, off, numel, kind in module._table:
        if kind == 0:
            used[off:off + numel] = True
    pad = ~used
    gscale = 1.0 / grad_scale()
    norm = float(((module.flat_grads.double() * _f32(gscale)) ** 2).sum().sqrt())
    opt = make_opt(module, 0.5 * norm)
    g0 = opt.param_groups[0]
    lr, (b1, b2), eps, wd, dec, ams = g0['lr'], g0['betas'], g0['eps'], g0['weight_decay'], g0['decoupled_weight_decay'], g0['amsgrad']
    moments = lambda: {'exp_avg': opt.exp_avg, 'exp_avg_sq': opt.exp_avg_sq, 'max_exp_avg_sq': opt.max_exp_avg_sq if ams else None}
    every = lambda: [('p', module.flat_params), ('g', module.flat_grads)] + [(k, a) for k, a in moments().items() if a is not None]
    if ams != (opt.max_exp_avg_sq is not None):
        fails.append(('%s: max_exp_avg_sq allocated %s with amsgrad %s' % (what, opt.max_exp_avg_sq is not None, ams), 0))
    for name, a in every():
        if bool((a[pad] != 0).any()):
            fails.append(('%s: padding of %s not zero before the step' % (what, name), float(a[pad].abs().max())))
    worst = dict((k, 0.0) for k in OUTPUTS)
    for k in range(2):
        g = module.flat_grads.clone()
        before = dict((key, None if a is None else a.clone()) for key, a in moments().items())
        before['p'] = module.flat_params.clone()
        opt.step()
        torch.cuda.synchronize()
        out2 = opt._norm_out.clone()
        c = read_state(opt._state)
        rc = check_consts(c, k + 1, lr, b1, b2)
        if not all(x <= 1.0 for x in rc.values()):
            fails.append(('%s: constants of step %d' % (what, k), rc))
        rn, rcoef = check_norm(g, gscale, 0.5 * norm, out2)
        if not (rn <= 1.0 and rcoef <= 1.0 and float(out2[1]) < 1.0):
            fails.append(('%s: norm / coefficient of step %d' % (what, k), (rn, rcoef, float(out2[1]))))
        if abs(float(opt.last_grad_norm()) - norm) > 2 * U * norm:
            fails.append(('%s: last_grad_norm() of step %d' % (what, k), float(opt.last_grad_norm())))
        # the bound's domain: g s, and the gradient the moments see (gr = g s coef, + wd p when coupled), are 0 or at least DOMAIN
        gr = g.double() * _f32(gscale) * float(out2[1])
        if wd != 0 and not dec:
            gr = gr + _f32(wd) * before['p'].double()
        dom = ((gr == 0) | (gr.abs() >= DOMAIN)) & ((g == 0) | ((g.double() * _f32(gscale)).abs() >= DOMAIN))
        if float(dom.float().mean()) < 0.9:
            fails.append(('%s: less than 90 %% of the real gradient is in the bound\'s domain' % what, float(dom.float().mean())))
        if not bool((g != 0).any()):
            fails.append(('%s: the gradient is all zero, no backward pass reached it' % what, 0))
        after = dict(moments(), p=module.flat_params)
        sel = lambda d: dict((key, None if a is None else a[dom]) for key, a in d.items())
        r, _ = check(sel(before), g[dom], sel(after), gscale, float(out2[1]), c, wd, dec, ams, lr, b1, b2, eps)
        for name, x in r.items():
            worst[name] = max(worst[name], x) if x == x else x
            if not (x <= 1.0):
                fails.append(('%s of the flat array of %s, step %d' % (name, what, k), x))
        for name, a in every():
            if not bool(torch.isfinite(a).all()):
                fails.append(('non-finite value in %s of %s after step %d' % (name, what, k), 0))
            if bool((a[pad] != 0).any()):
                fails.append(('%s: padding of %s not zero after step %d' % (what, name, k), float(a[pad].abs().max())))
    if opt.steps_taken() != 2 or opt.skipped_steps() != 0:
        fails.append(('%s: steps taken / skipped after two steps' % what, (opt.steps_taken(), opt.skipped_steps())))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('adam_exact flat array of %s n %d (%d padding elements): worst error / bound %s'
            % (what, n, int(pad.sum()), ', '.join('%s %.3g' % (k, worst[k]) for k in OUTPUTS)))
    return int(pad.sum())


def run_flat_array(log=print):
    """Adam(amsgrad, weight_decay 1e-4, max_grad_norm = half the norm) and AdamW(max_grad_norm likewise) on the real flat arrays of the
    2-stack chan-128 pose net (B 2) and its agent (optim_opts_exact.flat_nets, built once)"""
    from pose_adv_aug_amd.utils.optim import Adam, AdamW
    from tests.optim_opts_exact import flat_nets
    fails = []
    net, agent = flat_nets()
    pads = 0
    for cls, make in (('Adam', lambda mod, mx: Adam(mod, amsgrad=True, weight_decay=1e-4, max_grad_norm=mx)),
                      ('AdamW', lambda mod, mx: AdamW(mod, max_grad_norm=mx))):
        pads += _check_flat(net, make, '%s on the pose net' % cls, fails, log)
        pads += _check_flat(agent, make, '%s on the agent' % cls, fails, log)
    if pads == 0:
        fails.append(('neither flat array has alignment padding: nothing was tested', 0))
    return fails


def run_skip_case(log=print):
    """fp16 build, amsgrad, coupled decay and the clip coefficient on.  For inf / NaN / -inf at each of optim_exact.SKIP_POSITIONS: every
    array bit-unchanged, skipped + 1, step and the four constants unchanged after the poisoned step; the next finite step within the
    bound with the constants of t + 1 (a host-side step counter would make them those of t + 2)."""
    n, gscale = X.SKIP_N, 1.0 / 32768.0
    wd, decoupled, amsgrad = 1e-4, False, True
    fails = []
    p, g, v = make_inputs(n, 3300, gscale, False)
    m, vmax = make_state(n, 3300, v, False)
    S = AdamStepper(wd, decoupled, amsgrad, _t(p), _t(m), _t(v), _t(vmax))
    G = Guarded(_t(g), float('nan'))
    norm = float(((G.x.double() * _f32(gscale)) ** 2).sum().sqrt())
    out2 = grad_norm(G.x, n, gscale, 0.5 * norm)
    S.step(G, gscale, out2[1:])                     # one taken step first: the constants of t = 1 are in the state
    torch.cuda.synchronize()
    bits = lambda d: dict((k, a.view(torch.int32)) for k, a in d.items())
    for where, pos in X.SKIP_POSITIONS:
        for bad in (float('inf'), float('nan'), float('-inf')):
            what = '%s at %s' % (bad, where)
            Gb = Guarded(G.x, float('nan'))
            Gb.x[pos] = bad
            before, (t0, k0), s0 = S.arrays(), S.counts(), S.state.clone()
            S.step(Gb, gscale, out2[1:])
            torch.cuda.synchronize()
            a, b = bits(S.arrays()), bits(before)
            changed = sum(int((a[k] != b[k]).sum()) for k in a)
            if changed:
                fails.append(('an array changed on a skipped step: ' + what, changed))
            if S.counts() != (t0, k0 + 1):
                fails.append(('counts after a skipped step (were %s): %s' % ((t0, k0), what), S.counts()))
            if not torch.equal(S.state[2:], s0[2:]):
                fails.append(('step or a constant changed on a skipped step: ' + what, 0))
            S.step(G, gscale, out2[1:])
            torch.cuda.synchronize()
            c = read_state(S.state)
            rc = check_consts(c, t0 + 1)
            if not all(x <= 1.0 for x in rc.values()):
                fails.append(('constants of the next finite step (t = %d): %s' % (t0 + 1, what), rc))
            r, _ = check(before, G.x, S.arrays(), gscale, float(out2[1]), c, wd, decoupled, amsgrad)
            if not all(x <= 1.0 for x in r.values()):
                fails.append(('the next finite step: ' + what, r))
            if S.counts() != (t0 + 1, k0 + 1):
                fails.append(('counts after the next finite step: ' + what, S.counts()))
            if not S.guards_intact():
                fails.append(('guard elements changed: ' + what, 0))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('adam_exact skip: %d positions x 3 values, %d failures' % (len(X.SKIP_POSITIONS), len(fails)))
    return fails


if __name__ == '__main__':          # the fp16 build: tests/test_gpu_adam.py runs this with POSEADV_DTYPE=fp16
    from pose_adv_aug_amd._lib import lib as _l
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    torch.cuda.set_device(0)
    out = lambda s: print(s, flush=True)
    fails = []
    for n in X.SIZES:
        fails += run_case(n, log=out)
    fails += run_set_steps()
    fails += run_error_cases()
    fails += run_skip_case(log=out)
    fails += run_flat_array(log=out)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 ADAM EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)

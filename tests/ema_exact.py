"""Exact check of the weight EMA (ema_advance_kernel and ema_lerp_kernel, csrc/ema.hip; pa_ema_advance, pa_ema_lerp, pa_ema_counts,
pa_ema_set_updates; utils.optim.ModelEma): every element of the average after an update, against the float64 value of

    ref = e + w (p - e)

from the (e, p) the engine itself held before that update and the fp32 w the engine itself wrote into its state; over several updates
the reference restarts from the engine's previous average, so every update is a local check and bounds do not accumulate.

Bound, counted from the kernel's two operations, u = 2^-24:  dh = fl(p - e) = (p - e)(1 + a), |a| <= u (a difference of two fp32
numbers does not underflow: it is exact where it is subnormal);  e' = fl(fma(w, dh, e)) = (e + w dh)(1 + b) + c, |b| <= u, |c| <= 2^-150
where the result is subnormal.  So e' - ref = w (p - e) a (1 + b) + ref b + c, and

    |e' - ref| <= 2^-24 (|w (p - e)| + |ref|) (1 + 2^-23) + 2^-149.

Every element is reported as a ratio to that bound and must be <= 1.  copy = 1, a held step and p == e are checked bit for bit.

The state is checked exactly: w against float32(1.0 - d) with d = warmup ? min(decay32, (1 + updates) / (10 + updates)) : decay32 formed
in double on the host (decay32: the fp32 value the C ABI receives; IEEE double division, one rounding to fp32: no tolerance), decay_used
against float32(d), the counts and `apply` as integers.

tests/test_ema_cpu.py checks the reference, the bound and the state model on numpy alone and shows which defects they exclude;
tests/test_gpu_ema.py runs the cases below; the IEEE-half build (whose optimizers skip a step whose gradient holds inf / NaN: the
average must stay, and its count with it) runs this file as a child process, one storage type per process."""
import ctypes as C
import os
import sys

import numpy as np

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U = 2.0 ** -24
DECAYS = (0.0, 0.5, 0.999, 0.9999)


def _f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------------
# host model: numpy or torch arrays alike (operators and abs() only)
def host_decay(decay, warmup, updates):
    """the d of an update that starts at count `updates`, in double, from the fp32 decay the engine receives"""
    d = _f32(decay)
    return min(d, (1.0 + updates) / (10.0 + updates)) if warmup else d


def host_w(decay, warmup, updates):
    return _f32(1.0 - host_decay(decay, warmup, updates))


def expected_state(s0, decay, warmup, flag):
    """the state after pa_ema_advance from the state dict s0 (updates, held, apply, w, decay_used); flag: the optimizer's word, None = no pointer"""
    s = dict(s0)
    if flag:
        s['apply'], s['held'] = 0, s0['held'] + 1
        return s
    d = host_decay(decay, warmup, s0['updates'])
    s.update(w=_f32(1.0 - d), decay_used=_f32(d), apply=1, updates=s0['updates'] + 1)
    return s


def check_state(s0, s1, decay, warmup, flag):
    """the words of s1 that differ from expected_state(s0, ...): [] when the engine's state is exactly the model's"""
    want = expected_state(s0, decay, warmup, flag)
    return [(k, s1[k], want[k]) for k in ('updates', 'held', 'apply', 'w', 'decay_used') if not s1[k] == want[k]]


def reference(e, p, w):
    """(ref, bound) in float64 from float64 arrays that hold fp32 values and the engine's fp32 w"""
    step = w * (p - e)
    ref = e + step
    return ref, U * (abs(step) + abs(ref)) * (1.0 + 2.0 ** -23) + 2.0 ** -149


def _wide(x):
    return x.double() if hasattr(x, 'double') else np.asarray(x, dtype=np.float64)


def _bits(x):
    if hasattr(x, 'double'):
        import torch
        return x.view(torch.int32)
    return np.asarray(x).view(np.int32)


def bits_differ(a, b):
    """number of elements whose bit patterns differ"""
    return int((_bits(a) != _bits(b)).sum())


def ratio(e1, e0, p, w):
    """worst |e1 - ref| / bound over the elements (fp32 arrays: the average after, before, the parameters); NaN if e1 holds one"""
    ref, bound = reference(_wide(e0), _wide(p), float(w))
    r = abs(_wide(e1) - ref) / bound
    if not bool((r == r).all()):
        return float('nan')
    n = r.numel() if hasattr(r, 'numel') else r.size
    return float(r.max()) if n else 0.0


def check_arrays(e0, p, e1, s1, copy=False):
    """one figure for an update whose state after the prologue is s1: elements that differ bit for bit where that is the claim (a held
    step: e1 == e0; copy: e1 == p), else the worst error / bound.  It passes when the figure is <= 1 (0 differing elements)."""
    if not s1['apply']:
        return float(bits_differ(e1, e0)) * 2.0
    if copy:
        return float(bits_differ(e1, p)) * 2.0
    return ratio(e1, e0, p, s1['w'])


def emulate(e, p, w):
    """the kernel on numpy fp32 arrays: fl(p - e), then the fused multiply-add formed in double (the product of two fp32 values is exact
    there) and rounded to fp32"""
    d = (p.astype(np.float32) - e.astype(np.float32)).astype(np.float32)
    return (np.float64(np.float32(w)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def make_inputs(n, seed):
    """numpy fp32 (e, p) of mixed magnitude: e log-uniform in 1e-6 .. 1e3 with random signs and 5 % exact zeros; p is e itself (10 %), e
    moved by a relative 1e-7 .. 1e-1 (40 %: the late phase of training, p - e far below e), an unrelated number of up to 1e6 times the
    magnitude (the rest).  Returns (e, p, the mask p == e)."""
    r = np.random.Generator(np.random.PCG64([seed, n, 5]))
    sign = lambda: np.where(r.random(n) < 0.5, -1.0, 1.0)
    e = 10.0 ** r.uniform(-6, 3, n) * sign()
    e[r.random(n) < 0.05] = 0.0
    e = e.astype(np.float32)
    kind = r.random(n)
    near = (e.astype(np.float64) * (1.0 + 10.0 ** r.uniform(-7, -1, n) * sign())).astype(np.float32)
    far = (10.0 ** r.uniform(-6, 6, n) * sign()).astype(np.float32)
    p = np.where(kind < 0.1, e, np.where(kind < 0.5, near, far)).astype(np.float32)
    return e, p, kind < 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU cases
def read_state(state):
    """the engine's pa_ema_state (an 8-element int32 device tensor) as a dict"""
    import torch
    h = state.cpu()
    f = h.view(torch.float32)
    return {'updates': int(h[0]), 'held': int(h[1]), 'apply': int(h[2]), 'reserved': int(h[3]), 'w': float(f[4]), 'decay_used': float(f[5])}


class Engine(object):
    """one average (e, its pa_ema_state) behind the four entry points; e sits between guard floats"""
    def __init__(self, e):
        import torch
        from pose_adv_aug_amd._lib import lib
        from tests.optim_exact import Guarded
        self.L = lib()
        self.e = Guarded(e, 3.0)
        self.state = torch.zeros(8, dtype=torch.int32, device='cuda')

    def advance(self, decay, warmup, flag=None):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        ok(self.L.pa_ema_advance(ptr(self.state), float(decay), int(warmup), None if flag is None else ptr(flag), stream()), 'pa_ema_advance')

    def lerp(self, p, copy=0):
        """p: a Guarded parameter array (its guards hold NaN)"""
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        ok(self.L.pa_ema_lerp(ptr(self.e.x), ptr(p.x), p.x.numel(), ptr(self.state), int(copy), stream()), 'pa_ema_lerp')

    def counts(self):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        u, h = C.c_longlong(-1), C.c_longlong(-1)
        ok(self.L.pa_ema_counts(ptr(self.state), C.byref(u), C.byref(h), stream()), 'pa_ema_counts')
        return int(u.value), int(h.value)

    def set_updates(self, updates):
        from pose_adv_aug_amd._lib import check as ok, ptr, stream
        ok(self.L.pa_ema_set_updates(ptr(self.state), int(updates), stream()), 'pa_ema_set_updates')


def _update(S, P, decay, warmup, what, fails, p_is_e=None, copy=0, flag=None, flag_value=0):
    """one advance + lerp of the engine S on the Guarded parameters P, checked from S's own state and average before it.
    Returns the figure of check_arrays."""
    import torch
    s0, e0 = read_state(S.state), S.e.x.clone()
    S.advance(decay, warmup, flag)
    S.lerp(P, copy)
    torch.cuda.synchronize()
    s1 = read_state(S.state)
    for word in check_state(s0, s1, decay, warmup, flag_value):
        fails.append(('state word (got, expected) ' + what, word))
    x = check_arrays(e0, P.x, S.e.x, s1, copy)
    if not (x <= 1.0):
        fails.append(('average ' + what, x))
    if p_is_e is not None and s1['apply'] and not copy and not bool((S.e.x[p_is_e] == e0[p_is_e]).all()):
        fails.append(('p == e did not give e ' + what, int((S.e.x[p_is_e] != e0[p_is_e]).sum())))
    if S.counts() != (s1['updates'], s1['held']):
        fails.append(('pa_ema_counts against the state ' + what, S.counts()))
    if not (S.e.guards_intact() and P.guards_intact()):
        fails.append(('guard elements changed ' + what, 0))
    return x


def run_case(n, log=print):
    """Every decay, warm-up off (two averaging updates with fresh parameters, then one with copy = 1) and on (five consecutive updates
    from count 0, then one from count 9 -> 10 through pa_ema_set_updates): every element within the bound, p == e gives e, the state exact,
    guards bit-identical.  Returns the failures [(what, figure)]."""
    import torch
    from tests.optim_exact import Guarded, _t
    fails, worst = [], 0.0
    e, p0, same = make_inputs(n, 4000)
    same = _t(same)
    fresh = [Guarded(_t(p0).roll(97 * k + 1), float('nan')) for k in range(4)]          # fresh parameters: the same values at other elements
    for decay in DECAYS:
        for warmup in (0, 1):
            S = Engine(_t(e))
            what0 = 'n %d decay %g warmup %d' % (n, decay, warmup)
            rounds = [(Guarded(_t(p0), float('nan')), same)] + [(P, None) for P in fresh[:4 if warmup else 1]]
            for k, (P, mask) in enumerate(rounds):
                x = _update(S, P, decay, warmup, '%s update %d' % (what0, k), fails, mask)
                worst = max(worst, x) if x == x else x
            if warmup:
                S.set_updates(9)
                torch.cuda.synchronize()
                if S.counts() != (9, 0):
                    fails.append(('counts after pa_ema_set_updates(9) ' + what0, S.counts()))
                _update(S, fresh[0], decay, warmup, what0 + ' update from count 9', fails)
                if S.counts() != (10, 0) or read_state(S.state)['w'] != _f32(1.0 - min(_f32(decay), 10.0 / 19.0)):
                    fails.append(('count / w after the update from count 9 ' + what0, (S.counts(), read_state(S.state)['w'])))
            else:
                _update(S, fresh[1], decay, warmup, what0 + ' copy', fails, copy=1)
                if S.counts() != (3, 0):
                    fails.append(('counts after three updates ' + what0, S.counts()))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('ema_exact n %d: worst error / bound %.3g' % (n, worst))
    return fails


HOLD_N = 100003


def run_hold_case(log=print):
    """With warm-up on (so that w depends on the count) and decay 0.999: two updates, then the flag word 1 -- every element and every
    state word but held and apply unchanged bit for bit, held + 1, for the averaging and the copying launch alike -- then flag 0: the w
    of the un-advanced count, and an update within the bound."""
    import torch
    from tests.optim_exact import Guarded, _t
    n, decay = HOLD_N, 0.999
    fails = []
    e, p, _ = make_inputs(n, 4100)
    S = Engine(_t(e))
    P = [Guarded(_t(p).roll(97 * k), float('nan')) for k in range(2)]
    flag = torch.zeros(2, dtype=torch.int32, device='cuda')
    for k in range(2):
        _update(S, P[k], decay, 1, 'hold case, update %d' % k, fails, flag=flag)
    for copy in (0, 1):
        flag[0] = 1
        s0, e0 = S.state.clone(), S.e.x.clone()
        x = _update(S, P[0], decay, 1, 'hold case, flag 1 copy %d' % copy, fails, copy=copy, flag=flag, flag_value=1)
        if x != 0.0:
            fails.append(('elements changed on a held step, copy %d' % copy, x / 2))
        keep = [0, 3, 4, 5, 6, 7]
        if not torch.equal(S.state[keep], s0[keep]) or int(S.state[1]) != int(s0[1]) + 1 or int(S.state[2]) != 0:
            fails.append(('state after a held step, copy %d' % copy, S.state.tolist()))
        flag[0] = 0
        _update(S, P[1], decay, 1, 'hold case, flag 0 after the hold, copy %d' % copy, fails, flag=flag)
        want_w = host_w(decay, 1, int(s0[0]))
        if read_state(S.state)['w'] != want_w or host_w(decay, 1, int(s0[0]) + 1) == want_w:
            fails.append(('w after the hold is not that of the un-advanced count (or the counts do not tell)', read_state(S.state)['w']))
    if S.counts() != (4, 2):
        fails.append(('counts of the hold case', S.counts()))
    return fails


def run_error_cases():
    """every listed refusal: non-zero, a message, outputs and state untouched; n == 0 returns 0 and does nothing"""
    import torch
    from pose_adv_aug_amd._lib import lib, ptr, stream
    from tests.optim_exact import _t
    L = lib()
    n = 1023
    e, p, _ = make_inputs(n, 4200)
    state = torch.arange(8, dtype=torch.int32, device='cuda')
    arrays = dict(e=_t(e), p=_t(p), state=state)
    keep = dict((k, a.clone()) for k, a in arrays.items())
    a = dict((k, ptr(t)) for k, t in arrays.items())
    fails = []
    u, h = C.c_longlong(-7), C.c_longlong(-7)
    calls = [('pa_ema_advance accepted a NULL state', lambda: L.pa_ema_advance(None, 0.9, 0, None, stream()))]
    for what, d in (('decay 1', 1.0), ('decay < 0', -0.1), ('decay > 1', 1.5), ('decay NaN', float('nan')), ('decay inf', float('inf'))):
        calls.append(('pa_ema_advance accepted ' + what, lambda d=d: L.pa_ema_advance(a['state'], d, 0, None, stream())))
    calls += [('pa_ema_lerp accepted a NULL ema', lambda: L.pa_ema_lerp(None, a['p'], n, a['state'], 0, stream())),
              ('pa_ema_lerp accepted a NULL src', lambda: L.pa_ema_lerp(a['e'], None, n, a['state'], 0, stream())),
              ('pa_ema_lerp accepted a NULL state', lambda: L.pa_ema_lerp(a['e'], a['p'], n, None, 0, stream())),
              ('pa_ema_lerp accepted ema == src', lambda: L.pa_ema_lerp(a['e'], a['e'], n, a['state'], 0, stream())),
              ('pa_ema_lerp accepted ema == src with copy', lambda: L.pa_ema_lerp(a['e'], a['e'], n, a['state'], 1, stream())),
              ('pa_ema_counts accepted a NULL state', lambda: L.pa_ema_counts(None, C.byref(u), C.byref(h), stream())),
              ('pa_ema_set_updates accepted a NULL state', lambda: L.pa_ema_set_updates(None, 3, stream())),
              ('pa_ema_set_updates accepted updates < 0', lambda: L.pa_ema_set_updates(a['state'], -1, stream()))]
    for what, call in calls:
        rc = call()
        if rc == 0 or not L.pa_last_error():
            fails.append((what, rc))
    if (u.value, h.value) != (-7, -7):
        fails.append(('a refused pa_ema_counts wrote its outputs', (u.value, h.value)))
    state[2] = 1                                    # apply: a launch would write
    keep['state'][2] = 1
    if L.pa_ema_lerp(a['e'], a['p'], 0, a['state'], 0, stream()) != 0:
        fails.append(('pa_ema_lerp with n == 0 did not return 0', L.pa_last_error()))
    torch.cuda.synchronize()
    for k_, t in arrays.items():
        if not torch.equal(t.view(torch.int32), keep[k_].view(torch.int32)):
            fails.append(('a refused call changed ' + k_, 0))
    return fails


def _pad_mask(module, kind):
    import torch
    flat = module.flat_params if kind == 0 else module.flat_buffers
    used = torch.zeros(flat.numel(), dtype=torch.bool, device='cuda')
    for _, _, off, numel, k in module._table:
        if k == kind:
            used[off:off + numel] = True
    return ~used


def _check_flat(module, make_opt, what, buffers, fails, log):
    """three optimizer.step() + ema.update() rounds of ModelEma(module, 0.999, warm-up, buffers): parameters and buffers of the twin
    checked from its own previous arrays, the padding of both exactly 0 before and after, the twin a bit-exact copy at the start, the
    counts 3 / 0.  The module's running statistics are moved between the rounds (no forward pass runs here) and put back at the end.
    Returns the number of padding elements."""
    import torch
    from pose_adv_aug_amd.utils.optim import ModelEma
    opt = make_opt(module)
    ema = ModelEma(module, decay=0.999, warmup=True, buffers=buffers)
    twin = ema.module
    if type(twin) is not type(module) or twin.flat_params.data_ptr() == module.flat_params.data_ptr():
        fails.append(('%s: the twin is not a separate module of the same class' % what, type(twin).__name__))
    if bits_differ(twin.flat_params, module.flat_params) or bits_differ(twin.flat_buffers, module.flat_buffers) or twin._nbt != module._nbt:
        fails.append(('%s: the twin does not start as a bit-exact copy' % what, 0))
    pads = [_pad_mask(module, 0), _pad_mask(module, 1)]
    saved = module.flat_buffers.clone()
    worst = [0.0, 0.0]
    for k in range(3):
        e0 = [twin.flat_params.clone(), twin.flat_buffers.clone()]
        s0 = read_state(ema._state)
        module.flat_buffers.mul_(1.0 + 0.03 * (k + 1))
        opt.step()
        ema.update(opt)
        torch.cuda.synchronize()
        s1 = read_state(ema._state)
        for word in check_state(s0, s1, 0.999, True, 0):
            fails.append(('%s: state word (got, expected), round %d' % (what, k), word))
        for j, (name, src, dst) in enumerate((('parameters', module.flat_params, twin.flat_params), ('buffers', module.flat_buffers, twin.flat_buffers))):
            x = check_arrays(e0[j], src, dst, s1, copy=(j == 1 and buffers == 'copy'))
            worst[j] = max(worst[j], x) if x == x else x
            if not (x <= 1.0):
                fails.append(('%s of the twin of %s (buffers %s), round %d' % (name, what, buffers, k), x))
            if bits_differ(dst, e0[j]) == 0:
                fails.append(('%s of the twin of %s did not move in round %d' % (name, what, k), 0))
            if bool((dst[pads[j]] != 0).any()) or bool((src[pads[j]] != 0).any()):
                fails.append(('%s: padding of the %s not zero after round %d' % (what, name, k), 0))
            if not bool(torch.isfinite(dst).all()):
                fails.append(('non-finite %s in the twin of %s after round %d' % (name, what, k), 0))
        if twin._nbt != module._nbt:
            fails.append(('%s: num_batches_tracked of the twin' % what, twin._nbt))
    if (ema.updates(), ema.held()) != (3, 0):
        fails.append(('%s: updates / held after three rounds' % what, (ema.updates(), ema.held())))
    module.flat_buffers.copy_(saved)
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('ema_exact flat arrays of %s, buffers %s (%d + %d padding elements): worst error / bound parameters %.3g buffers %.3g'
            % (what, buffers, int(pads[0].sum()), int(pads[1].sum()), worst[0], worst[1]))
    return int(pads[0].sum())


def run_flat_array(log=print):
    """ModelEma behind RMSprop and behind Adam on the real flat arrays of the 2-stack chan-128 pose net (B 2) and its agent
    (optim_opts_exact.flat_nets, built once), buffers averaged and copied"""
    from pose_adv_aug_amd.utils.optim import Adam, RMSprop
    from tests.optim_opts_exact import flat_nets
    fails = []
    net, agent = flat_nets()
    pads = 0
    for cls, buffers in ((RMSprop, 'ema'), (Adam, 'copy'), (RMSprop, 'copy'), (Adam, 'ema')):
        pads += _check_flat(net, cls, '%s on the pose net' % cls.__name__, buffers, fails, log)
        pads += _check_flat(agent, cls, '%s on the agent' % cls.__name__, buffers, fails, log)
    if pads == 0:
        fails.append(('neither flat array has alignment padding: nothing was tested', 0))
    return fails


class ToyNet(object):
    """what an optimizer and ModelEma see of a net: n parameters in one tensor, 8 buffers, no engine handle behind them"""
    def __init__(self, n, p=None):
        import torch
        self.n = n
        self.flat_params = torch.zeros(n, device='cuda') if p is None else p.clone()
        self.flat_grads = torch.zeros(n, device='cuda')
        self.flat_buffers = torch.arange(8, dtype=torch.float32, device='cuda')
        self._table = [('w', (n,), 0, n, 0), ('b', (8,), 0, 8, 1)]
        self._nbt, self._last_B, self.default_batch, self.repacks = 0, 1, 1, 0

    def _twin(self):
        return ToyNet(self.n)

    def _ensure_table(self):
        pass

    def eval(self):
        return self

    def _net(self, B):
        return None

    def weights_changed(self):
        self.repacks += 1


def run_skip_case(log=print):
    """fp16 build, ModelEma(decay 0.999, warm-up) behind RMSprop and behind Adam on optim_exact.SKIP_N parameters.  One clean round
    first.  Then inf at each of optim_exact.SKIP_POSITIONS: the optimizer skips, and the average, its buffers, its count and its w do
    not move, held + 1; the next clean round moves them, within the bound, with the w of the un-advanced count."""
    import torch
    from pose_adv_aug_amd.utils.optim import Adam, ModelEma, RMSprop
    from tests import optim_exact as X
    from tests.optim_exact import _t
    n = X.SKIP_N
    fails = []
    p, g, _ = X.make_inputs(n, 4300, 1.0 / 32768.0, False)
    for cls in (RMSprop, Adam):
        net = ToyNet(n, _t(p))
        opt = cls(net)
        ema = ModelEma(net, decay=0.999, warmup=True)
        twin = ema.module
        clean = _t(g)

        def round_(grad, what, held):
            net.flat_grads.copy_(grad)
            net.flat_buffers.add_(1.0)
            e0, b0, s0, p0 = twin.flat_params.clone(), twin.flat_buffers.clone(), read_state(ema._state), net.flat_params.clone()
            opt.step()
            ema.update(opt)
            torch.cuda.synchronize()
            s1 = read_state(ema._state)
            for word in check_state(s0, s1, 0.999, True, 1 if held else 0):
                fails.append(('%s: state word (got, expected) %s' % (cls.__name__, what), word))
            if held != (bits_differ(net.flat_params, p0) == 0):
                fails.append(('%s: the optimizer did not %s %s' % (cls.__name__, 'skip' if held else 'step', what), 0))
            for name, a0, src, dst in (('parameters', e0, net.flat_params, twin.flat_params), ('buffers', b0, net.flat_buffers, twin.flat_buffers)):
                x = check_arrays(a0, src, dst, s1)
                if not (x <= 1.0):
                    fails.append(('%s: %s of the average %s' % (cls.__name__, name, what), x))
                if not held and bits_differ(dst, a0) == 0:
                    fails.append(('%s: %s of the average did not move %s' % (cls.__name__, name, what), 0))

        round_(clean, 'first clean round', False)
        for where, pos in X.SKIP_POSITIONS:
            bad = clean.clone()
            bad[pos] = float('inf')
            c0 = (ema.updates(), ema.held())
            round_(bad, 'inf at %s' % where, True)
            if (ema.updates(), ema.held()) != (c0[0], c0[1] + 1):
                fails.append(('%s: counts after a skipped step (were %s), inf at %s' % (cls.__name__, c0, where), (ema.updates(), ema.held())))
            round_(clean, 'clean round after inf at %s' % where, False)
            if (ema.updates(), ema.held()) != (c0[0] + 1, c0[1] + 1):
                fails.append(('%s: counts after the next clean step, inf at %s' % (cls.__name__, where), (ema.updates(), ema.held())))
        if opt.skipped_steps() != len(X.SKIP_POSITIONS) or ema.held() != len(X.SKIP_POSITIONS):
            fails.append(('%s: skipped steps / held updates' % cls.__name__, (opt.skipped_steps(), ema.held())))
    if os.environ.get('POSEADV_TEST_VERBOSE'):
        log('ema_exact skip: %d positions x 2 optimizers, %d failures' % (len(X.SKIP_POSITIONS), len(fails)))
    return fails


if __name__ == '__main__':          # the fp16 build: tests/test_gpu_ema.py runs this with POSEADV_DTYPE=fp16
    import torch
    from pose_adv_aug_amd._lib import lib as _l
    from tests import optim_exact as X
    assert _l().pa_dtype() == 1, 'run with POSEADV_DTYPE=fp16'
    torch.cuda.set_device(0)
    out = lambda s: print(s, flush=True)
    fails = []
    for n in X.SIZES:
        fails += run_case(n, log=out)
    fails += run_hold_case(log=out)
    fails += run_error_cases()
    fails += run_skip_case(log=out)
    fails += run_flat_array(log=out)
    print('FAILURES %d %s' % (len(fails), fails[:20]))
    print('FP16 EMA EXACT ' + ('PASSED' if not fails else 'FAILED'), flush=True)
    sys.exit(1 if fails else 0)

"""CPU checks of tests/ema_exact.py (the reference, the bound and the state model of the weight EMA) on numpy alone: an fp32 emulation of
the kernel is inside the bound, the reference is torch.lerp and agrees with torch's own EMA, each planted defect is outside; the new
symbols exist in both libraries, the refusals are decided on the host, ModelEma's launch sequence and the command line."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import ema_exact as X

N = 100003


def _lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


@pytest.fixture(scope='module')
def data():
    return X.make_inputs(N, 7)


@pytest.mark.parametrize('decay', X.DECAYS)
def test_the_emulated_kernel_is_inside_the_bound(data, decay):
    e, p, same = data
    w = X.host_w(decay, 0, 0)
    out = X.emulate(e, p, w)
    r = X.ratio(out, e, p, w)
    print('decay %g: worst error / bound of the emulated kernel %.3f' % (decay, r))
    assert 0.3 < r <= 1.0                               # inside, and not by a margin that would hide a second rounding
    assert np.array_equal(out[same], e[same])           # p == e gives e
    assert X.bits_differ(X.emulate(np.zeros(8, np.float32), np.zeros(8, np.float32), w), np.zeros(8, np.float32)) == 0      # padding


@pytest.mark.parametrize('decay', X.DECAYS)
def test_the_reference_is_torch_lerp_and_torchs_ema(data, decay):
    e, p, _ = data
    w = X.host_w(decay, 0, 0)
    ref, bound = X.reference(e.astype(np.float64), p.astype(np.float64), w)
    e64, p64 = torch.from_numpy(e).double(), torch.from_numpy(p).double()
    lerp = torch.lerp(e64, p64, w).numpy()
    # float64 against float64: the two forms of torch.lerp (e + w (p - e) below w = 0.5, p - (1 - w)(p - e) from there) round differently
    assert np.all(np.abs(lerp - ref) <= 4 * 2.0 ** -53 * (np.abs(e) + np.abs(p)))
    # torch's own EMA of CPU fp32 tensors, handed the fp32 decay the engine works with (its weight is then the engine's w).  fp32
    # accuracy: torch rounds the product w (p - e) before the sum where the kernel fuses it: one more rounding of that term, which
    # the term u |w (p - e)| of the bound pays a second time.
    fn = torch.optim.swa_utils.get_ema_multi_avg_fn(X._f32(decay))
    avg = [torch.from_numpy(e.copy())]
    fn(avg, [torch.from_numpy(p)], 0)
    assert np.all(np.abs(avg[0].double().numpy() - ref) <= 2 * bound)


def _alt_form(e, p, w):
    """e d + p w with d = 1 - w in fp32, every operation rounded"""
    w32 = np.float32(w)
    d32 = np.float32(1.0) - w32
    return (e * d32).astype(np.float32) + (p * w32).astype(np.float32)


def test_each_defect_is_outside(data):
    e, p, _ = data
    decay, warm = 0.999, 1
    s0 = dict(updates=3, held=1, apply=1, w=X.host_w(decay, warm, 2), decay_used=X._f32(X.host_decay(decay, warm, 2)))
    good = X.expected_state(s0, decay, warm, 0)
    assert good['updates'] == 4 and good['w'] == X._f32(1.0 - 4.0 / 13.0) and X.check_state(s0, good, decay, warm, 0) == []
    assert X.check_arrays(e, p, X.emulate(e, p, good['w']), good) <= 1.0
    # decay used where w belongs
    w = X.host_w(decay, 0, 0)
    r = X.ratio(X.emulate(e, p, X._f32(decay)), e, p, w)
    print('decay for w: error / bound %.3g' % r)
    assert r > 1e3
    # e d + p w with d = 1 - w in fp32: the same value to a few ulp, outside the bound of the two-operation form
    alt = _alt_form(e, p, w)
    r = X.ratio(alt, e, p, w)
    print('e d + p w: error / bound %.3g, %d of %d elements differ from the kernel' % (r, X.bits_differ(alt, X.emulate(e, p, w)), N))
    assert r > 1.0
    # an update applied on a held step / the count advanced on a held step
    held = X.expected_state(s0, decay, warm, 1)
    assert held == dict(s0, apply=0, held=2) and X.check_state(s0, held, decay, warm, 1) == []
    assert X.check_arrays(e, p, e.copy(), held) == 0.0
    assert X.check_arrays(e, p, X.emulate(e, p, s0['w']), held) > 1.0
    assert X.check_state(s0, dict(held, updates=4), decay, warm, 1) == [('updates', 4, 3)]
    assert X.check_state(s0, good, decay, warm, 1) != []                       # a flag that is not read at all
    # warm-up ignoring the count
    blind = dict(good, w=X.host_w(decay, 0, 0), decay_used=X._f32(decay))
    assert [k for k, _, _ in X.check_state(s0, blind, decay, warm, 0)] == ['w', 'decay_used']
    assert X.check_state(dict(s0, updates=10 ** 6), dict(blind, updates=10 ** 6 + 1), decay, warm, 0) == []     # (past the ramp it IS the decay)
    # copy = 1 is bit for bit
    assert X.check_arrays(e, p, p.copy(), good, copy=True) == 0.0 and X.check_arrays(e, p, X.emulate(e, p, 1.0), good, copy=True) > 1.0


def test_the_warm_up_schedule():
    assert X.host_decay(0.999, 1, 0) == 0.1 and X.host_decay(0.999, 1, 9) == 10.0 / 19.0 and X.host_decay(0.5, 1, 9) == 0.5
    assert X.host_decay(0.999, 0, 0) == X._f32(0.999) and X.host_decay(0.999, 1, 10 ** 5) == X._f32(0.999)
    assert X.host_w(0.0, 1, 0) == 1.0 and X.host_w(0.9999, 0, 5) == X._f32(1.0 - X._f32(0.9999))


NAMES = ('pa_ema_advance', 'pa_ema_lerp', 'pa_ema_counts', 'pa_ema_set_updates')


def test_the_symbols_exist_in_both_libraries():
    import pose_adv_aug_amd as P
    _lib()
    here = os.path.dirname(P.LIB_PATH)
    for so in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        l = C.CDLL(os.path.join(here, so))
        assert all(hasattr(l, n) for n in NAMES), so
    assert all(n in P.EXPORTS for n in NAMES)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'poseadv.h')).read()
    assert all(n + '(' in hdr for n in NAMES) and 'typedef struct pa_ema_state' in hdr


def test_refusals_are_decided_on_the_host():
    """The pointers are host addresses that are never dereferenced: every call below is refused before any device call, so it answers on
    a machine without a GPU."""
    L = _lib()
    buf = np.zeros(64, dtype=np.float32)
    addr = buf.ctypes.data + (-buf.ctypes.data) % 16
    e, p, s = C.c_void_p(addr), C.c_void_p(addr + 64), C.c_void_p(addr + 128)
    cnt = C.c_longlong(-7)

    def refused(rc, word):
        msg = L.pa_last_error()
        assert rc != 0 and word in msg, (rc, msg)

    refused(L.pa_ema_advance(None, 0.9, 0, None, None), b'pa_ema_advance: state is NULL')
    for d in (1.0, -0.1, 1.5, float('nan'), float('inf'), float('-inf')):
        refused(L.pa_ema_advance(s, d, 1, None, None), b'pa_ema_advance: decay must be finite and in [0, 1)')
    refused(L.pa_ema_lerp(None, p, 16, s, 0, None), b'pa_ema_lerp: state, ema or src is NULL')
    refused(L.pa_ema_lerp(e, None, 16, s, 0, None), b'pa_ema_lerp: state, ema or src is NULL')
    refused(L.pa_ema_lerp(e, p, 16, None, 0, None), b'pa_ema_lerp: state, ema or src is NULL')
    for copy in (0, 1):
        refused(L.pa_ema_lerp(e, e, 16, s, copy, None), b'pa_ema_lerp: ema and src are the same array')
    refused(L.pa_ema_lerp(C.c_void_p(addr + 4), p, 8, s, 0, None), b'16-byte aligned')
    refused(L.pa_ema_counts(None, C.byref(cnt), C.byref(cnt), None), b'pa_ema_counts: state is NULL')
    refused(L.pa_ema_set_updates(None, 3, None), b'pa_ema_set_updates: state is NULL')
    for v in (-1, 2 ** 31):
        refused(L.pa_ema_set_updates(s, v, None), b'pa_ema_set_updates: updates must be in 0 .. 2^31 - 1')
    assert cnt.value == -7 and not buf.any()


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
            self.log.append((name, args))
            return 0
        return call


class _HostNet(object):
    def __init__(self):
        self.flat_params, self.flat_grads, self.flat_buffers = torch.arange(12.), torch.ones(12), torch.arange(5.)
        self._table = [('a.weight', (2, 3), 0, 6, 0), ('a.bias', (3,), 8, 3, 0), ('bn.running_mean', (5,), 0, 5, 1)]
        self._nbt, self._last_B, self.default_batch, self.repacks, self.training = 4, 1, 1, 0, True

    def _twin(self):
        t = _HostNet()
        t.flat_params, t.flat_buffers, t._nbt = torch.zeros(12), torch.zeros(5), 0
        return t

    def _ensure_table(self):
        pass

    def _net(self, B):
        return None

    def weights_changed(self):
        self.repacks += 1

    def eval(self):
        self.training = False
        return self

    def state_dict(self):
        return {'a.weight': self.flat_params[0:6].view(2, 3)}


def test_update_is_one_prologue_and_two_launches_with_the_optimizers_flag(monkeypatch):
    from pose_adv_aug_amd import _lib
    from pose_adv_aug_amd.utils import optim
    rec = _Recorder()
    for mod in (optim, _lib):
        monkeypatch.setattr(mod, 'lib', lambda: rec)
    monkeypatch.setattr(optim, 'ptr', lambda x: x)
    monkeypatch.setattr(optim, 'stream', lambda: 12345)
    net = _HostNet()
    for cls, flag_of in ((optim.RMSprop, lambda o: o._skip_state), (optim.Adam, lambda o: o._state)):
        o = cls(net)
        ema = optim.ModelEma(net, decay=0.99, warmup=True, buffers='copy')
        twin = ema.module
        assert type(twin) is _HostNet and twin is not net and not twin.training
        assert torch.equal(twin.flat_params, net.flat_params) and torch.equal(twin.flat_buffers, net.flat_buffers) and twin._nbt == net._nbt
        assert twin.flat_params.data_ptr() != net.flat_params.data_ptr() and rec.log == []          # construction launches nothing
        net._nbt, repacks = net._nbt + 1, twin.repacks
        o.step()
        del rec.log[:]
        ema.update(o)
        assert [n for n, _ in rec.log] == ['pa_ema_advance', 'pa_ema_lerp', 'pa_ema_lerp']
        adv, lp, lb = (a for _, a in rec.log)
        assert adv[0] is ema._state and adv[1:3] == (0.99, 1) and adv[3] is flag_of(o) and adv[4] == 12345
        assert lp[0] is twin.flat_params and lp[1] is net.flat_params and lp[2:] == (12, ema._state, 0, 12345)
        assert lb[0] is twin.flat_buffers and lb[1] is net.flat_buffers and lb[2:] == (5, ema._state, 1, 12345)
        assert twin._nbt == net._nbt and twin.repacks == repacks + 1
        del rec.log[:]
        ema.buffers = 'ema'
        ema.update()                                        # no optimizer: no flag pointer
        assert rec.log[0][1][3] is None and rec.log[2][1][4] == 0
        sd = ema.state_dict()
        assert sorted(sd) == ['buffers', 'decay', 'module', 'updates', 'warmup'] and (sd['decay'], sd['warmup'], sd['buffers']) == (0.99, True, 'ema')
        del rec.log[:]
    for bad in (dict(decay=1.0), dict(decay=-0.1), dict(buffers='mean')):
        with pytest.raises(ValueError):
            optim.ModelEma(net, **bad)


def test_the_command_line(tmp_path):
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils import optim
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'e']
    opt = TrainOptions().parse(base)
    assert (opt.ema_decay, opt.ema_warmup, opt.ema_buffers) == (0.0, 0, 'ema')
    assert optim.make_ema(opt, None) is None                  # off: no twin, nothing touched
    assert optim.make_ema(types.SimpleNamespace(), None) is None
    opt = TrainOptions().parse(base + ['--ema_decay', '0.999', '--ema_warmup', '1', '--ema_buffers', 'copy'])
    assert (opt.ema_decay, opt.ema_warmup, opt.ema_buffers) == (0.999, 1, 'copy')
    for bad in (['--ema_decay', '1'], ['--ema_decay', '-0.5'], ['--ema_buffers', 'mean'], ['--ema_warmup', '2']):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + bad)

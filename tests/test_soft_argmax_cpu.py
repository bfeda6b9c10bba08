"""CPU checks of the soft-arg-max (tests/soft_argmax_exact.py holds the reference, the cases and the bound): the float64 reference against
a numpy.longdouble evaluation and against torch autograd of softmax, the kernel restated in numpy inside the bound and eight planted
defects far outside it, the constants of the bound against the header, the exported symbols, the refusals (host code: they answer
without a GPU), the Python argument errors and the options."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import abi_stub
from tests import soft_argmax_exact as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pa_soft_argmax', 'pa_soft_argmax_bwd', 'pa_exp_probe')


def _lib():
    import pose_adv_aug_amd as P
    if not os.path.isfile(P.LIB_PATH):
        P.build()
    return P.lib()


@pytest.mark.parametrize('name', S.CASES)
def test_reference_agrees_with_longdouble_and_with_autograd(name):
    """float64 reference against the formulas in numpy.longdouble throughout: inside the d terms alone (no fp32 rounding granted); its
    gradient against torch autograd of softmax in float64 (an independent route: no explicit maximum, no explicit formula)"""
    cs, ref, fb, want, bound = S.reference(name)
    assert np.finfo(np.longdouble).nmant > 52
    ex, ey, Z, dm = S.longdouble_eval(cs['maps'], cs['W'], cs['beta'], cs['dco'])
    _, d = S.backward_bound(ref, fb, cs['dco'], want, S.backward64(ref, cs['dco'])[1])
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    assert np.all(np.abs(ld(ref['ex']) - ex) <= fb['dx']) and np.all(np.abs(ld(ref['ey']) - ey) <= fb['dy']) and np.all(np.abs(ld(ref['Z']) - Z) <= fb['dZ'])
    assert np.all(np.abs(ld(want) - dm) <= d + 1e-300)
    assert np.all(fb['dx'] <= 1e-9 * np.abs(ref['ex'])) and np.all(np.isfinite(want))       # d is orders below u32 |ref| = 6e-8 |ref|
    h = torch.from_numpy(cs['maps'].astype(np.float64)).requires_grad_()
    p = torch.softmax(float(np.float32(cs['beta'])) * h, dim=2)
    xy = torch.stack((torch.from_numpy(ref['x']), torch.from_numpy(ref['y'])), dim=1)
    co = p @ xy
    (co * torch.from_numpy(cs['dco'].astype(np.float64))).sum().backward()
    assert S.ratio(co.detach().numpy()[..., 0], ref['ex'], 1e-11 * np.abs(ref['ex'])) <= 1.0
    # (autograd forms p (g - sum p g): it cancels where the reference subtracts ex first, so its error scales with beta (|gx| W + |gy| H))
    scale = cs['beta'] * (np.abs(cs['dco'][..., 0:1]) * cs['W'] + np.abs(cs['dco'][..., 1:2]) * cs['H']).astype(np.float64)
    assert np.all(np.abs(h.grad.numpy() - want) <= 1e-12 * scale + 1e-300)


@pytest.mark.parametrize('name', S.CASES)
def test_kernel_restatement_stays_inside_the_bound(name):
    cs = S.case(name)
    worst, fails = S.judge(name, *S.kernel_restatement(cs['maps'], cs['H'], cs['W'], cs['beta'], cs['dco'], cs['fast']))
    assert fails == [] and max(worst.values()) <= 1.0, (worst, fails)


@pytest.mark.parametrize('defect', sorted(S.DEFECTS))
def test_bound_tells_a_planted_defect(defect):
    """x and y swapped, p / H for the row (the 8 x 24 map), 0-based coordinates, beta missing in the backward, the maximum not subtracted,
    a running-max merge without rescale, the gradient centred on the arg-max, the last partial trip dropped: each leaves the bound of its
    named case by at least three orders of magnitude"""
    name = S.DEFECTS[defect]
    cs = S.case(name)
    worst, _ = S.judge(name, *S.kernel_restatement(cs['maps'], cs['H'], cs['W'], cs['beta'], cs['dco'], cs['fast'], defect=defect))
    assert max(worst.values()) >= 1e3, (defect, worst)


def test_cases_reach_the_edges_they_name():
    for h, w in S.FAST_SHAPES:
        pos = S.peak_positions(h, w)
        assert pos[0] == 0 and (h * w == 1 or pos[1] == h * w - 1)
    pos = S.peak_positions(96, 96)
    for edge in (64, S.THREADS, S.INFLIGHT * S.THREADS, 2 * S.INFLIGHT * S.THREADS, 2304):
        assert edge - 1 in pos and edge in pos
    assert 96 * 96 % (S.INFLIGHT * S.THREADS) != 0 and 8 * 24 % S.THREADS != 0
    maps, peaks = S._peaked(0, 3, 16, 96, 96)
    assert np.array_equal(maps.argmax(-1), peaks) and len(set(peaks.reshape(-1).tolist())) == len(pos)   # every position is some joint's maximum
    for name in ('fast_ramp_64x64', 'fast_ramp_8x24'):
        d = np.diff(S.case(name)['maps'][0].astype(np.float64), axis=-1)
        assert np.all(d[0::2] > 0) and np.all(d[1::2] < 0)              # strictly monotone: every element / none is a new running maximum
    assert S.case('generic_offset')['fast'] is False and S.case('fast_8x24_B1')['fast'] is True
    assert np.abs(S.case('range_3e4')['maps']).max() > 2.9e4 and np.abs(S.case('range_3e38')['maps']).min() > 2.9e38
    for name in S.CASES:
        cs = S.case(name)
        assert cs['maps'].shape == (cs['B'], cs['J'], cs['H'] * cs['W']) and np.all(np.isfinite(cs['maps']))


def test_bound_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, 'pose_adv_aug_amd', 'csrc', 'soft_argmax.h')).read()
    val = lambda n: int(re.search(r'#define\s+%s\s+(\d+)' % n, hdr).group(1))
    assert (val('PA_SAM_THREADS'), val('PA_SAM_INFLIGHT'), val('PA_SAM_GENERIC_THREADS'), val('PA_SAM_BWD_THREADS'), val('PA_SAM_BWD_CHUNKS')) == \
        (S.THREADS, S.INFLIGHT, S.GENERIC_THREADS, S.BWD_THREADS, S.BWD_CHUNKS)
    assert S.EXP_REL == 2 * S.EXP_MEASURED_REL and S.EXP_SUB == 2 * S.EXP_MEASURED_SUB
    prof = open(os.path.join(ROOT, 'profiles', 'soft_argmax.txt')).read()                    # the measurement the constant is twice of
    rel = float(re.search(r'largest relative error, normal results\s+(\S+)', prof).group(1))
    sub = float(re.search(r'largest absolute error, subnormal results\s+(\S+) x', prof).group(1))
    assert abs(S.EXP_MEASURED_REL - rel) <= 1e-3 * rel and abs(S.EXP_MEASURED_SUB - sub) <= 1e-3 * sub + 1e-12


def test_both_libraries_export_the_symbols_and_the_header_declares_them():
    import pose_adv_aug_amd as P
    _lib()
    here = os.path.dirname(P.LIB_PATH)
    for name in ('libposeadv_hip.so', 'libposeadv_hip_fp16.so'):
        l = C.CDLL(os.path.join(here, name))
        assert [s for s in SYMBOLS if not hasattr(l, s)] == [], name
    hdr = open(os.path.join(ROOT, 'include', 'poseadv.h')).read()
    assert set(SYMBOLS) <= set(re.findall(r'\b(pa_[a-z0-9_]+)\s*\(', hdr))
    assert set(SYMBOLS) <= set(P.EXPORTS)


def test_refusals_return_an_error_and_launch_nothing():
    """every refusal is decided on the host before any device call: it answers on a machine without a GPU"""
    L = _lib()
    buf = np.zeros(4096, dtype=np.float64)
    a = buf.ctypes.data
    a += a % 16
    p, q = C.c_void_p(a), C.c_void_p(a + 8192)

    def fwd(maps=p, layout=1, B=2, J=16, H=8, W=8, beta=1.0, coords=q, state=q):
        return L.pa_soft_argmax(maps, layout, B, J, H, W, beta, coords, state, None)

    def bwd(maps=p, layout=1, B=2, J=16, H=8, W=8, beta=1.0, state=q, dco=q, dmaps=q):
        return L.pa_soft_argmax_bwd(maps, layout, B, J, H, W, beta, state, dco, dmaps, None)

    common = [(dict(maps=None), b'NULL'), (dict(state=None), b'NULL'), (dict(B=0), b'>= 1'), (dict(J=0), b'>= 1'), (dict(H=0), b'>= 1'), (dict(W=-3), b'>= 1'),
              (dict(layout=2), b'layout'), (dict(layout=-1), b'layout'), (dict(beta=0.0), b'beta'), (dict(beta=-1.0), b'beta'),
              (dict(beta=float('inf')), b'beta'), (dict(beta=float('nan')), b'beta'), (dict(H=1 << 14, W=1 << 13), b'2^27'), (dict(B=1 << 16, J=1 << 15), b'2^31')]
    for call, extra in ((fwd, [(dict(coords=None), b'NULL')]), (bwd, [(dict(dco=None), b'NULL'), (dict(dmaps=None), b'NULL'), (dict(dmaps=p), b'alias')])):
        for kw, word in common + extra:
            assert call(**kw) != 0, kw
            assert word in L.pa_last_error(), (kw, L.pa_last_error())
    assert L.pa_exp_probe(None, q, 4, None) != 0 and L.pa_exp_probe(p, q, 0, None) != 0


def _stubbed(monkeypatch):
    from pose_adv_aug_amd.pylib import Evaluation
    fake = abi_stub.FakeLib(0)
    monkeypatch.setattr(Evaluation, 'lib', lambda: fake)
    monkeypatch.setattr(Evaluation, 'ptr', lambda t: t)
    monkeypatch.setattr(Evaluation, 'stream', lambda: 12345)
    monkeypatch.setattr(Evaluation, 'dev', lambda: torch.device('cpu'))
    return Evaluation, fake


def test_python_argument_errors_come_before_any_launch(monkeypatch):
    E, fake = _stubbed(monkeypatch)
    good = torch.zeros(2, 16, 8, 8)
    for bad, kw in ((good.double(), {}), (good.half(), {}), (good[0], {}), (good.numpy(), {}), (torch.zeros(2, 0, 8, 8), {}), (good, dict(layout='nhwc4')),
                    (good, dict(beta=0.0)), (good, dict(beta=-2.0)), (good, dict(beta=float('inf'))), (good, dict(beta=float('nan'))),
                    (good.to('meta'), {})):
        with pytest.raises(ValueError):
            E.soft_argmax(bad, **kw)
    assert fake.log == []
    # a good call: one launch with the layout number and the shape in the ABI's order; a heat that requires grad adds the backward launch
    out = E.soft_argmax(good, beta=2.0)
    assert tuple(out.shape) == (2, 16, 2) and out.dtype == torch.float32
    assert fake.names() == ['pa_soft_argmax'] and fake.log[0][1][1:7] == (0, 2, 16, 8, 8, 2.0)
    nhwc = torch.zeros(3, 4, 6, 16, requires_grad=True)
    out = E.soft_argmax(nhwc, layout='nhwc')
    assert fake.log[1][1][1:7] == (1, 3, 16, 4, 6, 1.0) and out.grad_fn is not None
    out.sum().backward()
    name, args = fake.log[2]
    assert name == 'pa_soft_argmax_bwd' and args[1:7] == (1, 3, 16, 4, 6, 1.0) and args[7] is fake.log[1][1][8]        # the state the forward wrote
    assert tuple(nhwc.grad.shape) == (3, 4, 6, 16) and tuple(args[8].shape) == (3, 16, 2)
    with torch.no_grad():
        assert E.soft_argmax(nhwc, layout='nhwc').grad_fn is None


def test_coord_l1_is_the_masked_mean_absolute_error():
    from pose_adv_aug_amd.pylib import Criterion
    g = torch.Generator().manual_seed(3)
    pred = (torch.rand(3, 16, 2, generator=g) * 64).requires_grad_()
    pts = torch.rand(3, 16, 2, generator=g, dtype=torch.float64) * 70 - 3          # some joints outside 0 < x <= 64
    inside = (pts[..., 0] > 0) & (pts[..., 1] > 0) & (pts[..., 0] <= 64) & (pts[..., 1] <= 64)
    assert 0 < int(inside.sum()) < 48
    loss = Criterion.coord_L1(pred, pts, size=(64, 64))
    want = (pred.detach().double() - pts).abs()[inside].mean()
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want)
    loss.backward()
    assert bool((pred.grad[~inside] == 0).all()) and bool((pred.grad[inside].abs() > 0).all())
    lower = (pts[..., 0] > 0) & (pts[..., 1] > 0)
    assert abs(float(Criterion.coord_L1(pred, pts)) - float((pred.detach().double() - pts).abs()[lower].mean())) <= 1e-4
    assert float(Criterion.coord_L1(pred, pts, valid=torch.zeros(3, 16, dtype=torch.bool))) == 0.0
    assert torch.equal(Criterion.coord_L1(pred, pts, valid=inside), loss.detach())
    for bad in (dict(pred_xy=pred[0]), dict(pts=pts[:2]), dict(valid=torch.ones(3, 15, dtype=torch.bool))):
        kw = dict(pred_xy=pred, pts=pts, valid=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            Criterion.coord_L1(kw['pred_xy'], kw['pts'], kw['valid'])


def test_layout_arguments_are_checked_before_the_engine_is_touched():
    from pose_adv_aug_amd.models.asn_stacked_hg import HourglassNet
    net = HourglassNet(1, 1, chan=128, res=128, default_batch=2)
    for call in (lambda: net.heatmaps(2, layout='nhwc4'), lambda: net.forward_autograd(x=torch.zeros(2, 3, 128, 128), layout='hwc')):
        with pytest.raises(ValueError):
            call()
    assert net._nets == {}


def test_options_parse_and_zero_selects_the_unchanged_loop(tmp_path, monkeypatch):
    from pose_adv_aug_amd import stack_hg
    from pose_adv_aug_amd.options.train_options import TrainOptions
    from pose_adv_aug_amd.utils import checkpoint, visualizer
    base = ['--exp_dir', str(tmp_path), '--exp_id', 'c', '--nEpochs', '1', '--is_train', '1']
    o = TrainOptions().parse(base)
    assert o.coord_loss == 0.0 and o.coord_beta == 1.0
    o = TrainOptions().parse(base + ['--coord_loss', '0.1', '--coord_beta', '2.5'])
    assert o.coord_loss == 0.1 and o.coord_beta == 2.5
    for bad in (['--coord_loss', '-1'], ['--coord_beta', '0']):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + bad)
    calls = []
    monkeypatch.setattr(stack_hg, 'create_hg', lambda **k: types.SimpleNamespace())
    monkeypatch.setattr(stack_hg, 'make_optimizer', lambda *a: types.SimpleNamespace(param_groups=[dict(lr=1e-3)]))
    monkeypatch.setattr(stack_hg, 'broadcast_parameters', lambda net: None)
    monkeypatch.setattr(stack_hg, 'Augmenter', lambda **k: None)
    monkeypatch.setattr(stack_hg, 'make_feeds', lambda *a: ([], []))
    monkeypatch.setattr(stack_hg, 'adjust_lr', lambda *a: None)
    monkeypatch.setattr(stack_hg, 'train', lambda *a, **k: (calls.append((len(a), k)), (0.0, 0.0))[1])
    monkeypatch.setattr(stack_hg, 'validate', lambda *a, **k: (0.0, 0.0, torch.zeros(0, 16, 2)))
    monkeypatch.setattr(checkpoint.Checkpoint, 'save_checkpoint', lambda self, *a: None)
    monkeypatch.setattr(visualizer.Visualizer, 'write_log', lambda self, m: None)
    stack_hg.main(base)
    assert len(calls) == 1 and calls[0][0] == 6 and sorted(calls[0][1]) == ['log']            # the call the loop has always made
    stack_hg.main(base + ['--coord_loss', '0.1'])
    assert len(calls) == 2 and sorted(calls[1][1]) == ['criterion', 'log'] and callable(calls[1][1]['criterion'])


def test_train_hands_the_criterion_to_train_step_on_the_joint_minor_maps(monkeypatch):
    from pose_adv_aug_amd import stack_hg
    seen = []
    ahead = types.SimpleNamespace(start=lambda b: None, take=lambda: 'data')
    monkeypatch.setattr(stack_hg, 'AugmentAhead', lambda aug: ahead)
    monkeypatch.setattr(stack_hg, 'train_step', lambda *a, **k: (seen.append(k), (torch.zeros(()), torch.zeros(()), torch.zeros(())))[1])
    monkeypatch.setattr(stack_hg, 'DeviceMeters', lambda names, dev: types.SimpleNamespace(update=lambda d: None, averages=lambda: dict(loss=0.0, pckh=0.0, pckh_origin_res=0.0)))
    net, opt = types.SimpleNamespace(train=lambda: None), types.SimpleNamespace(print_freq=100)
    stack_hg.train(['b0'], net, None, None, 0, opt, log=lambda m: None)
    crit = lambda outs, data: None
    stack_hg.train(['b0'], net, None, None, 0, opt, log=lambda m: None, criterion=crit)
    assert seen[0] == dict(data='data') and seen[1] == dict(data='data', criterion=crit, heat_layout='nhwc')

"""The opt-in stretch mode of the staged crop (pa_crop_stretch, HumanAug.crop_batch(stretch=True)) on the device: scipy's
toimage() min/max byte stretch reproduced, byte for byte against the REFERENCE's own crop -- tests/golden/crop_stretch.npz
(frames without a pure black / white pixel, tests/stretch_inputs.py) and ALL of tests/golden/crop.npz, the two cases the
default mode has to skip included.  Every bound asserted here is equality."""
import os

import numpy as np
import pytest
import torch

from tests import inputs
from tests import stretch_inputs as si

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
HS, WS, RES, GUARD = 720, 1280, 256, 4096


@pytest.fixture(scope='module')
def P():
    import pose_adv_aug_amd.pylib as P
    return P


def _sums(a):
    return [int(a[..., k].astype(np.int64).sum()) for k in range(3)] + [int((a[..., k].astype(np.int64) ** 2).sum()) for k in range(3)]


@pytest.fixture(scope='module')
def batch(P):
    """the sixteen cases of stretch_inputs in ONE padded 720 x 1280 batch: the 375 x 500 frame of case 10 sits top-left in its
    slot, and the padding around it alternates 0 / 255 -- a reduction that reads padding finds a black and a white pixel"""
    frames = si.frames()
    buf = np.zeros((len(si.CASES), HS, WS, 3), dtype=np.uint8)
    sizes = np.zeros((len(si.CASES), 2), dtype=np.int32)
    for i, case in enumerate(si.CASES):
        kind, H, W = case[:3]
        if (H, W) != (HS, WS):
            buf[i] = (255 * (np.arange(HS * WS * 3) & 1)).astype(np.uint8).reshape(HS, WS, 3)
        buf[i, :H, :W] = frames[(kind, H, W)]
        sizes[i] = (W, H)
    c = np.stack([si.centre_after_mirror(case) for case in si.CASES])
    s = np.array([case[4] for case in si.CASES], dtype=np.float32)
    params = P.HumanAug.make_params(c.astype(np.float64), s.astype(np.float64), [case[5] for case in si.CASES],
                                    flip=[case[6] for case in si.CASES], gain=np.array([case[7] for case in si.CASES], dtype=np.float64))
    return {'frames': torch.from_numpy(buf).cuda(), 'sizes': torch.from_numpy(sizes).cuda(), 'params': params, 'host': frames}


@pytest.fixture(scope='module')
def stretched(P, batch):
    out4, outf, out8 = P.HumanAug.crop_batch(batch['frames'], batch['params'], res=RES, want_nchw=True, want_u8=True,
                                             sizes=batch['sizes'], stretch=True)
    torch.cuda.synchronize()
    return out4, outf, out8


def _raw(name, frames, sizes, params, fill, res=RES):
    """pa_crop / pa_crop_stretch through ctypes on a workspace of the test's own: exactly the bytes the library asks for, pre-filled
    with `fill`, plus a guard.  Returns (return code, uint8 crops, guard intact?)."""
    from pose_adv_aug_amd._lib import lib, ptr, stream
    B = frames.shape[0]
    need = int((lib().pa_crop_stretch_workspace_bytes if name == 'pa_crop_stretch' else lib().pa_crop_workspace_bytes)(B, HS, WS, res))
    ws = torch.full((need + GUARD,), fill, dtype=torch.uint8, device='cuda')
    ws[need:] = 0xA5
    out8 = torch.full((B, res, res, 3), 77, dtype=torch.uint8, device='cuda')
    rc = getattr(lib(), name)(ptr(frames), HS, WS, ptr(sizes), ptr(params), B, res, ptr(ws), None, None, ptr(out8), stream())
    torch.cuda.synchronize()
    return rc, out8.cpu().numpy(), bool((ws[need:] == 0xA5).all())


def test_stretched_crop_equals_the_reference_crop(stretched):
    """one batch of all sixteen cases against the reference's own output on frames without pure black / white"""
    g = np.load(os.path.join(G, 'crop_stretch.npz'))
    out8 = stretched[2].cpu().numpy()
    for i, case in enumerate(si.CASES):
        sub = g['crop%02d_sub' % i]
        d = np.abs(out8[i][1::4, 2::4].astype(int) - sub.astype(int))
        print('case %2d: worst byte difference %d, fraction of differing bytes %.4f' % (i, int(d.max()), float((d > 0).mean())))
        assert d.max() == 0, (i, case, int(d.max()), float((d > 0).mean()))
        assert _sums(out8[i]) == [int(v) for v in g['crop%02d_sums' % i]], (i, case)
        if i in si.FULL:
            assert np.array_equal(out8[i], g['crop%02d_full' % i]), i


def test_stretched_crop_equals_every_case_of_the_first_fixture(P):
    """crop.npz, all 15 WARP_CASES -- the two without a pure black / white pixel, which the default mode cannot match, included;
    the network layouts are / 255 and bf16 NHWC4 of the same bytes"""
    g = np.load(os.path.join(G, 'crop.npz'))
    cases = inputs.WARP_CASES
    frames = {k: inputs.warp_frame(k) for k in sorted({c[0] for c in cases})}
    c = np.array([k[1] for k in cases], dtype=np.float32)
    flip = np.array([k[4] for k in cases])
    c[:, 0] = np.where(flip == 1, np.float32(1280) - c[:, 0], c[:, 0])
    s = np.array([k[2] for k in cases], dtype=np.float32)
    params = P.HumanAug.make_params(c.astype(np.float64), s.astype(np.float64), [k[3] for k in cases], flip=flip,
                                    gain=np.array([k[5] for k in cases], dtype=np.float64))
    out4, outf, out8 = P.HumanAug.crop_batch(np.stack([frames[k[0]] for k in cases]), params, res=RES, want_nchw=True, want_u8=True,
                                             stretch=True)
    out8 = out8.cpu().numpy()
    assert not all(k[6] for k in cases)
    for i, case in enumerate(cases):
        d = np.abs(out8[i][1::4, 2::4].astype(int) - g['crop%02d_sub' % i].astype(int))
        assert d.max() == 0, (i, case, int(d.max()), float((d > 0).mean()))
        assert _sums(out8[i]) == [int(v) for v in g['crop%02d_sums' % i]], (i, case)
        if 'crop%02d_full' % i in g.files:
            assert np.array_equal(out8[i], g['crop%02d_full' % i])
    ref = torch.from_numpy(out8).float() / 255
    assert torch.equal(outf.cpu(), ref.permute(0, 3, 1, 2))
    o4 = out4.float().cpu()
    assert torch.equal(o4[..., :3], ref.to(torch.bfloat16).float()) and float(o4[..., 3].abs().max()) == 0


def test_batch_independence_and_scratch_hygiene(batch, stretched):
    """the result depends neither on what the workspace held nor on the other samples of the batch, and nothing is written
    behind pa_crop_stretch_workspace_bytes"""
    want = stretched[2].cpu().numpy()
    for fill in (0x00, 0xFF):
        rc, got, guard = _raw('pa_crop_stretch', batch['frames'], batch['sizes'], batch['params'], fill)
        assert rc == 0 and guard, (fill, rc, guard)
        assert np.array_equal(got, want), fill
    for i in range(len(si.CASES)):
        rc, one, guard = _raw('pa_crop_stretch', batch['frames'][i:i + 1].contiguous(), batch['sizes'][i:i + 1].contiguous(),
                              batch['params'][i:i + 1].contiguous(), 0xFF if i & 1 else 0x00)
        assert rc == 0 and guard, i
        assert np.array_equal(one[0], want[i]), (i, si.CASES[i])


def test_default_mode_is_unchanged(P, batch):
    from oracle import crop as oc
    a = P.HumanAug.crop_batch(batch['frames'], batch['params'], res=RES, want_nchw=True, want_u8=True, sizes=batch['sizes'], stretch=False)
    b = P.HumanAug.crop_batch(batch['frames'], batch['params'], res=RES, want_nchw=True, want_u8=True, sizes=batch['sizes'])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    got = a[2].cpu().numpy()
    for i in (0, 2, 6):
        kind, H, W, _, s0, r0, flip, gain = si.CASES[i]
        ref = oc.crop(oc.source_image(batch['host'][(kind, H, W)], bool(flip), gain), si.centre_after_mirror(si.CASES[i]), np.float32(s0), r0,
                      RES, 200, quirk=False)
        assert np.array_equal(got[i], ref), i


def test_window_wholly_outside_the_frame(P):
    """the reference and the oracle raise there, so the device defines it: zeros, as pa_crop gives"""
    from oracle import crop as oc
    f = si.frame('soft')
    frames = torch.from_numpy(np.stack([f, f])).cuda()
    params = P.HumanAug.make_params(np.array([[-900.0, -900.0], [-900.0, -900.0]]), [1.0, 3.0], [0.0, 20.0])
    with pytest.raises(ValueError):
        oc.crop(oc.source_image(f), np.array([-900.0, -900.0], dtype=np.float32), np.float32(1.0), 0.0, RES, 200, quirk=True)
    rc, got, guard = _raw('pa_crop_stretch', frames, None, params, 0xFF)
    assert rc == 0 and guard
    assert got.shape == (2, RES, RES, 3) and not got.any()
    rc0, plain, _ = _raw('pa_crop', frames, None, params, 0xFF)
    assert rc0 == 0 and np.array_equal(plain, got)


def test_loops_crop_with_the_stretch(P):
    """the benchmark's synthetic people under the regular law with Augmenter(stretch=True): every crop equals
    oracle.crop_frame(quirk=True) byte for byte, and AugmentAhead hands over the same data"""
    from oracle import crop as oc
    from pose_adv_aug_amd.data import AugmentAhead, Augmenter, DeviceBatch
    b = DeviceBatch.synthetic(24, seed=3)
    data = Augmenter(seed=11, stretch=True).regular(b, want_nchw=True)
    p = b.params.cpu().numpy()
    assert ((p[:, 2] * 200 / 256) >= 2).any() and ((p[:, 2] * 200 / 256) < 2).any() and (p[:, 3] != 0).any()
    frames = b.frames.cpu().numpy()
    imgf = data['img'].cpu().numpy()
    for i in range(24):
        ref = oc.crop_frame(frames[i], p[i, 0:2], p[i, 2], p[i, 3], 256, flip=bool(p[i, 4]), gain=p[i, 5:8], quirk=True)
        d = np.abs(imgf[i] - ref)
        assert d.max() == 0, (i, p[i], float(d.max()) * 255, float((d > 0).mean()))
    ahead = AugmentAhead(Augmenter(seed=11, stretch=True))
    ahead.start(b)
    data2 = ahead.take()
    torch.cuda.synchronize()
    assert np.array_equal(b.params.cpu().numpy(), p)
    assert torch.equal(data2['img4'], data['img4'])
    assert torch.equal(data2['pts'], data['pts'])


def test_reference_signature_crop_with_the_stretch(P):
    from oracle import crop as oc
    case = si.CASES[1]
    f = si.frame('soft')
    cr = P.HumanAug.crop(f.astype(np.float64) / 255.0, list(case[3]), np.float32(case[4]), case[5], 256, 200, stretch=True)
    ref = oc.crop(oc.source_image(f), np.array(case[3], dtype=np.float32), np.float32(case[4]), case[5], 256, 200, quirk=True)
    assert cr.shape == (256, 256, 3) and cr.dtype == np.uint8 and np.array_equal(cr, ref)

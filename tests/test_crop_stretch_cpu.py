"""The stretch mode's fixture on the CPU: tests/golden/crop_stretch.npz holds outputs of the REFERENCE's own crop (made by
tests/golden/make_crop_stretch_goldens.py over the real Pillow) on frames without a pure black / white pixel;
oracle.crop(quirk=True) -- the specification of pa_crop_stretch -- must reproduce every array of it, and every case must
keep telling the two modes apart."""
import os

import numpy as np
import pytest

from tests import stretch_inputs as si

G = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def crops():
    """per case: (oracle crop with the stretch, oracle crop without)"""
    from oracle import crop as oc
    frames = si.frames()
    out = []
    for case in si.CASES:
        kind, H, W, _, s0, r0, flip, gain = case
        src = oc.source_image(frames[(kind, H, W)], bool(flip), gain)
        c = si.centre_after_mirror(case)
        out.append(tuple(oc.crop(src, c, np.float32(s0), r0, 256, 200, quirk=q) for q in (True, False)))
    return out


def test_oracle_with_the_quirk_equals_the_reference_crop(crops):
    """Bound asserted: every stored byte and sum equal."""
    g = np.load(os.path.join(G, 'crop_stretch.npz'))
    assert os.path.getsize(os.path.join(G, 'crop_stretch.npz')) < os.path.getsize(os.path.join(G, 'crop.npz'))
    for i, (on, _) in enumerate(crops):
        assert on.shape == (256, 256, 3) and on.dtype == np.uint8
        assert np.array_equal(on[1::4, 2::4], g['crop%02d_sub' % i]), (i, si.CASES[i])
        sums = [int(on[..., k].astype(np.int64).sum()) for k in range(3)] + [int((on[..., k].astype(np.int64) ** 2).sum()) for k in range(3)]
        assert sums == [int(v) for v in g['crop%02d_sums' % i]], (i, si.CASES[i])
        if i in si.FULL:
            assert np.array_equal(on, g['crop%02d_full' % i]), i
    assert all('crop%02d_full' % i in g.files for i in si.FULL)


def test_every_case_tells_the_two_modes_apart(crops):
    """the stretched crop differs from the unstretched one in at least a quarter of its bytes, in every case"""
    for i, (on, off) in enumerate(crops):
        frac = float((on != off).mean())
        print('case %2d: %.3f of the bytes differ, by up to %d' % (i, frac, int(np.abs(on.astype(int) - off.astype(int)).max())))
        assert frac >= 0.25, (i, si.CASES[i], frac)


def test_crop_stretch_option(tmp_path):
    """--crop_stretch: an int, off by default, written to opt.txt like every other option"""
    from pose_adv_aug_amd.options.train_options import TrainOptions
    opt = TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'd'])
    assert opt.crop_stretch == 0
    opt = TrainOptions().parse(['--exp_dir', str(tmp_path), '--exp_id', 'e', '--crop_stretch', '1'])
    assert opt.crop_stretch == 1
    assert 'crop_stretch: 1\n' in open(os.path.join(str(tmp_path), 'e', 'opt.txt')).read()
    assert 'crop_stretch: 0\n' in open(os.path.join(str(tmp_path), 'd', 'opt.txt')).read()


def test_augmenter_and_crop_take_the_mode():
    import inspect
    from pose_adv_aug_amd.data import Augmenter
    from pose_adv_aug_amd.pylib import HumanAug
    assert Augmenter(seed=1).stretch is False and Augmenter(seed=1, inp_res=256, out_res=64, stretch=True).stretch is True
    for fn in (HumanAug.crop_batch, HumanAug.crop, HumanAug._crop_workspace):
        assert inspect.signature(fn).parameters['stretch'].default is False

#!/usr/bin/env python3
"""Generate tests/golden/crop_stretch.npz by running THE REFERENCE's own crop() (pylib/HumanAug.py:117-176) behind its own
pre-processing (data/mpii_for_mpii.py:114-135), exactly as make_goldens.py:gen_crop does, on the frames and cases of
tests/stretch_inputs.py: frames without a pure black / white pixel, where scipy's toimage() min/max byte stretch is at work.
Run from the repo root:  python tests/golden/make_crop_stretch_goldens.py

The transliteration of the reference, the scipy.misc shim over the real Pillow and the import are make_goldens.py's.  Only
arrays are written.  Stored per case, as in crop.npz: every 4th pixel of the crop (rows 1::4, columns 2::4), per-channel
byte sums and sums of squares of the full crop, and the full crop for the cases of stretch_inputs.FULL."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, TMP, install_scipy_misc_shim, load_ref, transliterate  # noqa: E402,F401


def gen_crop_stretch(R):
    from tests import stretch_inputs as si
    sys.path.insert(0, TMP)
    from utils import imutils
    HumanAug = R['HumanAug']
    out = {}
    frames = si.frames()
    for i, (kind, H, W, c0, s0, r0, flip, gain) in enumerate(si.CASES):
        img = imutils.im_to_torch(frames[(kind, H, W)].copy())           # load_image: uint8 HWC -> fp32 CHW / 255
        c = torch.Tensor(list(c0))
        s = torch.Tensor([s0])
        if flip:
            img = torch.from_numpy(HumanAug.fliplr(img.numpy())).float()
            c[0] = img.size(2) - c[0]
        for k in range(3):
            img[k, :, :].mul_(gain[k]).clamp_(0, 1)
        inp = HumanAug.crop(imutils.im_to_numpy(img), c.numpy(), s.numpy(), r0, 256, 200)
        assert inp.dtype == np.uint8 and inp.shape == (256, 256, 3)
        out['crop%02d_sub' % i] = inp[1::4, 2::4].copy()
        out['crop%02d_sums' % i] = np.array([inp[..., k].astype(np.int64).sum() for k in range(3)]
                                            + [(inp[..., k].astype(np.int64) ** 2).sum() for k in range(3)])
        if i in si.FULL:
            out['crop%02d_full' % i] = inp
    out['frame_sums'] = np.array([[int(frames[k].astype(np.int64).sum())] for k in sorted(frames)])
    path = os.path.join(OUT, 'crop_stretch.npz')
    np.savez_compressed(path, **out)
    print('crop_stretch.npz', len(out), 'arrays', os.path.getsize(path) // 1024, 'KB')


if __name__ == '__main__':
    gen_crop_stretch(load_ref())

"""JPEG files for the decode tests, written at test time by the installed Pillow (which is also the reference decoder), and the
host stage of the decode through the library.  Not collected as a test."""
import io

import numpy as np
from PIL import Image

SIZES = [(64, 48), (83, 61), (17, 33), (33, 18), (130, 95), (16, 16), (9, 7)]          # (width, height)
CONTENTS = ['smooth', 'noise', 'checker']
SAMPLINGS = [0, 1, 2, 'gray']                                                          # Pillow's subsampling= 4:4:4, 4:2:2, 4:2:0
ENCODINGS = [(90, False, 0), (35, True, 0), (100, False, 3), (75, False, 1)]           # (quality, optimize, restart_marker_blocks)


def picture(content, w, h, seed=0):
    g = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if content == 'smooth':
        a = np.stack([128 + 100 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0), 128 + 110 * np.cos(xx / 13.0 - yy / 5.0),
                      255.0 * (xx + yy) / max(1, w + h - 2)], axis=2)
    elif content == 'noise':
        a = g.integers(0, 256, (h, w, 3)).astype(np.float64)
    else:
        c = ((xx // 3 + yy // 2) % 2) * 255.0
        a = np.stack([c, 255 - c, np.roll(c, 1, axis=1)], axis=2)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(arr, sampling, quality=90, optimize=False, restart=0, **kw):
    im = Image.fromarray(arr[:, :, 1]) if sampling == 'gray' else Image.fromarray(arr)
    buf = io.BytesIO()
    if sampling != 'gray':
        kw['subsampling'] = sampling
    if restart:
        kw['restart_marker_blocks'] = restart
    im.save(buf, format='JPEG', quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def host_decode(data, slack=0):
    """-> (rc, desc, coef) through pa_jpeg_info_host (for the buffer size) and pa_jpeg_entropy_host"""
    from pose_adv_aug_amd.pylib import Jpeg
    rc, info = Jpeg.jpeg_info(data)
    if rc:
        return rc, info, None
    coef = np.full(info.total_elems + slack, 0x7ABC, dtype=np.int16)
    rc, desc = Jpeg.jpeg_entropy(data, coef, capacity=info.total_elems)
    return rc, desc, coef

"""Frames and cases for the stretch mode of the crop (pa_crop_stretch, tests/golden/crop_stretch.npz): frames WITHOUT the
painted black / white squares of tests/inputs.py:warp_frame, so that scipy's toimage() min/max byte stretch is never the
identity -- what real photographs look like after an antialiased downscale."""
import numpy as np


def frame(kind, H=720, W=1280):
    """uint8 H x W x 3: 'soft' (the 'smooth' formula of inputs.warp_frame, no squares, clipped to [24, 231]), 'mid' (uniform
    bytes in [16, 240)), 'flat' (the constant 97: cmax == cmin)."""
    if kind == 'soft':
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        ch = [127.5 + 100 * np.sin(xx / (37.0 + 11 * k) + 0.3 * k) * np.cos(yy / (29.0 + 7 * k)) + 20 * np.sin((xx + yy) / 9.0 + k)
              for k in range(3)]
        return np.clip(np.rint(np.stack(ch, -1)), 24, 231).astype(np.uint8)
    if kind == 'mid':
        return np.random.default_rng(5).integers(16, 240, (H, W, 3), np.uint8)
    if kind == 'flat':
        return np.full((H, W, 3), 97, dtype=np.uint8)
    raise ValueError(kind)


# (frame kind, H, W, centre BEFORE the mirror, scale (final, fp32), rotation deg, flip, colour gains)
CASES = [
    ('soft', 720, 1280, (640.0, 360.0), 2.0, 0.0, 0, (1.0, 1.0, 1.0)),         # window stretch only
    ('soft', 720, 1280, (655.3, 371.8), 2.013, 25.0, 0, (1.0, 1.0, 1.0)),      # stretch over the padded window
    ('soft', 720, 1280, (629.5, 350.2), 3.47, 0.0, 0, (1.0, 1.0, 1.0)),        # frame stretch in fp32, then window stretch
    ('soft', 720, 1280, (651.0, 349.0), 3.1, 58.0, 1, (1.4, 0.6, 1.1)),        # clamp reaches 1
    ('mid', 720, 1280, (632.0, 352.0), 2.55, 0.0, 1, (0.7, 1.0, 0.9)),         # just below the downscale threshold
    ('mid', 720, 1280, (633.1, 366.6), 5.7, 33.0, 0, (0.8, 0.9, 0.7)),         # strong downscale with rotation
    ('soft', 720, 1280, (110.5, 90.25), 2.2, 12.0, 0, (1.0, 1.0, 1.0)),        # zero fill sets the minimum
    ('soft', 720, 1280, (60.0, 40.0), 3.3, 0.0, 0, (1.0, 1.0, 1.0)),           # pre-downscale and window outside the frame
    ('flat', 720, 1280, (640.0, 360.0), 1.5, 0.0, 0, (1.0, 1.0, 1.0)),         # cscale == 0: the reference gives an all-zero crop
    ('flat', 720, 1280, (640.0, 360.0), 3.0, -15.0, 0, (1.0, 1.0, 1.0)),       # cscale == 0 in the frame stretch
    ('soft', 375, 500, (260.5, 180.25), 2.9, 0.0, 0, (1.1, 0.8, 1.0)),         # a sized frame
    ('soft', 720, 1280, (640.0, 360.0), 1.2, -40.0, 0, (1.0, 1.0, 1.0)),       # upscale with rotation
    ('soft', 720, 1280, (640.0, 360.0), 2.0, 360.0, 0, (1.0, 1.0, 1.0)),       # padded, copied, un-padded
    ('soft', 720, 1280, (640.0, 360.0), 2.0, 180.0, 0, (0.9, 1.0, 1.0)),       # 180 degree path
    ('soft', 720, 1280, (640.0, 360.0), 2.0, 90.0, 0, (1.0, 1.0, 1.0)),        # 90 degree path
    ('mid', 720, 1280, (640.0, 360.0), 2.5625, 0.0, 0, (0.75, 0.75, 0.75)),    # scale factor 2.002, just above the threshold
]
FULL = (1, 5)          # cases whose whole crop is stored


def frames():
    """{(kind, H, W): frame} of every frame CASES uses"""
    return {k: frame(*k) for k in sorted({(c[0], c[1], c[2]) for c in CASES})}


def centre_after_mirror(case):
    """the centre crop() is handed: the caller mirrors it about the frame's own width (data/mpii_for_mpii.py:129), in fp32"""
    c = np.array(case[3], dtype=np.float32)
    if case[6]:
        c[0] = np.float32(case[2]) - c[0]
    return c

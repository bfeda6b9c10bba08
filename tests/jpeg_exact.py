"""The device half of the JPEG decode (include/poseadv.h: pa_jpeg_decode) restated in numpy: from the coefficient buffer and the
descriptor that pa_jpeg_entropy_host fills to the RGB image, in libjpeg's integer arithmetic (jidctint.c jpeg_idct_islow, jdsample.c
h2v1 / h2v2 "fancy" upsampling, jdcolor.c ycc_rgb_convert, the range-limit table of jdmaster.c).  Pillow decodes with libjpeg-turbo,
whose results are bit-identical to that definition, so  decode_rgb(coef, desc) == np.asarray(Image.open(f).convert('RGB')).

It serves two checks: the host entropy decoder against Pillow on a machine without a GPU (tests/test_jpeg_host_cpu.py), and the
device kernels against a second reference that shares the coefficients with them, which tells a kernel fault from an entropy-stage
fault (tests/test_gpu_jpeg.py).  Not collected as a test; nothing in pose_adv_aug_amd/ imports it.

All values are int32 with arithmetic right shifts (numpy's >> on signed integers)."""
import numpy as np


def _fix(x):
    return int(x * 8192 + 0.5)


F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = _fix(0.298631336), _fix(0.390180644), _fix(0.541196100), _fix(0.765366865)
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = _fix(0.899976223), _fix(1.175875602), _fix(1.501321110), _fix(1.847759065)
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = _fix(1.961570560), _fix(2.053119869), _fix(2.562915447), _fix(3.072711026)


def _idct_1d(x, shift):
    """x: list of eight int32 arrays (inputs 0..7 of one pass) -> list of the eight outputs, descaled by `shift`."""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    z1 = (x2 + x6) * F_0_541196100
    tmp2 = z1 - x6 * F_1_847759065
    tmp3 = z1 + x2 * F_0_765366865
    tmp0 = (x0 + x4) << 13
    tmp1 = (x0 - x4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1 = t0 + t3
    z2 = t1 + t2
    z3 = t0 + t2
    z4 = t1 + t3
    z5 = (z3 + z4) * F_1_175875602
    t0 = t0 * F_0_298631336
    t1 = t1 * F_2_053119869
    t2 = t2 * F_3_072711026
    t3 = t3 * F_1_501321110
    z1 = z1 * (-F_0_899976223)
    z2 = z2 * (-F_2_562915447)
    z3 = z3 * (-F_1_961570560) + z5
    z4 = z4 * (-F_0_390180644) + z5
    t0 = t0 + z1 + z3
    t1 = t1 + z2 + z4
    t2 = t2 + z2 + z3
    t3 = t3 + z1 + z4
    r = np.int32(1 << (shift - 1))
    outs = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return [(o + r) >> shift for o in outs]


def range_limit(v):
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.int32)


def idct_blocks(blocks, quant):
    """blocks: int16 [N][64] natural order, quant: [64] natural order -> uint8-valued int32 [N][8][8] (row, column)."""
    with np.errstate(over='ignore'):
        w = (blocks.astype(np.int32) * np.asarray(quant, dtype=np.int32)[None, :]).reshape(-1, 8, 8)
        cols = _idct_1d([w[:, k, :] for k in range(8)], 11)            # column pass: input k = row k of every column
        w = np.stack(cols, axis=1)
        rows = _idct_1d([w[:, :, k] for k in range(8)], 18)            # row pass: input k = column k of every row
        return range_limit(np.stack(rows, axis=2))


def component_planes(coef, desc):
    """The uint8 component planes over the MCU-padded block grids (stage (a) of the device decode)."""
    planes = []
    for c in range(desc.ncomp):
        cd = desc.comp[c]
        n = cd.bw * cd.bh
        blocks = np.asarray(coef[cd.offset:cd.offset + n * 64], dtype=np.int16).reshape(n, 64)
        px = idct_blocks(blocks, np.asarray(desc.quant[c][:], dtype=np.int32))
        planes.append(px.reshape(cd.bh, cd.bw, 8, 8).transpose(0, 2, 1, 3).reshape(cd.bh * 8, cd.bw * 8))
    return planes


def _upsample_h2v1(p):
    """p: int32 [dh][dw] -> [dh][2 dw]"""
    prev = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    even = (3 * p + prev + 1) >> 2
    odd = (3 * p + nxt + 2) >> 2
    even[:, 0] = p[:, 0]
    odd[:, -1] = p[:, -1]
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int32)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out


def _upsample_h2v2(p):
    """p: int32 [dh][dw] -> [2 dh][2 dw]"""
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), dtype=np.int32)
    for first, other in ((0, up), (1, down)):
        cs = 3 * p + other
        prev = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        even = (3 * cs + prev + 8) >> 4
        odd = (3 * cs + nxt + 7) >> 4
        even[:, 0] = (4 * cs[:, 0] + 8) >> 4
        odd[:, -1] = (4 * cs[:, -1] + 7) >> 4
        out[first::2, 0::2], out[first::2, 1::2] = even, odd
    return out


def _fx(x):
    return int(x * 65536 + 0.5)


def decode_rgb(coef, desc):
    """coef: int16 array holding the image's coefficients from element 0; desc: the pa_jpeg_desc of the same image -> uint8 [H][W][3]."""
    W, H = desc.width, desc.height
    planes = component_planes(coef, desc)
    if desc.ncomp == 1:
        y = planes[0][:H, :W]
        return np.stack([y, y, y], axis=2).astype(np.uint8)
    hmax, vmax = desc.comp[0].h, desc.comp[0].v
    y = planes[0][:H, :W]
    chroma = []
    for c in (1, 2):
        dw, dh = -(-W * desc.comp[c].h // hmax), -(-H * desc.comp[c].v // vmax)
        p = planes[c][:dh, :dw].astype(np.int32)                      # neighbours replicate at the edge of THIS region
        if (hmax, vmax) == (2, 1):
            p = _upsample_h2v1(p)
        elif (hmax, vmax) == (2, 2):
            p = _upsample_h2v2(p)
        else:
            assert (hmax, vmax) == (1, 1), (hmax, vmax)
        chroma.append(p[:H, :W] - 128)
    cb, cr = chroma
    r = y + ((_fx(1.40200) * cr + 32768) >> 16)
    g = y + ((-_fx(0.34414) * cb + 32768 - _fx(0.71414) * cr) >> 16)
    b = y + ((_fx(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)

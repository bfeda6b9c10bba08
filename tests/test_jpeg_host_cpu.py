"""The host half of the JPEG decode (pa_jpeg_info_host / pa_jpeg_entropy_host, include/poseadv.h) without a GPU: the coefficients
it produces, pushed through the numpy restatement of the device arithmetic (tests/jpeg_exact.py), equal Pillow's
Image.open(f).convert('RGB') byte for byte; files outside the supported set get PA_JPEG_UNSUPPORTED and nothing else; damaged input
gets an error code, never a crash or a write outside the coefficient buffer; the decoder is re-entrant.

Every JPEG is written at test time by the Pillow installed beside the test, which is also the reference decoder."""
import io
import threading

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_exact
from tests.jpeg_files import SIZES, CONTENTS, SAMPLINGS, ENCODINGS, picture, encode, pillow_rgb, host_decode


def same_desc(a, b):
    return bytes(a) == bytes(b)


@pytest.mark.parametrize('sampling', SAMPLINGS, ids=lambda s: 'sub%s' % s)
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_entropy_decode_then_restated_arithmetic_equals_pillow(size, content, sampling):
    """the 7 sizes x 3 contents x 4 samplings x 4 encodings = 336 cases, four encodings per parametrised case"""
    from pose_adv_aug_amd.pylib import Jpeg
    w, h = size
    arr = picture(content, w, h, seed=w + h)
    for quality, optimize, restart in ENCODINGS:
        data = encode(arr, sampling, quality, optimize, restart)
        rc, desc, coef = host_decode(data, slack=64)
        assert rc == 0, (quality, optimize, restart, rc, Jpeg.last_error())
        assert (desc.width, desc.height) == (w, h) and desc.ncomp == (1 if sampling == 'gray' else 3)
        assert desc.restart_interval == restart                                     # Pillow's "blocks" are MCUs
        assert (coef[desc.total_elems:] == 0x7ABC).all(), 'wrote behind the coefficients'
        want = pillow_rgb(data)
        got = jpeg_exact.decode_rgb(coef, desc)
        assert got.shape == want.shape and np.array_equal(got, want), (quality, optimize, restart, int(np.abs(got.astype(int) - want).max()))


def test_header_only_parse_agrees_with_pillow_and_the_full_decode():
    from pose_adv_aug_amd.pylib import Jpeg
    for k, (w, h) in enumerate(SIZES):
        for sampling in SAMPLINGS:
            data = encode(picture('smooth', w, h, k), sampling, 80, False, 2 if k % 2 else 0)
            rc, info = Jpeg.jpeg_info(data)
            assert rc == 0, Jpeg.last_error()
            assert (info.width, info.height) == Image.open(io.BytesIO(data)).size
            rc2, desc, coef = host_decode(data)
            assert rc2 == 0 and same_desc(info, desc)
            # the documented layout: planes back to back, MCU-padded grids
            hs, vs = (1, 1) if sampling == 'gray' else {0: (1, 1), 1: (2, 1), 2: (2, 2)}[sampling]
            mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
            off = 0
            for c in range(info.ncomp):
                cd = info.comp[c]
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                assert (cd.h, cd.v, cd.bw, cd.bh, cd.offset) == (ch, cv, mw * ch, mh * cv, off)
                off += cd.bw * cd.bh * 64
            assert info.total_elems == off
            # quantisation tables per component, natural order, as Pillow reports them
            q = Image.open(io.BytesIO(data)).quantization
            zig = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
            for c in range(info.ncomp):
                tab = q[0 if c == 0 else 1]
                assert sorted(tab) == sorted(info.quant[c][:])
                nat = [0] * 64
                for i in range(64):
                    nat[zig[i]] = tab[i]
                # Pillow hands the table out in zigzag or in natural order depending on its version: one of the two
                assert list(info.quant[c][:]) in (nat, list(tab))


def _sof_sampling_patched(data, hv):
    """the same file with the luma sampling byte of its frame header replaced (its scan no longer matches: header checks only)"""
    at = data.index(b'\xff\xc0')
    assert data[at + 9] == 3 and data[at + 10] == 1            # three components, the first has id 1
    return data[:at + 11] + bytes([hv]) + data[at + 12:]


def test_files_outside_the_supported_set_return_unsupported_and_nothing_else():
    from pose_adv_aug_amd.pylib import Jpeg
    arr = picture('smooth', 64, 48)
    cases = {'progressive': encode(arr, 2, progressive=True), 'narrow 4:2:0': encode(picture('noise', 4, 16), 2),
             'narrow 4:2:2': encode(picture('noise', 3, 9), 1)}
    buf = io.BytesIO()
    Image.fromarray(arr).convert('CMYK').save(buf, format='JPEG', quality=90)
    cases['cmyk'] = buf.getvalue()
    try:                                                          # Pillow >= 10.2; older versions leave this sub-case out
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format='JPEG', quality=90, keep_rgb=True)
        if Image.open(io.BytesIO(buf.getvalue())).mode == 'RGB' and b'JFIF' not in buf.getvalue()[:32]:
            cases['rgb'] = buf.getvalue()
    except (TypeError, ValueError, OSError):
        pass
    for name, data in cases.items():
        assert pillow_rgb(data).shape[2] == 3, name               # a good file for Pillow
    # 4:1:1 and 4:4:0: the installed Pillow (12.2) writes neither -- subsampling='4:1:1' is its legacy name for 4:2:0 and '4:4:0' is
    # refused -- so these two sub-cases are not written by Pillow; the frame header of a 4:2:2 file is patched instead, which is all
    # the sampling check reads (Pillow cannot decode the patched files, so they are not compared with it)
    base = encode(arr, 1)
    cases['4:1:1'] = _sof_sampling_patched(base, 0x41)
    cases['4:4:0'] = _sof_sampling_patched(base, 0x12)
    for name, data in cases.items():
        rc, _ = Jpeg.jpeg_info(data)
        assert rc == Jpeg.PA_JPEG_UNSUPPORTED, (name, rc, Jpeg.last_error())
        coef = np.zeros(1 << 16, dtype=np.int16)
        rc, desc = Jpeg.jpeg_entropy(data, coef)
        assert rc == Jpeg.PA_JPEG_UNSUPPORTED, (name, rc, Jpeg.last_error())
        assert not coef.any(), name


def test_restart_marker_behind_a_long_last_symbol_is_found():
    """The bit reader refills lazily, so at the end of a restart interval it may hold fewer than 8 padding bits without having met
    the marker yet (32 - 39 bits before the interval's last symbol, a 16-bit code with a large value): quality-100 files of a
    1-pixel checkerboard plus noise with a marker after every MCU hit that often.  Every one decodes, and equals Pillow."""
    from pose_adv_aug_amd.pylib import Jpeg
    yy, xx = np.mgrid[0:64, 0:64]
    for seed in range(60):
        g = np.random.default_rng(500 + seed)
        a = np.clip(((xx + yy) % 2) * 255 + g.integers(-40, 41, (64, 64)), 0, 255).astype(np.uint8)
        arr = np.stack([a, a, a], axis=2)
        for sampling in ('gray', 2):
            data = encode(arr, sampling, 100, False, 1)
            rc, desc, coef = host_decode(data)
            assert rc == 0, (seed, sampling, rc, Jpeg.last_error())
            assert np.array_equal(jpeg_exact.decode_rgb(coef, desc), pillow_rgb(data)), (seed, sampling)


def test_damaged_input_and_short_buffers_are_refused_without_a_crash():
    from pose_adv_aug_amd.pylib import Jpeg
    g = np.random.default_rng(77)
    for data in (encode(picture('noise', 33, 18), 2, 90, False, 1), encode(picture('smooth', 17, 33), 1, 60, True, 0)):
        rc, info = Jpeg.jpeg_info(data)
        assert rc == 0
        need = info.total_elems
        CANARY = 0x5A5A
        buf = np.full(need + 256, CANARY, dtype=np.int16)

        def run(blob, capacity=need):
            rc, desc = Jpeg.jpeg_entropy(blob, buf, capacity=capacity)
            assert (buf[capacity:] == CANARY).all(), 'wrote past capacity_elems'
            return rc
        for n in range(len(data) + 1):
            rc_i, _ = Jpeg.jpeg_info(data[:n])
            rc = run(data[:n])
            assert isinstance(rc, int) and isinstance(rc_i, int)
            if n < len(data) // 2:
                assert rc != 0, n
        assert run(data) == 0
        for _ in range(200):
            pos, val = int(g.integers(0, len(data))), int(g.integers(0, 256))
            blob = bytearray(data)
            blob[pos] = val
            rc = run(bytes(blob))
            assert isinstance(rc, int)
            if rc == 0:                                           # still decodable: the descriptor must fit the buffer it was given
                _, d2 = Jpeg.jpeg_info(bytes(blob))
                assert d2.total_elems <= need
        buf[:] = CANARY
        rc = run(data, capacity=need - 1)
        assert (buf == CANARY).all()                              # the refused call wrote nothing
        assert rc == Jpeg.PA_JPEG_CAPACITY and 'do not fit' in Jpeg.last_error()


def test_a_truncated_scan_is_an_error_not_a_silent_grey_image():
    from pose_adv_aug_amd.pylib import Jpeg
    data = encode(picture('noise', 64, 48), 2, 90)
    rc, desc, coef = host_decode(data[:len(data) * 2 // 3])
    assert rc == Jpeg.PA_JPEG_CORRUPT and 'ends early' in Jpeg.last_error()


def test_eight_threads_decode_concurrently_with_serial_results():
    files = [encode(picture(CONTENTS[k % 3], *SIZES[k % 7], seed=k), SAMPLINGS[k % 4], 70 + 3 * k, k % 2 == 0, k % 3) for k in range(8)]
    serial = [host_decode(f) for f in files]
    assert all(rc == 0 for rc, _, _ in serial)
    errors = []

    def work(k):
        try:
            for _ in range(20):
                rc, desc, coef = host_decode(files[k])
                if rc != 0 or not same_desc(desc, serial[k][1]) or not np.array_equal(coef, serial[k][2]):
                    errors.append(k)
        except Exception as e:                                    # noqa: BLE001 (reported through the list)
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors

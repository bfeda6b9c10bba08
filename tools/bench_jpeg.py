#!/usr/bin/env python3
"""The two halves of the device JPEG decode, timed on their own (profiles/jpeg_device_decode.txt).

    python tools/bench_jpeg.py host            # CPU only: pa_jpeg_entropy_host against Pillow's full decode, same process, same thread
    python tools/bench_jpeg.py device [reps]   # GPU: pa_jpeg_decode for B = 24 at 1280x720, 4:2:0, HIP events around the call, cold

The test frame is blurred noise (170-440 KB at quality 75-95): an assumption about MPII-like content, not MPII itself."""
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def frame_jpeg(quality, seed=0, w=1280, h=720, subsampling=2):
    from PIL import Image, ImageFilter
    g = np.random.default_rng(seed)
    im = Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).filter(ImageFilter.GaussianBlur(1.2))
    buf = io.BytesIO()
    im.save(buf, format='JPEG', quality=quality, subsampling=subsampling)
    return buf.getvalue()


def best_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def host(reps=15):
    from PIL import Image
    from pose_adv_aug_amd.pylib import Jpeg
    print('host entropy stage against Pillow\'s full decode, 1280x720 4:2:0, one thread, best / median of %d (ms per image)' % reps)
    for q in (75, 90, 95):
        data = frame_jpeg(q)
        rc, info = Jpeg.jpeg_info(data)
        assert rc == 0
        coef = np.zeros(info.total_elems, dtype=np.int16)

        def pil():
            np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))

        def ent():
            assert Jpeg.jpeg_entropy(data, coef)[0] == 0
        p, e = best_ms(pil, reps), best_ms(ent, reps)
        print('quality %2d  %4d KB  Pillow %6.2f / %6.2f   pa_jpeg_entropy_host %6.2f / %6.2f   ratio %.2f (best), %.2f (median)'
              % (q, len(data) // 1024, p[0], p[1], e[0], e[1], e[0] / p[0], e[1] / p[1]))


def device(reps=10):
    import torch
    from pose_adv_aug_amd.pylib import Jpeg
    B, Hs, Ws = 24, 720, 1280
    files = [frame_jpeg(90, seed=k) for k in range(4)]
    coefs, descs = [], []
    for k in range(B):
        data = files[k % len(files)]
        rc, info = Jpeg.jpeg_info(data)
        c = np.zeros(info.total_elems, dtype=np.int16)
        rc, d = Jpeg.jpeg_entropy(data, c)
        assert rc == 0
        coefs.append(c)
        descs.append(bytes(d))
    base = np.concatenate([[0], np.cumsum([c.size for c in coefs])]).astype(np.int64)
    coef = torch.from_numpy(np.concatenate(coefs)).cuda()
    ddesc = torch.from_numpy(np.frombuffer(b''.join(descs), dtype=np.uint8).copy()).cuda()
    dbase = torch.from_numpy(base[:-1].copy()).cuda()
    flush = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')          # other traffic between repetitions: caches hold none of the operands
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cold, warm = [], []
    for r in range(reps + 2):
        flush.add_(1)
        e0.record()
        frames, sizes = Jpeg.jpeg_decode_batch(coef, ddesc, dbase, Hs, Ws)
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            cold.append(e0.elapsed_time(e1) * 1e3)
        del frames
    for r in range(reps):
        e0.record()
        frames, sizes = Jpeg.jpeg_decode_batch(coef, ddesc, dbase, Hs, Ws)
        e1.record()
        torch.cuda.synchronize()
        warm.append(e0.elapsed_time(e1) * 1e3)
        del frames
    from PIL import Image
    frames, sizes = Jpeg.jpeg_decode_batch(coef, ddesc, dbase, Hs, Ws)
    ok = all(np.array_equal(frames[k].cpu().numpy(), np.asarray(Image.open(io.BytesIO(files[k % 4])).convert('RGB'))) for k in range(4))
    nbytes = coef.numel() * 2 + 2 * int(coef.numel()) + B * Hs * Ws * 3       # coefficients read + planes written and read + frames written
    print('pa_jpeg_decode B=%d %dx%d 4:2:0 (two launches, HIP events around the call; equals Pillow: %s)' % (B, Ws, Hs, ok))
    print('  cold (1 GiB of other traffic between repetitions): median %.1f us, min %.1f, max %.1f over %d' % (np.median(cold), min(cold), max(cold), len(cold)))
    print('  back to back:                                      median %.1f us, min %.1f' % (np.median(warm), min(warm)))
    print('  bytes moved: %.1f MB per batch, %.2f MB per image -> %.2f TB/s at the cold median' % (nbytes / 1e6, nbytes / 1e6 / B, nbytes / np.median(cold) / 1e6))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'host'
    if what == 'host':
        host()
    else:
        device(int(sys.argv[2]) if len(sys.argv) > 2 else 10)

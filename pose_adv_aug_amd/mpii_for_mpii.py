"""data/mpii_for_mpii.py of the reference as a feeder of `DeviceBatch`es.

The reference's `MPII(data.Dataset)` loads ONE annotated person per item: JSON record -> JPEG -> host augmentation ->
crop (data/mpii_for_mpii.py:83-163) in DataLoader worker processes.  Here the host only parses the JSON and decodes the
images (PIL, a thread pool); the frames of a batch are copied, top-left aligned, into one padded uint8 buffer on the
device together with their own (width, height), and everything from the MPII pre-normalisation on -- law, flip, colour,
crop, joint transform, heat maps -- happens in the device kernels (data.Augmenter).

JSON record fields used (data/mpii_for_mpii.py:29-47, 86-104):
  dataset ('MPII'), isValidation, img_paths, joint_self [16][3], objpos [2], scale_provided, normalizer."""
import json
import mmap
import os
import queue
import threading
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .data import DeviceBatch


# ---- decode workers (forked BEFORE they are needed, like the reference's DataLoader workers, stack-hg.py:75): a worker decodes
# one JPEG straight into a frame slot that it shares with the parent (anonymous shared mapping inherited over fork), so no
# pixel ever crosses a pipe; it returns only (width, height).
_SLOTS = {}            # slot id -> numpy uint8 view of the shared mapping (filled before the fork)


def _decode_into(args):
    path, slot, B, Hs, Ws, b = args
    from PIL import Image
    arr = _SLOTS[slot][:B * Hs * Ws * 3].reshape(B, Hs, Ws, 3)
    with Image.open(path) as im:
        a = np.asarray(im.convert('RGB'))
    h, w = a.shape[0], a.shape[1]
    arr[b, :h, :w] = a
    return w, h


def _nap(_):
    import time
    time.sleep(0.05)
    return os.getpid()


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:          # header only: PIL decodes lazily
        return im.size


class FrameSlots(object):
    """`depth` host buffers of `slot_bytes` shared with the forked decode pool, page-locked when the runtime allows it
    (hipHostRegister through torch's cudart binding), handed out through a free list."""

    def __init__(self, depth, slot_bytes, workers):
        import multiprocessing as mp
        self.slot_bytes = slot_bytes
        self.maps = []
        base = len(_SLOTS)
        for k in range(depth):
            m = mmap.mmap(-1, slot_bytes)                 # MAP_SHARED | MAP_ANONYMOUS: children of a fork see the same pages
            self.maps.append(m)
            _SLOTS[base + k] = np.frombuffer(m, dtype=np.uint8)
        self.ids = list(range(base, base + depth))
        self.pool = ProcessPoolExecutor(max_workers=max(1, workers), mp_context=mp.get_context('fork'))
        self.n_workers = len(set(self.pool.map(_nap, range(4 * max(1, workers)))))   # fork every worker NOW, before any helper thread exists (they inherit _SLOTS)
        self.pinned = False
        if torch.cuda.is_available():
            try:
                rt = torch.cuda.cudart()
                self.pinned = all(int(rt.cudaHostRegister(_SLOTS[i].ctypes.data, slot_bytes, 0)) == 0 for i in self.ids)
            except Exception:
                self.pinned = False
        self.free = queue.Queue()
        for i in self.ids:
            self.free.put(i)

    def close(self):
        self.pool.shutdown(wait=False, cancel_futures=True)


class CoefSlots(object):
    """`depth` page-locked host staging sets of the device-decode feed, handed out through a free list: the int16 coefficients of one
    batch (grown to the largest batch seen), its descriptors and its per-image coefficient offsets."""

    def __init__(self, depth, batch_size):
        from .pylib import Jpeg
        self.pin = torch.cuda.is_available()
        self.slots = [{'coef': self._host(1 << 16, torch.int16), 'descs': self._host(batch_size * Jpeg.DESC_BYTES, torch.uint8),
                       'base': self._host(batch_size, torch.int64)} for _ in range(depth)]
        self.free = queue.Queue()
        for k in range(depth):
            self.free.put(k)

    def _host(self, n, dtype):
        t = torch.empty(n, dtype=dtype)
        return t.pin_memory() if self.pin else t

    def coef(self, k, elems):
        """slot k's coefficient buffer with room for `elems` (sized from the descriptors of the batch it is about to hold)"""
        if self.slots[k]['coef'].numel() < elems:
            self.slots[k]['coef'] = self._host(int(elems * 1.25), torch.int16)
        return self.slots[k]['coef']


class MPII(object):
    def __init__(self, jsonfile, img_folder, inp_res=256, out_res=64, is_train=True, sigma=1,
                 scale_factor=0.25, rot_factor=30, std_size=200, log=print):
        self.img_folder, self.is_train = img_folder, is_train
        self.inp_res, self.out_res, self.sigma = inp_res, out_res, sigma
        self.scale_factor, self.rot_factor, self.std_size = scale_factor, rot_factor, std_size
        with open(jsonfile, 'r') as anno_file:
            self.anno = json.load(anno_file)
        log('loading json file is done...')
        self.train, self.valid = [], []
        for idx, val in enumerate(self.anno):                                  # data/mpii_for_mpii.py:33-42
            if val['dataset'] == 'MPII':
                if val['objpos'][0] <= 0 or val['objpos'][1] <= 0:
                    log('invalid center: %s\nimage name: %s\ndataset: %s' % (val['objpos'], val['img_paths'], val['dataset']))
                if val['isValidation'] == True:                                 # noqa: E712 (the JSON stores 0/1 floats too)
                    self.valid.append(idx)
                else:
                    self.train.append(idx)
        log(('total training images: %d' % len(self.train)) if is_train else ('total validation images: %d' % len(self.valid)))

    def __len__(self):
        return len(self.train) if self.is_train else len(self.valid)

    def record(self, index):
        """The per-person numbers of __getitem__ (:86-104) BEFORE any augmentation: (img_path, pts [16][2], c [2], s, normalizer)."""
        a = self.anno[(self.train if self.is_train else self.valid)[index]]
        pts = np.asarray(a['joint_self'], dtype=np.float32)[:, 0:2]
        c = np.asarray(a['objpos'], dtype=np.float32).copy()
        s = np.float32(a['scale_provided'])
        if a['dataset'] == 'MPII':
            c[1] = c[1] + 15 * s                                                # :101
            s = s * np.float32(1.25)                                            # :102
            normalizer = np.float32(a['normalizer']) * np.float32(0.6)          # :103
        else:
            raise ValueError('no such dataset {}'.format(a['dataset']))
        return os.path.join(self.img_folder, a['img_paths']), pts, c, s, normalizer

    @staticmethod
    def load_image(img_path):
        """utils/imutils.py:38-41 (RGB); kept as uint8 H x W x 3 -- the /255 happens in the warp kernel."""
        from PIL import Image
        with Image.open(img_path) as im:
            return np.array(im.convert('RGB'), dtype=np.uint8)          # a writable copy

    def load_batch(self, indices, pool=None):
        """Decode the images of `indices` and build the DeviceBatch (frames padded to the largest image of the batch)."""
        recs = [self.record(i) for i in indices]
        imgs = list(pool.map(self.load_image, [r[0] for r in recs])) if pool is not None else [self.load_image(r[0]) for r in recs]
        B = len(recs)
        Hs, Ws = max(i.shape[0] for i in imgs), max(i.shape[1] for i in imgs)
        frames = torch.zeros((B, Hs, Ws, 3), dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else torch.zeros((B, Hs, Ws, 3), dtype=torch.uint8)
        sizes = np.zeros((B, 2), dtype=np.int32)
        for b, im in enumerate(imgs):
            h, w = im.shape[0], im.shape[1]
            frames[b, :h, :w] = torch.from_numpy(im)
            sizes[b] = (w, h)
        batch = DeviceBatch(frames, np.stack([r[2] for r in recs]), np.asarray([r[3] for r in recs]),
                            np.stack([r[1] for r in recs]), np.asarray([r[4] for r in recs]), sizes=sizes, index=list(indices))
        if torch.cuda.is_available():            # the copies from the page-locked staging tensor are asynchronous: consumers on
            batch.ready = torch.cuda.Event()     # other streams (data.AugmentAhead) wait for this event
            batch.ready.record()
        return batch

    def batches(self, batch_size, shuffle=None, seed=0, drop_last=False, workers=8, rank=0, world=1, decoder='thread', prefetch=6):
        """A sized BatchFeed over the split (shuffle defaults to is_train, stack-hg.py:73-83): len() = number of batches,
        every iter() is one pass in a fresh order (seed + pass number).  Data parallel: all ranks draw the SAME order and
        rank r takes batches r, r + world, ... (equal counts on every rank).
        decoder='thread': the next batch is decoded by a thread pool (PIL drops the GIL inside the JPEG decoder) while the
        caller trains on the current one -- a few hundred images/s.
        decoder='process': the reference's DataLoader workers (stack-hg.py:75 num_workers) at the engine's rate: `workers`
        forked processes decode straight into page-locked frame slots shared with this process, `prefetch` batches are
        assembled concurrently and copied to the device on their own stream.
        decoder='device': only the Huffman stage of the JPEG decode runs on the host (pa_jpeg_entropy_host from `workers` threads:
        C++ with the GIL released, no fork, no shared mapping) into page-locked coefficient slots; the coefficients are copied to
        the device on the copy stream and pa_jpeg_decode (inverse DCT, upsampling, colour, padding) writes the same padded frames
        there, byte for byte.  A file outside the decoder's set (progressive, CMYK, ...: include/poseadv.h) is decoded with PIL
        as in the other feeds and copied into its frame behind the kernel; feed.fallbacks counts them.
        Any other value of `decoder` selects 'thread'.  feed.decoder names the path that runs."""
        from .data import BatchFeed
        n = len(self)
        nb_all = n // batch_size if drop_last else (n + batch_size - 1) // batch_size
        nb = nb_all // world if world > 1 else nb_all
        passes = [0]

        def chunks_of_pass():
            order = np.arange(n)
            if self.is_train if shuffle is None else shuffle:
                np.random.default_rng(seed + passes[0]).shuffle(order)
            passes[0] += 1
            chunks = [order[i:i + batch_size].tolist() for i in range(0, n, batch_size)][:nb_all]
            return chunks[rank::world][:nb] if world > 1 else chunks

        def one_pass_threads():
            chunks = chunks_of_pass()
            with ThreadPoolExecutor(max_workers=max(1, workers)) as pool, ThreadPoolExecutor(max_workers=1) as ahead:
                fut = ahead.submit(self.load_batch, chunks[0], pool) if chunks else None
                for k in range(len(chunks)):
                    batch = fut.result()
                    fut = ahead.submit(self.load_batch, chunks[k + 1], pool) if k + 1 < len(chunks) else None
                    yield batch

        def one_pass_processes():
            chunks = chunks_of_pass()
            slots = self._frame_slots(batch_size, workers, prefetch)
            copy_stream = torch.cuda.Stream()
            with ThreadPoolExecutor(max_workers=max(1, prefetch)) as assemblers:
                futs = [assemblers.submit(self._assemble, c, slots, copy_stream) for c in chunks[:prefetch]]
                released = 0
                try:
                    for k in range(len(chunks)):
                        batch, ev, slot = futs[k].result()
                        torch.cuda.current_stream().wait_event(ev)
                        batch.record_stream(torch.cuda.current_stream())     # allocated on the copy stream, consumed on the caller's
                        if k + prefetch < len(chunks):
                            futs.append(assemblers.submit(self._assemble, chunks[k + prefetch], slots, copy_stream))
                        yield batch
                        ev.synchronize()                      # (long done: the copy finished before the batch was trained on)
                        slots.free.put(slot)
                        released = k + 1
                finally:                                      # a pass abandoned early (next(iter(feed))): hand every slot back
                    for f in futs[released:]:
                        try:
                            _, ev, slot = f.result()
                            ev.synchronize()
                            slots.free.put(slot)
                        except Exception:
                            pass

        def one_pass_device():
            chunks = chunks_of_pass()
            slots = self._coef_slots(batch_size, prefetch)
            if getattr(self, '_decode_stream', None) is None:      # one per dataset; the assembler threads share it: every decode call owns its workspace (pylib/Jpeg.py)
                self._decode_stream = torch.cuda.Stream()
            copy_stream = self._decode_stream
            with ThreadPoolExecutor(max_workers=max(1, workers)) as pool, ThreadPoolExecutor(max_workers=max(1, prefetch)) as assemblers:
                futs = [assemblers.submit(self._assemble_device, c, slots, copy_stream, pool, feed) for c in chunks[:prefetch]]
                released = 0
                try:
                    for k in range(len(chunks)):
                        batch, ev, slot = futs[k].result()
                        torch.cuda.current_stream().wait_event(ev)
                        batch.record_stream(torch.cuda.current_stream())
                        if k + prefetch < len(chunks):
                            futs.append(assemblers.submit(self._assemble_device, chunks[k + prefetch], slots, copy_stream, pool, feed))
                        yield batch
                        ev.synchronize()                      # the coefficient upload is long done: the slot may be refilled
                        slots.free.put(slot)
                        released = k + 1
                finally:
                    for f in futs[released:]:
                        try:
                            _, ev, slot = f.result()
                            ev.synchronize()
                            slots.free.put(slot)
                        except Exception:
                            pass

        total = sum(min(batch_size, n - k * batch_size) for k in (range(rank, nb_all, world) if world > 1 else range(nb_all)))
        make_iter = {'process': one_pass_processes, 'device': one_pass_device}.get(decoder, one_pass_threads)
        feed = BatchFeed(nb, total if world == 1 else min(total, nb * batch_size), make_iter, dataset_size=n)
        feed.decoder = decoder if decoder in ('process', 'device') else 'thread'
        feed.fallbacks = 0                  # decoder='device': images so far that were decoded with PIL instead
        feed.lock = threading.Lock()
        return feed

    # ---- process-pool path
    MAX_FRAME = (1088, 1920)                  # slot size: MPII images are at most 1920 x 1080

    def _frame_slots(self, batch_size, workers, prefetch):
        key = (batch_size, workers, prefetch)
        if getattr(self, '_slots_key', None) != key:
            if getattr(self, '_slots', None) is not None:
                self._slots.close()
            self._slots = FrameSlots(prefetch + 2, batch_size * self.MAX_FRAME[0] * self.MAX_FRAME[1] * 3, workers)
            self._slots_key = key
        return self._slots

    def _assemble(self, indices, slots, copy_stream):
        """one batch: image headers -> decode tasks into a free slot -> asynchronous copy to the device on `copy_stream`"""
        recs = [self.record(i) for i in indices]
        sizes = np.asarray([_image_size(r[0]) for r in recs], dtype=np.int32)             # (w, h) per person
        B, Hs, Ws = len(recs), int(sizes[:, 1].max()), int(sizes[:, 0].max())
        if B * Hs * Ws * 3 > slots.slot_bytes:
            raise ValueError('images larger than the frame slots (%d x %d)' % (Ws, Hs))
        slot = slots.free.get()
        list(slots.pool.map(_decode_into, [(r[0], slot, B, Hs, Ws, b) for b, r in enumerate(recs)]))
        host = torch.from_numpy(_SLOTS[slot][:B * Hs * Ws * 3].reshape(B, Hs, Ws, 3))
        with torch.cuda.stream(copy_stream):
            frames = host.to(torch.device('cuda', torch.cuda.current_device()), non_blocking=slots.pinned)
            batch = DeviceBatch(frames, np.stack([r[2] for r in recs]), np.asarray([r[3] for r in recs]),
                                np.stack([r[1] for r in recs]), np.asarray([r[4] for r in recs]), sizes=sizes, index=list(indices))
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        batch.ready = ev
        return batch, ev, slot

    # ---- device-decode path
    def _coef_slots(self, batch_size, prefetch):
        key = (batch_size, prefetch)
        if getattr(self, '_cslots_key', None) != key:
            self._cslots = CoefSlots(prefetch + 2, batch_size)
            self._cslots_key = key
        return self._cslots

    @staticmethod
    def _read_and_describe(path):
        """a decode thread, first visit: the file's bytes and its descriptor (header parse only)"""
        from .pylib import Jpeg
        with open(path, 'rb') as f:
            data = f.read()
        rc, desc = Jpeg.jpeg_info(data)
        if rc == Jpeg.PA_JPEG_UNSUPPORTED or (rc != 0 and data[:2] != b'\xff\xd8'):       # a good file of another kind: PIL's turn
            return data, None, MPII.load_image(path)
        if rc != 0:
            raise _lib.PoseAdvError('%s: %s' % (path, Jpeg.last_error()))
        return data, desc, None

    @staticmethod
    def _entropy_into(args):
        """a decode thread, second visit: Huffman-decode into the image's share of the page-locked slot"""
        from .pylib import Jpeg
        path, data, coef = args
        rc, desc = Jpeg.jpeg_entropy(data, coef)
        if rc != 0:
            raise _lib.PoseAdvError('%s: %s' % (path, Jpeg.last_error()))
        return desc

    def _assemble_device(self, indices, slots, copy_stream, pool, feed):
        """one batch: file bytes + descriptors -> entropy decode into a free coefficient slot -> asynchronous upload and
        pa_jpeg_decode on `copy_stream` (-> PIL pixels of the files the decoder does not take, behind the kernel)"""
        import ctypes
        from .pylib import Jpeg
        recs = [self.record(i) for i in indices]
        B = len(recs)
        first = list(pool.map(self._read_and_describe, [r[0] for r in recs]))
        sizes = np.asarray([(d.width, d.height) if d is not None else (im.shape[1], im.shape[0]) for _, d, im in first], dtype=np.int32)
        Hs, Ws = int(sizes[:, 1].max()), int(sizes[:, 0].max())
        elems = [int(d.total_elems) if d is not None else 0 for _, d, _ in first]          # multiples of 64: every base is 16-byte aligned
        base = np.concatenate([[0], np.cumsum(elems)]).astype(np.int64)
        total = max(64, int(base[-1]))
        slot = slots.free.get()
        try:
            coef = slots.coef(slot, total)
            live = [b for b in range(B) if first[b][1] is not None]
            descs = list(pool.map(self._entropy_into, [(recs[b][0], first[b][0], coef[int(base[b]):int(base[b + 1])]) for b in live]))
            hd, hb = slots.slots[slot]['descs'], slots.slots[slot]['base']
            hd[:B * Jpeg.DESC_BYTES].zero_()                                                  # ncomp == 0: not decoded on the device
            for b, d in zip(live, descs):
                ctypes.memmove(hd.data_ptr() + b * Jpeg.DESC_BYTES, ctypes.addressof(d), Jpeg.DESC_BYTES)
            hb[:B] = torch.from_numpy(base[:B])
            dev = torch.device('cuda', torch.cuda.current_device())
            with torch.cuda.stream(copy_stream):
                dcoef = coef[:total].to(dev, non_blocking=slots.pin)
                ddesc = hd[:B * Jpeg.DESC_BYTES].to(dev, non_blocking=slots.pin)
                dbase = hb[:B].to(dev, non_blocking=slots.pin)
                frames, dsizes = Jpeg.jpeg_decode_batch(dcoef, ddesc, dbase, Hs, Ws, stream=copy_stream)
                for b in range(B):
                    if first[b][1] is None:
                        im = first[b][2]
                        frames[b, :im.shape[0], :im.shape[1]].copy_(torch.from_numpy(im))
                        dsizes[b].copy_(torch.from_numpy(sizes[b]))
                batch = DeviceBatch(frames, np.stack([r[2] for r in recs]), np.asarray([r[3] for r in recs]),
                                    np.stack([r[1] for r in recs]), np.asarray([r[4] for r in recs]), sizes=sizes, index=list(indices))
                batch.sizes = dsizes                     # (w, h) as the decode kernel wrote them: the same numbers as `sizes`
                ev = torch.cuda.Event()
                ev.record(copy_stream)
        except BaseException:
            if torch.cuda.is_available():
                copy_stream.synchronize()            # an upload already enqueued may still read the slot's page-locked buffers
            slots.free.put(slot)
            raise
        if len(live) < B:
            with feed.lock:
                feed.fallbacks += B - len(live)
        batch.ready = ev
        return batch, ev, slot

"""JPEG decode split between host and device (include/poseadv.h: pa_jpeg_*): the reference decodes its images on the host inside
DataLoader workers (utils/imutils.py:38-41); here only the serial Huffman stage stays there (C++ in the library, called from a
thread pool: ctypes drops the GIL for the call) and everything after the coefficients runs as two HIP kernels, byte-exact with
Pillow's Image.open(f).convert('RGB')."""
import ctypes as C

from ._dev import lib, check, ptr, dev, np, torch

PA_JPEG_UNSUPPORTED, PA_JPEG_CORRUPT, PA_JPEG_CAPACITY = 19024, 19025, 19026


class JpegComp(C.Structure):
    _fields_ = [('h', C.c_int32), ('v', C.c_int32), ('bw', C.c_int32), ('bh', C.c_int32), ('offset', C.c_int64)]


class JpegDesc(C.Structure):
    """pa_jpeg_desc"""
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('ncomp', C.c_int32), ('restart_interval', C.c_int32),
                ('total_elems', C.c_int64), ('comp', JpegComp * 3), ('quant', (C.c_uint16 * 64) * 3)]


DESC_BYTES = C.sizeof(JpegDesc)
assert DESC_BYTES == 480


def last_error():
    msg = lib().pa_last_error()
    return msg.decode() if msg else ''


def jpeg_info(data):
    """host: bytes of a JPEG file -> (return code, JpegDesc) from the markers up to SOS (0 = a file the device path takes,
    PA_JPEG_UNSUPPORTED = a good file it does not, anything else = corrupt)."""
    desc = JpegDesc()
    rc = lib().pa_jpeg_info_host(data, len(data), C.byref(desc))
    return rc, desc


def jpeg_entropy(data, coef, capacity=None):
    """host: Huffman-decode `data` into `coef` (a contiguous int16 numpy array or CPU tensor; at most `capacity` elements are
    written) -> (return code, JpegDesc)."""
    desc = JpegDesc()
    if isinstance(coef, torch.Tensor):
        p, n = coef.data_ptr(), coef.numel()
    else:
        assert coef.dtype == np.int16 and coef.flags['C_CONTIGUOUS']
        p, n = coef.ctypes.data, coef.size
    rc = lib().pa_jpeg_entropy_host(data, len(data), C.c_void_p(p), n if capacity is None else int(capacity), C.byref(desc))
    return rc, desc


def jpeg_decode_batch(coef, descs, coef_base, Hs, Ws, stream=None):
    """device: coef int16 [n], descs uint8 [B * DESC_BYTES] (B pa_jpeg_desc), coef_base int64 [B] -> (frames uint8 [B][Hs][Ws][3],
    sizes int32 [B][2]) on `stream` (a torch stream; None = the current one).  Entries with ncomp == 0 come back as an all-zero
    frame and a (0, 0) size: the caller's fallback fills them in.
    The component planes between the two launches live in a workspace allocated per call on that stream (torch's stream-ordered
    allocator): several threads may enqueue decodes on ONE stream concurrently -- the feed's assemblers do -- and a launch of
    another thread that lands between this call's two launches works on its own planes."""
    B = int(coef_base.numel())
    if descs.numel() != B * DESC_BYTES or descs.dtype != torch.uint8 or coef.dtype != torch.int16 or coef_base.dtype != torch.int64:
        raise ValueError('jpeg_decode_batch: coef int16, descs uint8 [B * %d], coef_base int64 [B]' % DESC_BYTES)
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        frames = torch.empty((B, Hs, Ws, 3), dtype=torch.uint8, device=dev())
        sizes = torch.zeros((B, 2), dtype=torch.int32, device=dev())
        ws = torch.empty(max(16, int(lib().pa_jpeg_workspace_bytes(B, int(Hs), int(Ws)))), dtype=torch.uint8, device=dev())
        check(lib().pa_jpeg_decode(ptr(coef), ptr(descs), ptr(coef_base), B, int(Hs), int(Ws), ptr(ws), ptr(frames), ptr(sizes),
                                   C.c_void_p(st.cuda_stream)), 'pa_jpeg_decode')
    return frames, sizes

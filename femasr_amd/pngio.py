"""Fast PNG output (opt-in): PNG's adaptive row filter on the GPU, deflate in independent bands on a thread pool, files
written behind the forward.  Nothing here changes a pixel: the files decode to exactly the bytes `Image.save` would have stored.

    filter_rows(img, filter='adaptive')           the DEFINITION (numpy, integers only) of the filtered scanlines
    filter_rows_gpu(u8, filter='adaptive')        the same bytes from ONE femasr_png_filter_rgb8 launch (csrc/png_filter.hip)
    filter_image(img) / filter_image_gpu(u8)      both for any pixel size: (H,W) gray, (H,W,2) gray + alpha, (H,W,3), (H,W,4) RGBA
    encode_png(rows, width, height, level, pool)  filtered scanlines -> the bytes of a PNG file (write_png: the same into a file object)
    adler32_combine(a1, a2, len2)                 the Adler-32 of a concatenation from the Adler-32 of its parts
    PngWriter(threads=8, depth=3)                 submit(u8_cuda, path): filter + D2H on the current stream, encode + write on threads
                                                  (jpeg_quality=Q: .jpg / .jpeg paths take the fast JPEG path of femasr_amd.jpegio)

Definition.  img: uint8 (H,W,3).  raw[y] = img[y].reshape(3W); per row y and byte i, with x = raw[y][i]:
    a = raw[y][i-3] (0 if i < 3),  b = raw[y-1][i] (0 if y == 0),  c = raw[y-1][i-3] (0 if either is outside)
    f0 = x,  f1 = x - a,  f2 = x - b,  f3 = x - ((a + b) >> 1),  f4 = x - paeth(a, b, c)                      (all mod 256)
    paeth: p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|;  a if pa <= pb and pa <= pc, else b if pb <= pc, else c
    cost_t = sum_i min(f_t[i], 256 - f_t[i]);  t* = the smallest t with the least cost ('adaptive'; a fixed filter 0..4 is t* itself)
    out[y] = [t*, f_t*[0], ..., f_t*[3W-1]]
out is uint8 (H, 1 + 3W): the byte stream PNG deflates for colour type 2, bit depth 8, no interlace.

The file.  The filtered stream is cut into bands of whole rows holding at least BAND_BYTES each (the last band takes the remainder; a
stream below BAND_BYTES is one band).  Every band is a raw deflate stream of its own (`zlib.compressobj(level, DEFLATED, -15)`); all but the
last end with Z_FULL_FLUSH - byte-aligned, no reference across it -, the last with Z_FINISH, so the concatenation behind a 2-byte zlib header
and in front of the Adler-32 of the whole stream is ONE valid zlib stream.  IHDR, one IDAT chunk per band, IEND.  The bytes depend on the
pixels, `level` and BAND_BYTES only - never on the number of threads or on timing.
"""
import struct
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

BAND_BYTES = 256 * 1024
MAX_THREADS = 16
ADAPTIVE = 5
_ADLER_MOD = 65521
_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': ADAPTIVE}
CHANNELS = {1: (0, 'L'), 2: (4, 'LA'), 3: (2, 'RGB'), 4: (6, 'RGBA')}      # channels -> (IHDR colour type at bit depth 8, PIL's mode)


def filter_code(filter):
    """0..4 for a fixed filter (int or name), 5 for 'adaptive'."""
    if isinstance(filter, str) and filter in _FILTERS:
        return _FILTERS[filter]
    if isinstance(filter, (int, np.integer)) and not isinstance(filter, bool) and 0 <= int(filter) <= 4:
        return int(filter)
    raise ValueError(f"png filter must be 0..4 or one of {sorted(_FILTERS)}, got {filter!r}")


def filter_rows(img, filter='adaptive'):
    """The definition (module docstring): uint8 (H,W,3) -> uint8 (H, 1 + 3W)."""
    code = filter_code(filter)
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f'filter_rows: expected a uint8 (H,W,3) image, got {img.dtype} {img.shape}')
    return _filter(img, 3, code)


def filter_image(img, filter='adaptive'):
    """The definition for any pixel size: uint8 (H,W) or (H,W,C), C in 1..4 -> uint8 (H, 1 + CW), with C in place of the 3 of the module
    docstring (the left neighbour of byte i is byte i - C).  C = 3: filter_rows."""
    code = filter_code(filter)
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in CHANNELS) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f'filter_image: expected a uint8 (H,W) or (H,W,C) image with C in 1..4, got {img.dtype} {img.shape}')
    return _filter(img, 1 if img.ndim == 2 else img.shape[2], code)


def _filter(img, bpp, code):
    H, W = img.shape[:2]
    n = bpp * W
    x = img.reshape(H, n).astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]

    def residual(t):
        if t == 0:
            return x
        if t == 1:
            return (x - a) & 255
        if t == 2:
            return (x - b) & 255
        if t == 3:
            return (x - ((a + b) >> 1)) & 255
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        return (x - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))) & 255

    out = np.empty((H, 1 + n), np.uint8)
    if code != ADAPTIVE:
        out[:, 0] = code
        out[:, 1:] = residual(code)
        return out
    best = None
    for t in range(5):
        f = residual(t)
        cost = np.minimum(f, 256 - f).sum(axis=1, dtype=np.int64)
        if best is None:
            best, kind, res = cost, np.zeros(H, np.uint8), f.astype(np.uint8)
        else:
            take = cost < best                       # strictly less: the smallest t keeps a tie
            best = np.where(take, cost, best)
            kind[take] = t
            res[take] = f[take]
    out[:, 0] = kind
    out[:, 1:] = res
    return out


def filter_rows_gpu(u8, filter='adaptive', out=None):
    """`filter_rows` of a uint8 (H,W,3) or (B,H,W,3) GPU tensor: (H, 1 + 3W) / (B, H, 1 + 3W), ONE launch on the current stream."""
    import torch
    from . import _lib
    code = filter_code(filter)
    if not torch.is_tensor(u8) or not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() not in (3, 4) or u8.shape[-1] != 3 or u8.numel() == 0:
        raise ValueError('filter_rows_gpu: expected a non-empty uint8 (H,W,3) or (B,H,W,3) GPU tensor')
    u8 = u8.contiguous()
    B = u8.shape[0] if u8.dim() == 4 else 1
    H, W = u8.shape[-3], u8.shape[-2]
    shape = tuple(u8.shape[:-2]) + (1 + 3 * W,)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=u8.device)
    elif not torch.is_tensor(out) or out.shape != shape or out.dtype != torch.uint8 or out.device != u8.device or not out.is_contiguous():
        raise ValueError(f'filter_rows_gpu: out= must be a contiguous uint8 tensor of shape {shape} on {u8.device}')
    with torch.cuda.device(u8.device):
        _lib.check(_lib.load().femasr_png_filter_rgb8(torch.cuda.current_stream(u8.device).cuda_stream, _lib.ptr(u8), B, H, W, code, _lib.ptr(out)))
    return out


def filter_image_gpu(u8, filter='adaptive', out=None):
    """`filter_image` of a uint8 (H,W), (H,W,C) or (B,H,W,C) GPU tensor, C in 1..4: (H, 1 + CW) / (B, H, 1 + CW), ONE femasr_png_filter_u8
    launch on the current stream.  A batch needs its channel axis: a 3-D tensor is (H,W,C)."""
    import torch
    from . import _lib
    code = filter_code(filter)
    if (not torch.is_tensor(u8) or not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() not in (2, 3, 4) or u8.numel() == 0 or
            (u8.dim() != 2 and u8.shape[-1] not in CHANNELS)):
        raise ValueError('filter_image_gpu: expected a non-empty uint8 (H,W), (H,W,C) or (B,H,W,C) GPU tensor with C in 1..4')
    u8 = u8.contiguous()
    C = 1 if u8.dim() == 2 else u8.shape[-1]
    lead = tuple(u8.shape) if u8.dim() == 2 else tuple(u8.shape[:-1])
    B = lead[0] if len(lead) == 3 else 1
    H, W = lead[-2:]
    shape = lead[:-1] + (1 + C * W,)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=u8.device)
    elif not torch.is_tensor(out) or out.shape != shape or out.dtype != torch.uint8 or out.device != u8.device or not out.is_contiguous():
        raise ValueError(f'filter_image_gpu: out= must be a contiguous uint8 tensor of shape {shape} on {u8.device}')
    with torch.cuda.device(u8.device):
        _lib.check(_lib.load().femasr_png_filter_u8(torch.cuda.current_stream(u8.device).cuda_stream, _lib.ptr(u8), B, H, W, C, code, _lib.ptr(out)))
    return out


def adler32_combine(adler1, adler2, len2):
    """Adler-32 of s1 + s2 from adler1 = adler32(s1), adler2 = adler32(s2) and len2 = len(s2)."""
    a1, b1 = adler1 & 0xffff, (adler1 >> 16) & 0xffff
    a2, b2 = adler2 & 0xffff, (adler2 >> 16) & 0xffff
    a = (a1 + a2 - 1) % _ADLER_MOD
    b = (b1 + b2 + (len2 % _ADLER_MOD) * (a1 - 1)) % _ADLER_MOD
    return (b << 16) | a


def zlib_header(level):
    """The 2-byte header zlib itself writes for `level` with a 32 KiB window."""
    flevel = 0 if level < 2 else 1 if level < 6 else 2 if level == 6 else 3
    head = (0x78 << 8) | (flevel << 6)
    head += 31 - head % 31
    return struct.pack('>H', head)


def band_rows(height, pitch):
    """[(first row, end row)] of the bands of a (height, pitch) filtered stream."""
    per = max(1, -(-BAND_BYTES // pitch))
    nb = max(1, height // per)
    return [(k * per, height if k == nb - 1 else (k + 1) * per) for k in range(nb)]


def _chunk(kind, body, crc=None):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(body, zlib.crc32(kind)) if crc is None else crc)


def _band(view, level, first, last):
    """One band in a worker: (bytes of its IDAT body without the stream's trailer, crc32 of b'IDAT' + those bytes, adler32, length)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = (zlib_header(level) if first else b'') + c.compress(view) + c.flush(zlib.Z_FINISH if last else zlib.Z_FULL_FLUSH)
    return body, zlib.crc32(body, zlib.crc32(b'IDAT')), zlib.adler32(view), len(view)


def _pieces(rows, width, height, level, pool, channels=3):
    rows = np.asarray(rows)
    if not isinstance(level, int) or isinstance(level, bool) or not 0 <= level <= 9:
        raise ValueError(f'png level must be an integer in 0..9, got {level!r}')
    if channels not in CHANNELS:
        raise ValueError(f'encode_png: channels must be 1 (gray), 2 (gray + alpha), 3 (RGB) or 4 (RGBA), got {channels!r}')
    if width < 1 or height < 1 or rows.dtype != np.uint8 or rows.shape != (height, 1 + channels * width) or not rows.flags.c_contiguous:
        raise ValueError(f'encode_png: rows must be a contiguous uint8 ({height}, {1 + channels * width}) array, got {rows.dtype} {rows.shape}')
    bands = band_rows(height, rows.shape[1])
    jobs = [(memoryview(rows[y0:y1]).cast('B'), level, k == 0, k == len(bands) - 1) for k, (y0, y1) in enumerate(bands)]
    done = [_band(*j) for j in jobs] if pool is None else list(pool.map(lambda j: _band(*j), jobs))
    adler = 1
    for _, _, ad, n in done:
        adler = adler32_combine(adler, ad, n)
    yield _SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, CHANNELS[channels][0], 0, 0, 0))
    for k, (body, crc, _, _) in enumerate(done):
        if k == len(done) - 1:
            tail = struct.pack('>I', adler)
            body, crc = body + tail, zlib.crc32(tail, crc)
        yield _chunk(b'IDAT', body, crc)
    yield _chunk(b'IEND', b'')


def encode_png(rows, width, height, level=6, pool=None, channels=3):
    """The bytes of the PNG file of a filtered stream `rows` (uint8 (height, 1 + channels width), host memory).  pool: a
    concurrent.futures executor for the bands (None: this thread); the result does not depend on it.  channels 1, 2, 3, 4: colour type
    0 (gray), 4 (gray + alpha), 2 (RGB), 6 (RGBA) at bit depth 8."""
    return b''.join(_pieces(rows, width, height, level, pool, channels))


def write_png(fileobj, rows, width, height, level=6, pool=None, channels=3):
    """`encode_png` written to a file object; returns the number of bytes."""
    n = 0
    for piece in _pieces(rows, width, height, level, pool, channels):
        fileobj.write(piece)
        n += len(piece)
    return n


def clamp_threads(threads):
    if not isinstance(threads, int) or isinstance(threads, bool) or threads < 1:
        raise ValueError(f'thread count must be an integer >= 1, got {threads!r}')
    return min(threads, MAX_THREADS)


class _PinnedPool:
    """Grow-only pool of pinned host buffers (a buffer is reused by the next image that fits in it)."""

    def __init__(self):
        self._free, self._lock = [], threading.Lock()

    def take(self, nbytes):
        import torch
        with self._lock:
            fit = [i for i, b in enumerate(self._free) if b.numel() >= nbytes]
            if fit:
                return self._free.pop(min(fit, key=lambda i: self._free[i].numel()))
            if self._free:                                   # grow: the largest too-small buffer makes room for the new one
                self._free.pop(max(range(len(self._free)), key=lambda i: self._free[i].numel()))
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)

    def give(self, buf):
        with self._lock:
            self._free.append(buf)


class PngWriter:
    """Writes uint8 (H,W,3) GPU images - and (H,W) gray, (H,W,2) gray + alpha, (H,W,4) RGBA ones - to files behind the caller's stream.

    submit(u8, path), on the current stream and in this order: the filter kernel, a non-blocking copy of its result into a pinned buffer,
    an event - then it returns.  A writer thread waits for the event, deflates the bands on the shared pool of `threads` threads and writes
    the file.  At most `depth` images are in flight: submit blocks beyond that.  A path that does not end in .png (any case) gets a plain
    D2H copy and `Image.save` in the writer thread.  The first exception of a worker is re-raised by the next submit or by close().
    No GPU stream and no process is created; thread counts are arguments (capped at 16), never derived from the machine.

    jpeg_quality=Q (1..100; None, the default: nothing changes): a path that ends in .jpg or .jpeg (any case) with a 1- or 3-channel image
    takes the fast JPEG path instead of `Image.save` - submit launches the coefficient kernel (femasr_amd.jpegio.coefficients_gpu:
    colour, DCT, quantisation at quality Q and chroma `jpeg_subsampling`, '420' or '444') and copies the int16 planes to a pinned buffer
    without blocking; the writer thread Huffman-codes bands of MCU rows on the shared pool and writes the file: the bytes of
    jpegio.encode_ref.  Two- and four-channel images on such a path stay with `Image.save`, which refuses them as ever."""

    def __init__(self, threads=8, depth=3, level=6, stage=None, jpeg_quality=None, jpeg_subsampling='420'):
        self.threads = clamp_threads(threads)
        self.depth = clamp_threads(depth)
        if not isinstance(level, int) or isinstance(level, bool) or not 0 <= level <= 9:
            raise ValueError(f'png level must be an integer in 0..9, got {level!r}')
        self.level = level
        self.jpeg_quality = self.jpeg_subsampling = None
        if jpeg_quality is not None:
            from . import jpegio
            self.jpeg_quality, self.jpeg_subsampling = jpegio._check_params(jpeg_quality, jpeg_subsampling)
        self._stage = stage or self._gpu_stage
        self._pinned = _PinnedPool()
        self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix='png-band')
        self._writers = ThreadPoolExecutor(self.depth, thread_name_prefix='png-file')
        self._slots = threading.Semaphore(self.depth)
        self._lock = threading.Lock()
        self._error = None
        self._pending = []
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except Exception:
            if exc_type is None:
                raise
        return False

    def _gpu_stage(self, u8, is_png):
        """(host array, wait(), release()): the part of submit that touches the GPU."""
        import torch
        if (not torch.is_tensor(u8) or not u8.is_cuda or u8.dtype != torch.uint8 or u8.numel() == 0 or
                not (u8.dim() == 2 or (u8.dim() == 3 and u8.shape[2] in (2, 3, 4)))):
            raise ValueError('PngWriter.submit: expected a non-empty uint8 (H,W,3) GPU tensor, or (H,W), (H,W,2), (H,W,4)')
        dev = filter_image_gpu(u8) if is_png else u8.contiguous()
        buf = self._pinned.take(dev.numel())
        host = buf[:dev.numel()].view(dev.shape)
        host.copy_(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(u8.device))
        keep = [dev]                                          # the device buffer lives until the copy has run

        def wait():
            ev.synchronize()
            keep.clear()
        return host.numpy(), wait, lambda: self._pinned.give(buf)

    def _gpu_jpeg_stage(self, u8):
        """(host int16 array of every plane, plane shapes, wait(), release()): the GPU part of a submit on the fast JPEG path."""
        import torch
        from . import jpegio
        flat, views = jpegio.coefficients_flat_gpu(u8, self.jpeg_quality, self.jpeg_subsampling)
        buf = self._pinned.take(2 * flat.numel())
        host = buf[:2 * flat.numel()].view(torch.int16)
        host.copy_(flat, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(u8.device))
        keep = [flat]                                         # the device buffer lives until the copy has run

        def wait():
            ev.synchronize()
            keep.clear()
        return host.numpy(), [tuple(v.shape) for v in views], wait, lambda: self._pinned.give(buf)

    def _jpeg_job(self, path, width, height, host, shapes, wait, release):
        try:
            from . import jpegio
            wait()
            comps, off = [], 0
            for shape in shapes:
                n = shape[0] * shape[1] * 64
                comps.append(host[off:off + n].reshape(shape))
                off += n
            data = jpegio.encode_jpeg(comps, width, height, self.jpeg_quality, self.jpeg_subsampling, self._pool)
            with open(path, 'wb') as f:
                f.write(data)
        except BaseException as e:                            # kept for the caller: nothing is dropped silently
            with self._lock:
                if self._error is None:
                    self._error = e
        finally:
            release()
            self._slots.release()

    def _raise_pending(self):
        with self._lock:
            err, self._error = self._error, None
        if err is not None:
            raise err

    def _job(self, path, is_png, width, height, channels, host, wait, release):
        try:
            wait()
            if is_png:
                with open(path, 'wb') as f:
                    write_png(f, host, width, height, self.level, self._pool, channels)
            else:
                from PIL import Image
                Image.fromarray(host, CHANNELS[channels][1]).save(path)
        except BaseException as e:                            # kept for the caller: nothing is dropped silently
            with self._lock:
                if self._error is None:
                    self._error = e
        finally:
            release()
            self._slots.release()

    def submit(self, u8, path):
        if self._closed:
            raise RuntimeError('PngWriter is closed')
        self._raise_pending()
        path = str(path)
        is_png = path.lower().endswith('.png')
        is_jpeg = (self.jpeg_quality is not None and path.lower().endswith(('.jpg', '.jpeg')) and
                   (len(u8.shape) == 2 or (len(u8.shape) == 3 and u8.shape[2] == 3)))
        self._slots.acquire()                                 # blocks while `depth` images are in flight
        try:
            height, width = int(u8.shape[0]), int(u8.shape[1])
            channels = int(u8.shape[2]) if len(u8.shape) == 3 else 1
            if is_jpeg:
                host, shapes, wait, release = self._gpu_jpeg_stage(u8)
            else:
                host, wait, release = self._stage(u8, is_png)
        except BaseException:
            self._slots.release()
            raise
        self._pending = [f for f in self._pending if not f.done()]
        if is_jpeg:
            self._pending.append(self._writers.submit(self._jpeg_job, path, width, height, host, shapes, wait, release))
        else:
            self._pending.append(self._writers.submit(self._job, path, is_png, width, height, channels, host, wait, release))

    def close(self):
        """Waits for every file; re-raises the first worker exception.  Idempotent."""
        if not self._closed:
            self._closed = True
            for f in self._pending:
                f.result()
            self._pending = []
            self._writers.shutdown(wait=True)
            self._pool.shutdown(wait=True)
        self._raise_pending()

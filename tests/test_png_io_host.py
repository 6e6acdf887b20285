"""Fast PNG output without a GPU (femasr_amd/pngio.py): the definition of the filtered scanlines, the banded encoder, the
writer's queueing and the C entry's refusals.

`_filter_rows_ref` below restates the definition byte by byte (pure Python integers, the formulas of the issue text); PIL's decoder is the
independent judge of every file."""
import ctypes
import io
import os
import struct
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from PIL import Image

from femasr_amd import _lib, pngio
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def _filter_rows_ref(img, filter='adaptive'):
    H, W = img.shape[:2]
    n = 3 * W
    raw = [[int(v) for v in img[y].reshape(-1)] for y in range(H)]
    out = np.empty((H, 1 + n), np.uint8)
    for y in range(H):
        f = [[] for _ in range(5)]
        for i in range(n):
            x = raw[y][i]
            a = raw[y][i - 3] if i >= 3 else 0
            b = raw[y - 1][i] if y >= 1 else 0
            c = raw[y - 1][i - 3] if y >= 1 and i >= 3 else 0
            for t, pred in enumerate((0, a, b, (a + b) >> 1, _paeth(a, b, c))):
                f[t].append((x - pred) % 256)
        cost = [sum(min(v, 256 - v) for v in ft) for ft in f]
        t = cost.index(min(cost)) if filter == 'adaptive' else filter
        out[y, 0] = t
        out[y, 1:] = f[t]
    return out


def _testset_image(name):
    g = load_golden('testset_all')
    i = [str(n) for n in g['names']].index(name)
    raw = g['file_bytes'][int(g['file_off'][i]):int(g['file_off'][i + 1])].tobytes()
    return Image.open(io.BytesIO(raw)).convert('RGB')


def _small_cases():
    rng = np.random.RandomState(7)
    cases = {f'noise{h}x{w}': rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((1, 1), (1, 7), (2, 1), (7, 5))}
    cases['flat33x70'] = np.full((33, 70, 3), 93, np.uint8)
    cases['only0_255'] = (rng.randint(0, 2, (9, 11, 3)) * 255).astype(np.uint8)
    cases['only127_128'] = (127 + rng.randint(0, 2, (9, 11, 3))).astype(np.uint8)
    return cases


def _chunks(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        out.append((kind, body, crc))
        pos += 12 + n
    assert pos == len(data)
    return out


def _decode(data):
    return np.array(Image.open(io.BytesIO(data)).convert('RGB'))


# ------------------------------------------------------------------------------------------------ definition and round trip
@pytest.mark.parametrize('name', sorted(_small_cases()))
def test_definition_and_round_trip(name):
    img = _small_cases()[name]
    H, W = img.shape[:2]
    rows = pngio.filter_rows(img)
    assert rows.dtype == np.uint8 and rows.shape == (H, 1 + 3 * W)
    if H * W <= 100:
        assert np.array_equal(rows, _filter_rows_ref(img))
        for t in range(5):
            assert np.array_equal(pngio.filter_rows(img, t), _filter_rows_ref(img, t)), t
    data = pngio.encode_png(rows, W, H)
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == 'PNG' and im.mode == 'RGB' and im.size == (W, H)
    assert np.array_equal(_decode(data), img)
    buf = io.BytesIO()
    assert pngio.write_png(buf, rows, W, H) == len(data) and buf.getvalue() == data      # the file-object form
    for t in range(5):                                                                    # every fixed filter round-trips
        fixed = pngio.filter_rows(img, t)
        assert (fixed[:, 0] == t).all()
        assert np.array_equal(_decode(pngio.encode_png(fixed, W, H)), img), t


@pytest.mark.parametrize('name', ['00003.png', 'frog.png'])
def test_round_trip_testset(name):
    img = np.array(_testset_image(name))
    rows = pngio.filter_rows(img)
    k = min(3, img.shape[0])
    assert np.array_equal(rows[:k], _filter_rows_ref(img[:k]))
    for level in (0, 1, 6, 9):
        assert np.array_equal(_decode(pngio.encode_png(rows, img.shape[1], img.shape[0], level)), img), level


def test_filter_choice_on_a_flat_image():
    """Row 0: None costs 70 * 3 * 93, Sub only the first pixel; from row 1 on Up and Paeth both cost 0 and the smaller type wins."""
    rows = pngio.filter_rows(np.full((33, 70, 3), 93, np.uint8))
    assert rows[:, 0].tolist() == [1] + [2] * 32
    assert not rows[1:, 1:].any()


def test_cost_is_signed_and_ties_go_to_the_smallest_type():
    # one pixel (128, 128, 128): every filter leaves 128 = the tie of min(f, 256 - f); all five cost 384 and None wins
    assert pngio.filter_rows(np.full((1, 1, 3), 128, np.uint8))[0].tolist() == [0, 128, 128, 128]
    # columns of 0 and 255: a byte 255 costs 1, not 255 - None costs 12, Sub 21 (every byte from the second pixel on is +-1)
    img = np.zeros((1, 8, 3), np.uint8)
    img[:, 1::2] = 255
    rows = pngio.filter_rows(img)
    assert np.array_equal(rows, _filter_rows_ref(img)) and rows[0, 0] == 0
    # 254 after 255 in every byte: Sub leaves 255 = -1 (cost 1 per byte) where None leaves 254 (cost 2 per byte)
    img = np.full((1, 6, 3), 254, np.uint8)
    img[:, 0] = 255
    assert pngio.filter_rows(img)[0].tolist() == [1, 255, 255, 255, 255, 255, 255] + [0] * 12


def test_refusals_of_the_definition():
    for bad in (np.zeros((4, 4, 3), np.int32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            pngio.filter_rows(bad)
    for f in (5, -1, 'best', True, 1.0):
        with pytest.raises(ValueError):
            pngio.filter_rows(np.zeros((2, 2, 3), np.uint8), f)
    rows = pngio.filter_rows(np.zeros((2, 2, 3), np.uint8))
    for kw in (dict(width=3), dict(height=1), dict(level=10), dict(level=-1)):
        with pytest.raises(ValueError):
            pngio.encode_png(rows, **dict(dict(width=2, height=2), **kw))


# ------------------------------------------------------------------------------------------------ container
def _big():
    """700 x 900 with structure and noise: 1.9 MB of filtered bytes, 7 bands."""
    rng = np.random.RandomState(11)
    y, x = np.mgrid[0:700, 0:900]
    base = np.stack([(x + y) // 5, x // 3 + 40, 255 - y // 3], -1)
    return np.clip(base + rng.randint(-3, 4, base.shape), 0, 255).astype(np.uint8)


def test_container():
    img = _big()
    H, W = img.shape[:2]
    rows = pngio.filter_rows(img)
    data = pngio.encode_png(rows, W, H)
    ch = _chunks(data)
    assert [k for k, _, _ in ch] == [b'IHDR'] + [b'IDAT'] * (len(ch) - 2) + [b'IEND']
    for kind, body, crc in ch:
        assert crc == zlib.crc32(kind + body), kind
    assert ch[0][1] == struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0) and ch[-1][1] == b''
    stream = b''.join(body for kind, body, _ in ch if kind == b'IDAT')
    assert zlib.decompress(stream) == rows.tobytes()
    assert struct.unpack('>I', stream[-4:])[0] == zlib.adler32(rows.tobytes())
    assert stream[0] & 15 == 8 and stream[0] >> 4 == 7 and (stream[0] * 256 + stream[1]) % 31 == 0 and not stream[1] & 32
    # the bands: whole rows, at least BAND_BYTES each, the last one takes the remainder; each is a deflate stream of its own
    bands = pngio.band_rows(H, rows.shape[1])
    assert len(bands) == len(ch) - 2 == 7 and bands[0][0] == 0 and bands[-1][1] == H
    for (y0, y1), (_, nxt) in zip(bands, bands[1:] + [(H, H)]):
        assert y1 == _ and (y1 - y0) * rows.shape[1] >= pngio.BAND_BYTES
    assert all((y1 - y0 - 1) * rows.shape[1] < pngio.BAND_BYTES for y0, y1 in bands[:-1])
    bodies = [body for kind, body, _ in ch if kind == b'IDAT']
    bodies[0], bodies[-1] = bodies[0][2:], bodies[-1][:-4]
    for (y0, y1), body in zip(bands, bodies):
        assert zlib.decompressobj(-15).decompress(body) == rows[y0:y1].tobytes()      # decodes alone: nothing refers across a band's start
    assert np.array_equal(_decode(data), img)


def test_one_band_below_band_bytes():
    img = _big()[:90]                                      # 90 * 2701 = 243 090 filtered bytes
    rows = pngio.filter_rows(img)
    assert rows.size < pngio.BAND_BYTES and pngio.band_rows(90, rows.shape[1]) == [(0, 90)]
    ch = _chunks(pngio.encode_png(rows, 900, 90))
    assert [k for k, _, _ in ch] == [b'IHDR', b'IDAT', b'IEND']
    assert pngio.band_rows(1, 4) == [(0, 1)] and pngio.band_rows(3, 3 * (1 << 20)) == [(0, 1), (1, 2), (2, 3)]


def test_adler_combine():
    rng = np.random.RandomState(5)
    data = rng.bytes(200000)
    for k in [0, 1, 5552, 65521, 199999, 200000] + [int(v) for v in rng.randint(0, 200001, 20)]:
        assert pngio.adler32_combine(zlib.adler32(data[:k]), zlib.adler32(data[k:]), len(data) - k) == zlib.adler32(data), k
    ones = b'\xff' * 70000                                 # sums that wrap the modulus many times
    assert pngio.adler32_combine(zlib.adler32(ones), zlib.adler32(ones), len(ones)) == zlib.adler32(ones + ones)
    for level in range(10):
        assert pngio.zlib_header(level) == zlib.compress(b'x', level)[:2]


def test_bytes_do_not_depend_on_the_pool():
    img = _big()
    rows = pngio.filter_rows(img)
    ref = pngio.encode_png(rows, 900, 700)
    with ThreadPoolExecutor(1) as p1, ThreadPoolExecutor(8) as p8:
        assert pngio.encode_png(rows, 900, 700, pool=p1) == ref
        assert pngio.encode_png(rows, 900, 700, pool=p8) == ref
        assert pngio.encode_png(rows, 900, 700, 3, p8) == pngio.encode_png(rows, 900, 700, 3) != ref


BANDING_FIXTURES = [(n, noise) for n in ('00003.png', '0032.jpg', 'OST_020.png', 'frog.png') for noise in (False, True)]


def _banding_cost(case):
    name, noise = case
    im = _testset_image(name)
    img = np.array(im.resize((im.width * 4, im.height * 4), Image.BICUBIC))
    if noise:
        img = np.clip(img.astype(np.int16) + np.random.RandomState(0).randint(-3, 4, img.shape), 0, 255).astype(np.uint8)
    rows = pngio.filter_rows(img)
    single = len(zlib.compress(rows, 6))
    banded = sum(len(body) for kind, body, _ in _chunks(pngio.encode_png(rows, img.shape[1], img.shape[0], 6)) if kind == b'IDAT')
    return name, noise, img.shape, single, banded


def test_banding_costs_at_most_one_percent():
    """The x4 PIL-bicubic upscales of four testset images, each with and without +-3 of noise (seed 0): the IDAT payload of the banded
    stream against ONE zlib stream of the same filtered rows at the same level.  (The eight cases run side by side: zlib releases the GIL.)"""
    with ThreadPoolExecutor(8) as pool:
        results = list(pool.map(_banding_cost, BANDING_FIXTURES))
    for name, noise, shape, single, banded in results:
        print(f'{name} noise={noise} {shape}: single {single}, banded {banded}, +{100.0 * (banded - single) / single:.3f} %')
    for name, noise, shape, single, banded in results:
        assert banded <= 1.01 * single, (name, noise, single, banded)


# ------------------------------------------------------------------------------------------------ writer
class _StubStage:
    """In place of the GPU stage: filters on the host; counts the images between stage and release; wait() blocks until `gate` is set."""

    def __init__(self):
        self.lock, self.gate = threading.Lock(), threading.Event()
        self.inflight = self.peak = self.staged = 0

    def __call__(self, img, is_png):
        with self.lock:
            self.inflight += 1
            self.staged += 1
            self.peak = max(self.peak, self.inflight)
        return (pngio.filter_rows(img) if is_png else img), self.gate.wait, self._release

    def _release(self):
        with self.lock:
            self.inflight -= 1


def test_writer_defaults_and_caps():
    with pngio.PngWriter(stage=_StubStage()) as w:
        assert (w.threads, w.depth, w.level) == (8, 3, 6)
    with pngio.PngWriter(threads=99, stage=_StubStage()) as w:
        assert w.threads == 16 == pngio.MAX_THREADS
    for kw in (dict(threads=0), dict(threads=2.0), dict(depth=0), dict(level=10)):
        with pytest.raises(ValueError):
            pngio.PngWriter(stage=_StubStage(), **kw)


def test_writer_depth_bound_and_files(tmp_path):
    rng = np.random.RandomState(2)
    imgs = [rng.randint(0, 256, (5 + i, 9 - i % 3, 3)).astype(np.uint8) for i in range(12)]
    stage = _StubStage()
    w = pngio.PngWriter(threads=2, depth=3, stage=stage)
    for i in range(3):
        w.submit(imgs[i], tmp_path / f'{i}.png')
    # three images are in flight (their writer threads wait at the gate): a fourth submit would block on the slot it cannot get
    assert stage.inflight == 3 and not w._slots.acquire(blocking=False)
    stage.gate.set()
    for i in range(3, 12):
        w.submit(imgs[i], tmp_path / (f'{i}.PNG' if i % 2 else f'{i}.bmp'))
    w.close()
    w.close()                                              # idempotent
    assert stage.staged == 12 and stage.inflight == 0 and stage.peak == 3
    for i, img in enumerate(imgs):
        path = tmp_path / (f'{i}.png' if i < 3 else f'{i}.PNG' if i % 2 else f'{i}.bmp')
        with Image.open(str(path)) as im:
            assert im.format == ('BMP' if path.suffix == '.bmp' else 'PNG')
            assert np.array_equal(np.array(im.convert('RGB')), img)
        if path.suffix != '.bmp':
            assert path.read_bytes() == pngio.encode_png(pngio.filter_rows(img), img.shape[1], img.shape[0])
    with pytest.raises(RuntimeError):
        w.submit(imgs[0], tmp_path / 'late.png')


def test_writer_reports_a_failed_write(tmp_path):
    stage = _StubStage()
    stage.gate.set()
    img = np.zeros((4, 4, 3), np.uint8)
    w = pngio.PngWriter(threads=1, stage=stage)
    w.submit(img, tmp_path / 'no_such_dir' / 'a.png')
    w.submit(img, tmp_path / 'ok.png')
    with pytest.raises(FileNotFoundError):
        w.close()
    assert (tmp_path / 'ok.png').exists() and stage.inflight == 0
    with pytest.raises(OSError):                            # the context manager form raises as well
        with pngio.PngWriter(threads=1, stage=stage) as w2:
            w2.submit(img, tmp_path / 'no_such_dir' / 'b.png')


# ------------------------------------------------------------------------------------------------ C entry and CLI surface
def test_header_and_binding_agree():
    import re
    with open(os.path.join(ROOT, 'include', 'femasr_hip.h')) as f:
        decl = dict(re.findall(r'^int (femasr_png_\w+)\(([^)]*)\);', f.read(), re.M))
    assert list(decl) == ['femasr_png_filter_rgb8']
    res, args = _lib.SIGNATURES['femasr_png_filter_rgb8']
    params = [p.strip() for p in decl['femasr_png_filter_rgb8'].split(',')]
    assert res is ctypes.c_int and len(args) == len(params) == 7
    for p, a in zip(params, args):
        assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == p.startswith('int '), p
    lib = _lib.load()
    assert lib.femasr_png_filter_rgb8.argtypes == args and lib.femasr_version() == _lib.ABI_VERSION == 107      # additive: the number stays


def test_abi_refuses_before_any_launch():
    """Every call returns FEMASR_ERR_INVALID; none may reach a launch - the pointers are fakes and this process has no GPU context."""
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)

    def call(img=fake, B=1, H=8, W=8, filter=5, out=fake):
        return lib.femasr_png_filter_rgb8(None, img, B, H, W, filter, out)
    for kw in (dict(img=None), dict(out=None)):
        assert call(**kw) == -1 and b'null' in lib.femasr_last_error()
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-8), dict(filter=-1), dict(filter=6),
               dict(W=(1 << 22) + 1), dict(W=(1 << 31) - 1), dict(B=1 << 16, H=1 << 15)):
        assert call(**kw) == -1, kw
    assert call(W=(1 << 22) + 1) == -1 and b'2^22' in lib.femasr_last_error()


def test_cli_options():
    from femasr_amd import inference
    ap = inference.build_parser()
    d = ap.parse_args([])
    assert d.io_threads == 0 and d.png_level == 6
    a = ap.parse_args(['--io-threads', '8', '--png-level', '3'])
    assert a.io_threads == 8 and a.png_level == 3


def test_decode_ahead_keeps_order_and_errors(tmp_path):
    from femasr_amd import inference
    paths = []
    for i in range(7):
        p = tmp_path / f'{i}.png'
        Image.fromarray(np.full((3, 4, 3), i, np.uint8), 'RGB').save(str(p))
        paths.append(str(p))
    for ahead in (0, 2):
        got = list(inference._decoded(paths, ahead))
        assert [p for p, _ in got] == paths and all(int(a[0, 0, 0]) == i and a.shape == (3, 4, 3) for i, (_, a) in enumerate(got))
        it = inference._decoded(paths[:2] + [str(tmp_path / 'missing.png')] + paths[2:], ahead)
        assert next(it)[0] == paths[0] and next(it)[0] == paths[1]
        with pytest.raises(FileNotFoundError):
            next(it)
    it = inference._decoded(paths, 2)                       # abandoned early: the reader thread ends
    next(it)
    it.close()
    assert not [t for t in threading.enumerate() if t.name == 'decode-ahead']

"""Fast JPEG output without a GPU (femasr_amd/jpegio.py): the definition of the coefficients, the scan and the file, the host
C++ Huffman coder against the plain-Python one, the writer's untouched default and the CLI surface.

Pillow's decoder is the independent judge of every file; a float64 DCT is the judge of the integer one.  The bounds that are measured
figures (MEASURED below) are recorded, with the cases they were measured on, in profiles/jpeg_io_report.txt."""
import ctypes
import functools
import io
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from PIL import Image

from femasr_amd import _lib, jpegio, pngio
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/jpeg_io_report.txt: the worst figures seen on the cases of this file
MEASURED = {
    'arbiter_levels': 3,           # gray levels between Pillow's decode and the float64 decode of the same coefficients (gray and '444')
    'psnr_deficit_db': 0.354,      # PSNR of Pillow's file minus PSNR of ours, same settings, worst image
    'size_ratio': 1.033,           # bytes of our file / bytes of Pillow's non-optimised file, worst image
}
PSNR_CAP_DB = 0.5                  # must hold whatever was measured
PIL_SUBSAMPLING = {'444': 0, '420': 2}


def _exact_dct():
    return jpegio._dct_exact() / 8192.0


def _natural(comp, q=None):
    """int16 (Hb, Wb, 64) zigzag -> float64 (Hb, Wb, 8, 8) F[w][u], times the natural-order table q if given."""
    nat = np.zeros(comp.shape, np.float64)
    nat[..., jpegio.ZIGZAG] = comp
    if q is not None:
        nat = nat * q
    return nat.reshape(comp.shape[:2] + (8, 8))


def _planes(blocks):
    hb, wb = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(8 * hb, 8 * wb)


def _float_decode(comps, quality, H, W):
    """Dequantise, float64 IDCT, inverse JFIF colour - the structure of a decoder (samples rounded and clamped, then the pixels)."""
    A = _exact_dct()
    tabs = jpegio.quant_tables(quality)
    planes = [np.clip(np.rint(_planes(np.einsum('vy,hwvu,ux->hwyx', A, _natural(c, tabs[0 if i == 0 else 1]), A)) + 128), 0, 255)
              for i, c in enumerate(comps)]
    if len(planes) == 1:
        return planes[0][:H, :W].astype(np.uint8)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255)[:H, :W].astype(np.uint8)


def _block_checker(h, w, channels=3):
    yy, xx = np.mgrid[0:h, 0:w]
    g = (((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)
    return g if channels == 1 else np.repeat(g[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (image, quality, subsampling): the files of the entropy, arbiter and pool tests."""
    rng = np.random.RandomState(11)
    out = {}
    for h, w in ((1, 1), (7, 9), (16, 16), (17, 33), (144, 40)):
        rgb = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        out[f'rgb420_{h}x{w}'] = (rgb, 90, '420')
        out[f'rgb444_{h}x{w}'] = (rgb, 75, '444')
        out[f'gray_{h}x{w}'] = (rgb[..., 1].copy(), 50, '420')
    out['noise_q100_444'] = (rng.randint(0, 256, (40, 48, 3)).astype(np.uint8), 100, '444')
    out['noise_q100_gray'] = (rng.randint(0, 256, (40, 48)).astype(np.uint8), 100, '444')
    out['checker_q100_444'] = (_block_checker(32, 40), 100, '444')
    smooth = np.clip(128 + np.cumsum(rng.randint(-3, 4, (37, 53, 3)), axis=0) + np.cumsum(rng.randint(-3, 4, (37, 53, 3)), axis=1), 0, 255)
    out['smooth_q90_444'] = (smooth.astype(np.uint8), 90, '444')
    out['smooth_q90_420'] = (smooth.astype(np.uint8), 90, '420')
    return out


@functools.lru_cache(maxsize=None)
def _case_file(name):
    """(coefficients, encode_ref's bytes) of a case, computed once."""
    img, q, ss = _cases()[name]
    comps = jpegio.coefficients_ref(img, q, ss)
    H, W, C = jpegio.check_shape(img.shape)
    data = jpegio.headers(W, H, C, q, ss) + jpegio.entropy_ref(comps, ss) + b'\xff\xd9'
    return comps, data


def _scan(data):
    at = data.index(b'\xff\xda')
    n = int.from_bytes(data[at + 2:at + 4], 'big')
    assert data[-2:] == b'\xff\xd9'
    return data[at + 2 + n:-2]


def _segments(data):
    out, p = [], 2
    assert data[:2] == b'\xff\xd8'
    while True:
        assert data[p] == 0xFF
        n = int.from_bytes(data[p + 2:p + 4], 'big')
        out.append((data[p + 1], data[p + 4:p + 2 + n]))
        if data[p + 1] == 0xDA:
            return out
        p += 2 + n


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize('quality', [1, 25, 50, 75, 90, 100])
def test_quantisation_tables_are_pillows(quality):
    rng = np.random.RandomState(quality)
    for img, ss in ((rng.randint(0, 256, (17, 33, 3)).astype(np.uint8), '420'), (rng.randint(0, 256, (9, 20)).astype(np.uint8), '444')):
        with Image.open(io.BytesIO(jpegio.encode_ref(img, quality, ss))) as ours:
            ours.load()
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, 'JPEG', quality=quality, subsampling=PIL_SUBSAMPLING[ss])
            with Image.open(io.BytesIO(buf.getvalue())) as theirs:
                assert ours.quantization == theirs.quantization and len(ours.quantization) == (2 if img.ndim == 3 else 1)
                assert ours.size == theirs.size and ours.mode == theirs.mode


def test_segments_and_huffman_tables():
    """The order of the segments, and the four DHT segments are the ones Pillow's (non-optimised) file carries."""
    img = np.random.RandomState(3).randint(0, 256, (17, 33, 3)).astype(np.uint8)
    ours = _segments(jpegio.encode_ref(img, 90, '420'))
    assert [m for m, _ in ours] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert [m for m, _ in _segments(jpegio.encode_ref(img[..., 0], 90))] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDD, 0xDA]
    assert dict(ours)[0xDD] == (3).to_bytes(2, 'big')                     # one interval per MCU row: 33 pixels are three 16-pixel MCUs
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=90)
    theirs = b''.join(body for m, body in _segments(buf.getvalue()) if m == 0xC4)
    tables = [body for m, body in ours if m == 0xC4]
    assert [t[0] for t in tables] == [0x00, 0x10, 0x01, 0x11] and all(t in theirs for t in tables)


def test_reciprocal_multipliers_divide_exactly():
    """The kernel's quotient for every (|c| <= 32767, Q in 1..255): 8.4 M pairs."""
    c, q = np.arange(32768, dtype=np.int64)[:, None], np.arange(1, 256, dtype=np.int64)[None, :]
    assert np.array_equal(((c + (q >> 1)) * jpegio.quant_multipliers(q)) >> 24, (c + (q >> 1)) // q)
    assert int(jpegio.quant_multipliers(q).max()) == 1 << 24


# ------------------------------------------------------------------------------------------------ the DCT
def _dct_inputs():
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:64, 0:64]
    step = np.zeros((64, 64), np.uint8)
    step[:, 29:] = 255
    step[37:] = 255 - step[37:]
    return {'noise': rng.randint(0, 256, (64, 64)).astype(np.uint8), 'only0_255': (rng.randint(0, 2, (64, 64)) * 255).astype(np.uint8),
            'checker1': (((yy + xx) & 1) * 255).astype(np.uint8), 'step': step, 'flat': np.full((64, 64), 201, np.uint8)}


def test_dct_within_derived_bound():
    """Q = 100: every table entry is 1, the coefficients are the DCT itself.  Held to jpegio.DCT_BOUND, the bound the module derives."""
    assert all(int(v) == 1 for q in jpegio.quant_tables(100) for v in q)
    assert 0.5 < jpegio.DCT_BOUND < 1.0
    A = _exact_dct()
    worst = {}
    for name, img in _dct_inputs().items():
        got = _natural(jpegio.coefficients_ref(img, 100)[0])
        v = img.astype(np.float64).reshape(8, 8, 8, 8).transpose(0, 2, 1, 3) - 128
        want = np.einsum('vy,hwyx,ux->hwvu', A, v, A)
        worst[name] = float(np.abs(got - want).max())
        print(f'dct error {name}: {worst[name]:.4f} (bound {jpegio.DCT_BOUND:.4f})')
    assert max(worst.values()) <= jpegio.DCT_BOUND, worst
    assert worst['flat'] < 0.5 and worst['noise'] > 0.3      # (the comparison is not vacuous)


def test_exact_cases():
    for v in (0, 1, 127, 128, 129, 254, 255):
        for comp in jpegio.coefficients_ref(np.full((9, 17), v, np.uint8), 100):
            assert (comp[..., 0] == 8 * (v - 128)).all() and not comp[..., 1:].any(), v
    rng = np.random.RandomState(6)
    for (h, w), ss in (((13, 19), '444'), ((13, 19), '420'), ((33, 17), '420'), ((1, 1), '420')):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        m = 16 if ss == '420' else 8
        padded = np.pad(img, ((0, -h % m), (0, -w % m), (0, 0)), mode='edge')
        for a, b in zip(jpegio.coefficients_ref(img, 90, ss), jpegio.coefficients_ref(padded, 90, ss)):
            assert a.dtype == np.int16 and np.array_equal(a, b)
        g, gp = jpegio.coefficients_ref(img[..., 0], 90, ss), jpegio.coefficients_ref(padded[:-(-h // 8) * 8, :-(-w // 8) * 8, 0], 90, ss)
        assert len(g) == 1 and np.array_equal(g[0], gp[0])
    red = np.zeros((16, 16, 3), np.uint8)
    red[..., 0] = 255
    cb, cr = ((-11059 * 255 + 32768) >> 16) + 128, min(((32768 * 255 + 32768) >> 16) + 128, 255)
    assert (cb, cr) == (85, 255)
    for ss in ('444', '420'):
        y, pb, pr = jpegio.coefficients_ref(red, 100, ss)
        assert (y[..., 0] == 8 * (((19595 * 255 + 32768) >> 16) - 128)).all() and (pb[..., 0] == 8 * (cb - 128)).all() and (pr[..., 0] == 8 * (cr - 128)).all()
        assert not y[..., 1:].any() and not pb[..., 1:].any() and not pr[..., 1:].any()
    shapes = [c.shape for c in jpegio.coefficients_ref(np.zeros((17, 33, 3), np.uint8), 50, '420')]
    assert shapes == [(4, 6, 64), (2, 3, 64), (2, 3, 64)]


# ------------------------------------------------------------------------------------------------ the scan
@pytest.mark.parametrize('name', sorted(_cases()))
def test_cxx_coder_equals_entropy_ref(name):
    img, q, ss = _cases()[name]
    comps, ref = _case_file(name)
    H, W, C = jpegio.check_shape(img.shape)
    assert jpegio.encode_jpeg(comps, W, H, q, ss) == ref
    my, mx, _ = jpegio.geometry(H, W, C, ss)
    lib = _lib.load()
    code = 0 if C == 1 else int(ss)
    whole = jpegio.entropy_rows(comps, ss, 0, my)
    assert whole == _scan(ref) == jpegio.entropy_ref(comps, ss)
    assert len(whole) <= lib.femasr_jpeg_entropy_bound(mx, C, code, my)
    pieces = [jpegio.entropy_rows(comps, ss, r, r + 1) for r in range(my)]
    assert b''.join(pieces) == whole                                      # any cut into row ranges gives the scan
    for r, piece in enumerate(pieces):
        assert len(piece) <= lib.femasr_jpeg_entropy_bound(mx, C, code, 1)
        assert piece == jpegio.entropy_ref(comps, ss, r, r + 1)
        assert (piece[-2:] == bytes((0xFF, 0xD0 + r % 8))) == (r != my - 1)
    if name == 'rgb420_144x40':
        assert my == 9 and pieces[7][-2:] == b'\xff\xd7' and pieces[8 - 0][-2:] != b'\xff\xd0' and pieces[0][-2:] == b'\xff\xd0'


def test_scan_corner_cases_really_occur():
    comps, data = _case_file('noise_q100_444')
    assert b'\xff\x00' in _scan(data)                                     # a stuffed 0xFF
    comps, data = _case_file('checker_q100_444')
    dc = comps[0][..., 0].astype(np.int64)
    assert int(np.abs(np.diff(dc, axis=1)).max()) == 2040                 # black -1024 next to white 1016: size category 11
    with Image.open(io.BytesIO(data)) as im:
        assert np.abs(np.array(im).astype(int) - _cases()['checker_q100_444'][0]).max() <= 2
    comps, _ = _case_file('rgb420_144x40')                                # nine MCU rows: RSTm wraps past 7
    assert comps[1].shape[0] == 9


def test_bytes_do_not_depend_on_the_pool():
    rng = np.random.RandomState(8)
    img = rng.randint(0, 256, (600, 500, 3)).astype(np.uint8)             # 38 MCU rows of 32 MCUs (24 KiB of coefficients each): 3 bands
    comps = jpegio.coefficients_ref(img, 90, '420')
    assert jpegio.band_rows(38, 32 * 6 * 128) == [(0, 11), (11, 22), (22, 38)]
    plain = jpegio.encode_jpeg(comps, 500, 600, 90, '420')
    for n in (1, 3, 8):
        with ThreadPoolExecutor(n) as pool:
            assert jpegio.encode_jpeg(comps, 500, 600, 90, '420', pool=pool) == plain, n
    assert _scan(plain) == b''.join(jpegio.entropy_rows(comps, '420', r0, r1) for r0, r1 in jpegio.band_rows(38, 32 * 6 * 128))
    with Image.open(io.BytesIO(plain)) as im:
        im.load()
        assert im.size == (500, 600)
    small, ref = _case_file('rgb420_17x33')
    for n in (1, 3, 8):
        with ThreadPoolExecutor(n) as pool:
            assert jpegio.encode_jpeg(small, 33, 17, 90, '420', pool=pool) == ref
    assert jpegio.band_rows(5, 1 << 30) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)] and jpegio.band_rows(5, 1) == [(0, 5)]
    assert jpegio.band_rows(7, jpegio.BAND_BYTES // 2) == [(0, 2), (2, 4), (4, 7)]


def test_small_buffer_is_refused_not_overrun():
    comps, ref = _case_file('noise_q100_444')
    lib = _lib.load()
    my, mx = comps[0].shape[:2]
    need = len(_scan(ref))
    p = [c.ctypes.data_as(ctypes.c_void_p) for c in comps]
    for cap in (0, 1, need // 2, need - 1):
        buf = np.full(need + 64, 0xA5, np.uint8)
        n = lib.femasr_jpeg_entropy_rows(p[0], p[1], p[2], 3, 444, my, mx, 0, my, buf.ctypes.data_as(ctypes.c_void_p), cap)
        assert n == -1 and b'do not hold' in lib.femasr_last_error(), cap
        assert (buf[cap:] == 0xA5).all(), cap
    buf = np.full(need + 64, 0xA5, np.uint8)
    assert lib.femasr_jpeg_entropy_rows(p[0], p[1], p[2], 3, 444, my, mx, 0, my, buf.ctypes.data_as(ctypes.c_void_p), need) == need
    assert buf[:need].tobytes() == _scan(ref) and (buf[need:] == 0xA5).all()
    # arguments that are no image, and coefficients outside baseline JPEG
    out = buf.ctypes.data_as(ctypes.c_void_p)
    for args in ((p[0], p[1], p[2], 2, 444, my, mx, 0, my), (p[0], p[1], p[2], 3, 422, my, mx, 0, my), (p[0], None, None, 3, 444, my, mx, 0, my),
                 (p[0], p[1], p[2], 1, 0, my, mx, 0, my), (p[0], p[1], p[2], 3, 444, my, mx, 1, 1), (p[0], p[1], p[2], 3, 444, my, mx, 0, my + 1),
                 (p[0], p[1], p[2], 3, 444, 0, mx, 0, 1), (None, p[1], p[2], 3, 444, my, mx, 0, my)):
        assert lib.femasr_jpeg_entropy_rows(*args, out, need) == -1, args[3:]
    assert lib.femasr_jpeg_entropy_bound(0, 3, 444, 1) == 0 == lib.femasr_jpeg_entropy_bound(4, 2, 444, 1) == lib.femasr_jpeg_entropy_bound(4, 3, 7, 1)
    for k, v in ((0, 2048), (5, 1024), (5, -1024)):
        bad = np.zeros((1, 1, 64), np.int16)
        bad[0, 0, k] = v
        assert lib.femasr_jpeg_entropy_rows(bad.ctypes.data_as(ctypes.c_void_p), None, None, 1, 0, 1, 1, 0, 1, out, need) == -1
        with pytest.raises(ValueError):
            jpegio.entropy_ref([bad])
    ok = np.zeros((1, 1, 64), np.int16)
    ok[0, 0, 0], ok[0, 0, 63] = -2047, 1023
    n = lib.femasr_jpeg_entropy_rows(ok.ctypes.data_as(ctypes.c_void_p), None, None, 1, 0, 1, 1, 0, 1, out, need)
    assert n > 0 and buf[:n].tobytes() == jpegio.entropy_ref([ok])


# ------------------------------------------------------------------------------------------------ Pillow as arbiter
def _arbiter_figures():
    """name -> gray levels between Pillow's decode of the file and the float64 decode of its own coefficients (gray and '444' cases)."""
    out = {}
    for name, (img, q, ss) in sorted(_cases().items()):
        comps, data = _case_file(name)
        with Image.open(io.BytesIO(data)) as im:
            assert im.format == 'JPEG' and im.size == (img.shape[1], img.shape[0]) and im.mode == ('L' if img.ndim == 2 else 'RGB'), name
            dec = np.array(im)
        if img.ndim == 2 or ss == '444':
            out[name] = int(np.abs(dec.astype(int) - _float_decode(comps, q, img.shape[0], img.shape[1]).astype(int)).max())
    return out


def test_pillow_decodes_what_the_coefficients_say():
    figures = _arbiter_figures()
    print('arbiter (gray levels):', figures)
    assert len(figures) >= 12
    assert max(figures.values()) <= MEASURED['arbiter_levels'] + 1, figures
    # what the bound is worth: two neighbouring coefficients of ONE block exchanged are far outside it
    img, q, ss = _cases()['noise_q100_gray']
    good = _case_file('noise_q100_gray')[0]
    comps = [good[0].copy()]
    by, bx = np.unravel_index(np.argmax(np.abs(good[0][..., 1].astype(int) - good[0][..., 2])), good[0].shape[:2])
    comps[0][by, bx, 1], comps[0][by, bx, 2] = good[0][by, bx, 2], good[0][by, bx, 1]
    with Image.open(io.BytesIO(jpegio.encode_jpeg(comps, img.shape[1], img.shape[0], q, ss))) as im:
        moved = np.abs(np.array(im).astype(int) - _float_decode(good, q, *img.shape[:2]).astype(int)).max()
    print('one exchanged pair of coefficients:', moved, 'gray levels')
    assert moved > 4 * (MEASURED['arbiter_levels'] + 1), moved


# ------------------------------------------------------------------------------------------------ quality and size against Pillow's encoder
def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@functools.lru_cache(maxsize=None)
def _parity_figures():
    """[(image, quality, subsampling, PSNR of Pillow's file - PSNR of ours in dB, our bytes / Pillow's bytes)] over the PNG images of the
    testset fixture."""
    g = load_golden('testset_all')
    rows = []
    for i, name in enumerate(str(n) for n in g['names']):
        if not name.endswith('.png'):
            continue
        raw = g['file_bytes'][int(g['file_off'][i]):int(g['file_off'][i + 1])].tobytes()
        img = np.array(Image.open(io.BytesIO(raw)).convert('RGB'))
        H, W = img.shape[:2]
        for ss in ('444', '420'):
            planes = jpegio.planes_ref(img, ss)
            f = [jpegio.fdct_ref(p) for p in planes]                       # (the DCT once per image and subsampling)
            for q in (50, 75, 90):
                tabs = jpegio.quant_tables(q)
                ours = jpegio.encode_jpeg([jpegio.quantise_ref(fi, tabs[0 if k == 0 else 1]) for k, fi in enumerate(f)], W, H, q, ss)
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, 'JPEG', quality=q, subsampling=PIL_SUBSAMPLING[ss])
                with Image.open(io.BytesIO(ours)) as a, Image.open(io.BytesIO(buf.getvalue())) as b:
                    assert a.size == b.size == (W, H)
                    rows.append((name, q, ss, _psnr(np.array(b), img) - _psnr(np.array(a), img), len(ours) / len(buf.getvalue())))
    return rows


def test_quality_and_size_match_pillows_encoder():
    rows = _parity_figures()
    assert len(rows) == 26 * 6
    worst_db = max(rows, key=lambda r: r[3])
    worst_size = max(rows, key=lambda r: r[4])
    print(f'worst PSNR deficit {worst_db[3]:.4f} dB ({worst_db[:3]}), mean {np.mean([r[3] for r in rows]):.4f} dB; '
          f'worst size ratio {worst_size[4]:.4f} ({worst_size[:3]}), mean {np.mean([r[4] for r in rows]):.4f}')
    assert MEASURED['psnr_deficit_db'] + 0.05 <= PSNR_CAP_DB
    assert worst_db[3] <= MEASURED['psnr_deficit_db'] + 0.05, worst_db
    assert worst_size[4] <= MEASURED['size_ratio'] + 0.02, worst_size


def test_coefficients_ref_is_the_sum_of_its_parts():
    img = _cases()['smooth_q90_420'][0]
    for ss in ('444', '420'):
        tabs = jpegio.quant_tables(75)
        parts = [jpegio.quantise_ref(jpegio.fdct_ref(p), tabs[0 if k == 0 else 1]) for k, p in enumerate(jpegio.planes_ref(img, ss))]
        assert all(np.array_equal(a, b) for a, b in zip(parts, jpegio.coefficients_ref(img, 75, ss)))


# ------------------------------------------------------------------------------------------------ refusals, CLI, C ABI, writer
def test_refusals():
    img = np.zeros((8, 8, 3), np.uint8)
    for q in (0, 101, -1, 50.0, '50', None, True):
        with pytest.raises(ValueError):
            jpegio.coefficients_ref(img, q, '420')
        with pytest.raises(ValueError):
            jpegio.encode_ref(img, q)
    for ss in ('422', '411', 4, None, ''):
        with pytest.raises(ValueError):
            jpegio.coefficients_ref(img, 50, ss)
    assert np.array_equal(jpegio.coefficients_ref(img, 50, 420)[1], jpegio.coefficients_ref(img, 50, '420')[1])      # (the integers are accepted)
    for bad in (img.astype(np.float32), img.astype(np.int16), np.zeros((0, 8, 3), np.uint8), np.zeros((8, 0), np.uint8), np.zeros((8, 8, 2), np.uint8),
                np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 1), np.uint8), np.zeros((8,), np.uint8), np.zeros((2, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            jpegio.coefficients_ref(bad, 50, '420')
        with pytest.raises(ValueError):
            jpegio.encode_ref(bad, 50, '420')
    for shape in ((65536, 1), (1, 65536), (1, 65536, 3)):
        with pytest.raises(ValueError):
            jpegio.coefficients_ref(np.zeros(shape, np.uint8), 50)
    assert jpegio.coefficients_ref(np.zeros((1, 65535), np.uint8), 50)[0].shape == (1, 8192, 64)
    comps = jpegio.coefficients_ref(img, 50, '444')
    with pytest.raises(ValueError):
        jpegio.encode_jpeg(comps, 9, 8, 50, '444')                        # planes of another image size
    with pytest.raises(ValueError):
        jpegio.encode_jpeg(comps, 8, 8, 50, '420')
    with pytest.raises(ValueError):
        jpegio.encode_jpeg(comps[:2], 8, 8, 50, '444')
    with pytest.raises(ValueError):
        jpegio.encode_jpeg([c.astype(np.int32) for c in comps], 8, 8, 50, '444')
    for kw in (dict(jpeg_quality=0), dict(jpeg_quality=101), dict(jpeg_quality=90, jpeg_subsampling='422')):
        with pytest.raises(ValueError):
            pngio.PngWriter(threads=1, stage=lambda u8, is_png: None, **kw)


def test_cli_flags():
    from femasr_amd import inference
    ap = inference.build_parser()
    text = ap.format_help()
    assert '--jpeg-quality' in text and '--jpeg-subsampling' in text
    args = ap.parse_args([])
    assert args.jpeg_quality is None and args.jpeg_subsampling is None
    inference.check_jpeg_flags(args)
    assert args.jpeg_subsampling is None
    args = ap.parse_args(['--jpeg-quality', '90'])
    inference.check_jpeg_flags(args)
    assert (args.jpeg_quality, args.jpeg_subsampling) == (90, '420')
    args = ap.parse_args(['--jpeg-quality', '35', '--jpeg-subsampling', '444'])
    inference.check_jpeg_flags(args)
    assert (args.jpeg_quality, args.jpeg_subsampling) == (35, '444')
    for argv in (['--jpeg-subsampling', '444'], ['--jpeg-subsampling', '420'], ['--jpeg-quality', '0'], ['--jpeg-quality', '101']):
        with pytest.raises(SystemExit):
            inference.check_jpeg_flags(ap.parse_args(argv))
    for argv in (['--jpeg-quality', '90', '--jpeg-subsampling', '422'], ['--jpeg-quality', 'high']):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    # main() refuses before it looks for a GPU or loads weights
    for argv in (['--jpeg-subsampling', '444', '--synthetic-seed', '1'], ['--jpeg-quality', '0', '--synthetic-seed', '1']):
        with pytest.raises(SystemExit) as e:
            inference.main(argv)
        assert 'jpeg' in str(e.value)


def test_header_and_binding_agree():
    from femasr_amd.csrc import build
    assert '#include "femasr_hip_jpeg.h"' in open(os.path.join(ROOT, 'include', 'femasr_hip.h')).read()
    hdr = open(os.path.join(ROOT, 'include', 'femasr_hip_jpeg.h')).read()
    decl = {name: (res, params) for res, name, params in re.findall(r'^(int|long long|size_t)\s+(femasr_[a-z0-9_]+)\s*\(([^;]*)\);', hdr, re.M)}
    assert set(decl) == set(_lib.JPEG_SIGNATURES) == {'femasr_jpeg_coefficients_u8', 'femasr_jpeg_entropy_rows', 'femasr_jpeg_entropy_bound'}
    restype = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'size_t': ctypes.c_size_t}
    ctype = lambda p: (ctypes.c_void_p if '*' in p else ctypes.c_size_t if p.startswith('size_t') else ctypes.c_int)      # noqa: E731
    for name, (res, params) in decl.items():
        want_res, want_args = _lib.JPEG_SIGNATURES[name]
        assert restype[res] is want_res, name
        assert [ctype(p.strip()) for p in params.replace('\n', ' ').split(',')] == want_args, name
    assert not set(_lib.JPEG_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.JPEG_SIGNATURES)
    assert lib.femasr_version() == _lib.ABI_VERSION == 107
    assert 'jpeg_dct.hip' in build.SOURCES and '../../include/femasr_hip_jpeg.h' in build.HEADERS
    # the coefficient entry refuses without touching a GPU
    for args in ((None, 8, 8, 3, 444), (1, 8, 8, 2, 444), (1, 8, 8, 3, 422), (1, 0, 8, 3, 444), (1, 8, 65536, 1, 0)):
        assert lib.femasr_jpeg_coefficients_u8(*args, 1, 1, 16, 16, 16, None) == -1, args
    assert lib.femasr_jpeg_coefficients_u8(1, 8, 8, 3, 444, 1, 1, 16, 16, 8, None) == -1 and b'aligned' in lib.femasr_last_error()
    assert lib.femasr_jpeg_coefficients_u8(1, 8, 8, 1, 0, 1, None, 16, 16, None, None) == -1


class _HostStage:
    """A `stage=` stub of PngWriter: host arrays in place of GPU tensors."""

    def __init__(self):
        self.calls = []

    def __call__(self, u8, is_png):
        self.calls.append(is_png)
        return (pngio.filter_image(u8) if is_png else np.ascontiguousarray(u8)), (lambda: None), (lambda: None)


def test_writer_without_jpeg_quality_is_unchanged(tmp_path):
    rng = np.random.RandomState(9)
    rgb, gray = rng.randint(0, 256, (17, 33, 3)).astype(np.uint8), rng.randint(0, 256, (24, 40)).astype(np.uint8)
    stage = _HostStage()
    with pngio.PngWriter(threads=2, stage=stage) as w:
        assert w.jpeg_quality is None and w.jpeg_subsampling is None
        w.submit(rgb, tmp_path / 'a.jpg')
        w.submit(gray, tmp_path / 'b.JPEG')
        w.submit(rgb, tmp_path / 'c.png')
    assert stage.calls == [False, False, True]
    for name, img in (('a.jpg', rgb), ('b.JPEG', gray)):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG')
        assert (tmp_path / name).read_bytes() == buf.getvalue(), name      # Image.save's own defaults, as on the parent commit
    assert (tmp_path / 'c.png').read_bytes() == pngio.encode_png(pngio.filter_rows(rgb), 33, 17)
    # with a quality set, images JPEG cannot hold stay on the Image.save branch, which refuses them as ever
    stage = _HostStage()
    w = pngio.PngWriter(threads=1, stage=stage, jpeg_quality=90)
    assert (w.jpeg_quality, w.jpeg_subsampling) == (90, '420')
    w.submit(rgb, tmp_path / 'd.bmp')
    w.submit(rng.randint(0, 256, (8, 8, 4)).astype(np.uint8), tmp_path / 'rgba.jpg')
    with pytest.raises(OSError):
        w.close()
    assert stage.calls == [False, False] and (tmp_path / 'd.bmp').exists()

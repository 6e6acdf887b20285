"""Gray / gray + alpha / RGBA through inference without a GPU (femasr_amd/channels.py, femasr_amd/pngio.py): the definitions,
the PNG writer for 1, 2 and 4 bytes per pixel, the decoder's mode table and the parser.  Pillow is the independent judge: its convert('L')
for the gray, its decoder for every file.  Everything is integers or fp64 in a fixed order: bit for bit, no tolerance."""
import ctypes
import io
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from PIL import Image

from femasr_amd import channels as CH
from femasr_amd import _lib, inference, pngio
from femasr_amd.models.femasr_model import imresize, imresize_tables


def _rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ gray
def test_gray_ref_is_pillows_convert_L():
    cube = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    grays = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    rand = _rng(1).integers(0, 256, (1 << 20, 3), dtype=np.uint8)
    for px in (cube, grays, rand):
        img = px.reshape(-1, 256 if len(px) % 256 == 0 else len(px), 3)
        want = np.array(Image.fromarray(img, 'RGB').convert('L'))
        assert np.array_equal(CH.gray_ref(img), want)
    assert np.array_equal(CH.gray_ref(grays), np.arange(256, dtype=np.uint8))              # (g,g,g) -> g
    assert CH.gray_ref(cube).tolist() == [0, 29, 150, 179, 76, 105, 226, 255]
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2, 3), np.float32)):
        with pytest.raises(ValueError):
            CH.gray_ref(bad)


# ------------------------------------------------------------------------------------------------ split / merge
@pytest.mark.parametrize('c', [1, 2, 3, 4])
def test_split_merge_round_trip(c):
    img = _rng(c).integers(0, 256, (5, 7, c), dtype=np.uint8)
    for x in ((img, img[..., 0]) if c == 1 else (img,)):
        rgb, a = CH.split_ref(x)
        assert rgb.shape == (5, 7, 3) and rgb.dtype == np.uint8 and (a is None) == (c in (1, 3))
        if c <= 2:
            assert all(np.array_equal(rgb[..., k], img[..., 0]) for k in range(3))
        else:
            assert np.array_equal(rgb, img[..., :3])
        if a is not None:
            assert a.shape == (5, 7) and np.array_equal(a, img[..., -1])
        back = CH.merge_ref(rgb, a, c)
        assert np.array_equal(back, img[..., 0] if c == 1 else img)
        ident = lambda v: v                                                                # a x1 'network': the driver is the round trip
        for mode in CH.ALPHA_MODES:
            assert np.array_equal(CH.upscale_ref(x, ident, 1, mode), x)


def test_split_merge_refusals():
    z = np.zeros((4, 4, 3), np.uint8)
    a = np.zeros((4, 4), np.uint8)
    for bad in (np.zeros((4, 4, 5), np.uint8), np.zeros((4,), np.uint8), np.zeros((2, 4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.int16),
                np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            CH.split_ref(bad)
    for alpha, c in ((None, 2), (None, 4), (a, 1), (a, 3), (None, 0), (None, 5), (a[:3], 4)):
        with pytest.raises(ValueError):
            CH.merge_ref(z, alpha, c)
    with pytest.raises(ValueError):
        CH.merge_ref(np.zeros((4, 4, 4), np.uint8), a, 4)
    with pytest.raises(ValueError):
        CH.upscale_ref(z, lambda v: v, 1, 'nearest')


# ------------------------------------------------------------------------------------------------ the bicubic alpha
def _smallest_length(s):
    for n in range(1, 64):
        try:
            imresize_tables(n, n * s, s)
            return n
        except ValueError:
            pass
    raise AssertionError('no length up to 63 is accepted')


@pytest.mark.parametrize('s', [2, 4])
def test_alpha_up_ref(s):
    a = _rng(s).integers(0, 256, (9, 13), dtype=np.uint8)
    got = CH.alpha_up_ref(a, s)
    want = np.rint(np.clip(imresize(a.astype(np.float64), s), 0, 255)).astype(np.uint8)
    assert got.dtype == np.uint8 and got.shape == (9 * s, 13 * s) and np.array_equal(got, want)
    for cell in (1, 3):                                                                    # 0 / 255 checkerboards: the bicubic overshoots, the clip is needed
        board = ((np.add.outer(np.arange(9) // cell, np.arange(13) // cell) & 1) * 255).astype(np.uint8)
        raw = imresize(board.astype(np.float64), s)
        assert raw.min() < -1 and (cell == 1 or raw.max() > 256)
        assert np.array_equal(CH.alpha_up_ref(board, s), np.rint(np.clip(raw, 0, 255)).astype(np.uint8))
    for v in (0, 1, 127, 128, 254, 255):
        assert (CH.alpha_up_ref(np.full((9, 13), v, np.uint8), s) == v).all(), v
    n0 = _smallest_length(s)
    for n in range(1, n0):
        with pytest.raises(ValueError):
            CH.alpha_up_ref(np.zeros((n, 9), np.uint8), s)
        with pytest.raises(ValueError):
            CH.alpha_up_ref(np.zeros((9, n), np.uint8), s)
    assert CH.alpha_up_ref(np.zeros((n0, n0), np.uint8), s).shape == (n0 * s, n0 * s)
    for bad_s in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            CH.alpha_up_ref(a, bad_s)


# ------------------------------------------------------------------------------------------------ PNG for 1, 2 and 4 bytes per pixel
def _idat(png):
    pos, body = 8, b''
    while pos < len(png):
        n, kind = struct.unpack('>I4s', png[pos:pos + 8])
        if kind == b'IDAT':
            body += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return body


def test_filter_image_c3_is_filter_rows():
    for h, w in ((1, 1), (2, 3), (7, 17)):
        img = _rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        for f in (0, 1, 2, 3, 4, 'adaptive'):
            assert np.array_equal(pngio.filter_image(img, f), pngio.filter_rows(img, f))
    for bad in (np.zeros((2, 2, 5), np.uint8), np.zeros((2, 2, 3), np.int8), np.zeros((2,), np.uint8), np.zeros((0, 2), np.uint8)):
        with pytest.raises(ValueError):
            pngio.filter_image(bad)


@pytest.mark.parametrize('c', [1, 2, 4])
def test_png_files_of_every_layout(c):
    mode = {1: 'L', 2: 'LA', 4: 'RGBA'}[c]
    for h in (1, 2, 7):
        for w in (1, 2, 3, 5, 16, 17):
            steps = _rng(100 * h + w).integers(-3, 4, (h, w, c))
            img = np.clip(128 + np.cumsum(steps, axis=0) + np.cumsum(steps, axis=1), 0, 255).astype(np.uint8)      # image-like: the filters compete
            img = img[..., 0] if c == 1 else img
            for f in (0, 1, 2, 3, 4, 'adaptive'):
                rows = pngio.filter_image(img, f)
                assert rows.shape == (h, 1 + c * w) and rows.dtype == np.uint8
                if f != 'adaptive':
                    assert (rows[:, 0] == f).all()
                png = pngio.encode_png(rows, w, h, channels=c)
                im = Image.open(io.BytesIO(png))
                assert im.mode == mode and im.size == (w, h) and np.array_equal(np.array(im), img), (h, w, f)
                assert zlib.decompress(_idat(png)) == rows.tobytes()
    with pytest.raises(ValueError):
        pngio.encode_png(pngio.filter_image(img), w, h, channels=3)                        # rows of another pixel size
    with pytest.raises(ValueError):
        pngio.encode_png(pngio.filter_image(img), w, h, channels=5)


def test_file_bytes_do_not_depend_on_the_thread_count():
    img = _rng(5).integers(0, 256, (1800, 300, 4), dtype=np.uint8)                        # 2 (gray) to 8 (RGBA) bands of 256 KiB
    for x, c in ((img, 4), (img[..., :2], 2), (img[..., 0], 1)):
        rows = pngio.filter_image(np.ascontiguousarray(x))
        assert len(pngio.band_rows(rows.shape[0], rows.shape[1])) >= 2
        one = pngio.encode_png(rows, 300, 1800, level=1, channels=c)
        for threads in (1, 3):
            with ThreadPoolExecutor(threads) as pool:
                assert pngio.encode_png(rows, 300, 1800, level=1, pool=pool, channels=c) == one
        buf = io.BytesIO()
        assert pngio.write_png(buf, rows, 300, 1800, level=1, channels=c) == len(one) and buf.getvalue() == one
        assert np.array_equal(np.array(Image.open(io.BytesIO(one))), x)


# ------------------------------------------------------------------------------------------------ decoder and parser
def test_decoder_mode_table(tmp_path):
    rng = _rng(9)
    rgba = rng.integers(0, 256, (6, 5, 4), dtype=np.uint8)
    cases = {'L': Image.fromarray(rgba[..., 0], 'L'), 'LA': Image.fromarray(rgba[..., :2], 'LA'), 'RGBA': Image.fromarray(rgba, 'RGBA'),
             'RGB': Image.fromarray(rgba[..., :3], 'RGB'), '1': Image.fromarray(rgba[..., 0], 'L').convert('1'),
             'I16': Image.fromarray(rgba[..., 0].astype(np.uint16) * 257)}
    pal = Image.fromarray(rgba[..., :3], 'RGB').quantize(8)
    cases['P'] = pal
    paths = {}
    for name, im in cases.items():
        paths[name] = str(tmp_path / f'{name}.png')
        im.save(paths[name])
    paths['Pt'] = str(tmp_path / 'Pt.png')
    pal.save(paths['Pt'], transparency=2)
    assert Image.open(paths['Pt']).mode == 'P' and 'transparency' in Image.open(paths['Pt']).info
    assert Image.open(paths['P']).mode == 'P' and 'transparency' not in Image.open(paths['P']).info
    assert Image.open(paths['I16']).mode.startswith('I;16')
    for name, path in paths.items():                                                       # without the flag: RGB as ever
        assert np.array_equal(inference._decode(path), np.array(Image.open(path).convert('RGB'))), name
    keep = {name: inference._decode(path, True) for name, path in paths.items()}
    assert keep['L'].shape == (6, 5) and np.array_equal(keep['L'], rgba[..., 0])
    assert keep['1'].shape == (6, 5) and set(np.unique(keep['1'])) <= {0, 255} and np.array_equal(keep['1'], np.array(cases['1'].convert('L')))
    assert keep['LA'].shape == (6, 5, 2) and np.array_equal(keep['LA'], rgba[..., :2])
    assert keep['RGBA'].shape == (6, 5, 4) and np.array_equal(keep['RGBA'], rgba)
    assert keep['Pt'].shape == (6, 5, 4) and np.array_equal(keep['Pt'], np.array(Image.open(paths['Pt']).convert('RGBA')))
    assert (keep['Pt'][..., 3] == 0).any() and (keep['Pt'][..., 3] == 255).any()
    for name in ('P', 'RGB', 'I16'):
        assert keep[name].shape == (6, 5, 3) and np.array_equal(keep[name], np.array(Image.open(paths[name]).convert('RGB'))), name
    assert all(v.dtype == np.uint8 for v in keep.values())
    got = list(inference._decoded([paths['LA'], paths['RGB']], 2, True))
    assert [a.shape for _, a in got] == [(6, 5, 2), (6, 5, 3)]


def test_parser_defaults():
    ap = inference.build_parser()
    d = ap.parse_args([])
    assert d.keep_format is False and d.alpha == 'bicubic'
    a = ap.parse_args(['--keep-format', '--alpha', 'network'])
    assert a.keep_format is True and a.alpha == 'network'
    with pytest.raises(SystemExit):
        ap.parse_args(['--alpha', 'nearest'])


def test_entries_refuse_before_any_launch():
    """Every call returns FEMASR_ERR_INVALID; none may reach a launch - the pointers are fakes and this process has no GPU context."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.femasr_channels_split_u8(None, p, 1, 4, 4, 3, p, p) == -1
    assert lib.femasr_channels_split_u8(None, p, 1, 4, 4, 1, p, p) == -1 and lib.femasr_channels_split_u8(None, p, 1, 4, 4, 2, p, None) == -1
    assert lib.femasr_channels_split_u8(None, p, 0, 4, 4, 1, p, None) == -1
    merge = lambda rgb, al, an, ch, s=1: lib.femasr_channels_merge_u8(None, rgb, al, an, 4, 4, s, ch, p, p, 4, p, p, 4, p)
    assert merge(p, None, None, 3) == -1 and merge(p, None, None, 2) == -1 and merge(p, p, p, 4) == -1 and merge(p, p, None, 1) == -1
    assert merge(None, None, p, 1) == -1 and merge(None, p, None, 4) == -1 and merge(p, None, None, 1, 0) == -1
    assert lib.femasr_png_filter_u8(None, p, 1, 4, 4, 5, 5, p) == -1 and lib.femasr_png_filter_u8(None, p, 1, 4, 4, 0, 5, p) == -1
    assert lib.femasr_png_filter_u8(None, p, 1, 1, (3 << 22) // 4 + 1, 4, 5, p) == -1 and b'2^22' in lib.femasr_last_error()

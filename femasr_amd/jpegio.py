"""Fast JPEG output (opt-in): the arithmetic half of a baseline JPEG encoder - colour, 8x8 DCT, quantisation, zigzag - in ONE
launch on the GPU, the entropy coding in independent restart intervals on the writer's thread pool (host C++ in the same library).

    coefficients_ref(img, quality, subsampling)     the DEFINITION (numpy, integers only): quantised zigzag coefficients per component
    coefficients_gpu(u8, quality, subsampling)      the same int16 planes from ONE femasr_jpeg_coefficients_u8 launch (csrc/jpeg_dct.hip)
    entropy_ref(components, subsampling)            plain-Python baseline Huffman coder of the scan (slow: small images only)
    encode_ref(img, quality, subsampling)           the whole file from the two above
    encode_jpeg(coeffs, width, height, quality, subsampling, pool=None)
                                                    the same bytes with femasr_jpeg_entropy_rows coding bands of MCU rows on `pool`
    quant_tables(quality) / quant_multipliers(q)    the two scaled tables; the reciprocal multipliers the kernel divides with
    decode_ref(components, quality, subsampling, H, W)   the DEFINITION of the way back (numpy, integers only): uint8 (H,W) / (H,W,3) pixels
    decode_gpu(planes, quality, subsampling, H, W, float32=False)
                                                    the same pixels from ONE femasr_jpeg_decode_u8 launch (csrc/degrade.hip)

Definition.  img: uint8 (H,W) gray or (H,W,3) RGB, 1 <= H, W <= 65535.  quality: an integer 1..100.  subsampling: '444' or '420' (a gray image
ignores it).  All arithmetic is integer (int32 suffices everywhere; numpy runs the sums in int64), `>>` is the arithmetic shift (floor).
  Colour (JFIF full range, 16-bit fixed point; a gray image is its own Y):
      Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
      Cb = clip(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255)
      Cr = clip((( 32768 R - 27439 G -  5329 B + 32768) >> 16) + 128, 0, 255)
  Padding: the last column, then the last row, are replicated up to a whole MCU (minimum coded unit): 8x8 pixels for gray and '444',
      16x16 for '420'.
  '420' chroma: (a + b + c + d + 2) >> 2 over each 2x2 cell of the padded Cb / Cr plane.
  DCT per 8x8 block p of a plane: v = p - 128;  T[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u > 0) = 1/2 (DCT_TABLE);
      row pass     R[y][u] = (sum_x T[u][x] v[y][x] + 512) >> 10          (R is 8 times the exact row transform: 3 more bits)
      column pass  F[w][u] = (sum_y T[w][y] R[y][u] + 32768) >> 16
      |sum_x| <= 128 * 23168 < 2^22, |R| <= 2897, |sum_y| <= 2897 * 23168 < 2^27: every intermediate fits int32 (R fits int16).
  Quantisation: base tables of Annex K (luminance for Y, chrominance for Cb / Cr), scaled by IJG's rule s = 5000 // q if q < 50 else 200 - 2 q,
      Q = clip((base s + 50) // 100, 1, 255);  k = sign(F) ((|F| + (Q >> 1)) // Q).
  Output: per component one int16 (Hb, Wb, 64) array, block (by, bx) of the padded plane, coefficient F[w][u] at position ZIGZAG^-1[8 w + u].
      gray: [Y];  '444': [Y, Cb, Cr] of (ceil(H/8), ceil(W/8)) blocks;  '420': Y of (2 ceil(H/16), 2 ceil(W/16)), Cb, Cr of (ceil(H/16), ceil(W/16)).

The DCT's distance from the exact one (DCT_BOUND, before quantisation).  dT = |T - T_exact| per entry (at most 0.472 on this table).
  row pass:    |R - 8 R_exact| <= 1/2 (the shift's rounding) + sum_x dT |v| / 1024 <= 1/2 + max_u sum_x dT[u][x] * 128 / 1024       =: E_R
  column pass: |F - F_exact| <= 1/2 + (max_w sum_y |T[w][y]|) E_R / 65536 + (max_w sum_y dT[w][y]) max|8 R_exact| / 65536,   max|8 R_exact| <= 2897
  With the table's own numbers this is dct_bound() = 0.918; what noise, checkerboards and steps show is 0.61 (tests/test_jpeg_io_host.py
  holds the derived figure, profiles/jpeg_io_report.txt has the measured ones).  A flat block of value p gives F[0][0] = 8 (p - 128) exactly and
  0 elsewhere: the rows of T for u > 0 sum to 0, and 23168^2 / 2^26 = 7.9983, off 8 by 0.0017 * 128 + 0.18 < 1/2.

The way back (decode_ref; the JPEG "noise" of femasr_amd.degrade is coefficients followed by this - Huffman coding is lossless, so no entropy
coder runs).  components: the int16 planes above, one (gray) or three.  Integers only, int32 suffices:
  Dequantisation: F[w][u] = clip(k Q, -2047, 2047).  What the encoder above writes satisfies |k Q| <= |F| + Q / 2 <= 1025 + 127, so the clip
      changes nothing there; it bounds the sums for planes from elsewhere.
  Column pass  C[y][u] = (sum_w T[w][y] F[w][u] + 512) >> 10        max_y sum_w |T[w][y]| = 21641: |sum| <= 21641 * 2047 < 2^26, |C| <= 43261
  Row pass     p[y][x] = clip(((sum_u T[u][x] C[y][u] + 32768) >> 16) + 128, 0, 255)        |sum| <= 21641 * 43261 < 2^30
      (the transposed passes of the encoder with its shifts: C is 8 times the exact column transform, p the exact inverse within the rounding)
  '420' chroma at pixel (y, x), c the decoded (padded) chroma plane: i = y >> 1, i' = i - 1 for even y and i + 1 for odd y, clamped to the
      plane (replicated edge), j, j' likewise from x:  (9 c[i][j] + 3 c[i'][j] + 3 c[i][j'] + c[i'][j'] + 8) >> 4   (the triangle filter)
  Colour (JFIF inverse, 16-bit fixed point; cb = Cb - 128, cr = Cr - 128; a gray image is its Y):
      R = clip(Y + ((91881 cr + 32768) >> 16), 0, 255)          |91881 * 128| < 2^24
      G = clip(Y + ((-22554 cb - 46802 cr + 32768) >> 16), 0, 255)
      B = clip(Y + ((116130 cb + 32768) >> 16), 0, 255)
  The planes are cropped to H x W.  Not libjpeg's decoder bit for bit (another IDCT, and libjpeg rounds the two passes of its upsampling
  separately): tests/test_degrade_host.py holds the distance from Pillow on the bytes of encode_ref, profiles/degrade_report.txt records it.

The scan (entropy_ref; femasr_jpeg_entropy_rows gives the same bytes).  Baseline Huffman with the four Annex K tables (DC / AC, luminance for
component 0, chrominance for 1 and 2).  ONE RESTART INTERVAL PER MCU ROW (DRI = MCUs per row): the DC predictors are 0 at the start of every
interval, the interval is padded with 1-bits to a byte, every 0xFF byte of it is followed by 0x00, and every interval but the last is followed by
RSTm, m = (index of the MCU row) mod 8.  MCU: gray [Y]; '444' [Y, Cb, Cr]; '420' [Y(2my, 2mx), Y(2my, 2mx+1), Y(2my+1, 2mx), Y(2my+1, 2mx+1), Cb, Cr].
A DC difference needs at most 11 extra bits (|diff| <= 2047), an AC coefficient at most 10 (|k| <= 1023): the definition stays inside that,
arrays from elsewhere that do not are refused.

The file (encode_ref, encode_jpeg): SOI, APP0 'JFIF' 1.01 with density 1:1 and no thumbnail, one DQT segment per table (8-bit, zigzag order),
SOF0, one DHT segment per Huffman table (DC0, AC0 and, for colour, DC1, AC1), DRI, SOS, the scan, EOI.  The bytes depend on the pixels,
`quality` and `subsampling` only - never on the thread count, the pool or timing: bands of MCU rows are cut by BAND_BYTES of coefficients.
The file is not libjpeg's: neither its coefficients (another DCT, another chroma filter) nor its bytes (restart intervals).
"""
import ctypes
import struct

import numpy as np

BAND_BYTES = 256 * 1024        # coefficient bytes per band of MCU rows at least (encode_jpeg); never derived from the thread count
MAX_DIM = 65535
SUBSAMPLINGS = ('444', '420')

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  np.int64)             # natural index 8 w + u of the coefficient at zigzag position k

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] +
                       [99] * 32, np.int64)

# Annex K Huffman tables: (number of codes of length 1..16, the symbols in code order)
_AC_LUMA_VALS = bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a'
    '535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7'
    'c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
_AC_CHROMA_VALS = bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a'
    '535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6'
    'c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')
HUFFMAN = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),                       # (class 0 = DC / 1 = AC, table id)
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), _AC_LUMA_VALS),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _AC_CHROMA_VALS),
}


def _dct_exact():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    a = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    return 8192.0 * a * np.cos((2 * x + 1) * u * np.pi / 16)


DCT_TABLE = np.rint(_dct_exact()).astype(np.int64)      # T[u][x]


def dct_bound():
    """The derived bound of the module docstring on |F - F_exact| before quantisation, from the table's own rounding errors."""
    dt = np.abs(DCT_TABLE - _dct_exact())
    e_r = 0.5 + dt.sum(axis=1).max() * 128 / 1024
    return 0.5 + np.abs(DCT_TABLE).sum(axis=1).max() * e_r / 65536 + dt.sum(axis=1).max() * 2897 / 65536


DCT_BOUND = dct_bound()


def _check_params(quality, subsampling):
    if not isinstance(quality, (int, np.integer)) or isinstance(quality, bool) or not 1 <= int(quality) <= 100:
        raise ValueError(f'jpeg quality must be an integer in 1..100, got {quality!r}')
    subsampling = str(subsampling) if isinstance(subsampling, (int, np.integer)) and not isinstance(subsampling, bool) else subsampling
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"jpeg subsampling must be '444' or '420', got {subsampling!r}")
    return int(quality), subsampling


def check_shape(shape, what='jpegio'):
    """(H, W, channels) of a (H,W) or (H,W,3) image shape; anything else is refused."""
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3) or min(shape) < 1:
        raise ValueError(f'{what}: expected a non-empty uint8 (H,W) gray or (H,W,3) RGB image, got shape {tuple(shape)}')
    if shape[0] > MAX_DIM or shape[1] > MAX_DIM:
        raise ValueError(f'{what}: JPEG holds at most {MAX_DIM} x {MAX_DIM} pixels, got {shape[1]} x {shape[0]}')
    return int(shape[0]), int(shape[1]), 1 if len(shape) == 2 else 3


def quant_tables(quality):
    """(luminance, chrominance): int64 (64,) in NATURAL order (index 8 w + u), IJG's scaling of the Annex K tables, 1..255."""
    quality, _ = _check_params(quality, '444')
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def quant_multipliers(q):
    """M = ceil(2^24 / Q): (n M) >> 24 == n // Q for every 0 <= n < 2^16 and 1 <= Q <= 255 (n (M Q - 2^24) < 2^16 * 255 < 2^24), in 64-bit
    arithmetic (n M reaches 2^40).  The kernel divides with these; the definition uses //."""
    q = np.asarray(q, np.int64)
    return ((1 << 24) + q - 1) // q


def geometry(height, width, channels, subsampling):
    """(MCU rows, MCUs per row, [(Hb, Wb) per component])."""
    m = 16 if channels == 3 and subsampling == '420' else 8
    my, mx = -(-height // m), -(-width // m)
    if channels == 1:
        return my, mx, [(my, mx)]
    if subsampling == '444':
        return my, mx, [(my, mx)] * 3
    return my, mx, [(2 * my, 2 * mx), (my, mx), (my, mx)]


def planes_ref(img, subsampling='420'):
    """The padded (and, for '420', subsampled) int64 planes the DCT runs on: [Y] or [Y, Cb, Cr], values 0..255."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f'jpegio: expected a uint8 image, got {img.dtype}')
    H, W, C = check_shape(img.shape)
    x = img.astype(np.int64)
    if C == 1:
        planes = [x]
    else:
        r, g, b = x[..., 0], x[..., 1], x[..., 2]
        planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                  np.clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0, 255),
                  np.clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0, 255)]
    m = 16 if C == 3 and subsampling == '420' else 8
    planes = [np.pad(p, ((0, -H % m), (0, -W % m)), mode='edge') for p in planes]
    if m == 16:
        planes[1:] = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in planes[1:]]
    return planes


def fdct_ref(plane):
    """int64 (8 Hb, 8 Wb) plane of 0..255 -> int64 (Hb, Wb, 8, 8) F[w][u] of the definition (not quantised)."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    v = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    r = (np.einsum('hwyx,ux->hwyu', v, DCT_TABLE) + 512) >> 10
    return (np.einsum('vy,hwyu->hwvu', DCT_TABLE, r) + 32768) >> 16


def quantise_ref(f, q):
    """F (.., 8, 8) and a natural-order table -> int16 (.., 64) in zigzag order."""
    f = f.reshape(f.shape[:-2] + (64,))
    k = np.sign(f) * ((np.abs(f) + (q >> 1)) // q)
    return np.ascontiguousarray(k[..., ZIGZAG].astype(np.int16))


def coefficients_ref(img, quality, subsampling='420'):
    """The definition (module docstring): uint8 (H,W) / (H,W,3) -> [int16 (Hb, Wb, 64)] per component, zigzag order, quantised."""
    quality, subsampling = _check_params(quality, subsampling)
    qy, qc = quant_tables(quality)
    return [quantise_ref(fdct_ref(p), qy if i == 0 else qc) for i, p in enumerate(planes_ref(img, subsampling))]


# ---- the way back ----

def idct_ref(f):
    """int64 (.., 8, 8) F[w][u] -> int64 (.., 8, 8) pixels p[y][x], 0..255 (module docstring)."""
    c = (np.einsum('wy,...wu->...yu', DCT_TABLE, f) + 512) >> 10
    return np.clip(((np.einsum('ux,...yu->...yx', DCT_TABLE, c) + 32768) >> 16) + 128, 0, 255)


def _plane_ref(comp, q):
    """int16 (Hb, Wb, 64) zigzag coefficients and a natural-order table -> int64 (8 Hb, 8 Wb) plane."""
    hb, wb = comp.shape[:2]
    nat = np.zeros((hb, wb, 64), np.int64)
    nat[..., ZIGZAG] = comp.astype(np.int64)
    f = np.clip(nat * q, -2047, 2047).reshape(hb, wb, 8, 8)
    return idct_ref(f).transpose(0, 2, 1, 3).reshape(8 * hb, 8 * wb)


def _upsample_ref(c, height, width):
    """The triangle filter of the module docstring: the (h, w) chroma plane at the pixels of a height x width image."""
    y, x = np.arange(height), np.arange(width)
    i, j = y >> 1, x >> 1
    i2 = np.clip(i + np.where(y & 1, 1, -1), 0, c.shape[0] - 1)
    j2 = np.clip(j + np.where(x & 1, 1, -1), 0, c.shape[1] - 1)
    return (9 * c[i][:, j] + 3 * c[i2][:, j] + 3 * c[i][:, j2] + c[i2][:, j2] + 8) >> 4


def decode_ref(components, quality, subsampling, height, width):
    """The definition (module docstring): [int16 (Hb, Wb, 64)] planes of a height x width image -> uint8 (H,W) gray or (H,W,3) RGB."""
    quality, subsampling = _check_params(quality, subsampling)
    comps = _layout(components, subsampling)[0]
    channels = len(comps)
    check_shape((height, width) if channels == 1 else (height, width, 3), 'decode_ref')
    if [c.shape[:2] for c in comps] != geometry(height, width, channels, subsampling)[2]:
        raise ValueError(f'decode_ref: planes {[c.shape for c in comps]} are not those of a {width} x {height} image')
    qy, qc = quant_tables(quality)
    planes = [_plane_ref(c, qy if i == 0 else qc) for i, c in enumerate(comps)]
    yy = planes[0][:height, :width]
    if channels == 1:
        return yy.astype(np.uint8)
    if subsampling == '420':
        cb, cr = (_upsample_ref(p, height, width) - 128 for p in planes[1:])
    else:
        cb, cr = (p[:height, :width] - 128 for p in planes[1:])
    rgb = np.stack([yy + ((91881 * cr + 32768) >> 16), yy + ((-22554 * cb - 46802 * cr + 32768) >> 16), yy + ((116130 * cb + 32768) >> 16)], axis=2)
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ---- the scan ----

def _codes(bits, vals):
    """symbol -> (code, length) of a table given as Annex C builds it."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_CODES = {key: _codes(*tab) for key, tab in HUFFMAN.items()}


def _layout(components, subsampling):
    """Checks the planes against each other; (MCU rows, MCUs per row, [(component, dy, dx)] blocks of an MCU)."""
    comps = [np.asarray(c) for c in components]
    if len(comps) not in (1, 3) or any(c.dtype != np.int16 or c.ndim != 3 or c.shape[2] != 64 or c.size == 0 for c in comps):
        raise ValueError('jpegio: components must be one or three non-empty int16 (Hb, Wb, 64) arrays')
    if len(comps) == 1:
        return comps, comps[0].shape[0], comps[0].shape[1], [(0, 0, 0)]
    _, subsampling = _check_params(50, subsampling)
    my, mx = comps[1].shape[:2]
    f = 2 if subsampling == '420' else 1
    if comps[2].shape != comps[1].shape or comps[0].shape[:2] != (f * my, f * mx):
        raise ValueError(f"jpegio: plane shapes {[c.shape for c in comps]} are not those of subsampling '{subsampling}'")
    blocks = [(0, dy, dx) for dy in range(f) for dx in range(f)] + [(1, 0, 0), (2, 0, 0)]
    return comps, my, mx, blocks


def _category(v):
    return int(abs(v)).bit_length()


def entropy_ref(components, subsampling='420', row0=0, row1=None):
    """The scan of MCU rows row0 .. row1 (default: all) as the module docstring defines it, each interval but the image's last followed by its
    RSTm.  Plain Python, one MCU at a time."""
    comps, my, mx, blocks = _layout(components, subsampling)
    row1 = my if row1 is None else row1
    if not 0 <= row0 < row1 <= my:
        raise ValueError(f'entropy_ref: rows {row0}..{row1} of {my}')
    f = 2 if len(blocks) == 6 else 1
    out = []
    for row in range(row0, row1):
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        for m in range(mx):
            for c, dy, dx in blocks:
                fy = f if c == 0 else 1
                blk = comps[c][fy * row + dy, fy * m + dx].tolist()
                tid = 0 if c == 0 else 1
                diff, pred[c] = blk[0] - pred[c], blk[0]
                size = _category(diff)
                if size > 11:
                    raise ValueError(f'entropy_ref: DC difference {diff} needs more than 11 bits')
                code, length = _CODES[(0, tid)][size]
                acc, nbits = (acc << length) | code, nbits + length
                if size:
                    acc, nbits = (acc << size) | ((diff if diff > 0 else diff - 1) & ((1 << size) - 1)), nbits + size
                ac, run = _CODES[(1, tid)], 0
                for k in range(1, 64):
                    v = blk[k]
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        code, length = ac[0xF0]
                        acc, nbits, run = (acc << length) | code, nbits + length, run - 16
                    size = _category(v)
                    if size > 10:
                        raise ValueError(f'entropy_ref: AC coefficient {v} needs more than 10 bits')
                    code, length = ac[(run << 4) | size]
                    acc, nbits = (acc << length) | code, nbits + length
                    acc, nbits = (acc << size) | ((v if v > 0 else v - 1) & ((1 << size) - 1)), nbits + size
                    run = 0
                if run:
                    code, length = ac[0x00]
                    acc, nbits = (acc << length) | code, nbits + length
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        out.append(acc.to_bytes(nbits // 8, 'big').replace(b'\xff', b'\xff\x00'))
        if row != my - 1:
            out.append(bytes((0xFF, 0xD0 + (row & 7))))
    return b''.join(out)


# ---- the file ----

def _segment(marker, body):
    return struct.pack('>BBH', 0xFF, marker, len(body) + 2) + body


def headers(width, height, channels, quality, subsampling):
    """Everything in front of the scan: SOI .. SOS."""
    quality, subsampling = _check_params(quality, subsampling)
    check_shape((height, width) if channels == 1 else (height, width, channels), 'jpegio.headers')
    _, mx, _ = geometry(height, width, channels, subsampling)
    tables = quant_tables(quality)[:1 if channels == 1 else 2]
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00' + struct.pack('>BBBHHBB', 1, 1, 0, 1, 1, 0, 0))]
    out += [_segment(0xDB, bytes([i]) + bytes(int(v) for v in q[ZIGZAG])) for i, q in enumerate(tables)]
    samp = [0x11] if channels == 1 else [0x22 if subsampling == '420' else 0x11, 0x11, 0x11]
    out.append(_segment(0xC0, struct.pack('>BHHB', 8, height, width, channels) +
                        b''.join(bytes([i + 1, s, 0 if i == 0 else 1]) for i, s in enumerate(samp))))
    for key in [(0, 0), (1, 0)] + ([(0, 1), (1, 1)] if channels == 3 else []):
        bits, vals = HUFFMAN[key]
        out.append(_segment(0xC4, bytes([(key[0] << 4) | key[1]]) + bytes(bits) + vals))
    out.append(_segment(0xDD, struct.pack('>H', mx)))
    out.append(_segment(0xDA, bytes([channels]) + b''.join(bytes([i + 1, 0x00 if i == 0 else 0x11]) for i in range(channels)) + b'\x00\x3f\x00'))
    return b''.join(out)


def encode_ref(img, quality, subsampling='420'):
    """The whole file of an image, from coefficients_ref and entropy_ref."""
    img = np.asarray(img)
    comps = coefficients_ref(img, quality, subsampling)
    H, W, C = check_shape(img.shape)
    return headers(W, H, C, quality, subsampling) + entropy_ref(comps, str(subsampling)) + b'\xff\xd9'


def band_rows(mcu_rows, row_bytes):
    """[(first MCU row, end MCU row)] of the bands: whole MCU rows holding at least BAND_BYTES of coefficients each (the last band takes the
    remainder; fewer than BAND_BYTES in all is one band)."""
    per = max(1, -(-BAND_BYTES // row_bytes))
    nb = max(1, mcu_rows // per)
    return [(k * per, mcu_rows if k == nb - 1 else (k + 1) * per) for k in range(nb)]


def entropy_rows(comps, subsampling, row0, row1):
    """MCU rows row0 .. row1 of the scan through femasr_jpeg_entropy_rows (host C++; ctypes drops the GIL for the call).  comps: contiguous
    int16 (Hb, Wb, 64) host arrays as `_layout` accepts them."""
    from . import _lib
    lib = _lib.load()
    my, mx = (comps[1] if len(comps) == 3 else comps[0]).shape[:2]
    code = 0 if len(comps) == 1 else int(subsampling)
    cap = lib.femasr_jpeg_entropy_bound(mx, len(comps), code, row1 - row0)
    buf = np.empty(cap, np.uint8)
    p = [c.ctypes.data_as(ctypes.c_void_p) for c in comps] + [None] * (3 - len(comps))
    n = lib.femasr_jpeg_entropy_rows(p[0], p[1], p[2], len(comps), code, my, mx, row0, row1, buf.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 0:
        _lib.check(int(n))
    return buf[:n].tobytes()


def encode_jpeg(coeffs, width, height, quality, subsampling='420', pool=None):
    """The bytes of the JPEG file of quantised coefficients `coeffs` ([int16 (Hb, Wb, 64)] host arrays as coefficients_ref returns them) - the
    bytes of encode_ref.  pool: a concurrent.futures executor for the bands (None: this thread); the result does not depend on it."""
    quality, subsampling = _check_params(quality, subsampling)
    comps, my, mx, blocks = _layout([np.ascontiguousarray(c) for c in coeffs], subsampling)
    channels = len(comps)
    if (my, mx, [c.shape[:2] for c in comps]) != geometry(height, width, channels, subsampling)[:3]:
        raise ValueError(f'encode_jpeg: planes {[c.shape for c in comps]} are not those of a {width} x {height} image')
    head = headers(width, height, channels, quality, subsampling)
    jobs = band_rows(my, mx * len(blocks) * 128)
    run = lambda j: entropy_rows(comps, subsampling, j[0], j[1])      # noqa: E731
    done = [run(j) for j in jobs] if pool is None else list(pool.map(run, jobs))
    return head + b''.join(done) + b'\xff\xd9'


# ---- the GPU stage ----

_TABLES = {}


def kernel_tables(quality):
    """The two tables as the kernel reads them: int32 (2, 128), luminance and chrominance - per table the quantiser Q of zigzag position k in
    [k], its multiplier (quant_multipliers) in [64 + k]."""
    return np.stack([np.concatenate((q[ZIGZAG], quant_multipliers(q[ZIGZAG]))) for q in quant_tables(quality)]).astype(np.int32)


def device_tables(quality, device):
    """kernel_tables on a device, cached per (quality, device)."""
    import torch
    device = torch.device(device)
    key = (int(quality), device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(kernel_tables(quality)).to(device)
    return _TABLES[key]


def coefficients_flat_gpu(u8, quality, subsampling='420'):
    """(flat int16 GPU tensor holding the planes one after the other, [views of it per component]) - coefficients_gpu in one allocation, so
    that one copy brings every plane to the host."""
    import torch
    from . import _lib
    quality, subsampling = _check_params(quality, subsampling)
    if not torch.is_tensor(u8) or not u8.is_cuda or u8.dtype != torch.uint8:
        raise ValueError('coefficients_gpu: expected a uint8 (H,W) or (H,W,3) GPU tensor')
    H, W, C = check_shape(tuple(u8.shape), 'coefficients_gpu')
    u8 = u8.contiguous()
    shapes = geometry(H, W, C, subsampling)[2]
    sizes = [hb * wb * 64 for hb, wb in shapes]
    tab = device_tables(quality, u8.device)                      # (cached: a capture must see a warm cache, as with every lazily built table)
    flat = torch.empty(sum(sizes), dtype=torch.int16, device=u8.device)
    views, off = [], 0
    for (hb, wb), n in zip(shapes, sizes):
        views.append(flat[off:off + n].view(hb, wb, 64))
        off += n
    p = [_lib.ptr(v) for v in views] + [None] * (3 - len(views))
    with torch.cuda.device(u8.device):
        _lib.check(_lib.load().femasr_jpeg_coefficients_u8(_lib.ptr(u8), H, W, C, 0 if C == 1 else int(subsampling), _lib.ptr(tab[0]),
                                                           None if C == 1 else _lib.ptr(tab[1]), p[0], p[1], p[2],
                                                           torch.cuda.current_stream(u8.device).cuda_stream))
    return flat, views


def coefficients_gpu(u8, quality, subsampling='420'):
    """`coefficients_ref` of a uint8 (H,W) or (H,W,3) GPU tensor: [int16 (Hb, Wb, 64) GPU tensors], ONE launch on the current stream."""
    return coefficients_flat_gpu(u8, quality, subsampling)[1]


def decode_gpu(planes, quality, subsampling, height, width, float32=False):
    """`decode_ref` of int16 (Hb, Wb, 64) GPU planes (16-byte aligned, as coefficients_gpu returns them): a uint8 (H,W) / (H,W,3) GPU tensor,
    or with float32=True the float32 tensor u8 / 255; ONE launch on the current stream."""
    import torch
    from . import _lib
    quality, subsampling = _check_params(quality, subsampling)
    planes = list(planes)
    if len(planes) not in (1, 3) or any(not torch.is_tensor(p) or not p.is_cuda or p.dtype != torch.int16 or not p.is_contiguous() for p in planes):
        raise ValueError('decode_gpu: expected one or three contiguous int16 (Hb, Wb, 64) GPU tensors')
    channels = len(planes)
    check_shape((height, width) if channels == 1 else (height, width, 3), 'decode_gpu')
    if [tuple(p.shape) for p in planes] != [s + (64,) for s in geometry(height, width, channels, subsampling)[2]]:
        raise ValueError(f'decode_gpu: planes {[tuple(p.shape) for p in planes]} are not those of a {width} x {height} image')
    dev = planes[0].device
    tab = device_tables(quality, dev)
    out = torch.empty((height, width) if channels == 1 else (height, width, 3), dtype=torch.float32 if float32 else torch.uint8, device=dev)
    p = [_lib.ptr(v) for v in planes] + [None] * (3 - channels)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().femasr_jpeg_decode_u8(torch.cuda.current_stream(dev).cuda_stream, p[0], p[1], p[2], channels,
                                                     0 if channels == 1 else int(subsampling), height, width, _lib.ptr(tab[0]),
                                                     None if channels == 1 else _lib.ptr(tab[1]), _lib.ptr(out), 1 if float32 else 0))
    return out

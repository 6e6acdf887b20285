"""Synthesis of low-quality (LQ) inputs on the GPU (opt-in): the BSRGAN degradation of the reference
(basicsr/data/bsrgan_util.py degradation_bsrgan(img, sf, use_crop=False, isp_model=None), which generate_dataset.py and BSRGANTrainDataset
call) and the classical "bicubic / sf" LQ, as explicit RECIPES of a few operations, each operation with a numpy definition here and ONE HIP
kernel (csrc/degrade.hip; the JPEG round trip: three).

    blur_ref / resize_ref / noise_ref / quantize_ref / jpeg_ref      the DEFINITIONS (numpy; float64 or integers), one per operation
    fspecial_gaussian / anisotropic_gaussian / shifted_gaussian      blur kernels, built on the host in float64
    tap_table(filter, n_in, n_out)                                   resize tables: 'bilinear', 'bicubic', 'area', 'matlab'
    sample_recipe(seed, name, h, w, sf, mode='bsrgan')               the Recipe of one file: JSON-serialisable, a function of its arguments alone
    degrade_ref(img_u8, recipe) -> uint8                             the whole chain through the definitions (host)
    apply_op(t, op) / degrade_u8(img_u8_cuda, recipe, out=None)      the same on the GPU: a cuda tensor in, a cuda tensor out

Between operations the image is float32 (H,W,3) RGB in [0,1], as in the reference.  Every definition computes in float64 (or integers) from
float32 inputs and float32 parameters and rounds to float32 ONCE at its end; the kernels accumulate in float32 in a stated order, restated
bit for bit in tests/degrade_ref.py and held to the definitions by derived bounds in tests/test_degrade_host.py.

blur(img, kernel, stride=1).  out[Y][X][c] = sum_i sum_j kernel[i][j] img[m(Y s + r - i)][m(X s + r - j)][c], r = k // 2: a TRUE convolution
  (the kernel is flipped), exactly scipy.ndimage.convolve(img, kernel[..., None], mode='mirror').  kernel: dense (k,k) float32, k odd in 3..25.
  m is the periodic reflection about the edge pixel centres (d c b | a b c d | c b a; period 2 (n - 1); m = 0 for n = 1): valid for any image
  size.  stride s in (1, 2, 4) keeps pixels [0::s, 0::s] - the reference's "blur with the shifted kernel, then nearest downsampling",
  computed only where it is kept.  Kernel, one float32 accumulator per channel from 0: i ascending outside, j ascending inside, multiply and
  add rounded separately (no fma).
    fspecial_gaussian(k, sigma)                 exp(-(x^2 + y^2) / (2 sigma^2)) on the centred grid, entries below eps * max zeroed, normalised
    anisotropic_gaussian(k, theta, l1, l2)      the pdf of N(0, Sigma) on the integer grid centred on the middle tap (gm_blur_kernel's grid),
                                                Sigma = V diag(l1, l2) V^-1, V = [[c, s], [s, -c]], (c, s) = (cos theta, sin theta); normalised
    shifted_gaussian(sf, sigma)                 fspecial_gaussian(25, sigma) sampled bilinearly at (x + (sf - 1) / 2, y + (sf - 1) / 2), the
                                                coordinates clipped to 0..24; renormalised.  shift_pixel without scipy's removed interp2d.
  All three are float64 on the host and cast to float32 once.

resize(img, out_h, out_w, filter).  Separable: H pass, then W pass, each output one accumulator over its taps in ascending order from 0; the
  result is clipped to [0,1].  Tables (tap_table): an int32 source index and a float32 weight per output coordinate and tap.
    'bilinear'  centre u = (x + 0.5) n_in / n_out - 0.5, taps floor(u), floor(u) + 1 with weights 1 - t, t
    'bicubic'   the same centre, 4 taps floor(u) - 1 .. floor(u) + 2, Keys' cubic with a = -0.75
    'area'      for n_in >= n_out: exact box coverage of [x r, (x + 1) r), r = n_in / n_out, fractional weights at both ends, over r;
                ceil(r) + 1 taps (unused ones weigh 0).  For n_in < n_out the sampler substitutes 'bilinear'.
                These three: half-pixel centres, indices clamped to the image (replicated border), no antialiasing.
    'matlab'    the antialiased bicubic of imresize_np: femasr_model.imresize_tables(n_in, n_out, n_out / n_in, True), the weights
                femasr_amd.resize / resample use, cast to float32.
  'bilinear', 'bicubic' and 'area' RESTATE the published semantics of cv2.resize's INTER_LINEAR / INTER_CUBIC / INTER_AREA.  They are NOT
  verified against cv2, which is not installed where this project is developed; they are verified against torch.nn.functional.interpolate
  (bilinear, bicubic; align_corners=False) and against block means (area).  cv2's INTER_LINEAR of float images works with these
  coefficients; its INTER_AREA for upscaling is a bilinear variant of its own, for which plain 'bilinear' stands here.

gaussian_noise(img, mode, factor, seed).  x + A n, rounded to float32, clipped to [0,1]; n standard normal.
  Normals.  base = splitmix64(seed) (synth._splitmix64 on uint64, wrapping).  Normal number j of the operation:
      u1 = ((splitmix64(base + 2 j) >> 11) + 1) 2^-53 in (0, 1],   u2 = (splitmix64(base + 2 j + 1) >> 11) 2^-53 in [0, 1),
      n_j = sqrt(-2 ln u1) cos(2 pi u2)        (Box-Muller in float64; 2 pi is the double 6.283185307179586)
  Pixel p (its index y W + x, plus `offset`) owns the normals 3 p, 3 p + 1, 3 p + 2.  No state: a value depends on (seed, p) alone.
      'color'        x_c + sigma n_{3p+c}                                   factor = sigma I
      'gray'         x_c + sigma n_{3p}      (one draw a pixel)             factor = sigma I
      'correlated'   ((x_c + A[c][0] n_{3p}) + A[c][1] n_{3p+1}) + A[c][2] n_{3p+2},  A A^T = the covariance (factor_of_covariance: eigh in
                     float64 on the host, negative eigenvalues of the reference's |L^2 U^T D U| taken as 0)
  in float64, every product and sum rounded on its own.

quantize(img): uint8(rint(float32(clip(x, 0, 1)) * float32(255))) - single2uint; the product is a float32 product, ties go to even.
jpeg(img, quality): quantize -> jpegio.coefficients_ref(u8, quality, '420') -> jpegio.decode_ref -> u8 / 255 in float32 (the last operation of
  a recipe returns the bytes).  Huffman coding is lossless, so the round trip through a file is exactly this.  Encoder and decoder are this
  project's (jpegio's docstring), not libjpeg's: the noise is JPEG noise of the same quality scale, not cv2's bit for bit.

Recipes.  sample_recipe follows degradation_bsrgan branch for branch: the optional 1/2 pre-shrink (p = 0.25, sf 4 only; one of the three
  cv2-style filters or 'matlab', p = 1/2 each), the shuffled seven steps with downsample3 kept behind downsample2, two blurs (anisotropic or
  isotropic, k = 2 randint(2, 11) + 3), downsample2 (p = 0.75: resize by 1 / U(1, 2 sf); else shifted-Gaussian blur with stride sf),
  downsample3 to exactly (h // sf, w // sf), Gaussian noise (level 2..25; u > 0.6 colour, u < 0.4 gray, else correlated), JPEG with p = 0.9 and
  Q in 30..95, and a final JPEG.  What differs from the reference, on purpose:
    * the draws come from ONE random.Random seeded by sha256(seed, name): a file's recipe does not depend on the other files, their order or
      a process pool.  The reference's global `random` / `np.random` streams are NOT reproduced;
    * the reference mod-crops with the remainders swapped (bsrgan_util.py:599 crops H by w % sf and W by h % sf); here H loses h % sf rows
      and W loses w % sf columns;
    * sigma, l1 and l2 are floored at 1e-3 (the reference divides by zero at an exact 0 draw);  sizes are floored at 1 pixel;
    * the camera ISP step (isp_model is None in the reference's callers), random_crop and degradation_bsrgan_plus are not included.
  sample_recipe(..., mode='bicubic') is the classical benchmark's one operation: the 'matlab' resample by 1 / sf ON THE BYTES
  (resample.resample_ref), after the same mod-crop.
"""
import hashlib
import json
import math
import random

import numpy as np

from . import jpegio
from .synth import _splitmix64

FILTERS = ('bilinear', 'bicubic', 'area', 'matlab')
NOISE_MODES = ('color', 'gray', 'correlated')
STRIDES = (1, 2, 4)
MIN_SPREAD = 1e-3          # floor of sigma, l1, l2
TWO_PI = 6.283185307179586


# ---------------------------------------------------------------------------------------------------------------- blur
def mirror_index(i, n):
    """m of the module docstring for an integer array i and a length n >= 1."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    t = np.mod(i, p)
    return np.where(t < n, t, p - t)


def check_kernel(kernel):
    kernel = np.asarray(kernel)
    if kernel.ndim != 2 or kernel.shape[0] != kernel.shape[1] or kernel.shape[0] % 2 == 0 or not 3 <= kernel.shape[0] <= 25:
        raise ValueError(f'blur: the kernel must be (k,k) with k odd in 3..25, got shape {kernel.shape}')
    return np.ascontiguousarray(kernel, np.float32)


def _check_image(img, what):
    img = np.asarray(img)
    if img.dtype != np.float32 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f'{what}: expected a non-empty float32 (H,W,3) image, got {img.dtype} {img.shape}')
    return img


def blur_values(img, kernel, stride=1):
    """The definition in float64 (any float image, (H,W,3)); the float32(kernel) weights."""
    kernel = check_kernel(kernel).astype(np.float64)
    if stride not in STRIDES:
        raise ValueError(f'blur: stride {stride!r} is not 1, 2 or 4')
    x = np.asarray(img, np.float64)
    k = kernel.shape[0]
    r = k // 2
    ys, xs = np.arange(0, x.shape[0], stride), np.arange(0, x.shape[1], stride)
    acc = np.zeros((len(ys), len(xs), x.shape[2]))
    for i in range(k):
        rows = x[mirror_index(ys + r - i, x.shape[0])]
        for j in range(k):
            acc = acc + kernel[i, j] * rows[:, mirror_index(xs + r - j, x.shape[1])]
    return acc


def blur_ref(img, kernel, stride=1):
    return blur_values(_check_image(img, 'blur_ref'), kernel, stride).astype(np.float32)


def fspecial_gaussian(k, sigma):
    siz = (k - 1.0) / 2.0
    x, y = np.meshgrid(np.arange(-siz, siz + 1), np.arange(-siz, siz + 1))
    h = np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    h[h < np.finfo(float).eps * h.max()] = 0
    return h / h.sum()


def anisotropic_covariance(theta, l1, l2):
    c, s = math.cos(theta), math.sin(theta)
    v = np.array([[c, s], [s, -c]])
    return v @ np.diag([l1, l2]) @ np.linalg.inv(v)


def anisotropic_gaussian(k, theta, l1, l2):
    cov = anisotropic_covariance(theta, l1, l2)
    g = np.arange(k, dtype=np.float64) - (k // 2)              # gm_blur_kernel: c = index - (k / 2 + 0.5) + 1
    cx, cy = np.meshgrid(g, g)                                  # k[y][x] = pdf([cx, cy])
    inv = np.linalg.inv(cov)
    e = inv[0, 0] * cx * cx + (inv[0, 1] + inv[1, 0]) * cx * cy + inv[1, 1] * cy * cy
    pdf = np.exp(-0.5 * e) / (2.0 * math.pi * math.sqrt(np.linalg.det(cov)))
    return pdf / pdf.sum()


def shifted_gaussian(sf, sigma, k=25):
    g = fspecial_gaussian(k, sigma)
    c = np.clip(np.arange(k, dtype=np.float64) + (sf - 1) * 0.5, 0, k - 1)
    i0 = np.minimum(np.floor(c).astype(np.int64), k - 2)
    t = c - i0
    rows = g[i0] * (1.0 - t)[:, None] + g[i0 + 1] * t[:, None]
    out = rows[:, i0] * (1.0 - t)[None, :] + rows[:, i0 + 1] * t[None, :]
    return out / out.sum()


def kernel_of(op):
    """The float32 (k,k) kernel of a blur operation of a recipe."""
    kind = op['kind']
    if kind == 'iso':
        k = fspecial_gaussian(op['k'], op['sigma'])
    elif kind == 'aniso':
        k = anisotropic_gaussian(op['k'], op['theta'], op['l1'], op['l2'])
    elif kind == 'shifted':
        k = shifted_gaussian(op['sf'], op['sigma'], op['k'])
    else:
        raise ValueError(f'blur: unknown kernel kind {kind!r}')
    return check_kernel(k)


# ---------------------------------------------------------------------------------------------------------------- resize
def _cubic_weights(t, a=-0.75):
    d = np.stack([1.0 + t, t, 1.0 - t, 2.0 - t], axis=1)
    near = ((a + 2.0) * d - (a + 3.0)) * d * d + 1.0
    far = ((a * d - 5.0 * a) * d + 8.0 * a) * d - 4.0 * a
    return np.where(d <= 1.0, near, far)


def tap_table(filt, n_in, n_out):
    """(weights float32 (n_out, taps), indices int32 (n_out, taps)) of one axis; every index lies in 0 .. n_in - 1."""
    if filt not in FILTERS:
        raise ValueError(f'resize: filter {filt!r} is not one of {FILTERS}')
    if n_in < 1 or n_out < 1:
        raise ValueError(f'resize: length {n_in} -> {n_out}')
    if filt == 'matlab':
        from .models.femasr_model import imresize_tables
        w, idx = imresize_tables(n_in, n_out, n_out / n_in, True)
        return np.ascontiguousarray(w, np.float32), np.ascontiguousarray(idx, np.int32)
    x = np.arange(n_out, dtype=np.float64)
    if filt == 'area' and n_in >= n_out:
        r = n_in / n_out
        lo, hi = x * r, np.minimum((x + 1.0) * r, float(n_in))
        first = np.floor(lo)
        j = first[:, None] + np.arange(math.ceil(r) + 1, dtype=np.float64)[None, :]
        w = np.clip(np.minimum(hi[:, None], j + 1.0) - np.maximum(lo[:, None], j), 0.0, None) / (hi - lo)[:, None]
        idx = j
    else:
        u = (x + 0.5) * (n_in / n_out) - 0.5
        f = np.floor(u)
        t = u - f
        if filt == 'bicubic':
            w, idx = _cubic_weights(t), f[:, None] + np.arange(-1, 3)[None, :]
        else:
            w, idx = np.stack([1.0 - t, t], axis=1), f[:, None] + np.arange(2)[None, :]
    return np.ascontiguousarray(w, np.float32), np.ascontiguousarray(np.clip(idx, 0, n_in - 1), np.int32)


def check_table(w, idx, n_in, n_out):
    w, idx = np.asarray(w), np.asarray(idx)
    if w.dtype != np.float32 or idx.dtype != np.int32 or w.ndim != 2 or w.shape != idx.shape or w.shape[0] != n_out or w.shape[1] < 1:
        raise ValueError(f'resize: a table must be float32 weights and int32 indices of ({n_out}, taps), got {w.dtype} {w.shape} / {idx.dtype} {idx.shape}')
    if idx.min() < 0 or idx.max() >= n_in:
        raise ValueError(f'resize: the table indexes {int(idx.min())}..{int(idx.max())}, outside the source 0..{n_in - 1}')


def resize_values(img, tables_h, tables_w):
    """The definition in front of the clip, float64: tables_* = (weights, indices) of the H and the W axis."""
    x = np.asarray(img, np.float64)
    (wh, ih), (ww, iw) = tables_h, tables_w
    check_table(wh, ih, x.shape[0], wh.shape[0])
    check_table(ww, iw, x.shape[1], ww.shape[0])
    out1 = np.zeros((wh.shape[0],) + x.shape[1:])
    for k in range(wh.shape[1]):
        out1 = out1 + wh[:, k].astype(np.float64)[:, None, None] * x[ih[:, k]]
    out2 = np.zeros((wh.shape[0], ww.shape[0], x.shape[2]))
    for k in range(ww.shape[1]):
        out2 = out2 + ww[:, k].astype(np.float64)[None, :, None] * out1[:, iw[:, k]]
    return out2


def resize_ref(img, out_h, out_w, filt):
    img = _check_image(img, 'resize_ref')
    v = resize_values(img, tap_table(filt, img.shape[0], out_h), tap_table(filt, img.shape[1], out_w))
    return np.clip(v.astype(np.float32), 0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------- noise
def noise_base(seed):
    return _splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], np.uint64))[0]


def normal_ref(seed, j):
    """Standard normals number j (an integer array) of the operation `seed`: float64 (module docstring)."""
    j = np.asarray(j).astype(np.uint64)
    base = noise_base(seed)
    with np.errstate(over='ignore'):
        c = base + np.uint64(2) * j
        h1, h2 = _splitmix64(c), _splitmix64(c + np.uint64(1))
    u1 = ((h1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (h2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def factor_of_covariance(cov):
    """A 3x3 factor A with A A^T = cov (eigh in float64; negative eigenvalues count as 0)."""
    lam, v = np.linalg.eigh(np.asarray(cov, np.float64))
    return v * np.sqrt(np.clip(lam, 0.0, None))[None, :]


def check_noise(mode, factor):
    if mode not in NOISE_MODES:
        raise ValueError(f'gaussian_noise: mode {mode!r} is not one of {NOISE_MODES}')
    a = np.asarray(factor, np.float64).reshape(-1)
    if a.size != 9 or not np.all(np.abs(a) <= 16.0):
        raise ValueError('gaussian_noise: the factor must be 9 finite numbers within -16..16')
    return a.reshape(3, 3)


def noise_values(img, mode, factor, seed, offset=0):
    """x + A n in float64, in front of the rounding and the clip.  img: (.., 3); its pixels are numbered from `offset` in C order."""
    a = check_noise(mode, factor)
    x = np.asarray(img, np.float64)
    flat = x.reshape(-1, 3)
    p = np.arange(flat.shape[0], dtype=np.uint64) + np.uint64(offset)
    n = [normal_ref(seed, np.uint64(3) * p + np.uint64(c)) for c in range(1 if mode == 'gray' else 3)]
    if mode == 'correlated':
        out = np.stack([((flat[:, c] + a[c, 0] * n[0]) + a[c, 1] * n[1]) + a[c, 2] * n[2] for c in range(3)], axis=1)
    else:
        out = np.stack([flat[:, c] + a[0, 0] * n[0 if mode == 'gray' else c] for c in range(3)], axis=1)
    return out.reshape(x.shape)


def noise_ref(img, mode, factor, seed, offset=0):
    return np.clip(noise_values(_check_image(img, 'noise_ref'), mode, factor, seed, offset).astype(np.float32), 0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------- bytes
def quantize_ref(img):
    """single2uint: float32 in, uint8 out."""
    x = np.clip(np.asarray(img, np.float32), np.float32(0), np.float32(1))
    return np.rint(x * np.float32(255)).astype(np.uint8)


def unit_ref(u8):
    """uint2single: float32(u8) / float32(255)."""
    return np.asarray(u8, np.uint8).astype(np.float32) / np.float32(255)


def jpeg_u8_ref(u8, quality, subsampling='420'):
    h, w = u8.shape[:2]
    return jpegio.decode_ref(jpegio.coefficients_ref(u8, quality, subsampling), quality, subsampling, h, w)


def jpeg_ref(img, quality, final=False):
    u8 = jpeg_u8_ref(quantize_ref(_check_image(img, 'jpeg_ref')), quality)
    return u8 if final else unit_ref(u8)


# ---------------------------------------------------------------------------------------------------------------- recipes
class Recipe(dict):
    """{'version', 'mode', 'sf', 'seed', 'name', 'size': [h, w], 'crop': [h', w'], 'out': [h // sf, w // sf], 'ops': [...]}: plain JSON types.
    ops: {'op': 'unit'} (bytes -> float32), {'op': 'blur', 'kind', 'k', ..., 'stride'}, {'op': 'resize', 'filter', 'out_h', 'out_w'},
    {'op': 'noise', 'mode', 'factor': [9], 'seed'}, {'op': 'jpeg', 'quality', 'final'}, {'op': 'resample_u8', 'out_h', 'out_w'} (bytes)."""

    def to_json(self):
        return json.dumps(self, sort_keys=True)

    @classmethod
    def from_json(cls, text):
        return cls(json.loads(text) if isinstance(text, (str, bytes)) else text)


def recipe_rng(seed, name):
    digest = hashlib.sha256(f'{int(seed)}\0{name}'.encode('utf-8')).digest()
    return random.Random(int.from_bytes(digest[:16], 'big'))


def _orth3(m):
    u, s, _ = np.linalg.svd(m)
    return u[:, s > s.max() * 3 * np.finfo(float).eps]          # scipy.linalg.orth


def _blur_op(rng, sf):
    wd2, wd = 4.0 + sf, 2.0 + 0.2 * sf
    if rng.random() < 0.5:
        l1, l2 = wd2 * rng.random(), wd2 * rng.random()
        return {'op': 'blur', 'kind': 'aniso', 'k': 2 * rng.randint(2, 11) + 3, 'theta': rng.random() * math.pi, 'l1': max(l1, MIN_SPREAD),
                'l2': max(l2, MIN_SPREAD), 'stride': 1}
    return {'op': 'blur', 'kind': 'iso', 'k': 2 * rng.randint(2, 11) + 3, 'sigma': max(wd * rng.random(), MIN_SPREAD), 'stride': 1}


def _noise_op(rng):
    level = rng.randint(2, 25)
    u = rng.random()
    sigma = level / 255.0
    if u > 0.6 or u < 0.4:
        return {'op': 'noise', 'mode': 'color' if u > 0.6 else 'gray', 'factor': (np.eye(3) * sigma).reshape(-1).tolist(), 'seed': rng.getrandbits(63)}
    d = np.diag([rng.random() for _ in range(3)])
    m = _orth3(np.array([rng.random() for _ in range(9)]).reshape(3, 3))
    cov = np.abs((25 / 255.0) ** 2 * (m.T @ d[:m.shape[1], :m.shape[1]] @ m)) if m.shape[1] == 3 else np.eye(3) * sigma ** 2
    return {'op': 'noise', 'mode': 'correlated', 'factor': factor_of_covariance(cov).reshape(-1).tolist(), 'seed': rng.getrandbits(63)}


def sample_recipe(seed, name, h, w, sf, mode='bsrgan'):
    """The Recipe of the file `name` (h x w pixels) at scale sf in (2, 4): a function of its arguments alone (module docstring)."""
    if sf not in (2, 4):
        raise ValueError(f'sample_recipe: sf {sf!r} is not 2 or 4')
    if mode not in ('bsrgan', 'bicubic'):
        raise ValueError(f"sample_recipe: mode {mode!r} is not 'bsrgan' or 'bicubic'")
    h, w = int(h), int(w)
    ch, cw = h - h % sf, w - w % sf
    if ch < sf or cw < sf:
        raise ValueError(f'sample_recipe: a {w} x {h} image is smaller than the scale {sf}')
    rec = Recipe(version=1, mode=mode, sf=sf, seed=int(seed), name=str(name), size=[h, w], crop=[ch, cw], out=[ch // sf, cw // sf], ops=[])
    ops = rec['ops']
    if mode == 'bicubic':
        ops.append({'op': 'resample_u8', 'out_h': ch // sf, 'out_w': cw // sf})
        return rec
    rng = recipe_rng(seed, name)
    pick = lambda: rng.choice(FILTERS[:3])      # noqa: E731  (cv2's interpolation 1, 2, 3)

    def resize(oh, ow, filt):
        nonlocal ch, cw
        oh, ow = max(1, int(oh)), max(1, int(ow))
        ops.append({'op': 'resize', 'filter': filt, 'out_h': oh, 'out_w': ow})
        ch, cw = oh, ow

    ops.append({'op': 'unit'})
    if sf == 4 and rng.random() < 0.25:                         # downsample1
        filt = pick() if rng.random() < 0.5 else 'matlab'
        if filt == 'matlab':
            try:
                tap_table('matlab', ch, ch // 2), tap_table('matlab', cw, cw // 2)
            except ValueError:                                  # too small for the antialiased tables
                filt = 'bicubic'
        resize(1 / 2 * ch, 1 / 2 * cw, filt)
        sf = 2
    order = rng.sample(range(7), 7)
    i2, i3 = order.index(2), order.index(3)
    if i2 > i3:
        order[i2], order[i3] = order[i3], order[i2]
    a = b = None
    for step in order:
        if step in (0, 1):
            ops.append(_blur_op(rng, sf))
        elif step == 2:
            a, b = cw, ch
            if rng.random() < 0.75:
                sf1 = rng.uniform(1, 2 * sf)
                resize(1 / sf1 * ch, 1 / sf1 * cw, pick())
            else:
                ops.append({'op': 'blur', 'kind': 'shifted', 'k': 25, 'sf': sf, 'sigma': rng.uniform(0.1, 0.6 * sf), 'stride': sf})
                ch, cw = -(-ch // sf), -(-cw // sf)
        elif step == 3:
            resize(1 / sf * b, 1 / sf * a, pick())
        elif step == 4:
            ops.append(_noise_op(rng))
        elif step == 5:
            if rng.random() < 0.9:
                ops.append({'op': 'jpeg', 'quality': rng.randint(30, 95), 'final': False})
    ops.append({'op': 'jpeg', 'quality': rng.randint(30, 95), 'final': True})
    assert [ch, cw] == rec['out'], (ch, cw, rec['out'])
    return rec


def check_recipe(recipe, shape):
    recipe = recipe if isinstance(recipe, Recipe) else Recipe.from_json(recipe)
    if tuple(shape[:2]) != tuple(recipe['size']) or len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"degrade: the recipe of '{recipe.get('name')}' is for a {recipe['size']} RGB image, got shape {tuple(shape)}")
    return recipe


def op_ref(x, op):
    """One operation through its definition (host)."""
    kind = op['op']
    if kind == 'unit':
        return unit_ref(x)
    if kind == 'blur':
        return blur_ref(x, kernel_of(op), op['stride'])
    if kind == 'resize':
        th, tw = op_tables(op, x.shape[0], x.shape[1])
        return np.clip(resize_values(_check_image(x, 'resize'), th, tw).astype(np.float32), 0.0, 1.0)
    if kind == 'noise':
        return noise_ref(x, op['mode'], op['factor'], op['seed'])
    if kind == 'jpeg':
        return jpeg_ref(x, op['quality'], op.get('final', False))
    if kind == 'resample_u8':
        from .resample import resample_ref
        return resample_ref(x, op['out_h'], op['out_w'])
    raise ValueError(f'degrade: unknown operation {kind!r}')


def op_tables(op, h, w):
    """The tap tables of a resize operation on an h x w image, per axis: 'area' on an axis that grows is 'bilinear'."""
    f = op['filter']
    return tuple(tap_table('bilinear' if f == 'area' and o > n else f, n, o) for n, o in ((h, op['out_h']), (w, op['out_w'])))


def degrade_ref(img_u8, recipe):
    """uint8 (h,w,3) -> uint8 (h // sf, w // sf, 3): the whole chain of `recipe` through the definitions."""
    img_u8 = np.asarray(img_u8)
    if img_u8.dtype != np.uint8:
        raise ValueError(f'degrade_ref: expected a uint8 image, got {img_u8.dtype}')
    recipe = check_recipe(recipe, img_u8.shape)
    x = np.ascontiguousarray(img_u8[:recipe['crop'][0], :recipe['crop'][1]])
    for op in recipe['ops']:
        x = op_ref(x, op)
    assert x.dtype == np.uint8 and list(x.shape[:2]) == list(recipe['out'])
    return x


# ---------------------------------------------------------------------------------------------------------------- GPU
CACHE_ENTRIES = 256
_CACHE = {}                 # insertion-ordered: the oldest entry leaves first
_KEEP = []                  # stack of lists: degrade_u8(keep=...) collects the table tensors its launches read


def _cached(key, device, make):
    """Device copies of host-built tables (blur kernels, tap tables), cached per operation.  Lifetime: the cache holds the CACHE_ENTRIES
    most recently MADE entries and drops the oldest one for each new one; a dropped tensor lives on while anyone else refers to it.  A
    captured graph replays with the raw addresses of its tables, so whoever captures keeps them alive (degrade_u8's `keep`)."""
    import torch
    key = (key, str(device))
    if key not in _CACHE:
        while len(_CACHE) >= CACHE_ENTRIES:
            del _CACHE[next(iter(_CACHE))]
        _CACHE[key] = tuple(torch.from_numpy(a).to(device) for a in make())
    if _KEEP:
        _KEEP[-1].extend(_CACHE[key])
    return _CACHE[key]


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _check_tensor(t, dtype, what):
    import torch
    from . import _lib
    if not torch.is_tensor(t):
        raise TypeError(f'{what}: expected a torch tensor, got {type(t).__name__}')
    if t.device.type != 'cuda':
        raise _lib.FemasrError(f'{what}: tensor on {t.device}: it runs on a GPU only (no CPU fallback)')
    if t.dtype != dtype or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f'{what}: expected a non-empty {dtype} (H,W,3) tensor, got {t.dtype} {tuple(t.shape)}')


def unit_gpu(u8, crop=None):
    """unit_ref of a uint8 (H,W,3) GPU tensor that is contiguous or a top-left crop of a contiguous one (a row pitch, no copy)."""
    import torch
    from . import _lib
    _check_tensor(u8, torch.uint8, 'unit_gpu')
    if crop is not None:
        u8 = u8[:crop[0], :crop[1]]
    h, w = u8.shape[:2]
    if u8.stride(2) != 1 or u8.stride(1) != 3 or u8.stride(0) % 3 or u8.stride(0) < 3 * w:
        u8 = u8.contiguous()
    out = torch.empty((h, w, 3), dtype=torch.float32, device=u8.device)
    with torch.cuda.device(u8.device):
        _lib.check(_lib.load().femasr_degrade_unit_f32(_stream(u8), _lib.ptr(u8), h, w, u8.stride(0) // 3, _lib.ptr(out)))
    return out


def blur_gpu(t, kernel, stride=1, key=None):
    import torch
    from . import _lib
    _check_tensor(t, torch.float32, 'blur_gpu')
    kernel = check_kernel(kernel)
    if stride not in STRIDES:
        raise ValueError(f'blur: stride {stride!r} is not 1, 2 or 4')
    t = t.contiguous()
    h, w = t.shape[:2]
    k_dev, = _cached(('blur', key if key is not None else kernel.tobytes()), t.device, lambda: [kernel])
    out = torch.empty((-(-h // stride), -(-w // stride), 3), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().femasr_degrade_blur_f32(_stream(t), _lib.ptr(t), h, w, _lib.ptr(k_dev), kernel.shape[0], stride, _lib.ptr(out)))
    return out


def resize_gpu(t, tables_h, tables_w, key=None):
    """tables_*: (weights, indices) host arrays of an axis (tap_table); checked here before they are uploaded, and the C entry checks the
    host index arrays again on every call."""
    import ctypes
    import torch
    from . import _lib
    _check_tensor(t, torch.float32, 'resize_gpu')
    t = t.contiguous()
    h, w = t.shape[:2]
    (wh, ih), (ww, iw) = tables_h, tables_w
    check_table(wh, ih, h, wh.shape[0])
    check_table(ww, iw, w, ww.shape[0])
    ih, iw = np.ascontiguousarray(ih), np.ascontiguousarray(iw)
    if key is None:
        key = tuple(a.tobytes() for a in (wh, ih, ww, iw))
    dwh, dih, dww, diw = _cached(('resize', key), t.device, lambda: [np.ascontiguousarray(a) for a in (wh, ih, ww, iw)])
    out = torch.empty((wh.shape[0], ww.shape[0], 3), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().femasr_degrade_resize_f32(_stream(t), _lib.ptr(t), h, w, _lib.ptr(out), wh.shape[0], ww.shape[0], _lib.ptr(dwh),
                                                         _lib.ptr(dih), wh.shape[1], _lib.ptr(dww), _lib.ptr(diw), ww.shape[1],
                                                         ctypes.c_void_p(ih.ctypes.data), ctypes.c_void_p(iw.ctypes.data)))
    return out


def noise_gpu(t, mode, factor, seed, offset=0, out=None):
    """noise_ref on the GPU; out=t runs in place.  t: float32 (..., 3), contiguous; its pixels are numbered from `offset`."""
    import ctypes
    import torch
    from . import _lib
    a = check_noise(mode, factor)
    if not torch.is_tensor(t) or t.device.type != 'cuda' or t.dtype != torch.float32 or t.shape[-1] != 3 or t.numel() < 3 or not t.is_contiguous():
        raise ValueError('noise_gpu: expected a non-empty contiguous float32 (..., 3) GPU tensor')
    out = torch.empty_like(t) if out is None else out
    if out.shape != t.shape or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
        raise ValueError('noise_gpu: out must be a contiguous tensor like the input')
    fac = (ctypes.c_double * 9)(*a.reshape(-1).tolist())
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().femasr_degrade_noise_f32(_stream(t), _lib.ptr(t), _lib.ptr(out), t.numel() // 3, int(offset), NOISE_MODES.index(mode),
                                                        fac, int(seed) & 0xFFFFFFFFFFFFFFFF))
    return out


def quantize_gpu(t):
    import torch
    from . import _lib
    if not torch.is_tensor(t) or t.device.type != 'cuda' or t.dtype != torch.float32 or t.numel() < 1:
        raise ValueError('quantize_gpu: expected a non-empty float32 GPU tensor')
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().femasr_degrade_quantize_u8(_stream(t), _lib.ptr(t), _lib.ptr(out), t.numel()))
    return out


def jpeg_gpu(t, quality, final=False, subsampling='420'):
    """jpeg_ref on the GPU: quantise, femasr_jpeg_coefficients_u8, femasr_jpeg_decode_u8 - three launches, no entropy coder."""
    import torch
    _check_tensor(t, torch.float32, 'jpeg_gpu')
    u8 = quantize_gpu(t)
    planes = jpegio.coefficients_gpu(u8, quality, subsampling)
    return jpegio.decode_gpu(planes, quality, subsampling, u8.shape[0], u8.shape[1], float32=not final)


def apply_op(t, op):
    """One operation of a recipe on the GPU: a cuda tensor in, a cuda tensor out, on the current stream."""
    kind = op['op']
    if kind == 'unit':
        return unit_gpu(t)
    if kind == 'blur':
        return blur_gpu(t, kernel_of(op), op['stride'], key=json.dumps(op, sort_keys=True))
    if kind == 'resize':
        th, tw = op_tables(op, t.shape[0], t.shape[1])
        return resize_gpu(t, th, tw, key=(json.dumps(op, sort_keys=True), t.shape[0], t.shape[1]))
    if kind == 'noise':
        return noise_gpu(t.contiguous(), op['mode'], op['factor'], op['seed'])
    if kind == 'jpeg':
        return jpeg_gpu(t, op['quality'], op.get('final', False))
    if kind == 'resample_u8':
        from .resample import resample_u8
        return resample_u8(t.contiguous(), op['out_h'], op['out_w'])
    raise ValueError(f'degrade: unknown operation {kind!r}')


def degrade_u8(img_u8, recipe, out=None, keep=None):
    """`degrade_ref` on the GPU: uint8 (h,w,3) cuda tensor -> uint8 (h // sf, w // sf, 3) cuda tensor.  The chain of apply_op calls over the
    mod-cropped image and nothing else; host work is building the kernels and tap tables of the recipe (cached per operation, _cached).
    Under a graph capture: run the recipe once before capturing - a cache miss inside the capture would upload a table with a synchronous
    H2D copy from pageable memory, which a capture does not take -, and pass a list as `keep`: it receives the device tables the launches
    read, which the owner of the graph holds for as long as the graph lives (the cache alone keeps only its newest CACHE_ENTRIES)."""
    import torch
    _check_tensor(img_u8, torch.uint8, 'degrade_u8')
    recipe = check_recipe(recipe, tuple(img_u8.shape))
    x = img_u8[:recipe['crop'][0], :recipe['crop'][1]]
    if keep is not None:
        _KEEP.append(keep)
    try:
        for op in recipe['ops']:
            x = apply_op(x, op)
    finally:
        if keep is not None:
            _KEEP.pop()
    if x.dtype != torch.uint8 or list(x.shape[:2]) != list(recipe['out']):
        raise ValueError(f"degrade_u8: the recipe ends in {x.dtype} {tuple(x.shape)}, not uint8 {recipe['out']}")
    if out is not None:
        if out.shape != x.shape or out.dtype != torch.uint8 or out.device != x.device:
            raise ValueError(f'degrade_u8: out must be a uint8 tensor of shape {tuple(x.shape)} on {x.device}')
        out.copy_(x)
        return out
    return x

"""Structured test content - flat, step, impulse and small-integer tensors - and INDEPENDENT references for it.

Every other parity test draws i.i.d. noise (synth.uniform / synth.synth_input): no repeated values, no exact zeros, no flat regions,
no isolated samples.  This module supplies what photographs are made of - black bars, clipped skies, hard edges, single hot pixels -
and references written directly from the definitions in int64 / float64 numpy.  The references import neither `oracle` nor the
library: on small-integer and impulse inputs every summation order is exact, so a kernel (and the oracle) must reproduce them
exactly, and a wrong tap, a transposed weight block, an off-by-one roll or a wrong tie rule shows as an integer mismatch at a
known coordinate.

Plain module, no fixtures: tests/test_structured_inputs_host.py (CPU) and tests/test_gpu_structured_inputs.py (GPU) import it."""
import numpy as np

from femasr_amd import synth

# ------------------------------------------------------------------ images: uint8 HWC, float view exactly u8 / 255
CONTENTS = ('black', 'white', 'gray173', 'pure_red', 'letterbox', 'step_v', 'step_h', 'impulse_centre', 'impulse_corner', 'checker1')


def _edge(n):
    """A step position near the middle that is not a multiple of 8 (never on a window or tile boundary)."""
    e = n // 2
    return e + 1 if e % 8 == 0 else e


def image(name, h, w, seed=0):
    """uint8 (h, w, 3) RGB image of the named content."""
    img = np.zeros((h, w, 3), np.uint8)
    if name == 'black':
        pass
    elif name == 'white':
        img[:] = 255
    elif name == 'gray173':
        img[:] = 173
    elif name == 'pure_red':
        img[:, :, 0] = 255
    elif name == 'letterbox':           # black bars, image noise between them
        bar = max(1, h // 4)
        body = synth.synth_input(seed, (1, 3, h, w), tag='letterbox')[0].transpose(1, 2, 0)
        img[bar:h - bar] = np.round(body[bar:h - bar].astype(np.float64) * 255.0).astype(np.uint8)
    elif name == 'step_v':              # 0 | 255, vertical edge
        img[:, _edge(w):] = 255
    elif name == 'step_h':              # 0 over 255, horizontal edge
        img[_edge(h):] = 255
    elif name == 'impulse_centre':
        img[h // 2, w // 2] = 255
    elif name == 'impulse_corner':
        img[0, 0] = 255
    elif name == 'checker1':            # 1-pixel checkerboard
        yy, xx = np.mgrid[0:h, 0:w]
        img[(yy + xx) % 2 == 1] = 255
    else:
        raise KeyError(name)
    return img


def to_float(img_u8):
    """uint8 HWC -> fp32 (1, 3, H, W), exactly u8 / 255 in fp32 (what img2tensor(...) / 255. gives)."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3
    return np.ascontiguousarray((img.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))[None])


# ------------------------------------------------------------------ NHWC feature maps of a chosen channel count
def feature(kind, shape, values=None, pos=None, amp=1.0):
    """fp32 (B, H, W, C) feature map.  'zero'; 'const' (values: a scalar or C per-channel constants); 'impulse' (amp at pixel pos =
    (y, x) of every channel and image, 0 elsewhere; on top of `values` if given); 'step' (0 left of the edge column, values right)."""
    b, h, w, c = shape
    x = np.zeros(shape, np.float32)
    vals = np.float32(1.0) if values is None else np.asarray(values, np.float32)
    if kind == 'zero':
        pass
    elif kind == 'const':
        x[:] = vals
    elif kind == 'impulse':
        if values is not None:
            x[:] = vals
        y0, x0 = (h // 2, w // 2) if pos is None else pos
        x[:, y0, x0, :] = np.float32(amp)
    elif kind == 'step':
        x[:, :, _edge(w):, :] = vals
    else:
        raise KeyError(kind)
    return x


def sparse_ints(rng, shape, lo, hi, keep=0.35):
    """int64 integers in [lo, hi], most of them zero."""
    return rng.integers(lo, hi + 1, shape) * (rng.random(shape) < keep)


# ------------------------------------------------------------------ independent references
def _acc_dtype(*arrays):
    return np.int64 if all(np.issubdtype(np.asarray(a).dtype, np.integer) for a in arrays if a is not None) else np.float64


def conv2d_ref(x, w_khwc, bias=None, stride=1, pad=0, up2=False, res1=None, res2=None):
    """out[n, y, x, o] = bias[o] + sum_{ky, kx, c} in[n, s y + ky - p, s x + kx - p, c] w[ky, kx, c, o] (+ res1 + res2), zeros outside
    the image; up2: `in` is the nearest-neighbour x2 enlargement of x.  int64 when every operand is an integer array, else float64."""
    dt = _acc_dtype(x, w_khwc, bias, res1, res2)
    x, w = np.asarray(x, dt), np.asarray(w_khwc, dt)
    if up2:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    b, h, wd, cin = x.shape
    kh, kw, cin_w, cout = w.shape
    assert cin == cin_w
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = np.zeros((b, ho, wo, cout), dt)
    for ky in range(kh):
        for kx in range(kw):
            out += xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :] @ w[ky, kx]
    for t in (bias, res1, res2):
        if t is not None:
            out += np.asarray(t, dt)
    return out


def conv2d_abs_bound(x, w_khwc, bias=None, stride=1, pad=0, up2=False, res1=None, res2=None):
    """max over outputs of sum |in| |w| + |bias| + |res|: no partial sum of any summation order exceeds it."""
    a = [None if t is None else np.abs(np.asarray(t)) for t in (x, w_khwc, bias, res1, res2)]
    return conv2d_ref(a[0], a[1], a[2], stride, pad, up2, a[3], a[4]).max()


def linear_ref(x_rows, w_io, bias=None, res1=None, res2=None):
    """out[m, n] = bias[n] + sum_k x[m, k] w[k, n] (+ residuals)."""
    dt = _acc_dtype(x_rows, w_io, bias, res1, res2)
    out = np.asarray(x_rows, dt) @ np.asarray(w_io, dt)
    for t in (bias, res1, res2):
        if t is not None:
            out = out + np.asarray(t, dt)
    return out


WINDOW = 8


def region_labels(h, w, shift):
    """SwinIR's attention-mask regions of the ROLLED grid: three slices per axis, [0, -8), [-8, -shift), [-shift, end)."""
    lab = np.zeros((h, w), np.int64)
    if shift == 0:
        return lab
    n = 0
    for ys in (slice(0, -WINDOW), slice(-WINDOW, -shift), slice(-shift, None)):
        for xs in (slice(0, -WINDOW), slice(-WINDOW, -shift), slice(-shift, None)):
            lab[ys, xs] = n
            n += 1
    return lab


def window_mean_ref(v, b, h, w, shift):
    """What shifted-window attention returns when every allowed key has the same weight: per query the mean of V over the keys of
    its 8x8 window (after a cyclic roll by -shift on both axes) that carry the query's region label; rolled back.
    v (b, h*w, c) integers -> (sums int64 (b, h*w, c), counts int64 (b, h*w)): the mean is sums / counts."""
    v = np.asarray(v)
    assert np.issubdtype(v.dtype, np.integer)
    c = v.shape[-1]
    g = np.roll(v.reshape(b, h, w, c).astype(np.int64), (-shift, -shift), axis=(1, 2))
    lab = region_labels(h, w, shift)
    sums = np.zeros_like(g)
    cnt = np.zeros((b, h, w), np.int64)
    for wy in range(0, h, WINDOW):
        for wx in range(0, w, WINDOW):
            gv = g[:, wy:wy + WINDOW, wx:wx + WINDOW].reshape(b, WINDOW * WINDOW, c)
            lv = lab[wy:wy + WINDOW, wx:wx + WINDOW].reshape(-1)
            same = (lv[:, None] == lv[None, :]).astype(np.int64)              # [query][key]
            sums[:, wy:wy + WINDOW, wx:wx + WINDOW] = np.einsum('qk,bkc->bqc', same, gv).reshape(b, WINDOW, WINDOW, c)
            cnt[:, wy:wy + WINDOW, wx:wx + WINDOW] = same.sum(1).reshape(WINDOW, WINDOW)
    sums = np.roll(sums, (shift, shift), axis=(1, 2)).reshape(b, h * w, c)
    cnt = np.roll(cnt, (shift, shift), axis=(1, 2)).reshape(b, h * w)
    return sums, cnt


def vq_argmin_ref(z_rows, codebook):
    """index[m] = the FIRST code of least squared distance sum_d (z[m, d] - e[j, d])^2, in int64."""
    z, e = np.asarray(z_rows), np.asarray(codebook)
    assert np.issubdtype(z.dtype, np.integer) and np.issubdtype(e.dtype, np.integer)
    z, e = z.astype(np.int64), e.astype(np.int64)
    idx = np.empty(len(z), np.int64)
    for m in range(len(z)):
        d = ((z[m][None, :] - e) ** 2).sum(1)
        idx[m] = int(np.flatnonzero(d == d.min())[0])
    return idx


def group_moments(x, groups=32):
    """float64 (mean, biased variance) per image and group of an NHWC map: (B, G) each, two-pass."""
    b, h, w, c = x.shape
    g = np.asarray(x, np.float64).reshape(b, h * w, groups, c // groups).transpose(0, 2, 1, 3).reshape(b, groups, -1)
    mean = g.mean(-1)
    return mean, ((g - mean[..., None]) ** 2).mean(-1)


def row_moments(x_rows):
    """float64 (mean, biased variance) per row."""
    r = np.asarray(x_rows, np.float64)
    mean = r.mean(-1)
    return mean, ((r - mean[:, None]) ** 2).mean(-1)


def first_mismatch(got, want):
    """'' when equal, else a message naming the first mismatching coordinate."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f'shapes differ: {got.shape} vs {want.shape}'
    bad = np.argwhere(got.astype(np.float64) != want.astype(np.float64))
    if len(bad) == 0:
        return ''
    at = tuple(int(i) for i in bad[0])
    return f'{len(bad)} of {got.size} differ, first at {at}: got {got[at]!r}, want {want[at]!r}'


# ------------------------------------------------------------------ the integer families both test files use
# name, (B, H, W, Cin), Cout, k, stride, pad, up2, form ('direct' | 'wino' | 'split' | 'bf16x3')
INT_CONV_CASES = [
    ('in_conv_k4_cin3', (2, 31, 33, 3), 64, 4, 1, 1, False, 'direct'),
    ('halo_17x23', (2, 17, 23, 64), 128, 3, 1, 1, False, 'direct'),            # tiles overhang both edges
    ('im2col_pad0', (1, 12, 12, 64), 64, 3, 1, 0, False, 'direct'),
    ('stride2_odd', (1, 15, 13, 64), 64, 3, 2, 1, False, 'direct'),
    ('k1', (1, 9, 11, 64), 96, 1, 1, 0, False, 'direct'),
    ('up2_phase', (1, 7, 9, 128), 64, 3, 1, 1, True, 'direct'),
    ('up2_phase_cout3', (1, 5, 6, 32), 3, 3, 1, 1, True, 'direct'),
    ('wino_17x23', (2, 17, 23, 64), 128, 3, 1, 1, False, 'wino'),
    ('wino_up2', (1, 8, 8, 32), 64, 3, 1, 1, True, 'wino'),
    ('split3x3', (1, 9, 11, 64), 96, 3, 1, 1, False, 'split'),
    ('split3x3_s2', (1, 15, 13, 64), 64, 3, 2, 1, False, 'split'),
    ('split1x1', (1, 9, 11, 64), 96, 1, 1, 0, False, 'split'),
    ('bf16x3_17x23', (2, 17, 23, 64), 128, 3, 1, 1, False, 'bf16x3'),
    ('bf16x3_up2', (1, 7, 9, 128), 64, 3, 1, 1, True, 'bf16x3'),
]
WINO_UNIT = 576         # 24^2: clears the denominators (4, 6, 12, 24) of both factors G of the F(4x4, 3x3) weight transform


def out_hw(shape, k, stride, pad, up2):
    h, w = (2 * shape[1], 2 * shape[2]) if up2 else (shape[1], shape[2])
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def int_conv_operands(case):
    """(x, w [kh][kw][Cin][Cout], bias, res1, res2) as int64 arrays.  Inputs sparse in {-2..2}, weights in {-3..3}, bias and both
    residuals in {-8..8}; the Winograd forms take inputs in {0, 1} and weights in {-576, 0, 576} (WINO_UNIT)."""
    name, shape, cout, k, stride, pad, up2, form = case
    rng = np.random.default_rng(sum(name.encode()) * 7919 + cout)
    ho, wo = out_hw(shape, k, stride, pad, up2)
    if form == 'wino':
        x = (rng.random(shape) < 0.35).astype(np.int64)
        w = rng.integers(-1, 2, (k, k, shape[3], cout)) * WINO_UNIT
    else:
        x = sparse_ints(rng, shape, -2, 2)
        w = rng.integers(-3, 4, (k, k, shape[3], cout))
    w[0, 0, 0, :] = (np.arange(cout) % 3 - 1) * WINO_UNIT if form == 'wino' else np.arange(cout) % 7 - 3      # tells the output channels apart
    bias = rng.integers(-8, 9, cout)
    res1 = rng.integers(-8, 9, (shape[0], ho, wo, cout))
    res2 = rng.integers(-8, 9, (shape[0], ho, wo, cout))
    return x, w, bias, res1, res2


INT_LINEAR_CASES = [(n, k) for n in (96, 160) for k in (64, 1024)]      # ragged N, K
INT_LINEAR_ROWS = 77 + 64 * 3                                            # a ragged last row tile


def int_linear_operands(n, k):
    rng = np.random.default_rng(1000 * n + k)
    x = sparse_ints(rng, (INT_LINEAR_ROWS, k), -2, 2)
    w = rng.integers(-3, 4, (k, n))
    w[0, :] = np.arange(n) % 7 - 3
    return x, w, rng.integers(-8, 9, n), rng.integers(-8, 9, (INT_LINEAR_ROWS, n)), rng.integers(-8, 9, (INT_LINEAR_ROWS, n))


ATT_CASES = [(b, h, w, heads, shift) for (b, h, w) in ((2, 16, 24), (1, 8, 8)) for heads in (1, 8) for shift in (0, 4)]
ATT_HEAD_DIM = 32          # the kernel's head dimension: C = 32 heads


def attention_operands(b, h, w, heads):
    """qkv (b, h*w, 3 C), C = 32 heads, with q = k = 0 and V[token, d] = (7 token + d) % 251 + 1, and V alone as int64."""
    c = ATT_HEAD_DIM * heads
    t = np.arange(b * h * w, dtype=np.int64).reshape(b, h * w, 1)
    v = (7 * t + np.arange(c, dtype=np.int64)[None, None, :]) % 251 + 1
    qkv = np.zeros((b, h * w, 3 * c), np.float32)
    qkv[:, :, 2 * c:] = v
    return qkv, v


VQ_CASES = [(n_e, 64, m) for n_e in (128, 64) for m in (1, 130, 333)]


def vq_operands(n_e, d, m):
    """Integer codebook in {-3..3} (with duplicated codes: exact ties), rows in {-4..4}; 40 identical rows and an all-zero row
    when M allows."""
    rng = np.random.default_rng(n_e * 1000 + m)
    cb = rng.integers(-3, 4, (n_e, d))
    cb[n_e - 5] = cb[7]                 # exact ties between far-apart codes and inside one 32-column tile
    cb[8] = cb[7]
    z = rng.integers(-4, 5, (m, d))
    if m >= 130:
        z[50:90] = z[50]
        z[100] = 0
        z[101] = cb[7]
    else:
        z[0] = cb[7]
    return z, cb


# ------------------------------------------------------------------ network cases and the conditions pinned on the CPU
# (tests/test_structured_inputs_host.py asserts every one of these without a GPU)
# LR sizes: mirror pad on both axes.  x4 pads 13 x 19 to 16 x 32.  x2 pads to multiples of 32, and a mirror pad holds at most 2 h
# rows (the reference's cat([x, flip(x)])[:h + pad]): 13 rows cannot reach 32 - the library refuses such a call -, so x2 takes the
# smallest odd height that can, 17 x 19 -> 32 x 32.
NET_LR = {'x4': (13, 19), 'x2': (17, 19)}
# weight seed: the first of 0..32 for which (a) no token of any content has its two best codes within (0, NEAR_TIE_ULP] ulp in the
# oracle and (b) the CPU emulation of linear_math='fp16' (operands rounded once to fp16, tests/fp16_front_ref.py) resolves every token of
# every content to the code the fp32 emulation picks.  (a) alone holds for seed 0, but fp16 operands move z by ~1e-3 relative, not by
# ulps: under seed 0 the emulation flips three tokens, and the GPU one each of x4 white / pure_red / step_v and x2 white.  Seeds 0..21 all
# miss (a) or (b); 22 has both, with the smallest gap 31 ulp (fp32) and 27 ulp (fp16 emulation).
NET_SEED = 22
NET_CASES = [('x4', c) for c in CONTENTS] + [('x2', c) for c in ('black', 'white', 'step_v', 'impulse_corner')]
NET_DROPPED = ()                # contents left out of the non-strict modes because no seed below 32 clears them: none

# GroupNorm clamp cases: gray level k / 255 as a constant map whose UNCLAMPED fp64 variance SS/N - mean^2, summed in the
# specified order, is negative.  (shape, k)
GN_CLAMP_TILED = ((1, 13, 21, 64), 250)         # 8x16-tile order (C / 32 a power of two): the partial-moments finalize kernel
GN_CLAMP_ROWS = ((1, 13, 21, 96), 14)           # row order (C / 32 = 3): the generic finalize kernel

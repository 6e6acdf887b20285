"""The bit-for-bit checker of the wavelet colour fix (femasr_amd/colorfix.py, csrc/colorfix.hip): the GPU's operation order restated in
float32 numpy.  `up` is the float64 imresize of the float32 planes rounded once; every later step is ONE float32 operation, in the
order and with the parentheses of the definition (numpy rounds every float32 array operation on its own: no fused multiply-add, no
wider intermediate).  The weights 1/4 and 1/2 are exact."""
import numpy as np

from femasr_amd.models.femasr_model import imresize

EPS = 2.0 ** -24
Q, HALF = np.float32(0.25), np.float32(0.5)


def up_f32(lq32, s):
    """femasr_amd.resize.imresize of float32 planes: fp64 accumulation in tap order, rounded once."""
    assert lq32.dtype == np.float32
    return imresize(lq32.astype(np.float64), s).astype(np.float32)


def blur_f32(d, levels):
    assert d.dtype == np.float32
    h, w = d.shape[-2:]
    ys, xs = np.arange(h), np.arange(w)
    for i in range(levels):
        r = 1 << i
        xm, xp = np.clip(xs - r, 0, w - 1), np.clip(xs + r, 0, w - 1)
        ym, yp = np.clip(ys - r, 0, h - 1), np.clip(ys + r, 0, h - 1)
        t = (Q * d[..., :, xm] + HALF * d) + Q * d[..., :, xp]
        d = (Q * t[..., ym, :] + HALF * t) + Q * t[..., yp, :]
        assert d.dtype == np.float32
    return d


def color_fix_f32(sr32, lq32, levels):
    """(..., sH, sW) and (..., H, W) float32 -> float32: what femasr_color_fix stores."""
    assert sr32.dtype == np.float32
    s = sr32.shape[-1] // lq32.shape[-1]
    return sr32 + blur_f32(up_f32(lq32, s) - sr32, levels)


def u8_planes(img_u8):
    """(..., H, W, 3) bytes -> (..., 3, H, W) float32 planes (float)byte / 255.0f, IEEE division."""
    assert img_u8.dtype == np.uint8
    return np.moveaxis(img_u8.astype(np.float32) / np.float32(255.0), -1, -3)


def quantise(planes):
    """(..., 3, H, W) -> (..., H, W, 3) bytes: rint(clamp(v, 0, 1) * 255), half to even (tensor2img)."""
    v = np.clip(planes, 0, 1)
    v = v * (np.float32(255.0) if planes.dtype == np.float32 else 255.0)
    return np.moveaxis(np.rint(v), -3, -1).astype(np.uint8)


def color_fix_u8(sr_u8, lq_u8, levels):
    """(..., sH, sW, 3) and (..., H, W, 3) bytes -> bytes: what femasr_color_fix_u8 stores."""
    return quantise(color_fix_f32(u8_planes(sr_u8), u8_planes(lq_u8), levels))


def bound(levels, sr, up):
    """(8 L + 6) 2^-24 V, V = max(max|sr|, max|up|): per level 4 roundings of a convex combination of values <= max|d| <= 2 V, the
    subtraction 2 eps V, the rounding of up eps V, the final add (|out| <= 3 V) 3 eps V."""
    v = max(float(np.abs(sr).max()), float(np.abs(up).max()))
    return (8 * levels + 6) * EPS * v


# the shapes of both test files, as LR (H, W, s): 20x28 is smaller than twice the largest radius of levels = 5 (both clamps act on one
# tap set), 66x38 is odd-sized and no multiple of any block, 96x160 spans several blocks
SHAPES = [(5, 7, 4), (33, 19, 2), (24, 40, 4)]
LEVELS = [1, 3, 5]
_CASES = {}


def case(h, w, s, batch):
    """Seeded inputs, built once and never written to: float32 sr (batch, 3, sH, sW) in [-0.1, 1.1], lq (batch, 3, H, W) in [0, 1], and
    uint8 images sr_u8 (batch, sH, sW, 3), lq_u8 (batch, H, W, 3)."""
    key = (h, w, s, batch)
    if key not in _CASES:
        g = np.random.default_rng(1000 * h + 10 * w + s)
        lq = g.random((2, 3, h, w), dtype=np.float32)
        sr = (up_f32(lq, s) + g.normal(0, 0.1, (2, 3, s * h, s * w)).astype(np.float32) +
              g.uniform(-0.1, 0.1, (2, 3, 1, 1)).astype(np.float32)).astype(np.float32)
        lq_u8 = g.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        sr_u8 = quantise(up_f32(u8_planes(lq_u8), s) + g.normal(0, 0.08, (2, 3, s * h, s * w)).astype(np.float32) +
                         np.array([0.06, -0.05, 0.04], np.float32).reshape(1, 3, 1, 1))
        for a in (lq, sr, lq_u8, sr_u8):
            a.setflags(write=False)
        _CASES[(h, w, s, 2)] = (sr, lq, sr_u8, lq_u8)
        _CASES[(h, w, s, 1)] = tuple(a[:1] for a in (sr, lq, sr_u8, lq_u8))
    return _CASES[key]

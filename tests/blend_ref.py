"""The overlap-blend canvas of `test_tile(..., blend=True)` in float64, straight from the definition:

    out[b, c, Y, X] = sum_k w_k(Y, X) v_k[b, c, Y - Ay_k, X - Ax_k] / sum_k w_k(Y, X),   w_k = wy_k(Y) wx_k(X)

over the tiles k whose upscaled window contains (Y, X), with the 1-D weights of femasr_amd.tiling.blend_weight_1d.  The
checker of tests/test_tile_blend_host.py and tests/test_gpu_tile_blend.py; numpy only.
"""
import numpy as np

from femasr_amd import tiling

EPS = 2.0 ** -24            # unit roundoff of fp32
BOUND = 16 * EPS            # |fp32 result - definition| <= (2n + 6) eps max|v| = 14 eps max|v| for n <= 4 covering tiles: the tests use 16


class BlendRef:
    """canvas (B, C, Ho, Wo) float64 and, per pixel: vmax = max |v| over the covering tiles' values (B, C, Ho, Wo), cover = how many
    windows contain it (Ho, Wo), wsum = sum of their weights (Ho, Wo), one = exactly one window, with weight exactly 1 (Ho, Wo)."""

    def __init__(self, tiles, values, s, height, width):
        """tiles: row-major `tiling.Tile`s; values[k]: tile k as a (B, C, th, tw) array (any float or integer dtype)."""
        b, c = values[0].shape[:2]
        ho, wo = height * s, width * s
        acc = np.zeros((b, c, ho, wo))
        self.vmax = np.zeros((b, c, ho, wo))
        self.wsum = np.zeros((ho, wo))
        self.cover = np.zeros((ho, wo), np.int32)
        wmax = np.zeros((ho, wo))
        for t, v in zip(tiles, values):
            ay, ax, th, tw, ly, ry, lx, rx = tiling.blend_geom(t, s)
            assert v.shape == (b, c, th, tw), (v.shape, (b, c, th, tw))
            w = tiling.blend_weight_1d(th, ly, ry)[:, None] * tiling.blend_weight_1d(tw, lx, rx)[None, :]
            v = v.astype(np.float64)
            win = (slice(ay, ay + th), slice(ax, ax + tw))
            acc[(slice(None), slice(None)) + win] += w * v
            self.vmax[(slice(None), slice(None)) + win] = np.maximum(self.vmax[(slice(None), slice(None)) + win], np.abs(v))
            self.wsum[win] += w
            self.cover[win] += 1
            wmax[win] = np.maximum(wmax[win], w)
        assert self.cover.min() >= 1
        self.canvas = acc / self.wsum
        self.one = (self.cover == 1) & (wmax == 1.0)

    def bound(self, floor=1.0):
        """Per-pixel error allowance of the fp32 evaluation: 16 * 2^-24 * max|v| over the covering tile values, floored at `floor`."""
        return BOUND * np.maximum(self.vmax, floor)


def tile_values(tiles, run, x):
    """[run(x[:, :, window]) as a (B, C, th, tw) numpy array for every tile]: one call per crop, like the reference's loop."""
    return [np.asarray(run(x[:, :, t.y0p:t.y1p, t.x0p:t.x1p]).cpu()) for t in tiles]


def check_u8(got, ref, max_tie_share=0.01):
    """got: uint8 array shaped like ref.canvas; must equal rint(clamp(ref.canvas, 0, 255)) except where the float64 value lies within
    16 * 2^-24 * 255 of k + 0.5: there either neighbour is accepted.  At most `max_tie_share` of the bytes may fall under the exception
    (counted from the definition alone).  Returns (bytes that differ outside the exception, share of near-tie bytes)."""
    d = np.clip(ref.canvas, 0.0, 255.0)
    want = np.rint(d)
    frac = d - np.floor(d)
    tie = np.abs(frac - 0.5) <= BOUND * 255
    share = float(tie.mean())
    lo, hi = np.floor(d), np.ceil(d)
    ok = np.where(tie, (got == lo) | (got == hi), got == want)
    return int((~ok).sum()), share

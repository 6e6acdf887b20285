"""numpy restatement of the x8 geometric self-ensemble (femasr_amd/ensemble.py): the checker of tests/test_self_ensemble_host.py
and of the bit-for-bit GPU tests (tests/test_gpu_self_ensemble.py).  Written from the INDEX FORMULAS of the definition (explicit gathers),
not from flips and transposes, so that the torch definition - which is written with flips and transposes - is checked against something
else.  An image batch is float32 (B,C,H,W) or uint8 (B,H,W,3); `axes` says where its rows and columns are."""
import numpy as np

SHAPES = [(1, 1), (1, 9), (9, 1), (31, 33), (63, 65), (64, 64), (65, 127), (130, 66)]      # brackets the kernels' 64x64 LDS tile (and a 32x32 one)


def axes(a):
    return (a.ndim - 3, a.ndim - 2) if a.dtype == np.uint8 else (a.ndim - 2, a.ndim - 1)


def _gather(a, rows, cols):
    """a[..., rows[i, j], cols[i, j](, :)] for index grids of the result's shape."""
    r, c = axes(a)
    a = np.moveaxis(a, (r, c), (0, 1))
    return np.ascontiguousarray(np.moveaxis(a[rows, cols], (0, 1), (r, c)))


def forward(x, k):
    """x_k by the definition's index formulas."""
    v, h, t = k & 1, (k >> 1) & 1, (k >> 2) & 1
    r, c = axes(x)
    H, W = x.shape[r], x.shape[c]
    if t == 0:
        i, j = np.mgrid[0:H, 0:W]
        return _gather(x, H - 1 - i if v else i, W - 1 - j if h else j)
    i, j = np.mgrid[0:W, 0:H]
    return _gather(x, H - 1 - j if v else j, W - 1 - i if h else i)


def inverse(y, k, out_hw):
    """z_k (out_hw = (sH, sW) of the ensemble's result) from y_k by the definition's index formulas."""
    v, h, t = k & 1, (k >> 1) & 1, (k >> 2) & 1
    sH, sW = out_hw
    i, j = np.mgrid[0:sH, 0:sW]
    if t == 0:
        return _gather(y, sH - 1 - i if v else i, sW - 1 - j if h else j)
    return _gather(y, sW - 1 - j if h else j, sH - 1 - i if v else i)


def expand(x):
    """(straight (4,B,...), transposed (4,B,...))."""
    return np.stack([forward(x, k) for k in range(4)]), np.stack([forward(x, 4 + k) for k in range(4)])


def round_eighth(s):
    """S / 8 rounded half to even, in integers."""
    s = np.asarray(s, np.int64)
    return (s + 3 + ((s >> 3) & 1)) >> 3


def merge(straight, transposed, order=range(8)):
    """float32: 0.125f * the sequential fp32 sum of z_k in `order` (the definition: 0..7); uint8: S / 8 of the bytes, half to even."""
    r, c = axes(straight[0])
    hw = (straight.shape[1 + r], straight.shape[1 + c])
    z = [inverse(straight[k], k, hw) for k in range(4)] + [inverse(transposed[k], 4 + k, hw) for k in range(4)]
    order = list(order)
    if straight.dtype == np.uint8:
        return round_eighth(sum(z[k].astype(np.int64) for k in order)).astype(np.uint8)
    acc = z[order[0]].astype(np.float32)
    for k in order[1:]:
        acc = (acc + z[k]).astype(np.float32)
    return (np.float32(0.125) * acc).astype(np.float32)


def merge_f64(straight, transposed):
    r, c = axes(straight[0])
    hw = (straight.shape[1 + r], straight.shape[1 + c])
    z = [inverse(straight[k], k, hw) for k in range(4)] + [inverse(transposed[k], 4 + k, hw) for k in range(4)]
    return sum(a.astype(np.float64) for a in z) / 8.0


# ------------------------------------------------------------------------------------------------------------------- inputs
def index_f32(b, c, h, w):
    """Index-valued float32: every element differs (exact below 2^24), so a misplaced one shows."""
    return np.arange(b * c * h * w, dtype=np.float32).reshape(b, c, h, w)


def pattern_u8(b, h, w):
    """uint8 (B,H,W,3): horizontally and vertically adjacent pixels and the three channels all differ, and so do the images."""
    i, j, ch, n = np.mgrid[0:h, 0:w, 0:3, 0:b]
    return np.ascontiguousarray(np.moveaxis((i * 7 + j * 13 + ch * 85 + n * 31 + (i * j) % 5) % 256, 3, 0).astype(np.uint8))


def spread_f32(shape, seed):
    """Seeded float32 with magnitudes spread over 2^-6 .. 2^6 and both signs: the summation order matters."""
    g = np.random.default_rng(seed)
    return (g.uniform(1.0, 2.0, shape) * np.exp2(g.integers(-6, 6, shape)) * g.choice([-1.0, 1.0], shape)).astype(np.float32)


def results_f32(b, c, h, w, seed):
    """Eight seeded results for an output of (h, w): (straight (4,b,c,h,w), transposed (4,b,c,w,h))."""
    return spread_f32((4, b, c, h, w), seed), spread_f32((4, b, c, w, h), seed + 1)


def results_u8(b, h, w, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (4, b, h, w, 3), dtype=np.uint8), g.integers(0, 256, (4, b, w, h, 3), dtype=np.uint8)


def paste(tiles_of, tiles, scale, canvas, u8):
    """The reference's overlap-discard paste (femasr_arch.py:443-446) of per-tile results `tiles_of(t)` onto `canvas` (torch or numpy)."""
    for t in tiles:
        o = tiles_of(t)
        ys, ye, xs, xe = t.out_src(scale)
        a, b, c, d = t.out_dst(scale)
        if u8:
            canvas[:, a:b, c:d, :] = o[:, ys:ye, xs:xe, :]
        else:
            canvas[:, :, a:b, c:d] = o[:, :, ys:ye, xs:xe]
    return canvas

"""Inputs shared by tests/test_niqe_host.py and tests/test_gpu_niqe.py: the textured test images, synthetic NIQE parameters, the definition's
results on them (computed once per process and never modified) and the score bar measured from the definition."""
import functools

import numpy as np

from femasr_amd.models import femasr_model as fm

#           name: (H, W, crop_border)
SHAPES = {
    'four_blocks': (192, 192, 0),       # 2 x 2 blocks with different statistics: a roll that wraps across blocks shows
    'ragged_crop': (200, 300, 4),       # 192 x 292 after the crop, 192 x 288 scored: 2 x 3 blocks in column-major order
    'two_blocks': (96, 192, 0),         # the least that gives a finite score; the vertical halo is all border
    'constant_block': (192, 192, 0),    # the top-left block (and the 12 pixels around it) constant 200: one NaN row, alpha 0.2
    'tie_pixels': (192, 192, 0),        # 60 pixels whose exact luma is k + 0.5
    'one_block': (96, 96, 0),           # one block: the covariance is undefined, the score NaN on both sides
}
REFUSED = (95, 200, 0)


@functools.lru_cache(maxsize=None)
def tie_triples():
    """The RGB triples whose exact luma (65481 R + 128553 G + 24966 B) / 255000 + 16 is k + 0.5, by integer search: (194, 3) uint8."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing='ij')
    out = []
    for r in range(256):
        n = 65481 * r + 128553 * g + 24966 * b
        gi, bi = np.nonzero(n % 255000 == 127500)
        out += [(r, int(x), int(y)) for x, y in zip(gi, bi)]
    out = np.array(sorted(out), dtype=np.uint8)
    out.setflags(write=False)
    return out


def textured(h, w, seed):
    """uint8 RGB: a smooth sinusoid plus Gaussian noise (sigma 8, 12 or 16 depending on the 96 x 96 block; uniform noise would pin every
    alpha at the grid's end), clipped."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 70 * np.sin(y / 23.0) * np.cos(x / 31.0)
    sigma = 8.0 + 4.0 * ((y // 96 + 2 * (x // 96)) % 3)
    common = rng.normal(size=(h, w)) * sigma
    img = base[..., None] + np.arange(3) * 6.0 + common[..., None] + rng.normal(size=(h, w, 3)) * 2.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image(name):
    h, w, _ = SHAPES[name]
    img = textured(h, w, seed=100 + sorted(SHAPES).index(name))
    if name == 'constant_block':
        img[:108, :108] = 200
    if name == 'tie_pixels':
        rng = np.random.RandomState(7)
        ties = tie_triples()
        ys, xs = rng.randint(0, h, 60), rng.randint(0, w, 60)
        img[ys, xs] = ties[rng.randint(0, len(ties), 60)]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def params():
    """Synthetic parameters: mu uniform in [0, 1), cov = A A^T / 36 + 0.1 I from a seeded normal A, the 7 x 7 Gaussian of sigma 7/6."""
    rng = np.random.RandomState(2024)
    mu = rng.rand(36)
    a = rng.normal(size=(36, 36))
    cov = a @ a.T / 36 + 0.1 * np.eye(36)
    r = np.arange(7) - 3.0
    win = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2 * (7.0 / 6.0) ** 2))
    win = win / win.sum()
    for v in (mu, cov, win):
        v.setflags(write=False)
    return mu, cov, win


@functools.lru_cache(maxsize=None)
def reference(name):
    """The definition on image(name): dict(y, z, y2, z2, margin, features, positions, score)."""
    mu, cov, win = params()
    crop = SHAPES[name][2]
    y = fm._niqe_y(image(name))
    if crop:
        y = y[crop:-crop, crop:-crop]
    out = {}
    feat, pos = fm.niqe_features(y, win, details=out)
    out.update(features=feat, positions=pos, score=fm.niqe_score_from_features(feat, mu, cov))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def score_bar():
    """Ten times the largest change of the score when the definition's features move by 1e-10 relative with random signs (100 trials per
    image): what a feature error at the features' own tolerance can do to the score, measured through the tail's pinv."""
    mu, cov, _ = params()
    rng = np.random.RandomState(99)
    worst = 0.0
    for name in SHAPES:
        ref = reference(name)
        if not np.isfinite(ref['score']):
            continue
        for _ in range(100):
            f = ref['features'] * (1 + 1e-10 * rng.choice([-1.0, 1.0], size=ref['features'].shape))
            worst = max(worst, abs(fm.niqe_score_from_features(f, mu, cov) - ref['score']))
    return 10 * worst

"""Synthesis of LQ inputs without a GPU (femasr_amd/degrade.py, jpegio.decode_ref): every definition against an independent
implementation (scipy, torch on the CPU, block means, Pillow's decoder), the float32 restatements of the kernels (tests/degrade_ref.py) within
derived bounds of the definitions, the recipes' structure and statistics, the CLI's argument checks and the dataset option.

`python tests/test_degrade_host.py` measures the distance of decode_ref from Pillow again and writes profiles/degrade_report.txt; MEASURED
below holds the figures of that file."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import degrade_ref as R
from femasr_amd import _lib, degrade as D, jpegio, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# profiles/degrade_report.txt: worst and mean |decode_ref - Pillow| in levels over pillow_cases(), per subsampling
MEASURED = {'gray': (1, 0.0302), '444': (3, 0.0637), '420': (28, 0.1858)}


def _img(h, w, seed=0, lo=0.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, (h, w, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- blur
def _kernels():
    rng = np.random.RandomState(5)
    asym = rng.uniform(0, 1, (7, 7))
    asym[0, :] += 3.0                                   # far from any symmetry: a missing flip shows
    asym[:, 1] += 2.0
    return {'box3': np.full((3, 3), 1 / 9.0), 'asym7': asym / asym.sum(), 'iso25': D.fspecial_gaussian(25, 4.0),
            'aniso13': D.anisotropic_gaussian(13, 0.7, 6.0, 1.5), 'shifted': D.shifted_gaussian(4, 1.8)}


@pytest.mark.parametrize('shape', [(1, 1), (3, 40), (5, 7), (31, 33)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_blur_definition_is_scipy_convolve_mirror(shape):
    from scipy import ndimage
    img = _img(*shape, seed=shape[0])
    for name, k in _kernels().items():
        k32 = k.astype(np.float32)
        want = ndimage.convolve(img.astype(np.float64), k32.astype(np.float64)[..., None], mode='mirror')
        got = D.blur_values(img, k32)
        assert np.abs(got - want).max() <= 1e-12, (name, shape)
        for s in (2, 4):
            assert np.array_equal(D.blur_values(img, k32, s), got[0::s, 0::s]), (name, s)
    if min(shape) > 1:                                      # the asymmetric kernel tells a convolution from a correlation
        asym = _kernels()['asym7']
        assert np.abs(D.blur_values(img, asym) - D.blur_values(img, asym[::-1, ::-1].copy())).max() > 1e-3


def test_blur_kernels():
    from scipy import stats
    for k, sigma in ((7, 0.8), (25, 3.3), (15, 0.1)):
        g = D.fspecial_gaussian(k, sigma)
        c = np.arange(k) - k // 2
        yy, xx = np.meshgrid(c, c, indexing='ij')
        pdf = stats.multivariate_normal.pdf(np.stack([xx, yy], -1), mean=[0, 0], cov=np.eye(2) * sigma ** 2)
        pdf = np.where(pdf < np.finfo(float).eps * pdf.max(), 0, pdf)
        assert np.abs(g - pdf / pdf.sum()).max() <= 1e-12 and abs(g.sum() - 1) <= 1e-12
    for k, theta, l1, l2 in ((7, 0.3, 5.0, 0.7), (25, 2.9, 7.5, 7.5), (13, 1.5707, 0.2, 3.0)):
        g = D.anisotropic_gaussian(k, theta, l1, l2)
        want = np.zeros((k, k))
        cov = D.anisotropic_covariance(theta, l1, l2)
        center = k / 2.0 + 0.5
        for y in range(k):                                  # gm_blur_kernel's loop and grid
            for x in range(k):
                want[y, x] = stats.multivariate_normal.pdf([x - center + 1, y - center + 1], mean=[0, 0], cov=cov)
        assert np.abs(g - want / want.sum()).max() <= 1e-12 and abs(g.sum() - 1) <= 1e-12
    # the shifted kernel: a bilinear shift by (sf - 1) / 2 of the Gaussian moves its centre of mass there (but for the clipped last rows)
    for sf in (2, 4):
        g = D.shifted_gaussian(sf, 1.2)
        c = np.arange(25)
        assert g.shape == (25, 25) and abs(g.sum() - 1) <= 1e-12
        assert abs((g.sum(1) * c).sum() - (12 - (sf - 1) / 2)) < 1e-6 and abs((g.sum(0) * c).sum() - (12 - (sf - 1) / 2)) < 1e-6
    assert np.allclose(D.shifted_gaussian(1, 1.2), D.fspecial_gaussian(25, 1.2), atol=1e-15)
    for bad in (np.ones((4, 4)), np.ones((27, 27)), np.ones((3, 5)), np.ones(3)):
        with pytest.raises(ValueError):
            D.check_kernel(bad)
    with pytest.raises(ValueError):
        D.blur_values(_img(4, 4), np.ones((3, 3)), 3)


def test_blur_restatement_within_its_bound():
    for shape, lo, hi in (((5, 7), 0, 1), ((31, 33), 0, 1), ((20, 9), -0.3, 1.4)):
        img = _img(*shape, seed=3, lo=lo, hi=hi)
        xmax = float(np.abs(img).max())
        for name, k in _kernels().items():
            for s in (1, 2, 4):
                err = np.abs(R.blur_f32(img, k, s).astype(np.float64) - D.blur_values(img, k, s)).max()
                assert err <= R.blur_bound(k.shape[0], xmax), (name, s, err)
                assert np.abs(D.blur_ref(img, k, s).astype(np.float64) - D.blur_values(img, k, s)).max() <= R.U * xmax * 1.01


# ---------------------------------------------------------------------------------------------------------------- resize
def _torch_resize(img, oh, ow, mode):
    t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    return torch.nn.functional.interpolate(t, size=(oh, ow), mode=mode, align_corners=False)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize('size', [(9, 14, 18, 28), (17, 23, 5, 8), (8, 8, 1, 1), (12, 10, 19, 7), (6, 259, 6, 64)], ids=str)
def test_bilinear_and_bicubic_are_torch_interpolate(size):
    """torch computes in float64 here with float64 coefficients; ours has float32 coefficients.  A coefficient is off by at most 2^-24 |w| < 2^-24
    * 1.27 (the cubic's largest value), a pass with `taps` of them by taps * 1.27 * 2^-24 * X, and the second pass sees inputs bounded by
    S X (S = sum |w| <= 1.6): together (taps_h + taps_w) * 1.27 * 1.6 * 2^-24 X, and 1e-12 for the two float64 summation orders."""
    h, w, oh, ow = size
    img = _img(h, w, seed=h + w)
    for filt, taps in (('bilinear', 2), ('bicubic', 4)):
        th, tw = D.tap_table(filt, h, oh), D.tap_table(filt, w, ow)
        assert th[0].shape == (oh, taps) and tw[1].shape == (ow, taps) and th[1].min() >= 0 and th[1].max() < h
        got = D.resize_values(img, th, tw)
        want = _torch_resize(img, oh, ow, filt)
        assert np.abs(got - want).max() <= 2 * taps * 1.27 * 1.6 * R.U + 1e-12, (filt, np.abs(got - want).max())


def test_area_is_the_block_mean_and_covers_fractions():
    rng = np.random.RandomState(2)
    for r in (1, 2, 4, 8):
        img = (rng.randint(0, 256, (3 * r, 5 * r, 3)) / 256.0).astype(np.float32)       # dyadic: the float64 sums are exact
        got = D.resize_values(img, D.tap_table('area', 3 * r, 3), D.tap_table('area', 5 * r, 5))
        want = img.astype(np.float64).reshape(3, r, 5, r, 3).mean(axis=(1, 3))
        assert np.array_equal(got, want), r
    for n_in, n_out in ((79, 10), (259, 64), (10, 7), (33, 33), (5, 1)):
        w, idx = D.tap_table('area', n_in, n_out)
        r = n_in / n_out
        assert w.shape[1] == int(np.ceil(r)) + 1 and np.abs(w.astype(np.float64).sum(1) - 1).max() <= w.shape[1] * R.U
        cover = np.zeros((n_out, n_in))
        np.add.at(cover, (np.arange(n_out)[:, None].repeat(w.shape[1], 1), idx), w)
        for x in range(n_out):                              # the exact coverage of [x r, (x + 1) r)
            lo, hi = x * r, min((x + 1) * r, n_in)
            want = np.clip(np.minimum(hi, np.arange(n_in) + 1) - np.maximum(lo, np.arange(n_in)), 0, None) / (hi - lo)
            assert np.abs(cover[x] - want).max() <= 2 * R.U, (n_in, n_out, x)
    # an axis that grows: the sampler substitutes bilinear
    op = {'op': 'resize', 'filter': 'area', 'out_h': 12, 'out_w': 5}
    th, tw = D.op_tables(op, 8, 10)
    assert np.array_equal(th[0], D.tap_table('bilinear', 8, 12)[0]) and np.array_equal(tw[0], D.tap_table('area', 10, 5)[0])


def test_matlab_tables_are_imresize():
    from femasr_amd.models.femasr_model import imresize
    img = _img(24, 36, seed=8)
    for scale in (0.5, 0.25):
        oh, ow = int(24 * scale), int(36 * scale)
        th, tw = D.tap_table('matlab', 24, oh), D.tap_table('matlab', 36, ow)
        want = imresize(img.astype(np.float64).transpose(2, 0, 1), scale).transpose(1, 2, 0)
        s = float(np.abs(th[0]).sum(1).max() * np.abs(tw[0]).sum(1).max())
        assert np.abs(D.resize_values(img, th, tw) - want).max() <= (th[0].shape[1] + tw[0].shape[1]) * s * R.U + 1e-12
    with pytest.raises(ValueError):
        D.tap_table('lanczos', 8, 4)
    w, idx = D.tap_table('bilinear', 8, 4)
    for bad_idx in (idx + 5, idx - 1):
        with pytest.raises(ValueError):
            D.check_table(w, bad_idx.astype(np.int32), 8, 4)


def test_resize_restatement_within_its_bound():
    for h, w, oh, ow in ((9, 14, 18, 28), (40, 79, 5, 10), (12, 259, 7, 64), (16, 16, 1, 1)):
        img = _img(h, w, seed=oh)
        for filt in D.FILTERS:
            if filt == 'matlab' and (oh >= h or min(oh, ow) < 4):
                continue
            op = {'op': 'resize', 'filter': filt, 'out_h': oh, 'out_w': ow}
            th, tw = D.op_tables(op, h, w)
            err = np.abs(R.resize_f32(img, th, tw).astype(np.float64) - np.clip(D.resize_values(img, th, tw), 0, 1)).max()
            assert err <= R.resize_bound(th, tw, 1.0), (filt, h, w, oh, ow, err)


# ---------------------------------------------------------------------------------------------------------------- noise
def test_noise_statistics_and_independence_of_the_split():
    n = 256 * 256
    zero = np.zeros((256, 256, 3), np.float32)
    rng = np.random.RandomState(4)
    m = rng.uniform(-1, 1, (3, 3))
    cov = (25 / 255.0) ** 2 * (m @ m.T)
    cases = {'color': np.eye(3) * 0.07, 'gray': np.eye(3) * 0.04, 'correlated': D.factor_of_covariance(cov)}
    assert np.allclose(cases['correlated'] @ cases['correlated'].T, cov, atol=1e-15)
    for mode, a in cases.items():
        v = D.noise_values(zero, mode, a.reshape(-1), seed=1234 + len(mode)).reshape(-1, 3)
        nominal = a[0, 0] ** 2 * (np.ones((3, 3)) if mode == 'gray' else np.eye(3)) if mode != 'correlated' else cov
        if mode == 'gray':
            assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 0], v[:, 2])
        sd = np.sqrt(np.diag(nominal))
        assert np.all(np.abs(v.mean(0)) <= 5 * sd / np.sqrt(n)), mode
        got = v.T @ v / n
        # standard error of a sample covariance of Gaussians: sqrt((c_ii c_jj + c_ij^2) / n)
        se = np.sqrt((np.outer(np.diag(nominal), np.diag(nominal)) + nominal ** 2) / n)
        assert np.all(np.abs(got - nominal) <= 5 * se), (mode, got, nominal)
    # the field does not depend on how the index range is split
    img = _img(20, 30, seed=6)
    whole = D.noise_values(img, 'correlated', cases['correlated'].reshape(-1), 77)
    cut = 7 * 30
    parts = [D.noise_values(img.reshape(-1, 3)[:cut], 'correlated', cases['correlated'].reshape(-1), 77),
             D.noise_values(img.reshape(-1, 3)[cut:], 'correlated', cases['correlated'].reshape(-1), 77, offset=cut)]
    assert np.array_equal(np.concatenate(parts).reshape(whole.shape), whole)
    assert not np.array_equal(D.noise_values(img, 'color', cases['color'].reshape(-1), 78), D.noise_values(img, 'color', cases['color'].reshape(-1), 79))
    out = D.noise_ref(img, 'color', cases['color'].reshape(-1), 5)
    assert out.dtype == np.float32 and out.min() >= 0 and out.max() <= 1
    normals = D.normal_ref(9, np.arange(1 << 16))
    assert np.isfinite(normals).all() and abs(normals.mean()) < 5 / 256 and abs(normals.var() - 1) < 5 * np.sqrt(2) / 256
    for bad in (('pink', np.eye(3)), ('color', np.eye(2)), ('color', np.eye(3) * 99), ('gray', np.full((3, 3), np.nan))):
        with pytest.raises(ValueError):
            D.check_noise(bad[0], bad[1])


# ---------------------------------------------------------------------------------------------------------------- bytes and JPEG
def test_quantize_and_unit():
    x = (np.arange(-51, 562) / 510.0).astype(np.float32)                    # every multiple of 1/510 in [-0.1, 1.1]
    got = D.quantize_ref(x)
    want = np.array([int(np.rint(np.float32(np.float32(min(max(v, 0), 1)) * np.float32(255)))) for v in x], np.uint8)
    assert np.array_equal(got, want)
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(D.quantize_ref(D.unit_ref(u)), u) and D.unit_ref(u).dtype == np.float32


def test_decode_intermediates_fit_int32_and_flat_images_return():
    t = np.abs(jpegio.DCT_TABLE)
    assert int(t.sum(0).max()) == 21641 and int(t.sum(1).max()) <= 23168
    c_max = (21641 * 2047 + 512) >> 10
    assert 21641 * 2047 < 1 << 26 and c_max == 43261 and 21641 * c_max + 32768 < 1 << 30
    for p in (0, 1, 17, 127, 128, 200, 254, 255):
        for shape in ((9, 17), (20, 13, 3)):
            img = np.full(shape, p, np.uint8)
            for ss in jpegio.SUBSAMPLINGS:
                comps = jpegio.coefficients_ref(img, 100, ss)
                assert np.array_equal(jpegio.decode_ref(comps, 100, ss, shape[0], shape[1]), img), (p, shape, ss)
    # the clip of the dequantised coefficients bounds planes that no encoder made
    wild = [np.full((1, 1, 64), v, np.int16) for v in (32767, -32768, 32767)]
    out = jpegio.decode_ref(wild, 1, '444', 8, 8)
    assert out.shape == (8, 8, 3) and out.dtype == np.uint8
    for bad in (([wild[0], wild[1]], '444', 8, 8), (wild, '422', 8, 8), (wild, '444', 9, 8), (wild, '420', 8, 8), ([wild[0].astype(np.int32)], '444', 8, 8)):
        with pytest.raises(ValueError):
            jpegio.decode_ref(bad[0], 50, bad[1], bad[2], bad[3])


def test_round_trip_is_idempotent_on_the_quantisers_lattice():
    """The pixels decode_ref returns for a smooth image lie on the quantiser's lattice: encoding them gives back the same coefficients
    (the two transforms are inverse within 1.2 coefficient levels - DCT_BOUND and its mirror image -, far below Q / 2 at these qualities,
    and the colour and chroma steps return to the same planes), so a second round trip changes nothing: gray, 4:4:4 and 4:2:0, bit for bit."""
    rng = np.random.RandomState(7)
    for ss, shape in (('444', (24, 32)), ('444', (24, 32, 3)), ('420', (32, 48, 3))):
        for q in (30, 60):
            smooth = np.clip(128 + 60 * np.sin(np.arange(shape[0])[:, None] / 5.0) * np.cos(np.arange(shape[1])[None, :] / 7.0), 40, 215)
            img = (smooth[..., None].repeat(3, 2) + rng.randint(-6, 7, shape[:2] + (3,))).astype(np.uint8)
            img = img[..., 0] if len(shape) == 2 else img
            once = jpegio.decode_ref(jpegio.coefficients_ref(img, q, ss), q, ss, shape[0], shape[1])
            assert not np.array_equal(once, img)
            twice = jpegio.decode_ref(jpegio.coefficients_ref(once, q, ss), q, ss, shape[0], shape[1])
            assert np.array_equal(twice, once), (ss, shape, q, int(np.abs(twice.astype(int) - once.astype(int)).max()))


def pillow_cases():
    rng = np.random.RandomState(11)
    out = []
    for h, w in ((70, 90), (40, 56)):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0), 128 + 90 * np.cos(xx / 13.0 + yy / 5.0), (2 * xx + 3 * yy) % 256], 2)
        out += [('smooth', np.clip(np.rint(smooth), 0, 255).astype(np.uint8)), ('noise', rng.randint(0, 256, (h, w, 3)).astype(np.uint8))]
    return out


def measure_pillow():
    """{subsampling: (worst, mean) |decode_ref - Pillow|} over pillow_cases() x Q (30, 60, 95), and the per-case lines of the report."""
    res, lines = {}, []
    for ss in ('gray', '444', '420'):
        worst, total, count = 0, 0.0, 0
        for name, rgb in pillow_cases():
            img = rgb[..., 1] if ss == 'gray' else rgb
            for q in (30, 60, 95):
                sub = '444' if ss == 'gray' else ss
                comps = jpegio.coefficients_ref(img, q, sub)
                ours = jpegio.decode_ref(comps, q, sub, img.shape[0], img.shape[1]).astype(np.int64)
                with Image.open(io.BytesIO(jpegio.encode_ref(img, q, sub))) as im:
                    theirs = np.array(im).astype(np.int64)
                d = np.abs(ours - theirs)
                rm = lambda v: float(np.sqrt(((v - img.astype(np.int64)) ** 2).mean()))      # noqa: E731
                lines.append(f'{ss:5s} {name:6s} {img.shape[0]}x{img.shape[1]} Q{q:<3d} max {int(d.max()):3d}  mean {d.mean():.4f}  '
                             f'rmse to source ours {rm(ours):.3f} Pillow {rm(theirs):.3f}')
                worst, total, count = max(worst, int(d.max())), total + float(d.sum()), count + d.size
        res[ss] = (worst, total / count)
    return res, lines


def test_decode_ref_against_pillow():
    """Pillow (libjpeg) decodes the bytes of encode_ref; decode_ref decodes the coefficients.  The two round at different stages (libjpeg's
    IDCT, its two-pass upsampling), so the comparison is a distance: max <= measured worst + 1 level, mean <= 1.25 x measured."""
    res, lines = measure_pillow()
    print('\n'.join(lines))
    for ss, (worst, mean) in res.items():
        print(f'{ss}: worst {worst}, mean {mean:.4f} (recorded {MEASURED[ss]})')
        assert worst <= MEASURED[ss][0] + 1 and mean <= 1.25 * MEASURED[ss][1], (ss, worst, mean)


def test_jpeg_op_definition():
    img = _img(21, 34, seed=9)
    out = D.jpeg_ref(img, 60)
    u8 = D.jpeg_ref(img, 60, final=True)
    assert out.dtype == np.float32 and out.shape == img.shape and u8.dtype == np.uint8 and np.array_equal(D.quantize_ref(out), u8)
    assert np.array_equal(u8, jpegio.decode_ref(jpegio.coefficients_ref(D.quantize_ref(img), 60, '420'), 60, '420', 21, 34))
    assert 5 < np.abs(u8.astype(int) - D.quantize_ref(img).astype(int)).mean() < 80       # it is lossy, and it is the same picture


# ---------------------------------------------------------------------------------------------------------------- recipes
def test_recipes_are_functions_of_seed_and_name():
    a = D.sample_recipe(123, 'a/b.png', 97, 83, 4)
    assert a == D.sample_recipe(123, 'a/b.png', 97, 83, 4) and a != D.sample_recipe(123, 'a/c.png', 97, 83, 4) and a != D.sample_recipe(124, 'a/b.png', 97, 83, 4)
    back = D.Recipe.from_json(a.to_json())
    assert back == a and isinstance(back, D.Recipe) and json.loads(json.dumps(a)) == a
    assert a['crop'] == [96, 80] and a['out'] == [24, 20] and a['size'] == [97, 83]
    for bad in (dict(sf=3), dict(mode='x'), dict(h=3)):
        kw = dict(dict(seed=1, name='n', h=40, w=40, sf=4), **bad)
        with pytest.raises(ValueError):
            D.sample_recipe(**kw)
    bic = D.sample_recipe(1, 'n', 67, 45, 2, mode='bicubic')
    assert bic['ops'] == [{'op': 'resample_u8', 'out_h': 33, 'out_w': 22}] and bic['crop'] == [66, 44]


def test_recipe_structure_and_branch_shares():
    n = 4000
    count = dict(pre=0, jpeg=0, ds2_resize=0, color=0, gray=0, correlated=0)
    for i in range(n):
        h, w = 64 + i % 7, 72 + i % 5
        r = D.sample_recipe(9, f'img{i}.png', h, w, 4)
        ops = r['ops']
        kinds = [o['op'] for o in ops]
        assert kinds[0] == 'unit' and kinds[-1] == 'jpeg' and ops[-1]['final'] and r['out'] == [h // 4, w // 4]
        pre = kinds[1] == 'resize' and (ops[1]['out_h'], ops[1]['out_w']) == (r['crop'][0] // 2, r['crop'][1] // 2) and \
            sum(o['op'] == 'resize' or (o['op'] == 'blur' and o['kind'] == 'shifted') for o in ops) == 3
        count['pre'] += pre
        body = ops[2:] if pre else ops[1:]
        down = [j for j, o in enumerate(body) if o['op'] == 'resize' or (o['op'] == 'blur' and o['kind'] == 'shifted')]
        assert len(down) == 2 and body[down[1]]['op'] == 'resize', kinds                  # downsample3 behind downsample2
        assert (body[down[1]]['out_h'], body[down[1]]['out_w']) == (h // 4, w // 4)
        count['ds2_resize'] += body[down[0]]['op'] == 'resize'
        blurs = [o for o in body if o['op'] == 'blur' and o['kind'] != 'shifted']
        noises = [o for o in body if o['op'] == 'noise']
        jpegs = [o for o in body if o['op'] == 'jpeg']
        assert len(blurs) == 2 and len(noises) == 1 and len(jpegs) in (1, 2)
        assert all(o['k'] % 2 == 1 and 7 <= o['k'] <= 25 and o['stride'] == 1 for o in blurs)
        assert all(30 <= o['quality'] <= 95 for o in jpegs)
        if body[down[0]]['op'] == 'blur':
            assert body[down[0]]['stride'] == (2 if pre else 4) and body[down[0]]['k'] == 25
        count['jpeg'] += len(jpegs) == 2
        count[noises[0]['mode']] += 1
        a = np.array(noises[0]['factor']).reshape(3, 3)
        assert np.isfinite(a).all() and np.abs(a).max() <= 25 / 255.0 * 3
    for key, p in (('pre', 0.25), ('jpeg', 0.9), ('ds2_resize', 0.75), ('color', 0.4), ('gray', 0.4), ('correlated', 0.2)):
        se = np.sqrt(p * (1 - p) / n)
        assert abs(count[key] / n - p) <= 5 * se, (key, count[key] / n, p)
    for sf, (h, w) in ((2, (67, 45)), (4, (67, 45)), (2, (96, 80)), (4, (9, 6))):
        for i in range(40):
            r = D.sample_recipe(i, 'x', h, w, sf)
            assert r['out'] == [h // sf, w // sf] and r['ops'][-1] == dict(r['ops'][-1], op='jpeg', final=True)


def test_degrade_ref_chains_and_the_bicubic_recipe_is_resample_ref():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (67, 45, 3)).astype(np.uint8)
    for sf in (2, 4):
        rec = D.sample_recipe(5, 'p.png', 67, 45, sf, mode='bicubic')
        crop = img[:67 - 67 % sf, :45 - 45 % sf]
        assert np.array_equal(D.degrade_ref(img, rec), resample.resample_ref(np.ascontiguousarray(crop), 67 // sf, 45 // sf))
    for seed in range(4):
        rec = D.sample_recipe(seed, 'p.png', 67, 45, 4)
        out = D.degrade_ref(img, D.Recipe.from_json(rec.to_json()))
        assert out.shape == (16, 11, 3) and out.dtype == np.uint8 and np.array_equal(out, D.degrade_ref(img, rec))
        x = np.ascontiguousarray(img[:64, :44])
        for op in rec['ops']:
            x = D.op_ref(x, op)
        assert np.array_equal(x, out)
    with pytest.raises(ValueError):
        D.degrade_ref(img[:60], rec)
    with pytest.raises(ValueError):
        D.degrade_ref(img.astype(np.float32), rec)


# ---------------------------------------------------------------------------------------------------------------- interface, CLI, dataset
def test_header_binding_and_refusals():
    """The C interface: femasr_hip_degrade.h is part of femasr_hip.h and declares what _lib binds; every refusal comes before any launch, so
    it is checked here, without a GPU."""
    import ctypes
    import re
    assert '#include "femasr_hip_degrade.h"' in open(os.path.join(ROOT, 'include', 'femasr_hip.h')).read()
    hdr = open(os.path.join(ROOT, 'include', 'femasr_hip_degrade.h')).read()
    assert set(re.findall(r'^int\s+(femasr_[a-z0-9_]+)\s*\(', hdr, re.M)) == set(_lib.DEGRADE_SIGNATURES)
    for name, (res, args) in _lib.DEGRADE_SIGNATURES.items():
        m = re.search(r'^int\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr, re.M | re.S)
        assert m and len(m.group(1).split(',')) == len(args), name
    from femasr_amd.csrc import build
    assert 'degrade.hip' in build.SOURCES and '../../include/femasr_hip_degrade.h' in build.HEADERS
    lib = _lib.load()
    assert lib.femasr_version() == _lib.ABI_VERSION
    buf = np.zeros(4096, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    odd = ctypes.c_void_p(buf.ctypes.data + 2)
    fac = (ctypes.c_double * 9)(*([0.1] * 9))
    nan = (ctypes.c_double * 9)(*([float('nan')] * 9))
    tabs = [np.zeros(8, np.int32) for _ in range(2)]        # index tables in host memory: one entry below 0, one at the source's size (8)
    tabs[0][5], tabs[1][7] = -1, 8
    low, high = (ctypes.c_void_p(t.ctypes.data) for t in tabs)
    calls = [('femasr_degrade_blur_f32', (None, p, 8, 8, p, 3, 1, p), {1: None, 2: 0, 3: -1, 4: None, 5: 4, 5.1: 27, 5.2: 1, 6: 3, 6.1: 0, 7: None, 7.1: odd, 1.1: odd}),
             ('femasr_degrade_resize_f32', (None, p, 8, 8, p, 4, 4, p, p, 2, p, p, 2, p, p),
              {1: None, 2: 0, 4: None, 5: 0, 6: -3, 7: None, 8: None, 9: 0, 10: None, 11: None, 12: 0, 12.1: 5000, 4.1: odd, 13: None, 14: None, 13.1: low, 13.2: high, 14.1: low, 14.2: high}),
             ('femasr_degrade_noise_f32', (None, p, p, 4, 0, 0, fac, 1), {1: None, 2: None, 3: 0, 5: 3, 5.1: -1, 6: None, 6.1: nan, 2.1: odd, 4: 1 << 61}),
             ('femasr_degrade_quantize_u8', (None, p, p, 4), {1: None, 2: None, 3: 0, 1.1: odd}),
             ('femasr_degrade_unit_f32', (None, p, 4, 4, 4, p), {1: None, 2: 0, 3: 0, 4: 3, 5: None, 5.1: odd}),
             ('femasr_jpeg_decode_u8', (None, p, p, p, 3, 444, 8, 8, p, p, p, 0), {1: None, 2: None, 3: None, 4: 2, 5: 422, 6: 0, 7: 65536, 8: None, 9: None, 10: None, 11: 2, 1.1: odd})]
    for name, base, bads in calls:
        fn = getattr(lib, name)
        for pos, val in bads.items():
            args = list(base)
            args[int(pos)] = val
            assert fn(*args) == -1 and name[7:].encode() in lib.femasr_last_error(), (name, pos)
    assert lib.femasr_jpeg_decode_u8(None, p, p, None, 1, 0, 8, 8, p, None, p, 0) == -1          # gray takes neither cb nor cr
    odd4 = ctypes.c_void_p(buf.ctypes.data + 2)
    assert lib.femasr_jpeg_decode_u8(None, p, p, p, 3, 444, 8, 8, p, p, odd4, 1) == -1          # a misaligned float output
    assert not buf.any()


def test_table_cache_drops_the_oldest_entry_only(monkeypatch):
    monkeypatch.setattr(D, '_CACHE', {})
    monkeypatch.setattr(D, 'CACHE_ENTRIES', 4)
    made = [D._cached(('k', i), 'cpu', lambda i=i: [np.full(3, i, np.float32)]) for i in range(6)]
    assert [k[0] for k in D._CACHE] == [('k', i) for i in range(2, 6)]                   # one out per one in, oldest first
    assert D._cached(('k', 5), 'cpu', lambda: [np.zeros(3, np.float32)])[0] is made[5][0]
    assert float(made[0][0][0]) == 0.0 and float(made[1][0][1]) == 1.0                   # a dropped tensor lives on with its holder
    keep = []
    monkeypatch.setattr(D, '_KEEP', [keep])
    got = D._cached(('k', 9), 'cpu', lambda: [np.ones(2, np.float32), np.ones(2, np.int32)])
    assert len(keep) == 2 and keep[0] is got[0] and keep[1] is got[1]


def test_cli_argument_checks(tmp_path):
    from femasr_amd import degrade_folder as F
    src = tmp_path / 'gt'
    src.mkdir()
    for argv in (['-i', str(src), '-o', str(tmp_path / 'o')], ['-i', str(src), '-o', str(tmp_path / 'o'), '-s', '3'],
                 ['-i', str(src), '-o', str(tmp_path / 'o'), '-s', '4', '--mode', 'nearest'],
                 ['-i', str(src), '-o', str(tmp_path / 'o'), '-s', '4', '--io-threads', '-1']):
        with pytest.raises(SystemExit):
            F.parse_args(argv)
    for argv, msg in ((['-i', str(tmp_path / 'none'), '-o', str(tmp_path / 'o'), '-s', '4'], 'not a directory'),
                      (['-i', str(src), '-o', str(src), '-s', '4'], 'must differ'),
                      (['-i', str(src), '-o', str(tmp_path / 'o'), '-s', '4', '--recipes', 'a.json', '--recipes-in', 'a.json'], 'not both'),
                      (['-i', str(src), '-o', str(tmp_path / 'o'), '-s', '4'], 'no images')):
        with pytest.raises(SystemExit) as e:
            F.main(argv)
        assert msg in str(e.value), (argv, e.value)
    # a replayed recipe carries its own scale and mode: arguments that contradict it are refused before anything runs
    Image.fromarray(np.zeros((16, 16, 3), np.uint8), 'RGB').save(str(src / 'a.png'))
    rj = tmp_path / 'r.json'
    rj.write_text(json.dumps({'a.png': D.sample_recipe(1, 'a.png', 16, 16, 2)}))
    for flags, msg in ((['-s', '4'], 'scale'), (['-s', '2', '--mode', 'bicubic'], 'mode')):
        with pytest.raises(SystemExit) as e:
            F.main(['-i', str(src), '-o', str(tmp_path / 'o'), '--recipes-in', str(rj)] + flags)
        assert msg in str(e.value) and 'a.png' in str(e.value), e.value
    rj.write_text(json.dumps({'b.png': D.sample_recipe(1, 'b.png', 16, 16, 2)}))
    with pytest.raises(SystemExit) as e:
        F.main(['-i', str(src), '-o', str(tmp_path / 'o'), '--recipes-in', str(rj), '-s', '2'])
    assert 'no recipe for a.png' in str(e.value)
    args = F.parse_args(['-i', str(src), '-o', 'o', '-s', '2'])
    assert (args.scale, args.mode, args.seed, args.io_threads, args.recipes, args.recipes_in) == (2, 'bsrgan', 123, 0, None, None)


def test_dataset_makes_lq_on_the_fly(tmp_path, monkeypatch):
    from femasr_amd import data
    rng = np.random.RandomState(1)
    gt = tmp_path / 'gt' / 'sub'
    gt.mkdir(parents=True)
    imgs = {}
    for name, shape in (('a.png', (41, 37, 3)), ('b.png', (32, 48, 3))):
        imgs[name] = rng.randint(0, 256, shape).astype(np.uint8)
        Image.fromarray(imgs[name], 'RGB').save(str(gt / name))
    calls = []

    def fake(img_u8, recipe, out=None):
        calls.append(recipe['name'])
        return torch.from_numpy(D.degrade_ref(img_u8.cpu().numpy(), recipe))
    monkeypatch.setattr(D, 'degrade_u8', fake)
    opt = {'type': 'PairedImageDataset', 'dataroot_gt': str(tmp_path / 'gt'), 'scale': 4, 'synth_lq': {'mode': 'bsrgan', 'seed': 7, 'device': 'cpu'}}
    ds = data.build_dataset(opt)
    assert len(ds) == 2
    for i, name in enumerate(('a.png', 'b.png')):
        item = ds[i]
        rel = os.path.join('sub', name)
        rec = D.sample_recipe(7, rel, imgs[name].shape[0], imgs[name].shape[1], 4)
        want = D.degrade_ref(imgs[name], rec)
        h, w = rec['crop']
        assert item['lq'].dtype == torch.float32 and tuple(item['lq'].shape) == (3, h // 4, w // 4) and tuple(item['gt'].shape) == (3, h, w)
        assert np.array_equal(item['lq'].numpy(), want.transpose(2, 0, 1).astype(np.float32) / 255.0)
        assert np.array_equal(item['gt'].numpy(), imgs[name][:h, :w].transpose(2, 0, 1).astype(np.float32) / 255.0)
        assert item['gt_path'].endswith(rel) and item['lq_path'] == item['gt_path']
        assert torch.equal(ds[i]['lq'], item['lq'])                                          # an epoch is reproducible
    assert calls == [os.path.join('sub', 'a.png')] * 2 + [os.path.join('sub', 'b.png')] * 2
    for bad in ({'mode': 'bsrgan'}, {'mode': 'x', 'seed': 1}):
        with pytest.raises((ValueError, KeyError)):
            data.build_dataset(dict(opt, synth_lq=bad))[0]
    with pytest.raises(ValueError):
        data.build_dataset({k: v for k, v in opt.items() if k != 'scale'})


if __name__ == '__main__':
    res, lines = measure_pillow()
    path = os.path.join(ROOT, 'profiles', 'degrade_report.txt')
    with open(path, 'w') as f:
        f.write('jpegio.decode_ref against Pillow decoding the bytes of jpegio.encode_ref (tests/test_degrade_host.py measure_pillow;\n'
                'differences in levels of 0..255; host only, no GPU involved)\n\n' + '\n'.join(lines) + '\n\n')
        for ss, (worst, mean) in res.items():
            f.write(f'{ss}: worst {worst}, mean {mean:.4f}\n')
    print(open(path).read())
    sys.exit(0)

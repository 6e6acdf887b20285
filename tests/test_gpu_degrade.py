"""-m gpu: synthesis of LQ inputs on the device (csrc/degrade.hip, femasr_amd/degrade.py, jpegio.decode_gpu).

Blur and resize are compared BIT FOR BIT with their float32 restatements (tests/degrade_ref.py, held to the float64 definitions in
test_degrade_host.py), quantisation and the JPEG decoder bit for bit with the definitions themselves (integers, one float32 product).
Noise alone has a tolerance, 1 float32 ulp in front of the clip:
  the definition and the kernel evaluate the same fp64 expression sqrt(-2 log u1) cos(2 pi u2) on the same u1, u2 (integers times 2^-53)
  and the same argument 2 pi u2 (one rounded product).  The device's double-precision log and cos are the ROCm device library's (OCML), which
  states at most 1 ulp for log and 2 ulp for cos outside huge arguments (ours are below 6.3) - the OpenCL double-precision limits are 3 and
  4 ulp -, numpy's libm is within 1 ulp; sqrt and the products are correctly rounded on both.  With e = 2^-53: log u1 is off by 1 e relative
  on either side, its square root by half of that plus e / 2, the cosine by 2 e, the product by e / 2 - the two normals differ by at most
  about 8 e relative, the sums x + A n by at most 8 e |A n| + e < 2^-48 for |A n| <= 3.  Two doubles that close round to the same float32 or
  to neighbours wherever a float32 ulp is at least 2^-48, that is for |x + A n| >= 2^-25: 1 ulp.  (Below 2^-25 the statement is about the
  absolute error 2^-48; the `mid` images of the test keep every value above 0.09, the clipped `full` images meet such a value with a
  probability of about 1e-8 a pixel.)"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import degrade_ref as R
import guard_arena as GA
import gpu_utils as G
from femasr_amd import _lib, degrade as D, jpegio
from test_gpu_jpeg_io import SHAPES, _content

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _img(h, w, seed=0, lo=0.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, (h, w, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- blur
def _blur_kernels():
    rng = np.random.RandomState(5)
    asym = rng.uniform(0, 1, (7, 7))
    asym[0, :] += 3.0
    asym[:, 1] += 2.0
    return {'box3': np.full((3, 3), 1 / 9.0, np.float32), 'asym7': (asym / asym.sum()).astype(np.float32),
            'iso25': D.fspecial_gaussian(25, 4.0).astype(np.float32), 'shifted25': D.shifted_gaussian(4, 1.8).astype(np.float32)}


def _blur_entry(img, kernel, stride):
    h, w = img.shape[:2]
    oh, ow = -(-h // stride), -(-w // stride)
    what = f'degrade_blur_f32 {h}x{w} k{kernel.shape[0]} s{stride}'

    def go():
        ops = G.Operands(what).inp('img', img).inp('k', kernel).out('out', oh * ow * 12).build()
        _lib.check(_lib.load().femasr_degrade_blur_f32(None, ops.p('img'), h, w, ops.p('k'), kernel.shape[0], stride, ops.p('out')))
        ops.check()
        return ops.get('out', torch.float32, (oh, ow, 3)).cpu().numpy()
    return GA.run_twice(go, what)


@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (31, 33), (32, 32), (65, 34)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_blur_equals_its_restatement(cuda_device, shape):
    img = _img(*shape, seed=shape[1])
    for name, k in _blur_kernels().items():
        for s in (1, 2, 4):
            got, want = _blur_entry(img, k, s), R.blur_f32(img, k, s)
            bad = np.argwhere(_bits(got) != _bits(want))
            assert got.shape == want.shape and bad.size == 0, f'{name} stride {s}: {len(bad)} values differ, first at {bad[0].tolist()}'


# ---------------------------------------------------------------------------------------------------------------- resize
def _resize_entry(img, th, tw, host=None):
    """host: the index tables the entry checks in host memory, where they differ from the device's (th[1], tw[1])."""
    h, w = img.shape[:2]
    (wh, ih), (ww, iw) = th, tw
    hh, hw = (np.ascontiguousarray(a, np.int32) for a in (host or (ih, iw)))
    oh, ow = wh.shape[0], ww.shape[0]
    what = f'degrade_resize_f32 {h}x{w} -> {oh}x{ow} taps {wh.shape[1]}/{ww.shape[1]}'

    def go():
        ops = G.Operands(what).inp('img', img).inp('wh', wh).inp('ih', ih).inp('ww', ww).inp('iw', iw).out('out', oh * ow * 12).build()
        _lib.check(_lib.load().femasr_degrade_resize_f32(None, ops.p('img'), h, w, ops.p('out'), oh, ow, ops.p('wh'), ops.p('ih'), wh.shape[1],
                                                         ops.p('ww'), ops.p('iw'), ww.shape[1], ctypes.c_void_p(hh.ctypes.data),
                                                         ctypes.c_void_p(hw.ctypes.data)))
        ops.check()
        return ops.get('out', torch.float32, (oh, ow, 3)).cpu().numpy()
    return GA.run_twice(go, what)


RESIZE_CASES = [('bilinear', 9, 14, 1, 1), ('bicubic', 9, 14, 1, 1), ('area', 9, 14, 1, 1),                       # to one pixel
                ('bilinear', 9, 14, 18, 28), ('bicubic', 9, 14, 18, 28), ('area', 9, 14, 18, 28), ('matlab', 9, 14, 18, 28),      # x2 up
                ('area', 79, 63, 10, 8), ('area', 40, 33, 7, 30),                                               # down by 7.9 (9 taps); a ratio per axis
                ('bicubic', 30, 12, 7, 31), ('bilinear', 12, 30, 31, 7),                                        # one axis down, the other up
                ('matlab', 24, 36, 12, 18), ('matlab', 64, 48, 16, 12),                                          # antialiased: 10 and 18 taps
                ('area', 6, 259, 6, 64), ('bicubic', 5, 259, 5, 64), ('bilinear', 4, 130, 3, 520)]              # more than one block's tile of columns


@pytest.mark.parametrize('case', RESIZE_CASES, ids=lambda c: f'{c[0]}_{c[1]}x{c[2]}_{c[3]}x{c[4]}')
def test_resize_equals_its_restatement(cuda_device, case):
    filt, h, w, oh, ow = case
    img = _img(h, w, seed=h + ow, lo=-0.2, hi=1.2)           # (values outside [0,1]: the clip of the epilogue has work)
    th, tw = D.op_tables({'op': 'resize', 'filter': filt, 'out_h': oh, 'out_w': ow}, h, w)
    got, want = _resize_entry(img, th, tw), R.resize_f32(img, th, tw)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert got.shape == want.shape == (oh, ow, 3) and bad.size == 0, f'{len(bad)} values differ, first at {bad[0].tolist()}'
    assert got.min() >= 0 and got.max() <= 1
    # the entry refuses host tables that point outside the image (test_refusals); a DEVICE table that differs from the checked host copy is
    # clamped by the kernel: the result of the clamped table, and no access outside the arena's regions
    wild = (th[0], (th[1].astype(np.int64) * 3 - 2).astype(np.int32))
    clamped = np.clip(wild[1], 0, h - 1)
    assert np.array_equal(_bits(_resize_entry(img, wild, tw, host=(clamped, tw[1]))), _bits(R.resize_f32(img, (wild[0], clamped), tw)))


# ---------------------------------------------------------------------------------------------------------------- noise
def _noise_entry(img, mode, factor, seed, offset=0):
    n = img.size // 3
    what = f'degrade_noise_f32 {n} pixels {mode}'
    fac = (ctypes.c_double * 9)(*np.asarray(factor, np.float64).reshape(-1).tolist())

    def go():
        ops = G.Operands(what).inp('img', img).out('out', n * 12).build()
        _lib.check(_lib.load().femasr_degrade_noise_f32(None, ops.p('img'), ops.p('out'), n, offset, D.NOISE_MODES.index(mode), fac, seed))
        ops.check()
        return ops.get('out', torch.float32, img.shape).cpu().numpy()
    return GA.run_twice(go, what)


def _factors():
    m = np.random.RandomState(4).uniform(-1, 1, (3, 3))
    return {'color': np.eye(3) * 0.03, 'gray': np.eye(3) * 0.02, 'correlated': D.factor_of_covariance((8 / 255.0) ** 2 * (m @ m.T))}


@pytest.mark.parametrize('shape', [(1, 1), (63, 65), (130, 70)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_noise_within_one_ulp_of_the_definition(cuda_device, shape):
    mid = _img(*shape, seed=1, lo=0.35, hi=0.65)             # |A n| <= 8.6 * 0.03 * sqrt(3): nothing is clipped, the comparison is in front of the clip
    full = _img(*shape, seed=2, lo=-0.1, hi=1.1)
    for mode, a in _factors().items():
        for img, clipped in ((mid, False), (full, True)):
            seed = 1000 + len(mode) + shape[0]
            got = _noise_entry(img, mode, a, seed)
            before = D.noise_values(img, mode, a.reshape(-1), seed).astype(np.float32)
            if not clipped:
                assert before.min() > 0 and before.max() < 1 and got.min() > 0 and got.max() < 1
            want = np.clip(before, 0, 1)
            worst = int(R.ulp_distance(got, want).max())
            print(f'noise {mode} {shape} clipped={clipped}: worst {worst} ulp, {int((R.ulp_distance(got, want) > 0).sum())} of {got.size} differ')
            assert worst <= 1, (mode, shape, clipped, worst)
            assert got.min() >= 0 and got.max() <= 1
            if mode == 'gray' and not clipped:
                d = got.astype(np.float64) - img
                assert np.abs(d[..., 0] - d[..., 1]).max() < 1e-7 and np.abs(d[..., 0] - d[..., 2]).max() < 1e-7
        # whole = two halves with offset pixel indices, bit for bit; in place = out of place
        whole = _noise_entry(mid, mode, a, 77)
        flat = mid.reshape(-1, 3)
        cut = flat.shape[0] // 3
        if cut:
            parts = [_noise_entry(np.ascontiguousarray(flat[:cut]), mode, a, 77), _noise_entry(np.ascontiguousarray(flat[cut:]), mode, a, 77, offset=cut)]
            assert np.array_equal(_bits(np.concatenate(parts).reshape(whole.shape)), _bits(whole)), mode
        t = torch.from_numpy(mid).to(cuda_device)
        out = D.noise_gpu(t, mode, a.reshape(-1), 77)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(whole)) and torch.equal(t.cpu(), torch.from_numpy(mid))
        same = D.noise_gpu(t, mode, a.reshape(-1), 77, out=t)
        assert same.data_ptr() == t.data_ptr() and torch.equal(t, out)


# ---------------------------------------------------------------------------------------------------------------- bytes
def test_quantize_and_unit_are_exact(cuda_device):
    x = np.concatenate([(np.arange(-51, 562) / 510.0), [np.nextafter(0.5 / 255, 0), np.nextafter(0.5 / 255, 1), -0.0, 2.0, -3.0]]).astype(np.float32)

    def go():
        ops = G.Operands('degrade_quantize_u8').inp('x', x).out('out', x.size).build()
        _lib.check(_lib.load().femasr_degrade_quantize_u8(None, ops.p('x'), ops.p('out'), x.size))
        ops.check()
        return ops.get('out', torch.uint8).cpu().numpy()
    assert np.array_equal(GA.run_twice(go, 'degrade_quantize_u8'), D.quantize_ref(x))
    u8 = np.random.RandomState(1).randint(0, 256, (9, 13, 3)).astype(np.uint8)
    u8[0, :, 0] = np.arange(13) * 21
    for h, w in ((9, 13), (8, 12), (1, 1)):                 # the whole image; a mod-crop through the row pitch

        def unit():
            ops = G.Operands(f'degrade_unit_f32 {h}x{w}').inp('u8', u8).out('out', h * w * 12).build()
            _lib.check(_lib.load().femasr_degrade_unit_f32(None, ops.p('u8'), h, w, 13, ops.p('out')))
            ops.check()
            return ops.get('out', torch.float32, (h, w, 3)).cpu().numpy()
        assert np.array_equal(_bits(GA.run_twice(unit, 'degrade_unit_f32')), _bits(D.unit_ref(u8[:h, :w])))
    t = torch.from_numpy(np.arange(256, dtype=np.uint8).reshape(-1, 1).repeat(3, 1).reshape(16, 16, 3).copy()).to(cuda_device)
    assert torch.equal(D.quantize_gpu(D.unit_gpu(t)), t)


# ---------------------------------------------------------------------------------------------------------------- JPEG decode
def _decode_entry(comps, quality, ss, h, w, f32):
    c = len(comps)
    tabs = jpegio.kernel_tables(quality)
    what = f'jpeg_decode_u8 {h}x{w}x{c} q{quality} {ss} {"f32" if f32 else "u8"}'

    def go():
        ops = G.Operands(what)
        for i, comp in enumerate(comps):
            ops.inp(f'c{i}', comp)
        ops.inp('qy', tabs[0])
        if c == 3:
            ops.inp('qc', tabs[1])
        ops.out('out', h * w * c * (4 if f32 else 1)).build()
        _lib.check(_lib.load().femasr_jpeg_decode_u8(None, ops.p('c0'), ops.p('c1'), ops.p('c2'), c, 0 if c == 1 else int(ss), h, w, ops.p('qy'), ops.p('qc'),
                                                     ops.p('out'), 1 if f32 else 0))
        ops.check()
        shape = (h, w) if c == 1 else (h, w, 3)
        return ops.get('out', torch.float32 if f32 else torch.uint8, shape).cpu().numpy()
    return GA.run_twice(go, what)


@pytest.mark.parametrize('hw', SHAPES, ids=lambda v: f'{v[0]}x{v[1]}')
def test_decode_equals_definition(cuda_device, hw):
    h, w = hw
    for ci, kind in enumerate(('noise', 'checker8', 'red')):
        for channels, subs in ((1, ('444',)), (3, ('444', '420'))):
            img = _content(kind, h, w, channels, 10 * ci + channels)
            for ss in subs:
                for q in (1, 50, 100):
                    comps = jpegio.coefficients_ref(img, q, ss)
                    want = jpegio.decode_ref(comps, q, ss, h, w)
                    got = _decode_entry(comps, q, ss, h, w, False)
                    bad = np.argwhere(got != want)
                    assert got.shape == want.shape and bad.size == 0, f'{kind} C={channels} {ss} q{q}: {len(bad)} pixels differ, first at {bad[0].tolist()}'
                    if q == 50:
                        assert np.array_equal(_bits(_decode_entry(comps, q, ss, h, w, True)), _bits(D.unit_ref(want))), (kind, channels, ss)
    # planes no encoder made: every int16 value, the clip of the dequantised coefficients at work
    rng = np.random.RandomState(h * 31 + w)
    for ss in jpegio.SUBSAMPLINGS:
        comps = [rng.randint(-32768, 32768, s + (64,)).astype(np.int16) for s in jpegio.geometry(h, w, 3, ss)[2]]
        assert np.array_equal(_decode_entry(comps, 30, ss, h, w, False), jpegio.decode_ref(comps, 30, ss, h, w)), ss


def test_decode_python_entry(cuda_device):
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    t = torch.from_numpy(img).to(cuda_device)
    for ss in ('444', '420'):
        planes = jpegio.coefficients_gpu(t, 75, ss)
        want = jpegio.decode_ref(jpegio.coefficients_ref(img, 75, ss), 75, ss, 37, 53)
        got = jpegio.decode_gpu(planes, 75, ss, 37, 53)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
        f = jpegio.decode_gpu(planes, 75, ss, 37, 53, float32=True)
        assert f.dtype == torch.float32 and np.array_equal(_bits(f.cpu().numpy()), _bits(D.unit_ref(want)))
    gray = jpegio.decode_gpu(jpegio.coefficients_gpu(t[..., 1].contiguous(), 50), 50, '420', 37, 53)
    assert np.array_equal(gray.cpu().numpy(), jpegio.decode_ref(jpegio.coefficients_ref(img[..., 1], 50), 50, '420', 37, 53))
    planes = jpegio.coefficients_gpu(t, 75, '420')
    for bad in ((planes[:2], 75, '420', 37, 53), (planes, 75, '444', 37, 53), (planes, 75, '420', 37, 70), (planes, 0, '420', 37, 53),
                ([p.cpu() for p in planes], 75, '420', 37, 53), ([p.int() for p in planes], 75, '420', 37, 53)):
        with pytest.raises(ValueError):
            jpegio.decode_gpu(*bad)
    # the JPEG operation: quantise -> coefficients -> decode
    x = _img(21, 34, seed=9)
    out = D.jpeg_gpu(torch.from_numpy(x).to(cuda_device), 60)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(D.jpeg_ref(x, 60)))
    assert np.array_equal(D.jpeg_gpu(torch.from_numpy(x).to(cuda_device), 60, final=True).cpu().numpy(), D.jpeg_ref(x, 60, final=True))


# ---------------------------------------------------------------------------------------------------------------- pipeline
PIPELINE = [((96, 80), 4, 5, 'bsrgan'), ((96, 80), 4, 18, 'bsrgan'), ((67, 45), 4, 24, 'bsrgan'), ((96, 80), 2, 4, 'bsrgan'), ((67, 45), 2, 11, 'bsrgan'),
            ((67, 45), 2, 0, 'bicubic')]


def _gt(size):
    h, w = size
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(h)
    base = np.stack([128 + 100 * np.sin(xx / 6.0) * np.cos(yy / 9.0), 128 + 90 * np.cos(xx / 4.0 + yy / 11.0), (5 * xx + 3 * yy) % 256], 2)
    return np.clip(base + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def _recipes():
    return [(size, D.sample_recipe(seed, 'fixed.png', size[0], size[1], sf, mode)) for size, sf, seed, mode in PIPELINE]


def test_pipeline_recipes_cover_every_operation_and_branch():
    seen = set()
    for _, r in _recipes():
        ops = r['ops']
        for o in ops:
            seen.add(o['op'])
            seen |= {f"blur_{o['kind']}_s{o['stride']}"} if o['op'] == 'blur' else set()
            seen |= {'f_' + o['filter']} if o['op'] == 'resize' else set()
            seen |= {'n_' + o['mode']} if o['op'] == 'noise' else set()
        seen.add('jpegs%d' % sum(o['op'] == 'jpeg' for o in ops))
        if r['mode'] == 'bsrgan' and r['sf'] == 4 and sum(o['op'] == 'resize' or o.get('kind') == 'shifted' for o in ops) == 3:
            seen.add('pre_matlab' if ops[1]['filter'] == 'matlab' else 'pre_cv2')
    assert seen >= {'unit', 'blur', 'resize', 'noise', 'jpeg', 'resample_u8', 'blur_iso_s1', 'blur_aniso_s1', 'blur_shifted_s2', 'blur_shifted_s4',
                    'f_bilinear', 'f_bicubic', 'f_area', 'f_matlab', 'n_color', 'n_gray', 'n_correlated', 'jpegs1', 'jpegs2', 'pre_cv2', 'pre_matlab'}, seen


@pytest.mark.parametrize('k', range(len(PIPELINE)), ids=lambda k: f'{PIPELINE[k][0][0]}x{PIPELINE[k][0][1]}_sf{PIPELINE[k][1]}_{PIPELINE[k][3]}{PIPELINE[k][2]}')
def test_pipeline(cuda_device, k):
    size, rec = _recipes()[k]
    gt = _gt(size)
    t = torch.from_numpy(gt).to(cuda_device)
    out = D.degrade_u8(t, rec)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (size[0] // rec['sf'], size[1] // rec['sf'], 3) and out.is_cuda
    # the chain of apply_op calls, bit for bit; each stage against its definition on that stage's GPU input
    x = t[:rec['crop'][0], :rec['crop'][1]]
    for op in rec['ops']:
        y = D.apply_op(x, op)
        x_host, y_host = x.cpu().numpy(), y.cpu().numpy()
        want = R.op_f32(np.ascontiguousarray(x_host), op)
        assert y_host.shape == want.shape and y_host.dtype == want.dtype, op
        if op['op'] == 'noise':
            assert int(R.ulp_distance(y_host, want).max()) <= 1, op
        elif want.dtype == np.float32:
            assert np.array_equal(_bits(y_host), _bits(want)), op
        else:
            assert np.array_equal(y_host, want), op
        x = y
    assert torch.equal(x, out)
    assert torch.equal(D.degrade_u8(t, rec), out)                                  # a second run
    assert torch.equal(D.degrade_u8(t, D.Recipe.from_json(rec.to_json()), out=torch.empty_like(out)), out)
    # a captured graph, replayed on another image (the tables are cached by now)
    other = torch.from_numpy(np.ascontiguousarray(gt[::-1, ::-1])).to(cuda_device)
    want_other = D.degrade_u8(other, rec)
    assert not torch.equal(want_other, out)
    static_in = t.clone()
    held = []                                                # the device tables the graph's launches read: they outlive the cache
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            static_out = D.degrade_u8(static_in, rec, keep=held)
    torch.cuda.current_stream(cuda_device).wait_stream(side)
    graph.replay()
    assert torch.equal(static_out, out)
    n_tables = sum(1 for o in rec['ops'] if o['op'] == 'blur') + 4 * sum(1 for o in rec['ops'] if o['op'] == 'resize')
    assert len(held) == n_tables and all(h.is_cuda for h in held)
    D._CACHE.clear()                                         # the cache forgets the tables; the graph's holder still has them
    static_in.copy_(other)
    graph.replay()
    assert torch.equal(static_out, want_other), 'replay on new input'
    with pytest.raises(ValueError):
        D.degrade_u8(t[:-1], rec)
    with pytest.raises(_lib.FemasrError):
        D.degrade_u8(t.cpu(), rec)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(cuda_device):
    lib = _lib.load()
    out = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=cuda_device)
    src = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda_device)
    p, o = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr())
    odd_o, odd_p = ctypes.c_void_p(out.data_ptr() + 2), ctypes.c_void_p(src.data_ptr() + 2)
    fac = (ctypes.c_double * 9)(*([0.1] * 9))
    s = torch.cuda.current_stream(cuda_device).cuda_stream
    tabs = [np.zeros(8, np.int32) for _ in range(3)]        # host index tables: in range; one entry below 0; one at the source's size (8)
    tabs[1][5], tabs[2][7] = -1, 8
    good, low, high = (ctypes.c_void_p(t.ctypes.data) for t in tabs)
    assert lib.femasr_degrade_resize_f32(s, p, 8, 8, ctypes.c_void_p(out.data_ptr() + 4096), 4, 4, p, p, 2, p, p, 2, good, good) == 0      # the base call is a valid one
    torch.cuda.synchronize(cuda_device)
    out.fill_(0x5A)
    calls = [(lib.femasr_degrade_blur_f32, (s, p, 8, 8, p, 3, 1, o), {1: None, 2: 0, 3: -1, 2.1: (1 << 24) + 1, 4: None, 5: 4, 5.1: 27, 5.2: 1, 6: 3, 6.1: 0, 7: None, 7.1: odd_o, 1.1: odd_p}),
             (lib.femasr_degrade_resize_f32, (s, p, 8, 8, o, 4, 4, p, p, 2, p, p, 2, good, good),
              {1: None, 2: 0, 4: None, 4.1: odd_o, 5: 0, 6: -3, 7: None, 8: None, 9: 0, 10: None, 11: None, 12: 0, 12.1: 5000, 13: None, 14: None, 13.1: low, 13.2: high,
               14.1: low, 14.2: high}),
             (lib.femasr_degrade_noise_f32, (s, p, o, 4, 0, 0, fac, 1), {1: None, 2: None, 2.1: odd_o, 3: 0, 4: 1 << 61, 5: 3, 5.1: -1, 6: None}),
             (lib.femasr_degrade_quantize_u8, (s, p, o, 4), {1: None, 1.1: odd_p, 2: None, 3: 0}),
             (lib.femasr_degrade_unit_f32, (s, p, 4, 4, 4, o), {1: None, 2: 0, 3: 0, 4: 3, 5: None, 5.1: odd_o}),
             (lib.femasr_jpeg_decode_u8, (s, p, p, p, 3, 444, 8, 8, p, p, o, 0), {1: None, 1.1: odd_p, 2: None, 3: None, 4: 2, 5: 422, 6: 0, 7: 65536, 8: None, 9: None, 10: None, 11: 2}),
             (lib.femasr_jpeg_decode_u8, (s, p, None, None, 1, 0, 8, 8, p, None, o, 1), {2: p, 10: odd_o})]
    for fn, base, bads in calls:
        for pos, val in bads.items():
            args = list(base)
            args[int(pos)] = val
            assert fn(*args) == -1 and lib.femasr_last_error(), (fn.__name__, pos)
    torch.cuda.synchronize(cuda_device)
    assert bool((out == 0x5A).all())
    # the Python surface refuses a table that indexes outside the source before anything is uploaded
    t = torch.zeros(8, 8, 3, device=cuda_device)
    w, idx = D.tap_table('bilinear', 8, 4)
    with pytest.raises(ValueError):
        D.resize_gpu(t, (w, idx + 7), (w, idx))
    for bad in (dict(kernel=np.ones((4, 4))), dict(kernel=np.ones((27, 27))), dict(kernel=np.ones((3, 3)), stride=3)):
        with pytest.raises(ValueError):
            D.blur_gpu(t, **bad)
    with pytest.raises(ValueError):
        D.noise_gpu(t, 'pink', np.eye(3).reshape(-1), 1)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_writes_degrade_u8_and_replays_recipes(cuda_device, tmp_path):
    from femasr_amd import degrade_folder as F
    src = tmp_path / 'gt'
    (src / 'sub').mkdir(parents=True)
    sizes = {'a.png': (41, 37), os.path.join('sub', 'b.png'): (32, 48), os.path.join('sub', 'c.png'): (24, 24), 'd.png': (50, 29)}
    for rel, size in sizes.items():
        Image.fromarray(_gt(size), 'RGB').save(str(src / rel))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = [sys.executable, '-m', 'femasr_amd.degrade_folder', '-i', str(src), '-s', '4']
    runs = {'first': ['-o', str(tmp_path / 'first'), '--seed', '31', '--recipes', str(tmp_path / 'r.json')],
            'again': ['-o', str(tmp_path / 'again'), '--seed', '999', '--recipes-in', str(tmp_path / 'r.json')]}
    for tag, flags in runs.items():
        p = subprocess.run(base + flags, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
    recipes = json.load(open(str(tmp_path / 'r.json')))
    assert sorted(recipes) == sorted(sizes)
    for rel, size in sizes.items():
        rec = D.sample_recipe(31, rel, size[0], size[1], 4)
        assert recipes[rel] == rec, rel
        first = (tmp_path / 'first' / rel).read_bytes()
        assert first == (tmp_path / 'again' / rel).read_bytes(), f'{rel}: --recipes-in did not reproduce the bytes'
        want = D.degrade_u8(torch.from_numpy(_gt(size)).to(cuda_device), rec).cpu().numpy()
        assert np.array_equal(np.array(Image.open(str(tmp_path / 'first' / rel))), want), rel
    # the fast PNG writer and the bicubic mode, in this process
    assert F.main(['-i', str(src), '-o', str(tmp_path / 'fast'), '-s', '4', '--seed', '31', '--io-threads', '2']) == 0
    assert F.main(['-i', str(src), '-o', str(tmp_path / 'bic'), '-s', '2', '--mode', 'bicubic']) == 0
    from femasr_amd import resample
    for rel, size in sizes.items():
        assert np.array_equal(np.array(Image.open(str(tmp_path / 'fast' / rel))), np.array(Image.open(str(tmp_path / 'first' / rel)))), rel
        gt = _gt(size)
        crop = np.ascontiguousarray(gt[:size[0] - size[0] % 2, :size[1] - size[1] % 2])
        assert np.array_equal(np.array(Image.open(str(tmp_path / 'bic' / rel))), resample.resample_ref(crop, size[0] // 2, size[1] // 2)), rel

"""Wavelet colour fix (femasr_amd/colorfix.py) without a GPU: the float64 definition's properties, the float32 restatement
(tests/colorfix_ref.py, the bit-for-bit checker of the GPU tests) against the definition within the derived bound, the uint8 rule, the
CLI flags, the YAML keys, the Python entry's refusals and the C ABI's refusals before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import colorfix_ref as R
from femasr_amd import _lib
from femasr_amd import colorfix as CF
from femasr_amd.models.femasr_model import imresize

FAKE = ctypes.c_void_p(1 << 20)             # a non-null, 256-byte aligned address nothing dereferences: every call below is refused first


# --------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('h,w,s', R.SHAPES)
def test_definition_reproduces_constants_and_is_linear(h, w, s):
    g = np.random.default_rng(h)
    for levels in (1, 5, 12):
        c = np.array([0.25, -3.0, 7.5]).reshape(1, 3, 1, 1)
        out = CF.wavelet_color_fix_f64(np.broadcast_to(c, (1, 3, s * h, s * w)), np.broadcast_to(c, (1, 3, h, w)), levels)
        assert np.abs(out - c).max() <= 8 * np.spacing(7.5)
        assert np.abs(CF.atrous_blur_f64(np.broadcast_to(c, (1, 3, s * h, s * w)), levels) - c).max() <= 8 * np.spacing(7.5)
    sr1, sr2 = g.random((2, 3, s * h, s * w)), g.random((2, 3, s * h, s * w))
    lq1, lq2 = g.random((2, 3, h, w)), g.random((2, 3, h, w))
    a, b = 0.75, -1.5
    lhs = CF.wavelet_color_fix_f64(a * sr1 + b * sr2, a * lq1 + b * lq2, 3)
    rhs = a * CF.wavelet_color_fix_f64(sr1, lq1, 3) + b * CF.wavelet_color_fix_f64(sr2, lq2, 3)
    assert np.abs(lhs - rhs).max() <= 1e-12


@pytest.mark.parametrize('h,w,s', R.SHAPES)
@pytest.mark.parametrize('levels', R.LEVELS)
def test_definition_is_high_of_content_plus_low_of_style(h, w, s, levels):
    sr, lq = (a.astype(np.float64) for a in R.case(h, w, s, 2)[:2])
    up = imresize(lq, s)
    out = CF.wavelet_color_fix_f64(sr, lq, levels)
    assert out.dtype == np.float64 and out.shape == sr.shape
    two_chains = sr - CF.atrous_blur_f64(sr, levels) + CF.atrous_blur_f64(up, levels)
    assert np.abs(out - two_chains).max() <= 1e-12
    assert np.array_equal(CF.wavelet_color_fix_f64(up, lq, levels), up)          # sr = up: d = 0, a fixed point
    assert np.abs(out - sr).max() > 1e-3                                          # (the cases are no fixed points)


def test_definition_takes_the_coarse_band_from_the_input():
    """A tone offset of the whole canvas disappears; a one-pixel checkerboard of detail survives away from the corners."""
    h, w, s, levels = 24, 40, 4, 3
    g = np.random.default_rng(3)
    lq = g.random((3, h, w))
    up = imresize(lq, s)
    yy, xx = np.mgrid[0:s * h, 0:s * w]
    k = 0.05 * (1 - 2 * ((yy + xx) & 1))
    out = CF.wavelet_color_fix_f64(up + 0.2 + k, lq, levels)
    far = np.ones((s * h, s * w), bool)
    n = (1 << levels) - 1
    for ys in (slice(0, n), slice(s * h - n, None)):
        for xs in (slice(0, n), slice(s * w - n, None)):
            far[ys, xs] = False
    assert np.abs(out - (up + k))[:, far].max() <= 1e-13
    assert np.abs(out - (up + k)).max() > 1e-4                                    # the border residue of the checkerboard near a corner


# --------------------------------------------------------------------------------------------------------------- the float32 restatement
@pytest.mark.parametrize('h,w,s', R.SHAPES)
@pytest.mark.parametrize('levels', R.LEVELS + [8])
def test_restatement_within_the_bound(h, w, s, levels):
    sr, lq = R.case(h, w, s, 2)[:2]
    got = R.color_fix_f32(sr, lq, levels)
    assert got.dtype == np.float32
    want = CF.wavelet_color_fix_f64(sr, lq, levels)
    b = R.bound(levels, sr, imresize(lq.astype(np.float64), s))
    ratio = float(np.abs(got.astype(np.float64) - want).max() / b)
    print(f'{h}x{w} x{s} levels {levels}: max |fp32 - definition| / ((8 L + 6) eps V) = {ratio:.3f}')
    assert ratio <= 1.0


@pytest.mark.parametrize('h,w,s', R.SHAPES)
@pytest.mark.parametrize('levels', R.LEVELS)
def test_restatement_u8_against_the_definition(h, w, s, levels):
    sr_u8, lq_u8 = R.case(h, w, s, 2)[2:]
    got = R.color_fix_u8(sr_u8, lq_u8, levels)
    assert got.dtype == np.uint8 and got.shape == sr_u8.shape
    srp, lqp = R.u8_planes(sr_u8), R.u8_planes(lq_u8)                             # the planes the definition is applied to: (float)byte / 255.0f
    want = CF.wavelet_color_fix_f64(srp, lqp, levels)
    b = R.bound(levels, srp, imresize(lqp.astype(np.float64), s)) * 255.0
    v = np.clip(want, 0, 1) * 255.0
    near = np.moveaxis(np.abs(v - np.floor(v) - 0.5) <= b, -3, -1)              # within the bound of k + 1/2: either neighbour is right
    share = float(near.mean())
    diff = got != R.quantise(want)
    print(f'{h}x{w} x{s} levels {levels}: near-tie share {share:.5f}, {int(diff.sum())} bytes differ, all of them near ties: {not (diff & ~near).any()}')
    assert share <= 0.01
    assert not (diff & ~near).any()
    assert (got != sr_u8).mean() > 0.5                                           # (the fix does something on these cases)


# --------------------------------------------------------------------------------------------------------------- callers
def test_cli_parser_carries_the_flags():
    from femasr_amd import inference
    ap = inference.build_parser()
    a = ap.parse_args([])
    assert a.color_fix is False and a.color_fix_levels == 5 and a.blend is False
    a = ap.parse_args(['-i', 'x.png', '--color-fix', '--color-fix-levels', '3', '--blend'])
    assert a.color_fix is True and a.color_fix_levels == 3 and a.blend is True


def test_yaml_keys_reach_the_network():
    from femasr_amd.models.femasr_model import FeMaSRModel
    seen = []

    class Net:
        color_fix_levels = 5

        def test(self, lq, **kw):
            seen.append(('test', kw, self.color_fix_levels))
            return lq

        def test_tile(self, lq, **kw):
            seen.append(('test_tile', kw, self.color_fix_levels))
            return lq

    small = torch.zeros(1, 3, 8, 8)
    big = torch.zeros(1, dtype=torch.uint8).expand(1, 3, 8000, 8001)             # (a stride-0 view: the size alone picks the branch)
    cases = [({}, {}, 5), ({'val': None}, {}, 5), ({'val': {'color_fix': False, 'color_fix_levels': 3}}, {}, 5),
             ({'val': {'color_fix': True}}, {'color_fix': True}, 5), ({'val': {'color_fix': True, 'color_fix_levels': 3}}, {'color_fix': True}, 3)]
    for opt, want, levels in cases:
        for lq, name in ((small, 'test'), (big, 'test_tile')):
            m = FeMaSRModel.__new__(FeMaSRModel)
            m.opt, m.net_g, m.lq = opt, Net(), lq
            m.test()
            assert seen.pop() == (name, want, levels)
    m = FeMaSRModel.__new__(FeMaSRModel)
    m.opt, m.net_g, m.lq = {'val': {'color_fix': True, 'tile_blend': True}}, Net(), big
    m.test()
    assert seen.pop() == ('test_tile', {'blend': True, 'color_fix': True}, 5)


def test_network_surface():
    import inspect
    from femasr_amd import distributed as fd
    from femasr_amd.archs import build_network
    from helpers import CONFIGS
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['x4']))
    assert net.color_fix_levels == 5
    for fn in (net.test, net.test_u8, net.test_tile, net.test_tile_u8, fd.test_tile_parallel):
        assert inspect.signature(fn).parameters['color_fix'].default is False
    # the tile driver's host path (the CPU-side tests of the partition logic) has no colour fix: GPU only, refused after the paste
    net.test = lambda t: torch.nn.functional.interpolate(t, scale_factor=4, mode='nearest')
    x = torch.rand(1, 3, 40, 40)
    assert net.test_tile(x, 32, 8).shape == (1, 3, 160, 160)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        net.test_tile(x, 32, 8, color_fix=True)


def test_python_entry_refusals():
    f = CF.wavelet_color_fix
    sr, lq = torch.zeros(1, 3, 16, 24), torch.zeros(1, 3, 4, 6)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        f(sr, lq)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        f(torch.zeros(16, 24, 3, dtype=torch.uint8), torch.zeros(4, 6, 3, dtype=torch.uint8))
    with pytest.raises(_lib.FemasrError):
        f(sr.to('meta'), lq.to('meta'))
    bad = [(sr, torch.zeros(1, 3, 4, 8)),                       # sH / H != sW / W
           (sr, torch.zeros(1, 3, 5, 6)),                       # no integer multiple
           (sr, torch.zeros(2, 3, 4, 6)),                       # batch differs
           (sr, torch.zeros(3, 4, 6)),                          # rank differs
           (sr, lq.double()), (sr.double(), lq.double()), (sr.half(), lq.half()),
           (sr, torch.zeros(1, 4, 6, 3, dtype=torch.uint8)),    # float32 with uint8
           (torch.zeros(1, 16, 24, 3, dtype=torch.uint8), torch.zeros(4, 6, 3, dtype=torch.uint8)),
           (torch.zeros(1, 16, 24, 4, dtype=torch.uint8), torch.zeros(1, 4, 6, 4, dtype=torch.uint8)),
           (torch.zeros(1, 3, 16, 24, dtype=torch.uint8), torch.zeros(1, 3, 4, 6, dtype=torch.uint8)),      # uint8 is HWC
           (torch.zeros(24), torch.zeros(6))]
    for a, b in bad:
        with pytest.raises(ValueError):
            f(a, b)
    for levels in (0, 13, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            f(sr, lq, levels)
        with pytest.raises(ValueError):
            CF.wavelet_color_fix_f64(sr.numpy(), lq.numpy(), levels)
    for out in (torch.zeros(1, 3, 16, 25), torch.zeros(1, 3, 16, 24, dtype=torch.float64), torch.zeros(1, 3, 24, 16).transpose(2, 3)):
        with pytest.raises(ValueError):
            f(sr, lq, out=out)
    with pytest.raises(TypeError):
        f(sr.numpy(), lq.numpy())
    with pytest.raises(ValueError):
        CF.wavelet_color_fix_f64(np.zeros((3, 16, 24)), np.zeros((3, 4, 8)))


# --------------------------------------------------------------------------------------------------------------- the C ABI
def _call(fn, units=3, H=6, W=10, sH=24, sW=40, s=4, levels=5, sr=FAKE, lq=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 40, wh=FAKE, ih=FAKE, ww=FAKE,
          iw=FAKE, taps=6):
    return fn(None, sr, lq, units, H, W, sH, sW, s, levels, wh, ih, taps, ww, iw, taps, out, ws, ws_bytes)


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 107 and lib.femasr_version() == 107
    for name in ('femasr_color_fix_workspace_bytes', 'femasr_color_fix', 'femasr_color_fix_u8'):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None


def test_abi_workspace_size():
    lib = _lib.load()
    n = ctypes.c_size_t(7)
    assert lib.femasr_color_fix_workspace_bytes(3, 6, 10, 24, 40, 4, ctypes.byref(n)) == 0
    a256 = lambda v: -(-v // 256) * 256
    assert n.value == 2 * a256(3 * 24 * 40 * 4) + a256(3 * 24 * 10 * 8)          # two fp32 buffers and the resize's fp64 intermediate
    n = ctypes.c_size_t(7)
    for args in ((0, 6, 10, 24, 40, 4), (3, 0, 10, 0, 40, 4), (3, 6, 10, 24, 40, 0), (3, 6, 10, 25, 40, 4), (3, 6, 10, 24, 44, 4),
                 (3, 6, 10, 12, 20, 4), (1, 1 << 14, 1 << 15, 1 << 15, 1 << 16, 2)):
        assert lib.femasr_color_fix_workspace_bytes(*args, ctypes.byref(n)) == -1 and n.value == 7
    assert lib.femasr_color_fix_workspace_bytes(3, 6, 10, 24, 40, 4, None) == -1


@pytest.mark.parametrize('name', ['femasr_color_fix', 'femasr_color_fix_u8'])
def test_abi_refuses_before_any_launch(name):
    """Every call below returns FEMASR_ERR_INVALID; none may reach a launch - the pointers are fakes and this process has no GPU context."""
    lib = _lib.load()
    fn = getattr(lib, name)
    for kw in (dict(sr=None), dict(lq=None), dict(out=None), dict(ws=None), dict(wh=None), dict(ih=None), dict(ww=None), dict(iw=None)):
        assert _call(fn, **kw) == -1, kw
        assert b'null' in lib.femasr_last_error()
    for kw in (dict(units=0), dict(units=-2), dict(H=0, sH=0), dict(W=0, sW=0), dict(H=-6, sH=-24), dict(s=0), dict(s=-4), dict(taps=0),
               dict(sH=25), dict(sW=41), dict(sH=12, sW=20), dict(s=2), dict(H=12, W=20),          # sH != s H or sW != s W
               dict(levels=0), dict(levels=13), dict(levels=-1),
               dict(H=1 << 14, W=1 << 15, sH=1 << 15, sW=1 << 16, s=2),                           # a plane of 2^31 elements
               dict(ws_bytes=0), dict(ws=ctypes.c_void_p((1 << 20) + 8))):
        assert _call(fn, **kw) == -1, kw
    need = ctypes.c_size_t()
    assert lib.femasr_color_fix_workspace_bytes(1, 6, 10, 24, 40, 4, ctypes.byref(need)) == 0      # the smallest group: one plane, also for uint8
    assert _call(fn, ws_bytes=need.value - 1) == -1
    assert b'workspace' in lib.femasr_last_error()

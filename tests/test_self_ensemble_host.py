"""x8 geometric self-ensemble (femasr_amd/ensemble.py) without a GPU: the definition (index formulas against flip / transpose
compositions, the torch functions against the numpy restatement tests/ensemble_ref.py), the uint8 rounding rule, the fp32 summation order
(with the control that a wrong order changes bits), the tile schedule of `_tiled` on host tensors with a stand-in forward, and the plumbing
(CLI flag, YAML key, keyword surface, header and binding, the C ABI's refusals before any launch)."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ensemble_ref as R
from femasr_amd import _lib, tiling
from femasr_amd import ensemble as E
from femasr_amd.archs import build_network
from femasr_amd.archs import femasr_arch as A
from helpers import CONFIGS

FAKE = ctypes.c_void_p(1 << 20)             # a non-null address nothing dereferences: every call below is refused first
NONSQUARE = [(5, 7), (1, 9), (9, 1), (12, 4)]


def _asym(shape, dtype):
    g = np.random.default_rng(sum(shape))
    return g.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8 else g.random(shape).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('h,w', NONSQUARE + [(6, 6)])
@pytest.mark.parametrize('dtype', [np.float32, np.uint8])
def test_variants_are_distinct_and_invertible(h, w, dtype):
    x = _asym((2, h, w, 3) if dtype == np.uint8 else (2, 3, h, w), dtype)
    r, c = R.axes(x)
    fw = [R.forward(x, k) for k in range(8)]
    for k in range(8):
        assert fw[k].shape[r] == (w if k & 4 else h) and fw[k].shape[c] == (h if k & 4 else w)
        assert np.array_equal(R.inverse(fw[k], k, (h, w)), x)                                     # inverse_k(forward_k(x)) == x
        # the index formulas are the flip / transpose compositions T^t(H^h(V^v(x)))
        y = np.flip(x, r) if k & 1 else x
        y = np.flip(y, c) if k & 2 else y
        y = np.swapaxes(y, r, c) if k & 4 else y
        assert np.array_equal(fw[k], y)
        z = np.swapaxes(fw[k], r, c) if k & 4 else fw[k]                                          # and the inverse V^v(H^h(T^t(y)))
        z = np.flip(z, c) if k & 2 else z
        z = np.flip(z, r) if k & 1 else z
        assert np.array_equal(z, x)
        # the torch functions of the package are the same maps
        t = torch.from_numpy(x)
        assert np.array_equal(E.forward_variant(t, k).numpy(), fw[k]) and E.forward_variant(t, k).is_contiguous()
        assert np.array_equal(E.inverse_variant(torch.from_numpy(fw[k]), k).numpy(), x)
    if min(h, w) > 1:
        for a in range(8):
            for b in range(a + 1, 8):
                assert fw[a].shape != fw[b].shape or not np.array_equal(fw[a], fw[b]), (a, b)      # eight different maps


@pytest.mark.parametrize('h,w', NONSQUARE + [(6, 6)])
def test_torch_definition_equals_the_restatement(h, w):
    x, xu = R.index_f32(2, 3, h, w), R.pattern_u8(2, h, w)
    for a in (x, xu):
        s, t = E.expand(torch.from_numpy(a))                                                      # host tensors: the torch definition
        rs, rt = R.expand(a)
        assert np.array_equal(s.numpy(), rs) and np.array_equal(t.numpy(), rt)
        assert (E.as_batch(s, t) is not None) == (h == w)
        if h == w:
            assert np.array_equal(E.as_batch(s, t).numpy(), np.concatenate([rs, rt]))
    ys, yt = R.results_f32(2, 3, h, w, 5)
    got = E.merge(torch.from_numpy(ys), torch.from_numpy(yt))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), R.merge(ys, yt).view(np.uint32))
    us, ut = R.results_u8(2, h, w, 6)
    out = torch.zeros(2, h, w, 3, dtype=torch.uint8)
    assert E.merge(torch.from_numpy(us), torch.from_numpy(ut), out=out) is out and np.array_equal(out.numpy(), R.merge(us, ut))
    # round trip: merge(expand(x)) == x (fp32: integer-valued below 2^20, the eight-term sum is exact; uint8: S = 8 x)
    assert np.array_equal(R.merge(*R.expand(x)), x) and np.array_equal(R.merge(*R.expand(xu)), xu)
    bs, bt = E.result_buffers(torch.from_numpy(x), 4)
    assert tuple(bs.shape) == (4, 2, 3, 4 * h, 4 * w) and tuple(bt.shape) == (4, 2, 3, 4 * w, 4 * h) and (E.as_batch(bs, bt) is not None) == (h == w)


def test_uint8_rounding_is_half_to_even():
    s = np.arange(0, 2041)
    assert np.array_equal(R.round_eighth(s), np.rint(s / 8.0).astype(np.int64))
    t = torch.arange(0, 2041, dtype=torch.int32)
    assert np.array_equal(((t + 3 + ((t >> 3) & 1)) >> 3).numpy(), np.rint(s / 8.0).astype(np.int32))
    # through merge: eight results whose bytes sum to every S at least once
    g = np.random.default_rng(0)
    us, ut = g.integers(0, 256, (4, 1, 40, 40, 3), dtype=np.uint8), g.integers(0, 256, (4, 1, 40, 40, 3), dtype=np.uint8)
    z = [R.inverse(us[k], k, (40, 40)) for k in range(4)] + [R.inverse(ut[k], 4 + k, (40, 40)) for k in range(4)]
    want = np.rint(sum(a.astype(np.float64) for a in z) / 8.0).astype(np.uint8)
    assert np.array_equal(R.merge(us, ut), want) and np.array_equal(E.merge(torch.from_numpy(us), torch.from_numpy(ut)).numpy(), want)


@pytest.mark.parametrize('h,w', [(31, 33), (64, 64)])
def test_fp32_merge_order(h, w):
    """The restatement is within 8 * 2^-24 * max|z| of the float64 mean (seven adds of partial sums <= 8 max|z|, each rounding <= 2^-24 of
    that, times 1/8 exactly: 7 * 2^-24 max|z|), and the SAME sum taken k descending differs in bits on these inputs: the bitwise GPU
    test can see a wrong order."""
    ys, yt = R.results_f32(2, 3, h, w, 11)
    got = R.merge(ys, yt)
    zmax = max(float(np.abs(ys).max()), float(np.abs(yt).max()))
    err = float(np.abs(got.astype(np.float64) - R.merge_f64(ys, yt)).max())
    print(f'{h}x{w}: max |fp32 - f64| = {err:.3g}, bound {8 * 2.0 ** -24 * zmax:.3g}')
    assert err <= 8 * 2.0 ** -24 * zmax
    down = R.merge(ys, yt, order=range(7, -1, -1))
    assert not np.array_equal(got.view(np.uint32), down.view(np.uint32))
    assert float(np.abs(down.astype(np.float64) - R.merge_f64(ys, yt)).max()) <= 8 * 2.0 ** -24 * zmax


# --------------------------------------------------------------------------------------------------------------- the tile schedule
def _fake_test(self, t):
    """Stand-in of FeMaSRNet.test (no `out=`): depends on every pixel of the crop, on its shape and on the POSITION inside it (the ramp is
    not symmetric under any flip or transpose), so a variant mapped back wrongly, a mis-paste or a mis-order is visible; per image, so
    independent of the batch."""
    self.calls.append(int(t.shape[0]))
    up = F.interpolate(t, scale_factor=4, mode='nearest')
    ramp = torch.arange(up.shape[2], dtype=torch.float32)[:, None] * 0.37 + torch.arange(up.shape[3], dtype=torch.float32)[None, :] * 0.011
    return up * 0.5 + up * ramp * 0.01 + t.amax(dim=(1, 2, 3), keepdim=True) + 0.001 * t.shape[2] + 0.01 * t.shape[3]


def _to_f32(u8):
    return u8.permute(0, 3, 1, 2).float() / 255.0


def _to_u8(y):
    return (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _fake_test_u8(self, t, bgr=False):
    return _to_u8(_fake_test(self, _to_f32(t)) * 0.25)


def _make_net(max_tile_batch):
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['x4']))
    net.calls = []
    net.test = _fake_test.__get__(net)
    net.test_u8 = _fake_test_u8.__get__(net)
    net.max_tile_batch = max_tile_batch
    return net


def _tile_ensemble(net, run, crop):
    """The ensemble of one crop from eight SEPARATE stand-in calls on the package's torch variants, merged by the numpy restatement."""
    ys = np.stack([run(E.forward_variant(crop, k)).numpy() for k in range(4)])
    yt = np.stack([run(E.forward_variant(crop, 4 + k)).numpy() for k in range(4)])
    return torch.from_numpy(R.merge(ys, yt))


@pytest.mark.parametrize('shape,ts,pad,mtb', [((1, 3, 40, 52), 16, 4, 16), ((2, 3, 33, 40), 16, 4, 3), ((1, 3, 32, 32), 16, 0, 5)])
def test_tiled_schedule_on_host_tensors(shape, ts, pad, mtb):
    torch.manual_seed(0)
    x = torch.rand(shape)
    xu8 = (x.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()
    b, _, h, w = shape
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    ref = _make_net(mtb)
    want = R.paste(lambda t: _tile_ensemble(ref, ref.test, x[:, :, t.y0p:t.y1p, t.x0p:t.x1p]), tiles, 4, torch.zeros(b, 3, 4 * h, 4 * w), False)
    want8 = R.paste(lambda t: _tile_ensemble(ref, ref.test_u8, xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :]), tiles, 4,
                    torch.zeros(b, 4 * h, 4 * w, 3, dtype=torch.uint8), True)
    net = _make_net(mtb)
    y = net.test_tile(x, ts, pad, self_ensemble=True)
    assert torch.equal(y, want)                                                                   # per-tile ensemble + reference paste
    assert net.calls and max(net.calls) <= max(mtb, b), net.calls                                 # no forward call exceeds max_tile_batch images
    assert sum(net.calls) == 8 * b * len(tiles)
    if mtb >= 8 * b:
        assert max(net.calls) > b                                                                 # (and variants do share calls when there is room)
    plain = net.test_tile(x, ts, pad)
    assert not torch.equal(y, plain)
    net.calls.clear()
    y8 = net.test_tile_u8(xu8, ts, pad, self_ensemble=True)
    assert y8.dtype == torch.uint8 and torch.equal(y8, want8) and max(net.calls) <= max(mtb, b)
    assert torch.equal(net.test_tile_u8(xu8[0], ts, pad, self_ensemble=True), want8[0])           # an image without batch axis (batch 2: its first)

    # two ranks through a list-returning gather stand-in: the other rank's share computed here, tile by tile
    def fake_gather(fmt, run, crop, empty, results, classes, batch, channel, scale):
        other = {}
        for hw, tl in tiling.partition(classes, 1, 2).items():
            other[hw] = torch.cat([net._ensemble(fmt, run, crop(t)) for t in tl], 0) if tl else empty(hw, channel, scale)
        return [results, other]
    g32 = functools.partial(fake_gather, A._FP32, net.test, lambda t: x[:, :, t.y0p:t.y1p, t.x0p:t.x1p].contiguous(),
                            lambda hw, c, s: x.new_zeros((0, c, hw[0] * s, hw[1] * s)))
    gu8 = functools.partial(fake_gather, A._U8, net.test_u8, lambda t: xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :].contiguous(),
                            lambda hw, c, s: xu8.new_zeros((0, hw[0] * s, hw[1] * s, c)))
    assert torch.equal(net.test_tile(x, ts, pad, rank=0, world_size=2, gather=g32, self_ensemble=True), y)
    assert torch.equal(net.test_tile_u8(xu8, ts, pad, rank=0, world_size=2, gather=gu8, self_ensemble=True), y8)
    assert net.test_tile(x, ts, pad, rank=0, world_size=2, gather=g32, paste=False, self_ensemble=True) is None
    yb = net.test_tile(x, ts, pad, blend=True, self_ensemble=True) if 2 * pad <= ts else None     # blend on top: the same tiles, blended
    assert yb is None or (yb.shape == y.shape and (pad == 0 or not torch.equal(yb, y)))


def test_helper_split_does_not_change_the_result():
    """The ensemble helper on host tensors: one class of eight for a square batch, two classes otherwise; any max_tile_batch, `out=`."""
    torch.manual_seed(1)
    for shape in ((1, 3, 8, 8), (2, 3, 6, 10)):
        x = torch.rand(shape)
        want = _tile_ensemble(_make_net(1), _make_net(1).test, x)
        for mtb, calls in ((1, [shape[0]] * 8), (16, [8] if shape[2] == shape[3] else [4 * shape[0]] * 2), (5, None)):
            net = _make_net(mtb)
            out = torch.empty(shape[0], 3, 4 * shape[2], 4 * shape[3])
            assert net._ensemble(A._FP32, net.test, x, out) is out and torch.equal(out, want)
            assert calls is None or net.calls == calls, (mtb, net.calls)
            assert max(net.calls) <= max(mtb, shape[0])


# --------------------------------------------------------------------------------------------------------------- plumbing
def test_cli_parser_has_the_flag():
    from femasr_amd import inference
    ap = inference.build_parser()
    assert ap.parse_args([]).self_ensemble is False
    a = ap.parse_args(['-i', 'x.png', '--self-ensemble', '--color-fix'])
    assert a.self_ensemble is True and a.color_fix is True


def test_yaml_key_reaches_the_call():
    from femasr_amd.models.femasr_model import FeMaSRModel
    seen = []

    class Net:
        color_fix_levels = 5

        def test(self, lq, **kw):
            seen.append(('test', kw))
            return lq

        def test_tile(self, lq, **kw):
            seen.append(('test_tile', kw))
            return lq

    small = torch.zeros(1, 3, 8, 8)
    big = torch.zeros(1, dtype=torch.uint8).expand(1, 3, 8000, 8001)             # (a stride-0 view: the size alone picks the branch)
    cases = [({}, {}), ({'val': None}, {}), ({'val': {'self_ensemble': False}}, {}), ({'val': {'self_ensemble': True}}, {'self_ensemble': True}),
             ({'val': {'self_ensemble': True, 'color_fix': True}}, {'self_ensemble': True, 'color_fix': True})]
    for opt, want in cases:
        for lq, name in ((small, 'test'), (big, 'test_tile')):
            m = FeMaSRModel.__new__(FeMaSRModel)
            m.opt, m.net_g, m.lq = opt, Net(), lq
            m.test()
            assert seen.pop() == (name, want)
    m = FeMaSRModel.__new__(FeMaSRModel)
    m.opt, m.net_g, m.lq = {'val': {'self_ensemble': True, 'tile_blend': True}}, Net(), big
    m.test()
    assert seen.pop() == ('test_tile', {'blend': True, 'self_ensemble': True})


def test_keyword_surface():
    from femasr_amd import distributed as fd
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['x4']))
    for fn in (net.test, net.test_u8, net.test_tile, net.test_tile_u8, fd.test_tile_parallel):
        assert inspect.signature(fn).parameters['self_ensemble'].default is False
    for fn in (net.test_with_indices, net.forward, net.decode_indices, net.encode_and_decode):   # eight index maps have no mean
        assert 'self_ensemble' not in inspect.signature(fn).parameters
    seen = []
    net.test_tile = lambda x, ts, pad, **kw: seen.append(kw) or x
    fd.test_tile_parallel(net, torch.zeros(1, 3, 8, 8), 16, 4, self_ensemble=True)
    fd.test_tile_parallel(net, torch.zeros(1, 3, 8, 8), 16, 4)
    assert seen == [{'blend': False, 'self_ensemble': True}, {'blend': False}]


SYMBOLS = ('femasr_dihedral_expand', 'femasr_dihedral_expand_u8', 'femasr_dihedral_merge', 'femasr_dihedral_merge_u8')


def test_header_and_binding_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'femasr_hip.h')) as f:
        decl = dict(re.findall(r'^int (femasr_dihedral_\w+)\(([^)]*)\);', f.read(), re.M))
    assert sorted(decl) == sorted(SYMBOLS)
    lib = _lib.load()
    assert _lib.ABI_VERSION == 107 and lib.femasr_version() == 107                              # additive: the number stays
    for name in SYMBOLS:
        res, args = _lib.SIGNATURES[name]
        params = [p.strip() for p in decl[name].split(',')]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == p.startswith('int '), (name, p)
        assert getattr(lib, name).argtypes == args


def _expand(fn, u8, B=1, C=3, H=8, W=8, x=FAKE, s=FAKE, t=FAKE):
    return fn(None, x, B, H, W, s, t) if u8 else fn(None, x, B, C, H, W, s, t)


def _merge(fn, u8, B=1, C=3, H=8, W=8, s=FAKE, t=FAKE, out=FAKE):
    return fn(None, s, t, B, H, W, out) if u8 else fn(None, s, t, B, C, H, W, out)


@pytest.mark.parametrize('u8', [False, True])
def test_abi_refuses_before_any_launch(u8):
    """Every call below returns FEMASR_ERR_INVALID; none may reach a launch - the pointers are fakes and this process has no GPU context."""
    lib = _lib.load()
    ex = lib.femasr_dihedral_expand_u8 if u8 else lib.femasr_dihedral_expand
    mg = lib.femasr_dihedral_merge_u8 if u8 else lib.femasr_dihedral_merge
    for kw in (dict(x=None), dict(s=None), dict(t=None)):
        assert _expand(ex, u8, **kw) == -1 and b'null' in lib.femasr_last_error()
    for kw in (dict(s=None), dict(t=None), dict(out=None)):
        assert _merge(mg, u8, **kw) == -1 and b'null' in lib.femasr_last_error()
    shapes = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-8), dict(H=1 << 16, W=1 << 15), dict(H=(1 << 31) - 1, W=2),
              dict(H=1 << 15, W=1 << 15, B=1 << 14)]                                              # ..., a plane of 2^31 elements or more, too many tiles
    if not u8:
        shapes += [dict(C=0), dict(C=-3)]
    for kw in shapes:
        assert _expand(ex, u8, **kw) == -1, kw
        assert _merge(mg, u8, **kw) == -1, kw
    assert _expand(ex, u8, H=1 << 16, W=1 << 15) == -1 and b'2^31' in lib.femasr_last_error()


def test_python_entry_refusals():
    x = torch.zeros(1, 3, 4, 6)
    for bad in (torch.zeros(3, 4, 6), torch.zeros(1, 3, 4, 6, dtype=torch.float64), torch.zeros(1, 4, 6, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            E.expand(bad)
    with pytest.raises(TypeError):
        E.expand(x.numpy())
    s, t = E.expand(x)
    for out in (torch.zeros(1, 3, 6, 4), torch.zeros(1, 3, 4, 6, dtype=torch.float64), torch.zeros(1, 3, 6, 4).transpose(2, 3)):
        with pytest.raises(ValueError):
            E.merge(s, t, out=out)
    with pytest.raises(ValueError):
        E.merge(s, s)                                                                             # transposed results of the wrong shape
    with pytest.raises(ValueError):
        E.merge(s[:3], t[:3])
    for k in (-1, 8, 1.0, True):
        with pytest.raises(ValueError):
            E.forward_variant(x, k)

"""-m gpu: the wavelet colour fix (femasr_amd.colorfix.wavelet_color_fix -> femasr_color_fix / femasr_color_fix_u8).

The checker is the float32 restatement of tests/colorfix_ref.py: the kernels must reproduce it BIT FOR BIT (tests/test_color_fix_host.py
holds the restatement itself within the derived bound (8 L + 6) 2^-24 V of the float64 definition).  The shapes are the smallest that can
go wrong: 20x28 is smaller than twice the largest radius (both clamps act on one tap set), 66x38 is odd and no multiple of a block,
96x160 spans several blocks.  The properties (fixed point, tone, detail, tiles) are built so that their inputs are EXACT in float32 where
the claim is an exact one; the integration cases compare every caller's `color_fix=True` with `wavelet_color_fix` applied to the same
call without the option, bit for bit."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import colorfix_ref as R
from femasr_amd import colorfix as CF
from femasr_amd import resize, synth, tiling
from femasr_amd.archs import build_network
from helpers import CONFIGS, synth_weights

pytestmark = pytest.mark.gpu
EPS = R.EPS


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()              # (a copy: the shared cases are read-only)


def _tone_inputs(h, w, s, seed=0):
    """lq in [0.6, 0.9]: up = imresize(lq, s) then lies in [0.5, 1) (bicubic overshoot < 0.05), one binade of float32, so up + c with
    c in {-1/4, -1/8, -1/16} and up +- 2^-6 are exact float32 sums."""
    g = torch.Generator().manual_seed(seed)
    lq = (0.6 + 0.3 * torch.rand((2, 3, h, w), generator=g)).cuda()
    up = resize.imresize(lq, s)
    assert float(up.min()) >= 0.52 and float(up.max()) <= 0.98
    return lq, up


# --------------------------------------------------------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize('h,w,s', R.SHAPES)
@pytest.mark.parametrize('batch', [1, 2])
@pytest.mark.parametrize('levels', R.LEVELS)
def test_equals_the_restatement_bitwise(cuda_device, h, w, s, batch, levels):
    sr, lq, sr_u8, lq_u8 = R.case(h, w, s, batch)
    got = CF.wavelet_color_fix(_dev(sr), _dev(lq), levels)
    want = R.color_fix_f32(sr, lq, levels)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    got8 = CF.wavelet_color_fix(_dev(sr_u8), _dev(lq_u8), levels)
    want8 = R.color_fix_u8(sr_u8, lq_u8, levels)
    assert got8.dtype == torch.uint8 and tuple(got8.shape) == want8.shape
    assert np.array_equal(got8.cpu().numpy(), want8)
    assert not np.array_equal(want8, sr_u8) and not np.array_equal(want, sr)


def test_forms_groups_and_in_place(cuda_device, monkeypatch):
    """Unbatched uint8, other leading axes, out=, in place over sr, and planes worked through in groups of one (a workspace cap of one
    byte): all the same bits."""
    h, w, s, levels = 33, 19, 2, 3
    sr, lq, sr_u8, lq_u8 = R.case(h, w, s, 2)
    want, want8 = _dev(R.color_fix_f32(sr, lq, levels)), _dev(R.color_fix_u8(sr_u8, lq_u8, levels))
    a, b, a8, b8 = _dev(sr), _dev(lq), _dev(sr_u8), _dev(lq_u8)
    assert torch.equal(CF.wavelet_color_fix(a8[1], b8[1], levels), want8[1])                       # (sH,sW,3) with (H,W,3)
    assert torch.equal(CF.wavelet_color_fix(a[0, 1], b[0, 1], levels), want[0, 1])                 # one plane
    assert torch.equal(CF.wavelet_color_fix(a.view(6, 66, 38), b.view(6, 33, 19), levels), want.view(6, 66, 38))
    monkeypatch.setattr(CF, 'WORKSPACE_CAP', 1)
    assert torch.equal(CF.wavelet_color_fix(a, b, levels), want) and torch.equal(CF.wavelet_color_fix(a8, b8, levels), want8)
    monkeypatch.undo()
    out = torch.full_like(a, 7.0)
    assert CF.wavelet_color_fix(a, b, levels, out=out) is out and torch.equal(out, want)
    a2, a82 = a.clone(), a8.clone()
    assert CF.wavelet_color_fix(a2, b, levels, out=a2) is a2 and torch.equal(a2, want)            # in place
    assert CF.wavelet_color_fix(a82, b8, levels, out=a82) is a82 and torch.equal(a82, want8)
    assert torch.equal(a, _dev(sr)) and torch.equal(b8, _dev(lq_u8))                               # inputs untouched otherwise
    st = torch.cuda.Stream(device=cuda_device)                                                     # a side stream, and a second run
    st.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(st):
        y = CF.wavelet_color_fix(a, b, levels)
    st.synchronize()
    assert torch.equal(y, want) and torch.equal(CF.wavelet_color_fix(a, b, levels), want)


# --------------------------------------------------------------------------------------------------------------- 2. fixed point
@pytest.mark.parametrize('h,w,s', R.SHAPES)
@pytest.mark.parametrize('levels', R.LEVELS)
def test_upsampled_input_is_a_fixed_point(cuda_device, h, w, s, levels):
    lq = _dev(R.case(h, w, s, 2)[1])
    sr = resize.imresize(lq, s)
    assert torch.equal(CF.wavelet_color_fix(sr, lq, levels), sr)                                   # d = 0 everywhere


# --------------------------------------------------------------------------------------------------------------- 3. tone
@pytest.mark.parametrize('h,w,s', R.SHAPES)
@pytest.mark.parametrize('levels', R.LEVELS)
def test_tone_offset_is_removed(cuda_device, h, w, s, levels):
    """sr = up + c, one constant per channel: the blur reproduces constants, so the output is `up` within the bound."""
    lq, up = _tone_inputs(h, w, s)
    c = torch.tensor([-0.25, -0.125, -0.0625], device=cuda_device).view(1, 3, 1, 1)
    sr = up + c
    assert torch.equal(sr.double(), up.double() + c.double())                                      # the construction is exact
    out = CF.wavelet_color_fix(sr, lq, levels)
    b = R.bound(levels, sr.cpu().numpy(), up.cpu().numpy())
    err = float((out.double() - up.double()).abs().max())
    print(f'max |out - up| = {err:.3g}, bound {b:.3g}')
    assert err <= b


# --------------------------------------------------------------------------------------------------------------- 4. detail
@pytest.mark.parametrize('h,w,s,levels', [(5, 7, 4, 1), (33, 19, 2, 1), (24, 40, 4, 1), (33, 19, 2, 3), (24, 40, 4, 3), (24, 40, 4, 5)])
def test_checkerboard_detail_passes(cuda_device, h, w, s, levels):
    """A +-a one-pixel checkerboard added to sr comes out unchanged: the output moves by exactly that checkerboard, within 2 eps V.
    levels = 1: at every pixel that is not on the plane's border.  The first level's horizontal pass cancels the checkerboard except in
    the first and last column (the clamp doubles a tap there), its vertical pass cancels that except in the four corner pixels; every
    LATER level (radius 2, 4, ..) spreads those four corner values up to 2^levels - 2 pixels inward, so for levels > 1 the claim holds -
    and is asserted - outside the four corner squares of side 2^levels - 1 (derived from the definition; it is the definition's
    behaviour, tests/test_color_fix_host.py shows it in float64)."""
    lq, up = _tone_inputs(h, w, s, seed=levels)
    a = 2.0 ** -6
    c = torch.tensor([-0.25, -0.125, -0.0625], device=cuda_device).view(1, 3, 1, 1)
    yy, xx = torch.meshgrid(torch.arange(s * h, device=cuda_device), torch.arange(s * w, device=cuda_device), indexing='ij')
    k = a * (1 - 2 * ((yy + xx) & 1)).float()
    sr0 = up + c
    sr1 = sr0 + k
    assert torch.equal(sr1.double(), up.double() + c.double() + k.double())                        # exact in float32
    out0, out1 = CF.wavelet_color_fix(sr0, lq, levels), CF.wavelet_color_fix(sr1, lq, levels)
    keep = torch.ones((s * h, s * w), dtype=torch.bool, device=cuda_device)
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    if levels > 1:
        n = (1 << levels) - 1
        for ys in (slice(0, n), slice(s * h - n, None)):
            for xs in (slice(0, n), slice(s * w - n, None)):
                keep[ys, xs] = False
    assert int(keep.sum()) > 0.5 * keep.numel()
    v = max(float(sr1.abs().max()), float(up.abs().max()))
    dev_ = ((out1.double() - out0.double()) - k.double()).abs()[:, :, keep]
    print(f'max |(out1 - out0) - checkerboard| = {float(dev_.max()):.3g}, allowed {2 * EPS * v:.3g}')
    assert float(dev_.max()) <= 2 * EPS * v
    assert float(((out1.double() - out0.double()) - k.double()).abs().max()) > a / 256           # (the corner pixels do differ: a/4 after the first level, times 3/4 per later pass)


# --------------------------------------------------------------------------------------------------------------- 5. tiles
def _const(t):                          # tests/test_gpu_tile_blend.py's stand-in: one constant per tile and image
    return t.amax(dim=(1, 2, 3), keepdim=True).expand(t.shape[0], t.shape[1], t.shape[2] * 4, t.shape[3] * 4)


def _standin_net(test=None, test_u8=None):
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['x4']))
    net.test = test or _fake
    net.test_u8 = test_u8 or _fake_u8
    net.max_tile_batch = 3
    return net


def test_blended_tile_offsets_are_flattened(cuda_device):
    """f: the blend=True canvas of one constant per tile on the regular 96x128, 32/8, x4 geometry (margins L = 32 on every inner side): f
    moves by at most range(f) / (2 L) per pixel and axis.  With sr = up + f and levels = 3 the output is up + f - B(f), and B is a convex
    combination over offsets <= 7 pixels per axis, so |out - up| <= 7 range(f) (1 / (2 L) + 1 / (2 L)) + bound.  (The float32 rounding of
    the sum up + f, <= 2^-24 V, changes f by that much per pixel; the slope term counts every tap at the full offset 7 and full slope on
    both axes at once and dwarfs it.)  The field itself is as large as range(f) / 2: the claim is not vacuous."""
    h, w, ts, pad, L, levels = 96, 128, 32, 8, 32, 3
    g = torch.Generator().manual_seed(0)
    amp = torch.tensor([[0.9, 0.3, 0.7, 0.2], [0.4, 1.0, 0.1, 0.8], [0.6, 0.25, 0.95, 0.5]])
    inner = ((torch.arange(h) % ts >= pad) & (torch.arange(h) % ts < ts - pad))[:, None] & ((torch.arange(w) % ts >= pad) & (torch.arange(w) % ts < ts - pad))[None, :]
    x = (torch.rand((1, 3, h, w), generator=g) * amp.repeat_interleave(ts, 0).repeat_interleave(ts, 1) * inner).cuda()
    f = _standin_net(_const).test_tile(x, ts, pad, blend=True)
    rng = float(f.max() - f.min())
    assert rng > 0.5
    lq = torch.rand((1, 3, h, w), generator=g).cuda()
    up = resize.imresize(lq, 4)
    sr = up + f
    assert float((sr - up).abs().max()) >= rng / 2
    out = CF.wavelet_color_fix(sr, lq, levels)
    allow = 7 * rng * (1 / (2 * L) + 1 / (2 * L)) + R.bound(levels, sr.cpu().numpy(), up.cpu().numpy())
    err = float((out.double() - up.double()).abs().max())
    print(f'range(f) {rng:.3f}: max |out - up| = {err:.4f}, allowed {allow:.4f}; before the fix {float((sr - up).abs().max()):.4f}')
    assert err <= allow


# --------------------------------------------------------------------------------------------------------------- 6. integration
def _fake(t):                           # tests/test_distributed_cpu.py's stand-in: depends on every pixel of the crop and on its shape
    return F.interpolate(t, scale_factor=4, mode='nearest') * 0.5 + t.amax(dim=(1, 2, 3), keepdim=True) + 0.001 * t.shape[2] + 0.01 * t.shape[3]


def _fake_u8(t, bgr=False):             # (n, h, w, 3) uint8 -> (n, 4h, 4w, 3) uint8
    y = _fake(t.permute(0, 3, 1, 2).float() / 255.0) * 0.25
    return (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _images(batch, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((batch, 3, h, w), generator=g).cuda(), torch.randint(0, 256, (batch, h, w, 3), generator=g, dtype=torch.uint8).cuda()


@pytest.mark.parametrize('blend', [False, True])
def test_tiled_standin_equals_fix_of_the_plain_call(cuda_device, blend):
    """test_tile / test_tile_u8 at 70x100, 32/8 (ragged last tiles, 9 shape classes), batch 2: color_fix=True is the fix of the canvas the
    same call returns without it, against the whole input; batch 2 is the two single calls; a second run and a side stream repeat the
    bits; two ranks through the in-process gather stand-in give the single-rank canvas."""
    net = _standin_net()
    net.color_fix_levels = 3
    x, xu8 = _images(2, 70, 100, seed=5)
    want = CF.wavelet_color_fix(net.test_tile(x, 32, 8, blend=blend), x, 3)
    want8 = CF.wavelet_color_fix(net.test_tile_u8(xu8, 32, 8, blend=blend), xu8, 3)
    y, y8 = net.test_tile(x, 32, 8, blend=blend, color_fix=True), net.test_tile_u8(xu8, 32, 8, blend=blend, color_fix=True)
    assert torch.equal(y, want) and torch.equal(y8, want8)
    assert not torch.equal(y, net.test_tile(x, 32, 8, blend=blend)) and not torch.equal(y8, net.test_tile_u8(xu8, 32, 8, blend=blend))
    net.color_fix_levels = 5                                                                       # the attribute is what sets the levels
    assert torch.equal(net.test_tile(x, 32, 8, blend=blend, color_fix=True), CF.wavelet_color_fix(net.test_tile(x, 32, 8, blend=blend), x, 5))
    net.color_fix_levels = 3
    for i in range(2):                                                                             # batch 2 == the two single calls
        assert torch.equal(net.test_tile(x[i:i + 1], 32, 8, blend=blend, color_fix=True)[0], y[i])
        assert torch.equal(net.test_tile_u8(xu8[i], 32, 8, blend=blend, color_fix=True), y8[i])
    assert torch.equal(net.test_tile(x, 32, 8, blend=blend, color_fix=True), y)                    # a second run
    st = torch.cuda.Stream(device=cuda_device)
    st.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(st):
        ys, y8s = net.test_tile(x, 32, 8, blend=blend, color_fix=True), net.test_tile_u8(xu8, 32, 8, blend=blend, color_fix=True)
    st.synchronize()
    assert torch.equal(ys, y) and torch.equal(y8s, y8)

    def fake_gather(run, crop, empty, results, classes, batch, channel, scale):                    # (tests/test_gpu_tile_blend.py's)
        other = {}
        for hw, tl in tiling.partition(classes, 1, 2).items():
            other[hw] = torch.cat([run(crop(t)) for t in tl], 0) if tl else empty(hw, channel, scale)
        return [results, other]
    g32 = functools.partial(fake_gather, net.test, lambda t: x[:, :, t.y0p:t.y1p, t.x0p:t.x1p], lambda hw, c, s: x.new_zeros((0, c, hw[0] * s, hw[1] * s)))
    gu8 = functools.partial(fake_gather, net.test_u8, lambda t: xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :], lambda hw, c, s: xu8.new_zeros((0, hw[0] * s, hw[1] * s, c)))
    assert torch.equal(net.test_tile(x, 32, 8, rank=0, world_size=2, gather=g32, blend=blend, color_fix=True), y)
    assert torch.equal(net.test_tile_u8(xu8, 32, 8, rank=0, world_size=2, gather=gu8, blend=blend, color_fix=True), y8)
    assert net.test_tile(x, 32, 8, rank=0, world_size=2, gather=g32, paste=False, blend=blend, color_fix=True) is None


_REAL = {}


def _real(cn):
    if cn not in _REAL:
        import gpu_utils as G
        _REAL[cn] = G.build_net(cn, synth_weights(cn, 0, 'trained'))
    return _REAL[cn]


@pytest.mark.parametrize('cn,h,w', [('x4', 16, 24), ('x2', 24, 24)])
def test_network_whole_image(cuda_device, cn, h, w):
    """test / test_u8 on the real network (synthetic weights): the option is the fix of the plain call's result; out=, use_graph=True
    (the fix runs after the replay), a side stream, batch 2 against two single calls, a second run."""
    net = _real(cn)
    s = net.scale_factor
    x = torch.from_numpy(synth.synth_input(10, (2, 3, h, w))).cuda()
    xu8 = (x.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    plain, plain8 = net.test(x), net.test_u8(xu8)
    want, want8 = CF.wavelet_color_fix(plain, x, 5), CF.wavelet_color_fix(plain8, xu8, 5)
    y, y8 = net.test(x, color_fix=True), net.test_u8(xu8, color_fix=True)
    assert torch.equal(y, want) and torch.equal(y8, want8) and not torch.equal(y, plain) and not torch.equal(y8, plain8)
    assert torch.equal(net.test(x), plain) and torch.equal(net.test_u8(xu8), plain8)              # off: nothing changes
    out, out8 = torch.empty_like(plain), torch.empty_like(plain8)
    assert net.test(x, out=out, color_fix=True) is out and torch.equal(out, want)
    assert net.test_u8(xu8, out=out8, color_fix=True) is out8 and torch.equal(out8, want8)
    for i in range(2):
        assert torch.equal(net.test(x[i:i + 1], color_fix=True)[0], y[i]) and torch.equal(net.test_u8(xu8[i], color_fix=True), y8[i])
    assert torch.equal(net.test(x, color_fix=True), y) and torch.equal(net.test_u8(xu8, color_fix=True), y8)
    st = torch.cuda.Stream(device=cuda_device)
    st.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(st):
        ys, y8s = net.test(x, color_fix=True), net.test_u8(xu8, color_fix=True)
    st.synchronize()
    assert torch.equal(ys, y) and torch.equal(y8s, y8)
    net.use_graph = True
    try:
        assert torch.equal(net.test(x, color_fix=True), y)                                        # capture, then the fix outside it
        assert torch.equal(net.test(x, color_fix=True), y)                                        # replay
        assert torch.equal(net.test(x), plain)
        assert net.test(x, out=out.zero_(), color_fix=True) is out and torch.equal(out, want)
    finally:
        net.use_graph = False
        net._graphs = {}
    assert tuple(y.shape) == (2, 3, h * s, w * s)


def test_network_tiled(cuda_device):
    """The real x4 network through test_tile / test_tile_u8 at 70x100, 32/8, blend on and off."""
    net = _real('x4')
    x = torch.from_numpy(synth.synth_input(10, (1, 3, 70, 100))).cuda()
    u8 = (x[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    for blend in (False, True):
        plain, plain8 = net.test_tile(x, 32, 8, blend=blend), net.test_tile_u8(u8, 32, 8, blend=blend)
        y, y8 = net.test_tile(x, 32, 8, blend=blend, color_fix=True), net.test_tile_u8(u8, 32, 8, blend=blend, color_fix=True)
        assert torch.equal(y, CF.wavelet_color_fix(plain, x, 5)) and not torch.equal(y, plain)
        assert torch.equal(y8, CF.wavelet_color_fix(plain8, u8, 5)) and not torch.equal(y8, plain8)
        assert y8.shape == (280, 400, 3)

"""-m gpu: the overlap-blend paste (`test_tile(..., blend=True)` -> femasr_blend_tiles / femasr_blend_tiles_u8).

The kernels are driven through the tile driver with GPU stand-ins for `test()` / `test_u8()` (no weights needed: every offset, origin
and stride of the gather is visible in the canvas) and then with the real network on synthetic weights.  The checker is the float64
definition of tests/blend_ref.py; the fp32 allowance is 16 * 2^-24 * max|v| over the covering tile values, floored at 16 * 2^-24
(derived in DESIGN.md 14: (2n + 6) eps max|v| with n <= 4 covering tiles), the uint8 canvas must equal rint(definition) except within
16 * 2^-24 * 255 of a tie."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from blend_ref import BOUND, BlendRef, check_u8, tile_values
from femasr_amd import _lib, synth, tiling
from femasr_amd.archs import build_network
from helpers import CONFIGS, synth_weights

pytestmark = pytest.mark.gpu
S, TS, PAD = 4, 32, 8
GEOMS = [(70, 100), (96, 128)]          # 3 x 4 tiles each; 70x100: ragged last tiles (bodies of 6 and 4 pixels, narrower than the pad), 9 shape classes


# --------------------------------------------------------------------------------------------------------------- stand-ins
def _up(t):
    return F.interpolate(t, scale_factor=S, mode='nearest')


def _const(t):                          # the crop's per-sample max, broadcast: one constant per tile and image
    return t.amax(dim=(1, 2, 3), keepdim=True).expand(t.shape[0], t.shape[1], t.shape[2] * S, t.shape[3] * S)


def _fake(t):                           # tests/test_distributed_cpu.py's stand-in: depends on every pixel of the crop and on its shape
    return _up(t) * 0.5 + t.amax(dim=(1, 2, 3), keepdim=True) + 0.001 * t.shape[2] + 0.01 * t.shape[3]


def _fake_u8(t, bgr=False):             # (n, h, w, 3) uint8 -> (n, 4h, 4w, 3) uint8
    y = _fake(t.permute(0, 3, 1, 2).float() / 255.0) * 0.25
    return (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _standin_net(fn=_fake):
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['x4']))
    net.test = fn
    net.test_u8 = _fake_u8
    net.max_tile_batch = 3
    return net


def _image(dev, batch, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((batch, 3, h, w), generator=g).to(dev)


def _image_u8(dev, batch, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (batch, h, w, 3), generator=g, dtype=torch.uint8).to(dev)


def _assert_within(got, ref):
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.canvas)
    ratio = float((err / ref.bound()).max())
    print(f'max |fp32 - definition| / (16 eps max|v|) = {ratio:.3f}')
    assert ratio <= 1.0, ratio


# --------------------------------------------------------------------------------------------------------------- a. every tile agrees
@pytest.mark.parametrize('h,w', GEOMS)
@pytest.mark.parametrize('batch', [1, 2])
def test_agreeing_tiles_reproduce_the_image(cuda_device, h, w, batch):
    """Stand-in = nearest x4 of the crop: every window then holds the global upsampled image, and a weighted mean of equal values is
    that value - any wrong offset, origin, stride or batch index of the gather shows."""
    x = _image(cuda_device, batch, h, w)
    got = _standin_net(_up).test_tile(x, TS, PAD, blend=True)
    want = _up(x)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = (got.double() - want.double()).abs()
    assert bool((err <= BOUND * want.double().abs().clamp(min=1.0)).all()), float(err.max())


# --------------------------------------------------------------------------------------------------------------- b. no seams
def test_constant_tiles_blend_without_a_step(cuda_device):
    """One constant per tile on the regular 96x128 geometry (margins 32 on every inner side): the blended canvas moves by at most
    range * (1 / (2 Ly) + 1 / (2 Lx)) + bound between adjacent pixels (the weights sum to 1 there and one pixel moves a ramp by
    1 / (2 L)), while the overlap-discard paste of the SAME tiles steps by the full |c_A - c_B| where two bodies meet."""
    h, w, L = 96, 128, PAD * S
    amp = torch.tensor([[0.9, 0.3, 0.7, 0.2], [0.4, 1.0, 0.1, 0.8], [0.6, 0.25, 0.95, 0.5]])
    # (every cell's content sits at least tile_pad inside it, so a window's max is its own body's and neighbouring constants differ a lot)
    inner = ((torch.arange(h) % TS >= PAD) & (torch.arange(h) % TS < TS - PAD))[:, None] & ((torch.arange(w) % TS >= PAD) & (torch.arange(w) % TS < TS - PAD))[None, :]
    x = _image(cuda_device, 2, h, w) * (amp.repeat_interleave(TS, 0).repeat_interleave(TS, 1) * inner).to(cuda_device)
    net = _standin_net(_const)
    yb, yp = net.test_tile(x, TS, PAD, blend=True).double(), net.test_tile(x, TS, PAD).double()
    tiles = tiling.enumerate_tiles(h, w, TS, PAD)
    c = torch.stack([x[:, :, t.y0p:t.y1p, t.x0p:t.x1p].amax(dim=(1, 2, 3)) for t in tiles], 1).double().view(2, 3, 4)     # (image, ty, tx)
    rng = (c.amax(dim=(1, 2)) - c.amin(dim=(1, 2))).view(2, 1, 1, 1)
    allow = rng * (1 / (2 * L) + 1 / (2 * L)) + BOUND * c.amax(dim=(1, 2)).clamp(min=1.0).view(2, 1, 1, 1)
    for d in (2, 3):
        step = yb.diff(dim=d).abs()
        print(f'axis {d}: largest blended step {float(step.max()):.5f}, allowed {float(allow.min()):.5f}')
        assert bool((step <= allow).all())
    P = TS * S
    for tx in range(1, 4):               # vertical seams of the paste: exactly the neighbours' constants on either side
        want = (c[:, :, tx] - c[:, :, tx - 1]).repeat_interleave(P, 1).view(2, 1, h * S)
        assert torch.equal(yp[:, :, :, tx * P] - yp[:, :, :, tx * P - 1], want.expand(2, 3, h * S))
    for ty in range(1, 3):
        want = (c[:, ty, :] - c[:, ty - 1, :]).repeat_interleave(P, 1).view(2, 1, w * S)
        assert torch.equal(yp[:, :, ty * P, :] - yp[:, :, ty * P - 1, :], want.expand(2, 3, w * S))
    assert float(yp.diff(dim=3).abs().max()) > 10 * float(allow.max())      # the seam is real, and the blend removes it
    assert float(yp.diff(dim=2).abs().max()) > 10 * float(allow.max())


# --------------------------------------------------------------------------------------------------------------- c, d. the definition
@pytest.mark.parametrize('h,w', GEOMS)
@pytest.mark.parametrize('batch', [1, 2])
def test_standin_against_the_definition(cuda_device, h, w, batch):
    x = _image(cuda_device, batch, h, w, seed=h + batch)
    net = _standin_net()
    got = net.test_tile(x, TS, PAD, blend=True)
    tiles = tiling.enumerate_tiles(h, w, TS, PAD)
    ref = BlendRef(tiles, tile_values(tiles, net.test, x), S, h, w)
    _assert_within(got, ref)
    # d. one covering window with weight exactly 1: 0 + 1 * v, over 1 - the overlap-discard value bit for bit
    plain = net.test_tile(x, TS, PAD)
    one = np.broadcast_to(ref.one, ref.canvas.shape)
    assert one.any() and not one.all()
    assert np.array_equal(got.cpu().numpy()[one], plain.cpu().numpy()[one])
    assert not torch.equal(got, plain)


@pytest.mark.parametrize('h,w', GEOMS)
def test_standin_u8_against_the_definition(cuda_device, h, w):
    xu8 = _image_u8(cuda_device, 2, h, w, seed=h)
    net = _standin_net()
    got = net.test_tile_u8(xu8, TS, PAD, blend=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h * S, w * S, 3)
    tiles = tiling.enumerate_tiles(h, w, TS, PAD)
    vals = [net.test_u8(xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :]).permute(0, 3, 1, 2).cpu().numpy() for t in tiles]
    ref = BlendRef(tiles, vals, S, h, w)
    bad, share = check_u8(got.permute(0, 3, 1, 2).cpu().numpy(), ref)
    print(f'{bad} bytes differ outside the near-tie rule; near-tie share {share:.5f}')
    assert bad == 0 and share <= 0.01, (bad, share)
    plain = net.test_tile_u8(xu8, TS, PAD)
    one = np.broadcast_to(ref.one[None, :, :, None], tuple(got.shape))
    assert np.array_equal(got.cpu().numpy()[one], plain.cpu().numpy()[one])
    assert torch.equal(net.test_tile_u8(xu8[1], TS, PAD, blend=True), got[1])          # (H,W,3) in -> (sH,sW,3) out


# --------------------------------------------------------------------------------------------------------------- e. nothing to blend
@pytest.mark.parametrize('h,w,ts,pad', [(64, 64, 32, 0), (70, 100, 32, 0), (24, 28, 32, 8)])
def test_without_overlap_blend_is_the_paste(cuda_device, h, w, ts, pad):
    """tile_pad = 0, and an image that fits one tile: every pixel has one window, weight 1 - the whole canvas equals blend=False bitwise."""
    net = _standin_net()
    x, xu8 = _image(cuda_device, 2, h, w), _image_u8(cuda_device, 2, h, w)
    assert torch.equal(net.test_tile(x, ts, pad, blend=True), net.test_tile(x, ts, pad))
    assert torch.equal(net.test_tile_u8(xu8, ts, pad, blend=True), net.test_tile_u8(xu8, ts, pad))


# --------------------------------------------------------------------------------------------------------------- f. invariance
def test_invariance(cuda_device):
    h, w = 70, 100
    net = _standin_net()
    x, xu8 = _image(cuda_device, 2, h, w, seed=5), _image_u8(cuda_device, 2, h, w, seed=5)
    y, yu = net.test_tile(x, TS, PAD, blend=True), net.test_tile_u8(xu8, TS, PAD, blend=True)
    # a second run
    assert torch.equal(net.test_tile(x, TS, PAD, blend=True), y) and torch.equal(net.test_tile_u8(xu8, TS, PAD, blend=True), yu)
    # batch 2 == the two single calls
    for i in range(2):
        assert torch.equal(net.test_tile(x[i:i + 1], TS, PAD, blend=True)[0], y[i])
        assert torch.equal(net.test_tile_u8(xu8[i], TS, PAD, blend=True), yu[i])
    # a side stream
    st = torch.cuda.Stream(device=cuda_device)
    st.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(st):
        ys, yus = net.test_tile(x, TS, PAD, blend=True), net.test_tile_u8(xu8, TS, PAD, blend=True)
    st.synchronize()
    assert torch.equal(ys, y) and torch.equal(yus, yu)

    # two "ranks" in one process (the fake gather of tests/test_gpu_network.py): which rank computed a tile must not show
    def fake_gather(run, crop, empty, results, classes, batch, channel, scale):
        other = {}
        for hw, tl in tiling.partition(classes, 1, 2).items():
            other[hw] = torch.cat([run(crop(t)) for t in tl], 0) if tl else empty(hw, channel, scale)
        return [results, other]
    g32 = functools.partial(fake_gather, net.test, lambda t: x[:, :, t.y0p:t.y1p, t.x0p:t.x1p],
                            lambda hw, c, s: x.new_zeros((0, c, hw[0] * s, hw[1] * s)))
    gu8 = functools.partial(fake_gather, net.test_u8, lambda t: xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :],
                            lambda hw, c, s: xu8.new_zeros((0, hw[0] * s, hw[1] * s, c)))
    assert torch.equal(net.test_tile(x, TS, PAD, rank=0, world_size=2, gather=g32, blend=True), y)
    assert torch.equal(net.test_tile_u8(xu8, TS, PAD, rank=0, world_size=2, gather=gu8, blend=True), yu)


# --------------------------------------------------------------------------------------------------------------- g. refusals
def test_refusals_leave_the_canvas_alone(cuda_device):
    lib = _lib.load()
    tiles = tiling.enumerate_tiles(40, 40, TS, PAD)
    n, s = len(tiles), 2
    geo = torch.tensor(tiling.blend_table(tiles, s), dtype=torch.int32, device=cuda_device)
    buf = torch.zeros((n, 3, 48 * s, 48 * s), device=cuda_device)
    tab = torch.tensor([buf[k].data_ptr() for k in range(n)], dtype=torch.int64, device=cuda_device)
    for dtype, fn, bc in ((torch.float32, lib.femasr_blend_tiles, (1, 3)), (torch.uint8, lib.femasr_blend_tiles_u8, (1,))):
        canvas = torch.full((1, 3, 40 * s, 40 * s), 7, dtype=dtype, device=cuda_device)
        args = lambda tab_, geo_, n_, ny=2, nx=2: (None, tab_, geo_, n_, ny, nx, TS * s) + bc + (40 * s, 40 * s, canvas.data_ptr())
        assert fn(*args(tab.data_ptr(), None, n)) == -1                    # FEMASR_ERR_INVALID: a null table
        assert b'null' in lib.femasr_last_error()
        assert fn(*args(None, geo.data_ptr(), n)) == -1
        assert fn(*args(tab.data_ptr(), geo.data_ptr(), 0)) == -1          # n = 0
        assert fn(*args(tab.data_ptr(), geo.data_ptr(), n, 2, 3)) == -1    # n != tiles_y * tiles_x
        assert fn(*args(tab.data_ptr(), geo.data_ptr(), n)[:-1] + (None,)) == -1
        torch.cuda.synchronize(cuda_device)
        assert bool((canvas == 7).all())


# --------------------------------------------------------------------------------------------------------------- the real network
_REAL = {}


def _real(cn, h, w):
    """(net, x, uint8 image, tiles) on synthetic weights, built once per configuration."""
    if cn not in _REAL:
        import gpu_utils as G
        net = G.build_net(cn, synth_weights(cn, 0, 'trained'))
        x = torch.from_numpy(synth.synth_input(10, (1, 3, h, w))).cuda()
        u8 = (x[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
        _REAL[cn] = (net, x, u8, tiling.enumerate_tiles(h, w, TS, PAD))
    return _REAL[cn]


REAL_CASES = [('x4', 70, 100), ('x2', 72, 72)]


@pytest.mark.parametrize('cn,h,w', REAL_CASES)
def test_network_against_the_definition(cuda_device, cn, h, w):
    """h. test_tile(x, 32, 8, blend=True) against the float64 definition applied to the tiles net.test(crop) returns one crop at a time."""
    net, x, _, tiles = _real(cn, h, w)
    s = net.scale_factor
    got = net.test_tile(x, TS, PAD, blend=True)
    ref = BlendRef(tiles, tile_values(tiles, net.test, x), s, h, w)
    assert tuple(got.shape) == (1, 3, h * s, w * s)
    _assert_within(got, ref)
    assert not torch.equal(got, net.test_tile(x, TS, PAD))


@pytest.mark.parametrize('cn,h,w', REAL_CASES)
def test_network_u8_against_the_definition(cuda_device, cn, h, w):
    """i. test_tile_u8(..., blend=True) == rint(clamp(definition on the test_u8 tiles)); within 16 * 2^-24 * 255 of k + 0.5 either
    neighbour is accepted, and at most 1 % of the bytes may be that close to a tie (counted from the definition alone).
    j. bgr=True (BGR in and out) is the channel-flipped canvas, bit for bit.
    The near-tie share of these two cases, counted on the CPU from the oracle's tiles (the bits fp32_strict produces): x4 0.05 %, x2 0.52 %."""
    net, _, u8, tiles = _real(cn, h, w)
    s = net.scale_factor
    got = net.test_tile_u8(u8, TS, PAD, blend=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h * s, w * s, 3)
    vals = [net.test_u8(u8[t.y0p:t.y1p, t.x0p:t.x1p, :].contiguous())[None].permute(0, 3, 1, 2).cpu().numpy() for t in tiles]
    ref = BlendRef(tiles, vals, s, h, w)
    bad, share = check_u8(got[None].permute(0, 3, 1, 2).cpu().numpy(), ref)
    print(f'{bad} bytes differ outside the near-tie rule; near-tie share {share:.5f}')
    assert share <= 0.01, share
    assert bad == 0, bad
    assert not torch.equal(got, net.test_tile_u8(u8, TS, PAD))
    assert torch.equal(net.test_tile_u8(u8.flip(-1), TS, PAD, blend=True, bgr=True).flip(-1), got)          # cv2-style channel order in and out

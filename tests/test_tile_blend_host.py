"""Overlap-blend paste (`test_tile(..., blend=True)`) without a GPU: the weight definition, the geometry table, the
host path of the tile driver against the float64 definition (tests/blend_ref.py), the 2-rank gloo run and the CLI flag.  The network
needs a GPU, so `test()` / `test_u8()` are the deterministic per-tile stand-ins of tests/test_distributed_cpu.py (copied)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from blend_ref import BOUND, BlendRef, check_u8, tile_values
from femasr_amd import distributed as fd
from femasr_amd import tiling
from femasr_amd.archs import build_network
from helpers import CONFIGS

S = 4
# (H, W, tile_size, tile_pad): the last bodies of 70x100 (6 and 4 pixels) are narrower than the pad - the irregular case, where the
# weights of the covering windows do not sum to 1; 96x128 is regular; pad 0 has no overlap at all
GEOMS = [(70, 100, 32, 8), (96, 128, 32, 8), (64, 64, 32, 0)]


# --------------------------------------------------------------------------------------------------------------- stand-in network
def _fake_test(self, t):
    # depends on every pixel of the tile (max: exact, batch-size independent) and on position -> any mis-paste / mis-order is visible
    up = F.interpolate(t, scale_factor=4, mode='nearest')
    return up * 0.5 + t.amax(dim=(1, 2, 3), keepdim=True) + 0.001 * t.shape[2] + 0.01 * t.shape[3]


def _to_f32(u8):          # imgproc.u8_to_input on the host: (B,H,W,3) uint8 -> (B,3,H,W) float in [0,1]
    return u8.permute(0, 3, 1, 2).float() / 255.0


def _to_u8(y):            # imgproc.output_to_u8 (tensor2img): clamp, x255, round half to even -> (B,H,W,3) uint8
    return (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _fake_test_u8(self, t, bgr=False):
    # stand-in of FeMaSRNet.test_u8 (no `out=`: test_tile_u8 copies): the fp32 stand-in between the CLI's decode and tensor2img
    return _to_u8(_fake_test(self, _to_f32(t)) * 0.25)


def _make_net():
    net = build_network(dict(type='FeMaSRNet', **CONFIGS['x4']))
    net.test = _fake_test.__get__(net)
    net.test_u8 = _fake_test_u8.__get__(net)
    net.max_tile_batch = 3
    return net


# --------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('lead,trail', [(0, 0), (32, 32), (0, 32), (32, 0), (8, 24), (12, 12), (20, 0), (6, 6)])
def test_weights_are_positive_and_one_outside_the_ramps(lead, trail):
    n = 192
    w = tiling.blend_weight_1d(n, lead, trail)
    assert w.dtype == np.float64 and w.shape == (n,)
    assert (w > 0).all() and (w <= 1).all()
    assert (w[2 * lead:n - 2 * trail] == 1.0).all()                     # exactly 1 outside the 2 * margin wide ramp bands
    if lead:
        assert (w[:2 * lead] < 1).all() and w[0] == 1 / (4 * lead)      # the ramp: pixel centres, (2 i + 1) / (4 L)
        assert np.array_equal(w[:2 * lead], (2 * np.arange(2 * lead) + 1) / (4.0 * lead))
    if trail:
        assert (w[n - 2 * trail:] < 1).all() and w[-1] == 1 / (4 * trail)
    assert np.array_equal(tiling.blend_weight_1d(n, trail, lead), w[::-1])


@pytest.mark.parametrize('margin', [2, 4, 6, 8, 12, 20, 32, 36, 64])
def test_two_regular_neighbours_sum_to_one(margin):
    """Body edge between tiles A and B, both with margin m on that side: over the 2m overlap pixels A's trailing ramp and B's leading
    ramp sum to 1 - within 2 ulp of float64, exactly when 4m is a power of two (every quotient is then exact)."""
    n = 4 * margin + 16
    a = tiling.blend_weight_1d(n, 0, margin)[n - 2 * margin:]
    b = tiling.blend_weight_1d(n, margin, 0)[:2 * margin]
    s = a + b
    assert np.abs(s - 1.0).max() <= 2 * np.spacing(1.0)
    if (4 * margin) & (4 * margin - 1) == 0:
        assert (s == 1.0).all()


@pytest.mark.parametrize('h,w,ts,pad', GEOMS)
def test_geometry_cover_and_partition_of_unity(h, w, ts, pad):
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    ref = BlendRef(tiles, [np.ones((1, 1, (t.y1p - t.y0p) * S, (t.x1p - t.x0p) * S)) for t in tiles], S, h, w)
    assert ref.cover.min() >= 1 and ref.cover.max() <= (4 if pad else 1)
    assert (ref.wsum > 0).all()
    assert np.abs(ref.canvas - 1.0).max() <= 4 * np.spacing(1.0)         # a weighted MEAN: constants are reproduced
    nx = -(-w // ts)
    for t in tiles:                                                       # only the own cell and its +-1 neighbours can cover a pixel
        ay, ax, th, tw = tiling.blend_geom(t, S)[:4]
        ty, tx = divmod(t.index, nx)
        assert ay >= (ty - 1) * ts * S and ay + th <= (ty + 2) * ts * S and ax >= (tx - 1) * ts * S and ax + tw <= (tx + 2) * ts * S
    if (h, w) == (70, 100):
        assert np.abs(ref.wsum - 1.0).max() > 0.1                        # ragged last tiles break the partition of unity: the division is needed
    else:
        assert np.abs(ref.wsum - 1.0).max() <= 4 * np.spacing(1.0)
    if pad == 0:
        assert ref.one.all()


def test_blend_needs_pad_at_most_half_a_tile():
    tiling.check_blend(32, 16)
    tiling.check_blend(32, 0)
    for ts, pad in ((32, 17), (30, 16), (8, 8)):
        with pytest.raises(ValueError):
            tiling.check_blend(ts, pad)
    net = _make_net()
    calls = []
    net.test = lambda t: calls.append(1)
    with pytest.raises(ValueError):
        net.test_tile(torch.rand(1, 3, 70, 100), 32, 17, blend=True)
    with pytest.raises(ValueError):
        net.test_tile_u8(torch.zeros(70, 100, 3, dtype=torch.uint8), 30, 16, blend=True)
    assert not calls                                                      # refused before any work


@pytest.mark.parametrize('h,w,ts,pad', GEOMS)
@pytest.mark.parametrize('s', [2, 4])
def test_table_against_the_tile_fields(h, w, ts, pad, s):
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    tab = tiling.blend_table(tiles, s)
    assert len(tab) == tiling.BLEND_FIELDS * len(tiles) and all(isinstance(v, int) for v in tab)
    assert np.array(tab).max() < 2 ** 31
    for t in tiles:
        ay, ax, th, tw, ly, ry, lx, rx = tab[8 * t.index:8 * t.index + 8]
        assert (ay, ax) == (t.y0p * s, t.x0p * s) and (th, tw) == (t.in_hw[0] * s, t.in_hw[1] * s)
        ys, ye, xs, xe = t.out_src(s)                                     # the body inside the window: what the margins leave
        assert (ly, th - ry, lx, tw - rx) == (ys, ye, xs, xe)
        assert (ay + ly, ax + lx) == t.out_dst(s)[0::2]
        if pad:                                                           # margin 0 <=> that side of the body is the image border
            assert (ly == 0) == (t.y0 == 0) and (ry == 0) == (t.y1 == h) and (lx == 0) == (t.x0 == 0) and (rx == 0) == (t.x1 == w)
        else:
            assert (ly, ry, lx, rx) == (0, 0, 0, 0)
        assert pad * s >= max(ly, ry, lx, rx)


# --------------------------------------------------------------------------------------------------------------- the host path
@pytest.mark.parametrize('h,w,ts,pad', GEOMS)
@pytest.mark.parametrize('batch', [1, 2])
def test_host_path_against_the_definition(h, w, ts, pad, batch):
    torch.manual_seed(h + batch)
    x = torch.rand(batch, 3, h, w)
    net = _make_net()
    got = net.test_tile(x, ts, pad, blend=True)
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    ref = BlendRef(tiles, tile_values(tiles, net.test, x), S, h, w)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.canvas.shape
    err = np.abs(got.numpy().astype(np.float64) - ref.canvas)
    assert (err <= ref.bound()).all(), float((err / ref.bound()).max())
    plain = net.test_tile(x, ts, pad)
    one = np.broadcast_to(ref.one, ref.canvas.shape)
    assert np.array_equal(got.numpy()[one], plain.numpy()[one])          # one window, weight 1: the overlap-discard value, bit for bit
    if pad == 0:
        assert torch.equal(got, plain)
    else:
        assert not torch.equal(got, plain)


@pytest.mark.parametrize('h,w,ts,pad', GEOMS)
def test_host_path_u8_against_the_definition(h, w, ts, pad):
    torch.manual_seed(h)
    xu8 = (torch.rand(2, h, w, 3) * 255).round().to(torch.uint8)
    net = _make_net()
    got = net.test_tile_u8(xu8, ts, pad, blend=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h * S, w * S, 3)
    tiles = tiling.enumerate_tiles(h, w, ts, pad)
    vals = [net.test_u8(xu8[:, t.y0p:t.y1p, t.x0p:t.x1p, :]).permute(0, 3, 1, 2).numpy() for t in tiles]
    ref = BlendRef(tiles, vals, S, h, w)
    bad, share = check_u8(got.permute(0, 3, 1, 2).numpy(), ref)
    assert bad == 0 and share <= 0.01, (bad, share)
    assert torch.equal(net.test_tile_u8(xu8[0], ts, pad, blend=True), got[0])          # (H,W,3) in -> (sH,sW,3) out


# --------------------------------------------------------------------------------------------------------------- two ranks (gloo)
def _worker(rank, world, port, x, xu8, ts, pad, expect, expect_u8, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    fd.init_from_env('gloo')
    y = fd.test_tile_parallel(_make_net(), x, ts, pad, blend=True)
    yu = fd.test_tile_parallel(_make_net(), xu8, ts, pad, blend=True)
    q.put((rank, bool(torch.equal(y, expect)), yu.dtype == torch.uint8 and bool(torch.equal(yu, expect_u8))))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_blend_equals_single_rank_bitwise():
    """Gather form and a fixed visiting order make ownership invisible: every rank's canvas is the single-rank canvas, bit for bit."""
    torch.manual_seed(0)
    x = torch.rand(2, 3, 70, 100)
    xu8 = (torch.rand(70, 100, 3) * 255).round().to(torch.uint8)
    net = _make_net()
    expect, expect_u8 = net.test_tile(x, 32, 8, blend=True), net.test_tile_u8(xu8, 32, 8, blend=True)
    assert not torch.equal(expect, net.test_tile(x, 32, 8))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, x, xu8, 32, 8, expect, expect_u8, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == [(0, True, True), (1, True, True)]


# --------------------------------------------------------------------------------------------------------------- callers
def test_cli_parser_accepts_blend():
    from femasr_amd import inference
    ap = inference.build_parser()
    assert ap.parse_args([]).blend is False
    args = ap.parse_args(['-i', 'x.png', '--blend', '--tile_size', '96'])
    assert args.blend is True and args.tile_size == 96 and args.tile_pad == 16


def test_model_option_tile_blend():
    """`val: tile_blend: true` reaches the tiled branch of FeMaSRModel.test; absent means the default call, unchanged."""
    from femasr_amd.models.femasr_model import FeMaSRModel
    seen = []

    class Net:
        def test_tile(self, lq, **kw):
            seen.append(kw)
            return lq

    for opt, want in (({}, {}), ({'val': None}, {}), ({'val': {'tile_blend': False}}, {}), ({'val': {'tile_blend': True}}, {'blend': True})):
        m = FeMaSRModel.__new__(FeMaSRModel)
        m.opt, m.net_g = opt, Net()
        m.lq = torch.zeros(1, dtype=torch.uint8).expand(1, 3, 8000, 8001)            # (a stride-0 view: the size alone picks the branch)
        m.test()
        assert seen.pop() == want

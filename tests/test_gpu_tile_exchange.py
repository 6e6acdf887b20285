"""-m gpu: the tile-parallel exchange with REAL forwards on one device - slab writes, gather, paste and blend.

`femasr_amd.distributed.test_tile_parallel` (the CLI's call when WORLD_SIZE > 1) runs here as every rank of a world of N in turn, with the
loopback of tests/loopback_dist.py in place of `torch.distributed` (two rounds: record, then replay with every row known;
tests/test_loopback_dist_host.py holds that method against the single-process result and shows that a wrong gather fails it).  So the
forward's crop kernel stores through `out=` into views at element offsets inside the flat send slab of `TileGather` (fp32 (n,C,H,W) and
uint8 (n,H,W,C); empty views for classes a rank owns no tile of; an unused tail on the lighter ranks), and femasr_paste_tiles[_u8] /
femasr_blend_tiles[_u8] read the tiles at r * cap + offset inside the (world, cap) receive buffer.

The reference is the same net's single-process `test_tile` / `test_tile_u8` with the same options (held to the oracle and the reference's
goldens in test_gpu_network.py); the plain mode is also held to a canvas assembled with torch slicing from one `test(crop)` per tile in
the reference's loop order.  Every comparison is bit for bit.  Not covered by this module or any other: more than one device, xGMI, the
scaling curve."""
import pytest
import torch

import loopback_dist as LB
from femasr_amd import distributed as fd, synth, tiling
from helpers import synth_weights

pytestmark = pytest.mark.gpu

TS, PAD = 16, 4
FORMATS = ['f32', 'u8']
_NETS, _REFS = {}, {}


def _net(cn):
    if cn not in _NETS:
        import gpu_utils as G
        _NETS[cn] = G.build_net(cn, synth_weights(cn, 0, 'trained'))
    return _NETS[cn]


@pytest.fixture(autouse=True)
def _fresh_exchanges(cuda_device):
    fd._exchanges.clear()
    yield
    fd._exchanges.clear()


def _image(fmt, b, h, w, seed=21):
    """fp32 (b,3,h,w), or the bytes of the same image: (h,w,3) - the CLI's data type - for b == 1, else (b,h,w,3)."""
    x = torch.from_numpy(synth.synth_input(seed, (b, 3, h, w))).cuda()
    if fmt == 'f32':
        return x
    xu8 = (x.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    return xu8[0] if b == 1 else xu8


def _bhw(x):
    if x.dtype == torch.uint8:
        return (1,) + tuple(x.shape[:2]) if x.dim() == 3 else tuple(x.shape[:3])
    return (x.shape[0],) + tuple(x.shape[2:])


def _single(net, x, ts, pad, **opts):
    return (net.test_tile_u8 if x.dtype == torch.uint8 else net.test_tile)(x, ts, pad, **opts)


def _want(cn, x, ts, pad, seed=21, **opts):
    """The single-process canvas, computed once per case of the module and never written to."""
    key = (cn, str(x.dtype), tuple(x.shape), ts, pad, seed, tuple(sorted(opts.items())))
    if key not in _REFS:
        _REFS[key] = _single(_net(cn), x, ts, pad, **opts)
    return _REFS[key]


def _sliced(net, x, ts, pad):
    """The reference's loop (one call per tile, row-major, overlap-discard paste onto zeros) with torch slicing: no batching, no kernels
    of the tile driver."""
    b, h, w = _bhw(x)
    s = net.scale_factor
    u8 = x.dtype == torch.uint8
    xb = x.unsqueeze(0) if (u8 and x.dim() == 3) else x
    out = torch.zeros((b, h * s, w * s, 3) if u8 else (b, 3, h * s, w * s), dtype=x.dtype, device=x.device)
    for t in tiling.enumerate_tiles(h, w, ts, pad):
        ys, ye, xs, xe = t.out_src(s)
        a, bb, c, d = t.out_dst(s)
        if u8:
            out[:, a:bb, c:d, :] = net.test_u8(xb[:, t.y0p:t.y1p, t.x0p:t.x1p, :].contiguous())[:, ys:ye, xs:xe, :]
        else:
            out[:, :, a:bb, c:d] = net.test(xb[:, :, t.y0p:t.y1p, t.x0p:t.x1p])[:, :, ys:ye, xs:xe]
    return out[0] if (u8 and x.dim() == 3) else out


def _exchange(monkeypatch, net, x, world, ts, pad, wants, what, root_only=False, rounds=2, before=None, **opts):
    """Play every rank of `world` through test_tile_parallel in two rounds; the slabs of the rounds agree, every pasting rank's canvas is
    each of `wants`, the others return None.  Returns the loopback."""
    loop = LB.Loopback(world)
    monkeypatch.setattr(fd, 'dist', loop)
    got = LB.play(loop, lambda r: fd.test_tile_parallel(net, x, ts, pad, root_only=root_only, **opts), rounds=rounds, before=before)
    b, h, w = _bhw(x)
    sizes = LB.payload_sizes(h, w, ts, pad, world, b, 3, net.scale_factor)
    loop.assert_rounds_equal(lambda rank, call: sizes[rank])
    for r in range(world):
        assert loop.recorded(r).numel() == max(max(sizes), 1)                  # every rank joined the collective, with `cap` elements
        if root_only and r > 0:
            assert got[r] is None, f'{what}: rank {r} of world {world} pasted with root_only'
        else:
            for want in wants:
                LB.assert_canvas(got[r], want, r, world, f'{what} root_only={root_only} {opts}')
    return loop


# ------------------------------------------------------------------------------------------------------------------ 1. the plain mode
@pytest.fixture(scope='module')
def plain(cuda_device):
    """{format: (image, single-process canvas, canvas from per-tile calls and slicing)} of the x4 40x56 case; the two canvases agree."""
    out = {}
    for fmt in FORMATS:
        x = _image(fmt, 1, 40, 56)
        want, sliced = _want('x4', x, TS, PAD), _sliced(_net('x4'), x, TS, PAD)
        assert LB.first_difference(want, sliced) is None, (fmt, LB.first_difference(want, sliced))
        out[fmt] = (x, want, sliced)
    return out


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('world', [2, 3, 8])
def test_plain_every_rank_every_world(monkeypatch, plain, world, fmt):
    x, want, sliced = plain[fmt]
    for root_only in (False, True):
        _exchange(monkeypatch, _net('x4'), x, world, TS, PAD, (want, sliced), '40x56', root_only=root_only)


@pytest.mark.parametrize('fmt', FORMATS)
def test_world_of_one_uses_the_gather_it_is_given(monkeypatch, plain, fmt):
    """`_tiled` honours a gather object at world_size == 1 (one rank of a real collective takes the slab, gather and paste path);
    test_tile_parallel itself keeps its short-circuit there."""
    x, want, sliced = plain[fmt]
    net = _net('x4')
    loop = LB.Loopback(1)
    monkeypatch.setattr(fd, 'dist', loop)
    fn = net.test_tile_u8 if fmt == 'u8' else net.test_tile
    got = LB.play(loop, lambda r: fn(x, TS, PAD, rank=0, world_size=1, gather=fd._exchange_for(None)))
    loop.assert_rounds_equal()
    assert loop.recorded(0).numel() == LB.payload_sizes(40, 56, TS, PAD, 1, 1, 3, 4)[0] > 40 * 56 * 16 * 3      # every window, halos included, went through the slab
    for w in (want, sliced):
        LB.assert_canvas(got[0], w, 0, 1, 'world 1')
    loop.begin_round()
    loop.set_rank(0)
    assert fn(x, TS, PAD, rank=0, world_size=1, gather=fd._exchange_for(None), paste=False) is None and len(loop.rounds[-1]) == 1
    loop.begin_round()
    LB.assert_canvas(fd.test_tile_parallel(net, x, TS, PAD), want, 0, 1, 'short-circuit')
    assert not loop.rounds[-1]                                                  # no collective
    with pytest.raises(ValueError):
        fn(x, TS, PAD, rank=0, world_size=2)


# ------------------------------------------------------------------------------------------------------------------ 2. ranks that own nothing
@pytest.mark.parametrize('fmt', FORMATS)
def test_ranks_without_tiles(monkeypatch, fmt):
    """24x24 at world 8: four tiles, ranks 4-7 own none (sizes[r] == 0, `cap` from the others)."""
    x = _image(fmt, 1, 24, 24, seed=22)
    assert LB.payload_sizes(24, 24, TS, PAD, 8, 1, 3, 4)[4:] == [0, 0, 0, 0]
    net = _net('x4')
    _exchange(monkeypatch, net, x, 8, TS, PAD, (_want('x4', x, TS, PAD, seed=22), _sliced(net, x, TS, PAD)), '24x24')


# ------------------------------------------------------------------------------------------------------------------ 3. a batch of byte images
def test_uint8_batch_of_two(monkeypatch):
    """(2,40,56,3) at world 3: batch-major placement inside every class view."""
    x = _image('u8', 2, 40, 56, seed=23)
    net = _net('x4')
    assert not torch.equal(x[0], x[1])
    _exchange(monkeypatch, net, x, 3, TS, PAD, (_want('x4', x, TS, PAD, seed=23), _sliced(net, x, TS, PAD)), 'batch 2')


# ------------------------------------------------------------------------------------------------------------------ 4. blend, colour fix
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('world,color_fix', [(2, False), (8, False), (3, True)])
def test_blend_and_color_fix(monkeypatch, plain, world, color_fix, fmt):
    """blend=True: the pointer table of femasr_blend_tiles[_u8] holds addresses inside the receive buffer; the colour fix runs on the
    pasting ranks only."""
    x, plain_want, _ = plain[fmt]
    opts = dict(blend=True, color_fix=True) if color_fix else dict(blend=True)
    want = _want('x4', x, TS, PAD, **opts)
    assert LB.first_difference(want, plain_want) is not None
    _exchange(monkeypatch, _net('x4'), x, world, TS, PAD, (want,), 'blend', root_only=color_fix, **opts)
    if color_fix:
        _exchange(monkeypatch, _net('x4'), x, world, TS, PAD, (want,), 'blend', **opts)


# ------------------------------------------------------------------------------------------------------------------ 5. the self-ensemble
@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('max_tile_batch', [16, 8])
def test_self_ensemble_merges_into_the_slab(monkeypatch, plain, max_tile_batch, fmt):
    x, plain_want, _ = plain[fmt]
    net = _net('x4')
    want = _want('x4', x, TS, PAD, self_ensemble=True)                         # (at the default split; the result does not depend on it)
    assert LB.first_difference(want, plain_want) is not None
    keep = net.max_tile_batch
    try:
        net.max_tile_batch = max_tile_batch
        _exchange(monkeypatch, net, x, 3, TS, PAD, (want,), f'self_ensemble max_tile_batch {max_tile_batch}', self_ensemble=True)
    finally:
        net.max_tile_batch = keep


# ------------------------------------------------------------------------------------------------------------------ 6. the x2 net
@pytest.mark.parametrize('fmt', FORMATS)
def test_x2_net(monkeypatch, fmt):
    """72x88 at 32/8, world 3: three tiles per rank, byte slab offsets that are multiples of 12 only."""
    x = _image(fmt, 1, 72, 88, seed=24)
    net = _net('x2')
    assert net.scale_factor == 2
    _exchange(monkeypatch, net, x, 3, 32, 8, (_want('x2', x, 32, 8, seed=24), _sliced(net, x, 32, 8)), 'x2 72x88')


# ------------------------------------------------------------------------------------------------------------------ 7. captured graphs
def test_graph_replay_copies_into_the_slab(monkeypatch, plain):
    """use_graph = True at world 2: `out.copy_(so)` into the slab view, first behind a capture (round 1), then behind a replay."""
    x, want, sliced = plain['f32']                                              # the eager canvases
    net = _net('x4')
    try:
        net.use_graph = True
        _exchange(monkeypatch, net, x, 2, TS, PAD, (want, sliced), 'use_graph')
    finally:
        net.use_graph = False
        net._graphs = {}


# ------------------------------------------------------------------------------------------------------------------ 8. a side stream
@pytest.mark.parametrize('fmt', FORMATS)
def test_on_a_side_stream(monkeypatch, plain, cuda_device, fmt):
    x, want, sliced = plain[fmt]
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    net = _net('x4')
    results = {}
    with torch.cuda.stream(side):
        for root_only in (False, True):
            loop = LB.Loopback(3)
            monkeypatch.setattr(fd, 'dist', loop)
            results[root_only] = (loop, LB.play(loop, lambda r: fd.test_tile_parallel(net, x, TS, PAD, root_only=root_only)))
            fd._exchanges.clear()
    side.synchronize()
    sizes = LB.payload_sizes(40, 56, TS, PAD, 3, 1, 3, 4)
    for root_only, (loop, got) in results.items():
        loop.assert_rounds_equal(lambda rank, call: sizes[rank])
        for r in range(3):
            if root_only and r > 0:
                assert got[r] is None
            else:
                for w in (want, sliced):
                    LB.assert_canvas(got[r], w, r, 3, f'side stream root_only={root_only}')


# ------------------------------------------------------------------------------------------------------------------ 9. geometry changes
@pytest.mark.parametrize('fmt', FORMATS)
def test_geometry_change_on_a_live_exchange(monkeypatch, plain, fmt):
    """Per rank 40x56, 24x24, 40x56 through the SAME `_exchange_for` entry: the TileExchange drops and rebuilds its buffers."""
    xa, want_a, _ = plain[fmt]
    xb = _image(fmt, 1, 24, 24, seed=22)
    want_b = _want('x4', xb, TS, PAD, seed=22)
    net = _net('x4')
    world = 3
    loop = LB.Loopback(world)
    monkeypatch.setattr(fd, 'dist', loop)

    def three(r):
        ex, out = fd._exchange_for(None), []
        for x in (xa, xb, xa):
            out.append(fd.test_tile_parallel(net, x, TS, PAD))
            assert fd._exchange_for(None) is ex
        return out
    got = LB.play(loop, three)
    sizes = [LB.payload_sizes(h, w, TS, PAD, world, 1, 3, 4) for h, w in ((40, 56), (24, 24), (40, 56))]
    assert max(sizes[0]) != max(sizes[1])                                       # another `cap`: new buffers
    loop.assert_rounds_equal(lambda rank, call: sizes[call][rank])
    for r in range(world):
        LB.assert_canvas(got[r][0], want_a, r, world, 'first 40x56')
        LB.assert_canvas(got[r][1], want_b, r, world, '24x24 in between')
        LB.assert_canvas(got[r][2], want_a, r, world, 'second 40x56')
        LB.assert_canvas(got[r][2], got[r][0], r, world, 'second 40x56 against the first')


# ------------------------------------------------------------------------------------------------------------------ 10. slab hygiene
@pytest.mark.parametrize('fmt', FORMATS)
def test_slab_hygiene(monkeypatch, plain, fmt):
    """World 3: the send slab prefilled with 0xFF bytes (round 2) and with 0x7F bytes (round 3).  The first sizes[rank] elements are the same
    bytes in both - no word of the payload is left unwritten or computed from the prefill - and the elements from sizes[rank] to `cap`
    still hold the prefill: no kernel writes into the unused tail."""
    x, want, _ = plain[fmt]
    net = _net('x4')
    world = 3
    classes = tiling.shape_classes(tiling.enumerate_tiles(40, 56, TS, PAD))
    sizes = LB.payload_sizes(40, 56, TS, PAD, world, 1, 3, 4)
    cap = max(sizes)
    assert sum(1 for n in sizes if n < cap) >= 2                                # tails exist
    fills, tgs = {1: 0xFF, 2: 0x7F}, {}

    def prefill(rank, k):
        if k in fills:
            ex = fd._exchange_for(None)
            ex.send_views(classes, 1, 3, 4, x.dtype, x.device)                 # the arguments `_tiled` passes
            tgs[(rank, k)] = ex._tg
            LB._bytes(ex._tg.send).fill_(fills[k])

    def check_same_buffers(rank):
        y = fd.test_tile_parallel(net, x, TS, PAD)
        k = len(loop.rounds) - 1
        assert k not in fills or fd._exchange_for(None)._tg is tgs[(rank, k)], 'the call built other buffers than the prefilled ones'
        return y
    loop = LB.Loopback(world)
    monkeypatch.setattr(fd, 'dist', loop)
    got = LB.play(loop, check_same_buffers, rounds=3, before=prefill)
    loop.assert_rounds_equal(lambda rank, call: sizes[rank])
    for r in range(world):
        LB.assert_canvas(got[r], want, r, world, 'prefilled slabs')
        first, a, b = (loop.recorded(r, round_=k) for k in range(3))
        n = sizes[r]
        assert a.numel() == b.numel() == cap
        for other, name in ((b, 'the 0x7F run'), (first, 'the run without prefill')):
            ne = LB._bytes(a[:n]) != LB._bytes(other[:n])
            assert not bool(ne.any()), (f'rank {r} of world {world} {fmt}: payload depends on the prefill, first at element '
                                        f'{int(torch.nonzero(ne)[0]) // a.element_size()} of {n} (0xFF run against {name})')
        for slab, fill in ((a, 0xFF), (b, 0x7F)):
            bad = LB._bytes(slab[n:]) != fill
            assert not bool(bad.any()), (f'rank {r} of world {world} {fmt}: the unused tail was written, first at element '
                                         f'{n + int(torch.nonzero(bad)[0]) // slab.element_size()} of {cap}')

"""CPU: the loopback stand-in of tests/loopback_dist.py is a faithful all-gather, and the method can fail.

The stand-in networks of tests/test_distributed_cpu.py (per-tile functions of every pixel and of the tile's shape) go through
`femasr_amd.distributed.test_tile_parallel` with the loopback in place of `torch.distributed`, worlds of 2, 3 and 8 ranks played one after
another in two rounds; every rank's canvas must be the single-process `test_tile` / `test_tile_u8`.  The same calls run over real gloo
groups in test_distributed_cpu.py; tests/test_gpu_tile_exchange.py uses the loopback for the real network on one GPU.

Geometries (tile 16, pad 4): 40x56 -> 12 tiles in 9 shape classes (at world 8 every rank owns 1-2 tiles; at worlds 2 and 3 every rank owns
none of the tiles of several classes: empty class views in its slab); 24x24 -> 4 tiles (at world 8 ranks 4-7 own nothing at all)."""
import pytest
import torch

import loopback_dist as LB
from femasr_amd import distributed as fd, tiling
from test_distributed_cpu import _make_net

TS, PAD = 16, 4
GEOMS = [(40, 56), (24, 24)]
_NET = []


def _net():
    if not _NET:                    # (the stand-in keeps no state between calls: one serves every rank)
        _NET.append(_make_net())
    return _NET[0]


@pytest.fixture(autouse=True)
def _fresh_exchanges():
    fd._exchanges.clear()
    yield
    fd._exchanges.clear()


def _images(h, w, batch=1):
    g = torch.Generator().manual_seed(100 * h + w)
    x = torch.rand((batch, 3, h, w), generator=g)
    xu8 = (x.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()
    return x, (xu8[0] if batch == 1 else xu8)            # (H,W,3): the CLI's data type


def test_partitions_are_the_ones_described():
    own = {(hw, world): tiling.assign(tiling.shape_classes(tiling.enumerate_tiles(*hw, TS, PAD)), world) for hw in GEOMS for world in (2, 3, 8)}
    count = lambda o: sum(len(tl) for tl in o.values())
    assert all(sum(count(o) for o in own[(40, 56), w]) == 12 and len(own[(40, 56), w][0]) == 9 for w in (2, 3, 8))
    assert all(1 <= count(o) <= 2 for o in own[(40, 56), 8])
    for w in (2, 3):
        assert all(sum(1 for tl in o.values() if not tl) >= 2 for o in own[(40, 56), w])          # empty class views on every rank
    assert [count(o) for o in own[(24, 24), 8]] == [1, 1, 1, 1, 0, 0, 0, 0]
    # the negative control below needs two ranks whose slabs differ
    assert LB.payload_sizes(40, 56, TS, PAD, 2, 1, 3, 4)[0] > 0 and LB.payload_sizes(40, 56, TS, PAD, 2, 1, 3, 4)[1] > 0


@pytest.mark.parametrize('world', [2, 3, 8])
@pytest.mark.parametrize('hw', GEOMS)
@pytest.mark.parametrize('root_only', [False, True])
def test_every_rank_rebuilds_the_single_process_canvas(monkeypatch, world, hw, root_only):
    net = _net()
    for x in _images(*hw):
        want = (net.test_tile_u8 if x.dtype == torch.uint8 else net.test_tile)(x, TS, PAD)
        loop = LB.Loopback(world)
        monkeypatch.setattr(fd, 'dist', loop)
        got = LB.play(loop, lambda r: fd.test_tile_parallel(net, x, TS, PAD, root_only=root_only))
        channel = 3
        sizes = LB.payload_sizes(*hw, TS, PAD, world, 1, channel, 4)
        loop.assert_rounds_equal(lambda rank, call: sizes[rank])
        for r in range(world):
            slab = loop.recorded(r)
            assert slab.numel() == max(max(sizes), 1) and slab.dtype == want.dtype              # one call per rank and round, `cap` elements
            if root_only and r > 0:
                assert got[r] is None
            else:
                LB.assert_canvas(got[r], want, r, world, f'{hw} root_only={root_only}')


def test_batched_uint8_and_first_round_is_not_the_answer(monkeypatch):
    """(2,40,56,3) bytes at world 3; and the method's premise: in round 1 rank 0 pastes rows nobody has produced yet (0xFF), so its canvas
    is NOT the result - only the second round's is."""
    net = _net()
    _, xu8 = _images(40, 56, batch=2)
    want = net.test_tile_u8(xu8, TS, PAD)
    loop = LB.Loopback(3)
    monkeypatch.setattr(fd, 'dist', loop)
    first = LB.play(loop, lambda r: fd.test_tile_parallel(net, xu8, TS, PAD), rounds=1)
    assert LB.first_difference(first[0], want) is not None and LB.first_difference(first[2], want) is None
    second = LB.play(loop, lambda r: fd.test_tile_parallel(net, xu8, TS, PAD), rounds=1)
    for r in range(3):
        LB.assert_canvas(second[r], want, r, 3, 'batch of 2')


@pytest.mark.parametrize('world,swap', [(2, (0, 1)), (3, (0, 2)), (8, (1, 6))])
def test_negative_control_swapped_rows_give_another_canvas(monkeypatch, world, swap):
    """A gather that hands rank a's slab out as rank b's (and the reverse) must be visible on every pasting rank, in both formats:
    a gather this harness could not tell from a wrong one would prove nothing."""
    net = _net()
    own = tiling.assign(tiling.shape_classes(tiling.enumerate_tiles(40, 56, TS, PAD)), world)
    assert [t.index for tl in own[swap[0]].values() for t in tl] != [t.index for tl in own[swap[1]].values() for t in tl]
    for x in _images(40, 56):
        want = (net.test_tile_u8 if x.dtype == torch.uint8 else net.test_tile)(x, TS, PAD)
        loop = LB.Loopback(world, swap=swap)
        monkeypatch.setattr(fd, 'dist', loop)
        got = LB.play(loop, lambda r: fd.test_tile_parallel(net, x, TS, PAD))
        for r in range(world):
            assert LB.first_difference(got[r], want) is not None, (world, r, x.dtype)
            with pytest.raises(AssertionError, match=f'rank {r} of world {world}'):
                LB.assert_canvas(got[r], want, r, world, 'swapped')


def test_loopback_refuses_ranks_that_disagree_on_cap_and_marks_unknown_rows():
    loop = LB.Loopback(2)
    loop.begin_round()
    loop.set_rank(0)
    out = torch.zeros(8)
    h = loop.all_gather_into_tensor(out, torch.arange(4.0), async_op=True)
    assert h.wait() and torch.equal(out[:4], torch.arange(4.0)) and bool(torch.isnan(out[4:]).all())       # 0xFF words: not yet known
    assert loop.all_gather_into_tensor(out, torch.arange(4.0)) is None                                       # call 1 of rank 0
    loop.set_rank(1)
    with pytest.raises(AssertionError):
        loop.all_gather_into_tensor(torch.zeros(6), torch.zeros(3))                                           # another cap than rank 0's
    loop.set_rank(1)
    o8 = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(AssertionError):
        loop.all_gather_into_tensor(o8, torch.zeros(4, dtype=torch.uint8))                                    # another format
    loop.set_rank(1)
    loop.all_gather_into_tensor(out, torch.full((4,), 7.0))
    assert torch.equal(out, torch.cat([torch.arange(4.0), torch.full((4,), 7.0)]))

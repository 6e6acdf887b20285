"""A loopback stand-in for `torch.distributed`: the ranks of a world of N played one after another in ONE process.

`femasr_amd.distributed` reaches its collectives through the module attribute `dist`; a test replaces that attribute with a
`Loopback` (pytest's own `monkeypatch.setattr(fd, 'dist', loop)`), sets the rank it plays and calls the product code as that rank.
The stand-in provides exactly what distributed.py uses: is_initialized, get_world_size, get_rank, all_gather_into_tensor.

The gather is "record, then replay".  Every call keeps a clone of the WHOLE send tensor under (rank, number of the call in this round)
and fills the receive buffer row by row: the caller's own row from its send tensor, every row some rank has recorded so far from the
most recent recording, every row nobody has produced yet with 0xFF bytes (fp32: a NaN, uint8: 255 - a premature read shows).  So a test
plays TWO rounds (`play`): the first records and its results are thrown away, the second runs with every row known.  The forward is
deterministic, so a rank's slab must be the same bytes in both rounds (`assert_rounds_equal`).

tests/test_loopback_dist_host.py holds this helper against the single-process result on host tensors and shows, with a loopback that
swaps two ranks' rows, that a wrong gather does not pass."""
import torch


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


class _Done:
    """The work handle of `async_op=True`: the loopback's collective is complete when the call returns."""

    def wait(self):
        return True


class Loopback:
    def __init__(self, world, swap=None):
        """swap=(a, b): the NEGATIVE CONTROL - rows a and b of every receive buffer change places (a gather that delivers rank a's slab as
        rank b's and the reverse)."""
        self.world, self.rank, self.swap = world, 0, swap
        self.rounds = []            # one {(rank, call number): clone of the send tensor} per round
        self._calls = 0

    # ------------------------------------------------------------------ what a test drives
    def begin_round(self):
        self.rounds.append({})

    def set_rank(self, rank):
        assert 0 <= rank < self.world
        self.rank, self._calls = rank, 0

    def recorded(self, rank, call=0, round_=-1):
        return self.rounds[round_][(rank, call)]

    def assert_rounds_equal(self, used=None):
        """Every (rank, call) of the last round was also made in the round before it, with the same bytes in its first
        `used(rank, call)` elements (default: the whole slab; the tail past a rank's payload is nobody's to define)."""
        prev, last = self.rounds[-2], self.rounds[-1]
        assert sorted(prev) == sorted(last) and last, f'the two rounds made different calls: {sorted(prev)} / {sorted(last)}'
        for (rank, call), slab in last.items():
            n = slab.numel() if used is None else used(rank, call)
            a, b = _bytes(prev[(rank, call)][:n]), _bytes(slab[:n])
            if not torch.equal(a, b):
                first = int(torch.nonzero(a != b)[0]) // slab.element_size()
                raise AssertionError(f'world {self.world} rank {rank} call {call} {slab.dtype}: the send slab differs between the two rounds, '
                                     f'first at element {first} of {n}')

    # ------------------------------------------------------------------ what femasr_amd.distributed calls
    def is_initialized(self):
        return True

    def get_world_size(self, group=None):
        return self.world

    def get_rank(self, group=None):
        return self.rank

    def all_gather_into_tensor(self, out, inp, group=None, async_op=False):
        assert self.rounds, 'begin_round() first'
        key = (self.rank, self._calls)
        self._calls += 1
        assert inp.dim() == 1 and out.dim() == 1 and out.dtype == inp.dtype and out.numel() == self.world * inp.numel(), \
            f'rank {self.rank}: receive buffer {tuple(out.shape)} {out.dtype} for {self.world} x send {tuple(inp.shape)} {inp.dtype}'
        for rnd in self.rounds:                                     # all ranks agree on `cap` (and the format) of the same call
            for (r, c), rec in rnd.items():
                assert c != key[1] or (rec.numel() == inp.numel() and rec.dtype == inp.dtype), \
                    f'call {c}: rank {r} sent {rec.numel()} {rec.dtype}, rank {self.rank} sends {inp.numel()} {inp.dtype}'
        self.rounds[-1][key] = inp.clone()
        rows = {}
        for r in range(self.world):
            if r == self.rank:
                rows[r] = inp
                continue
            rows[r] = next((rnd[(r, key[1])] for rnd in reversed(self.rounds) if (r, key[1]) in rnd), None)
        if self.swap is not None:
            a, b = self.swap
            rows[a], rows[b] = rows[b], rows[a]
        recv = out.view(self.world, -1)
        for r, row in rows.items():
            if row is None:
                _bytes(recv[r]).fill_(0xFF)
            else:
                recv[r].copy_(row)
        return _Done() if async_op else None


def play(loop, call, rounds=2, before=None):
    """`rounds` rounds of `call(rank)` for every rank in turn; before(rank, round number) runs first with the rank already set.
    Returns the last round's results, one per rank."""
    out = []
    for k in range(rounds):
        loop.begin_round()
        out = []
        for r in range(loop.world):
            loop.set_rank(r)
            if before is not None:
                before(r, k)
            out.append(call(r))
    return out


def payload_sizes(height, width, tile_size, tile_pad, world, batch, channel, scale):
    """Elements of every rank's payload for this geometry (what TileGather.sizes holds), from the partition alone."""
    from femasr_amd import tiling
    classes = tiling.shape_classes(tiling.enumerate_tiles(height, width, tile_size, tile_pad))
    return [sum(len(tl) * batch * channel * hw[0] * scale * hw[1] * scale for hw, tl in o.items()) for o in tiling.assign(classes, world, scale)]


def first_difference(got, want):
    """None when the tensors hold the same bits (NaNs included), else the coordinate of the first element that differs."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return ('shape/dtype', tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    a, b = got.contiguous(), want.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    ne = a != b
    if not bool(ne.any()):
        return None
    return tuple(int(v) for v in torch.nonzero(ne)[0])


def assert_canvas(got, want, rank, world, what):
    """Bit for bit; the message names the rank, the world size, the format and the first differing canvas coordinate."""
    d = first_difference(got, want)
    assert d is None, f'{what}: rank {rank} of world {world}, {want.dtype}: canvas differs from the single-process result, first at {d}'

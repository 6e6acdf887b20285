"""Guard-band arena of the kernel tests: every operand of a call in ONE allocation, at its exact size, between poison.

The caching allocator rounds every tensor up (512 bytes, megabytes for large ones) and packs tensors next to each other, so a
kernel that stores one tile past `out`, or loads past the last element of an input, passes a test that gives each operand a
tensor of its own.  Here the operands of one call are regions of one uint8 tensor that is filled with a repeating 4-byte poison:

  [ margin >= 1 MiB | region | >= 4 KiB poison | region | ... | margin >= 1 MiB ]

  * a region starts on a 256-byte boundary (what include/femasr_hip.h asks of a workspace and what torch gives a tensor) and
    has EXACTLY the size asked for: the byte behind it is poison;
  * kind 'in': holds the caller's data and must be unchanged after the call; 'out': poison before the call, may change;
    'scratch': as 'out', but its contents are never compared;
  * Arena.check(what), after the call and a synchronise, compares (on the arena's device) every byte outside the 'out' and
    'scratch' regions with its value before the call: a stray STORE anywhere within the margins is reported with the nearest
    region, the offset from that region's start and end (`end+0` is the first byte behind the region) and the number of bytes.

run_twice(fn) is the READ side: fn runs once per poison on identical inputs, and every 'out' region must come out bit-identical.
  0xFFFFFFFF  NaN as fp32, NaN in either half as fp16 / bf16, -1 as an integer;
  0x7F7F7F7F  3.39e38 as fp32 and in either half as bf16 (large and finite), a large positive integer; as fp16 either half is
              a NaN again (0x7F7F has fp16's exponent field all ones), of another sign and payload than 0xFFFF: an fp16 kernel
              that computes with it yields NaN in both runs, which the comparison with the reference catches.
An output element that was never written keeps its prefill and differs between the runs; so does an output that depends on a
byte outside its inputs - behind an input's last element, uninitialised scratch, the unwritten padding of a packed image.

What the method cannot see: an out-of-bounds LOAD whose value is discarded (a masked lane, a product with an exact zero that
the poison does not turn into NaN / Inf, a row that is computed and not stored) changes nothing and is not detected.  Finding it
would take a fault, and this project provokes none: every access a wrong kernel could plausibly make stays inside the margins.
No GPU-specific code: `device` may be 'cpu' (tests/test_guard_arena_host.py).
"""
import contextlib

import numpy as np
import torch

MARGIN = 1 << 20        # untouched bytes at each end of an arena
SEPARATOR = 4096        # least poison between two regions
ALIGN = 256             # region starts
POISONS = (0xFFFFFFFF, 0x7F7F7F7F)
KINDS = ('in', 'out', 'scratch')

_POISON = [POISONS[0]]  # poison of the arenas Plan.build makes (run_twice switches it)
_RECORD = []            # stack of lists: arenas built while a run_twice pass is recording
QUERIED = set()         # names of the library's size queries that sized a region (gpu_utils.q / qp)


class GuardError(AssertionError):
    pass


def _up(n, a):
    return (n + a - 1) // a * a


def _bytes(data):
    """Any torch tensor / numpy array -> flat uint8 torch tensor of its bytes (on its own device)."""
    t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
    return t.contiguous().reshape(-1).view(torch.uint8)


class Region:
    def __init__(self, arena, name, kind, off, nbytes):
        self.arena, self.name, self.kind, self.off, self.nbytes = arena, name, kind, off, nbytes
        self.compared = kind == 'out'       # run_twice compares it between the poisons (stays so once frozen as an input)

    @property
    def view(self):
        """The region's bytes (uint8 view into the arena)."""
        return self.arena.buf[self.off:self.off + self.nbytes]

    @property
    def ptr(self):
        return self.arena.buf.data_ptr() + self.off

    def as_(self, dtype, shape=(-1,)):
        """View of the region as `dtype` (the region's size must be a multiple of the element size)."""
        return self.view.view(dtype).reshape(shape)

    def __repr__(self):
        return f"{self.kind} region '{self.name}' ({self.nbytes} bytes at arena offset {self.off})"


class Arena:
    """One uint8 tensor of MARGIN + nbytes + MARGIN bytes (nbytes: room for the regions with their alignment and separators,
    Arena.room_for) filled with the repeating 4-byte `poison`."""

    def __init__(self, nbytes, device, poison):
        self.poison = int(poison) & 0xFFFFFFFF
        self.device = torch.device(device)
        total = _up(2 * MARGIN + int(nbytes), ALIGN)
        raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=self.device)
        skip = (-raw.data_ptr()) % ALIGN
        self.buf = raw[skip:skip + total]
        assert self.buf.data_ptr() % ALIGN == 0
        self.buf.view(torch.int32).fill_(self.poison - (1 << 32) if self.poison >= 1 << 31 else self.poison)
        self.regions = []
        self._next = MARGIN
        self._before = None
        if _RECORD:
            _RECORD[-1].append(self)

    @staticmethod
    def room_for(sizes):
        """nbytes that holds regions of these sizes, whatever the order."""
        return sum(_up(int(s), ALIGN) + SEPARATOR for s in sizes) + ALIGN

    def region(self, nbytes, kind, data=None, name=None):
        """Carve the next region; returns (device pointer, uint8 view).  'in': `data` (exactly nbytes bytes) is copied in."""
        assert kind in KINDS, kind
        assert self._before is None, 'region() after the first check(): carve every region first'
        nbytes = int(nbytes)
        off = _up(self._next, ALIGN)
        if off + nbytes + MARGIN > self.buf.numel():
            raise ValueError(f'arena of {self.buf.numel()} bytes has no room for {nbytes} more (next offset {off})')
        r = Region(self, name or f'#{len(self.regions)}', kind, off, nbytes)
        if kind == 'in':
            src = _bytes(data)
            assert src.numel() == nbytes, f"'{r.name}': data has {src.numel()} bytes, the region {nbytes}"
            r.view.copy_(src)
        else:
            assert data is None, "only an 'in' region takes data"
        self.regions.append(r)
        self._next = off + nbytes + SEPARATOR
        return r.ptr, r.view

    def add(self, name, kind, nbytes, data=None, compared=None):
        """region() that returns the Region object.  compared=False: an 'out' region whose contents may legitimately differ from run to
        run (guarded like any other, left out of run_twice's comparison; say why at the call)."""
        self.region(nbytes, kind, data, name)
        if compared is not None:
            self.regions[-1].compared = bool(compared) and kind == 'out'
        return self.regions[-1]

    def _arm(self):
        if self._before is None:
            self._before = self.buf.clone()

    def arm(self):
        """Record the bytes 'before the call' (check() does it on first use otherwise: call arm() once the inputs are in place)."""
        self._arm()
        return self

    def freeze(self, region):
        """An 'out' region whose contents are final (a packed weight image) becomes an 'in' region of the calls that follow; run_twice
        still compares it between the poisons.  A 'scratch' region frozen this way (a table of device addresses) is not compared."""
        self._arm()
        self._before[region.off:region.off + region.nbytes] = region.view
        region.kind = 'in'

    def _nearest(self, i):
        def dist(r):
            return 0 if r.off <= i < r.off + r.nbytes else (r.off - i if i < r.off else i - (r.off + r.nbytes) + 1)
        return min(self.regions, key=dist) if self.regions else None

    def check(self, what=''):
        """Every byte outside the 'out' / 'scratch' regions equals its value at arm() (synchronise first on a GPU)."""
        assert self._before is not None, 'check() without arm(): the bytes before the call were never recorded'
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
        diff = self.buf != self._before
        for r in self.regions:
            if r.kind != 'in':
                diff[r.off:r.off + r.nbytes] = False
        changed = int(diff.sum())
        if changed == 0:
            return
        first = int(torch.nonzero(diff)[0])
        r = self._nearest(first)
        if r is None:
            raise GuardError(f'{what}: {changed} guard byte(s) changed, the first at arena offset {first} (no region carved)')
        inside = r.off <= first < r.off + r.nbytes
        where = 'inside' if inside else ('before' if first < r.off else 'after')
        raise GuardError(f"{what}: {changed} byte(s) changed outside the writable regions; the first is {where} {r}: "
                         f"start{first - r.off:+d}, end{first - (r.off + r.nbytes):+d} "
                         f"(arena offset {first}, was 0x{int(self._before[first]):02x}, is 0x{int(self.buf[first]):02x})")

    def outs(self):
        return [r for r in self.regions if r.kind == 'out']


def new_arena(sizes, device='cuda'):
    """An arena with room for regions of `sizes`, filled with the poison of the current run_twice pass."""
    return Arena(Arena.room_for(sizes), device, _POISON[0])


@contextlib.contextmanager
def _pass(poison):
    prev = _POISON[0]
    _POISON[0] = poison
    _RECORD.append([])
    try:
        yield _RECORD[-1]
    finally:
        _RECORD.pop()
        _POISON[0] = prev


def run_twice(build_and_launch, what=''):
    """build_and_launch() builds its operands in arenas (new_arena, or the wrappers of tests/gpu_utils.py), launches and returns
    the caller's result; it must give the same inputs each time.  It runs once per poison; then
      (a) check() passes on every arena of either run,
      (b) the two runs made the same regions and every 'out' region is bit-identical between them.
    Returns the first run's result: (c), the comparison with the reference, is the caller's."""
    runs = []
    for p in POISONS:
        with _pass(p) as arenas:
            res = build_and_launch()
            assert arenas, f'{what}: no arena was built'
            for a in arenas:
                a.arm()
                a.check(f'{what} (poison 0x{p:08X})')
        runs.append((res, arenas))
    (res, a0), (_, a1) = runs
    assert len(a0) == len(a1), f'{what}: {len(a0)} arenas in the first run, {len(a1)} in the second'
    for x, y in zip(a0, a1):
        lx, ly = [(r.name, r.kind, r.compared, r.nbytes) for r in x.regions], [(r.name, r.kind, r.compared, r.nbytes) for r in y.regions]
        assert lx == ly, f'{what}: the two runs carved different regions: {lx} / {ly}'
        for rx, ry in zip(x.regions, y.regions):
            if not rx.compared or torch.equal(rx.view, ry.view):
                continue
            ne = rx.view != ry.view
            first, n = int(torch.nonzero(ne)[0]), int(ne.sum())
            still = (int((rx.view.view(torch.int32) == x.buf.view(torch.int32)[0]).sum()) if rx.nbytes % 4 == 0 else -1)
            raise GuardError(f"{what}: {rx} depends on the poison: {n} byte(s) differ between the runs with 0x{POISONS[0]:08X} and "
                             f"0x{POISONS[1]:08X}, the first at start{first:+d}, end{first - rx.nbytes:+d} "
                             f"({still} whole word(s) of it hold the first run's poison: never written, or copied from "
                             f"outside the inputs; the rest was computed from such bytes)")
    return res

"""x8 geometric self-ensemble (femasr_amd/ensemble.py, csrc/ensemble.hip) on one MI355X: what the two data-movement kernels
cost, beside the same arrays through stock torch, and what the option costs a whole tiled call.

    python tools/bench_self_ensemble.py [--batch 2] [--lr 272] [--scale 4] [--warmup 3] [--steps 10] [--repeats 7] [--image 1440] [--no-tile]
                                        [--out profiles/self_ensemble_bench.txt]

Kernels: device events around `steps` back-to-back native calls on preallocated buffers after warm-up, median of `repeats` with the
run-to-run spread ((max - min) / median): expand at a tile's input shape (batch x lr^2), merge at its output shape (batch x (scale lr)^2),
float32 (3 channels) and uint8.  Achieved bytes/s on the ALGORITHMIC traffic, 9 x element count x element size per call (expand reads one
and writes eight, merge reads eight and writes one).  Yardstick: the stock-torch restatement on the same arrays in the same process
(flip / transpose / contiguous per variant; inverse maps and sequential adds), timed the same way; its allocations come from torch's caching
allocator and are part of what a user of it pays.
Whole call: `test_tile_u8` on a seeded image^2 input at 240 / 16 with synthetic weights, option off and on, with the peak device memory of
each and the kernels' share of the call (tiles x (expand + merge) at the tile's shape over the call's time).
Seeded synthetic inputs; reads no reference and no oracle."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def events_ms(fn, warmup, steps, repeats):
    """(median ms per call, (max - min) / median over the repeats)."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med


def native_calls(x, ys, yt):
    """(expand, merge) closures over preallocated buffers: x the batch to expand, (ys, yt) eight results to merge."""
    import torch
    from femasr_amd import _lib
    from femasr_amd import ensemble as E
    lib = _lib.load()
    u8 = x.dtype == torch.uint8
    r, c = E._batch(x)
    xs, xt = E._pair(x, r, c)
    out = torch.empty_like(ys[0])
    stream = torch.cuda.current_stream().cuda_stream
    ex, mg = (lib.femasr_dihedral_expand_u8, lib.femasr_dihedral_merge_u8) if u8 else (lib.femasr_dihedral_expand, lib.femasr_dihedral_merge)
    p = _lib.ptr

    def expand():
        _lib.check(ex(stream, p(x), *E._native_dims(x), p(xs), p(xt)))

    def merge():
        _lib.check(mg(stream, p(ys), p(yt), *E._native_dims(out), p(out)))
    return expand, merge, (xs, xt, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--lr', type=int, default=272, help="a tile's input edge (240 + 2 * 16)")
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--image', type=int, default=1440)
    ap.add_argument('--no-tile', action='store_true', help='skip the whole test_tile_u8 call')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from femasr_amd import ensemble as E
    b, lr, s = a.batch, a.lr, a.scale
    hr = lr * s
    lines = [f'# tools/bench_self_ensemble.py on {torch.cuda.get_device_name(0)}: expand at {b} x {lr}x{lr}, merge at {b} x {hr}x{hr} (3 channels), warmup '
             f'{a.warmup}, steps {a.steps}, median of {a.repeats} and (max - min) / median (device events, back-to-back calls)',
             '# traffic: algorithmic, 9 x element count x element size per call; for orientation colorfix.hip reaches 2.0 - 2.4 TB/s on this chip']

    def say(line):
        lines.append(line)
        print(line, flush=True)
    g = torch.Generator().manual_seed(0)
    per_tile = {}
    for u8 in (False, True):
        def rnd(shape):
            return (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if u8 else torch.rand(shape, generator=g) * 2 - 1).cuda()
        x = rnd((b, lr, lr, 3) if u8 else (b, 3, lr, lr))
        ys = rnd((4, b, hr, hr, 3) if u8 else (4, b, 3, hr, hr))
        yt = rnd((4, b, hr, hr, 3) if u8 else (4, b, 3, hr, hr))
        expand, merge, keep = native_calls(x, ys, yt)
        expand(), merge()
        torch.cuda.synchronize()
        ts, tt = E.expand_torch(x)                                           # the two agree before anything is timed
        assert torch.equal(keep[0], ts) and torch.equal(keep[1], tt) and torch.equal(keep[2], E.merge_torch(ys, yt))
        del ts, tt
        name = 'uint8  ' if u8 else 'float32'
        for what, fn, ref, n in (('expand', expand, lambda: [E.forward_variant(x, k) for k in range(8)], x.numel()),
                                 ('merge ', merge, lambda: E.merge_torch(ys, yt), ys[0].numel())):
            ms, sp = events_ms(fn, a.warmup, a.steps, a.repeats)
            tms, tsp = events_ms(ref, a.warmup, a.steps, a.repeats)
            by = 9 * n * x.element_size()
            verdict = 'not slower' if ms <= tms * (1 + max(sp, tsp)) else 'SLOWER'
            say(f'{name} {what} {ms:8.4f} ms (spread {100 * sp:4.1f} %)  {by / 1e6:8.1f} MB algorithmic  {by / (ms * 1e-3) / 1e12:5.2f} TB/s   '
                f'stock torch {tms:8.4f} ms (spread {100 * tsp:4.1f} %): {tms / ms:5.1f}x the kernel, {verdict} than stock torch')
        if u8:                                                               # one tile's worth (batch 1) for the share of the whole call
            x1, y1s, y1t = x[:1].contiguous(), ys[:, :1].contiguous(), yt[:, :1].contiguous()
            e1, m1, keep1 = native_calls(x1, y1s, y1t)
            per_tile = events_ms(e1, a.warmup, a.steps, a.repeats)[0] + events_ms(m1, a.warmup, a.steps, a.repeats)[0]
            del x1, y1s, y1t, keep1
        del x, ys, yt, keep
        torch.cuda.empty_cache()
    if not a.no_tile:
        from femasr_amd import synth, tiling
        from femasr_amd.archs.femasr_arch import FeMaSRNet
        net = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=s)
        w = synth.fill_state_dict(net.state_dict(), 0, 'trained')
        net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        net = net.cuda().eval()
        n = a.image
        img = torch.randint(0, 256, (n, n, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
        tiles = len(tiling.enumerate_tiles(n, n, 240, 16))
        res = {}
        for on in (False, True):
            kw = {'self_ensemble': True} if on else {}
            net.test_tile_u8(img, 240, 16, **kw)                             # warm-up, and the allocator's pool for this mode
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ms, sp = events_ms(lambda: net.test_tile_u8(img, 240, 16, **kw), 0, 1, 3)
            res[on] = (ms, sp, torch.cuda.max_memory_allocated() / 2 ** 20)
        (off, osp, omem), (onn, nsp, nmem) = res[False], res[True]
        say(f'test_tile_u8 {n}x{n} (240 / 16, {tiles} tiles, synthetic weights): off {off:9.2f} ms (spread {100 * osp:.1f} %, peak {omem:8.1f} MiB), '
            f'self_ensemble=True {onn:9.2f} ms (spread {100 * nsp:.1f} %, peak {nmem:8.1f} MiB): {onn / off:.2f}x; expand + merge of {tiles} tiles at '
            f'{per_tile:.4f} ms each = {100 * tiles * per_tile / onn:.2f} % of the call')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

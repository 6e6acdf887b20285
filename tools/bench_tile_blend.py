"""The overlap-blend paste against the overlap-discard paste on the same tiles, on one MI355X: a 1440x1440 x4 canvas at tile_size 240,
tile_pad 16 (36 tiles, 9 shape classes; 5760x5760 output), fp32 NCHW and uint8 HWC.

    python tools/bench_tile_blend.py [--size 1440] [--tile_size 240] [--tile_pad 16] [--steps 20] [--repeats 5] [--no-network] [--out profiles/FILE.txt]

Kernel times: the tiles of every shape class (seeded random values: neither kernel's time depends on them), the address / geometry tables
and the paste's rectangles are built once; then device events around `steps` back-to-back calls on the current stream after a warm-up,
the median of `--repeats` such measurements.  "paste" is what the parent path does per canvas: zero the canvas, one femasr_paste_tiles
launch per shape class; "blend" is the ONE femasr_blend_tiles launch (no zeroing: every element is written).  Achieved bytes/s are over the
algorithmic traffic computed from the shapes: the canvas written once plus the bytes read (blend: every window whole; paste: the bodies;
the paste's zero fill is counted as a second canvas write).  Whole call (skipped with --no-network): FeMaSRNet.test_tile / test_tile_u8
on synthetic weights with `time_split`, blend off and on, the median `last_split_ms` of `--repeats` calls, and the peak device memory.
Reads neither the reference nor the oracle."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1440)
    ap.add_argument('--tile_size', type=int, default=240)
    ap.add_argument('--tile_pad', type=int, default=16)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-network', action='store_true')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()

    import torch
    from femasr_amd import _lib, synth, tiling
    from femasr_amd.archs.femasr_arch import _FP32, _U8, FeMaSRNet
    if not torch.cuda.is_available():
        raise SystemExit('bench_tile_blend needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    s, n_img, ts, pad = 4, args.size, args.tile_size, args.tile_pad
    tiling.check_blend(ts, pad)
    tiles = tiling.enumerate_tiles(n_img, n_img, ts, pad)
    classes = tiling.shape_classes(tiles)
    ny = nx = math.ceil(n_img / ts)
    ho = wo = n_img * s
    lines = [f'tile blend vs paste: {n_img}x{n_img} x{s} at ({ts}, {pad}): {len(tiles)} tiles, {len(classes)} shape classes, canvas {ho}x{wo}',
             f'device events around {args.steps} back-to-back calls, median of {args.repeats}']

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return statistics.median(ms), min(ms), max(ms)

    stream = torch.cuda.current_stream(dev).cuda_stream
    for fmt, name in ((_FP32, 'fp32 NCHW'), (_U8, 'uint8 HWC')):
        isz = fmt.dtype.itemsize
        g = torch.Generator().manual_seed(1)
        res = {}
        for hw, tl in classes.items():
            shape = tiling.tile_shape(fmt.dtype, len(tl), 3, hw[0] * s, hw[1] * s)
            res[hw] = (torch.rand(shape, generator=g) if isz == 4 else torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)).to(dev)
        canvas_b = torch.empty(tiling.tile_shape(fmt.dtype, 1, 3, ho, wo), dtype=fmt.dtype, device=dev)
        canvas_p = torch.empty_like(canvas_b)
        ptrs = [0] * len(tiles)
        pastes = []
        for hw, tl in classes.items():
            th, tw = hw[0] * s, hw[1] * s
            rects, hmax = [], 0
            for k, t in enumerate(tl):
                ptrs[t.index] = res[hw].data_ptr() + k * 3 * th * tw * isz
                ys, ye, xs, xe = t.out_src(s)
                rects += [ys, xs, t.y0 * s, t.x0 * s, ye - ys, xe - xs]
                hmax = max(hmax, ye - ys)
            pastes.append((res[hw], len(tl), th, tw, torch.tensor(rects, dtype=torch.int32, device=dev), hmax))
        tab = torch.tensor(ptrs, dtype=torch.int64, device=dev)
        geo = torch.tensor(tiling.blend_table(tiles, s), dtype=torch.int32, device=dev)
        bc = fmt.native_bc(1, 3)

        def blend():
            _lib.check(getattr(lib, fmt.blend)(stream, tab.data_ptr(), geo.data_ptr(), len(tiles), ny, nx, ts * s, *bc, ho, wo, canvas_b.data_ptr()))

        def paste():
            canvas_p.zero_()
            for blk, n, th, tw, rd, hmax in pastes:
                _lib.check(getattr(lib, fmt.paste)(stream, blk.data_ptr(), *bc, n, th, tw, rd.data_ptr(), hmax, ho, wo, canvas_p.data_ptr()))

        canvas_bytes = 3 * ho * wo * isz
        window_bytes = sum(3 * (t.in_hw[0] * s) * (t.in_hw[1] * s) * isz for t in tiles)
        for what, fn, traffic in (('blend', blend, canvas_bytes + window_bytes), ('paste', paste, 3 * canvas_bytes)):
            med, lo, hi = timed(fn)
            lines.append(f'{name:10s} {what}: {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})   algorithmic traffic {traffic / 1e6:7.1f} MB '
                         f'-> {traffic / (med * 1e-3) / 1e12:.2f} TB/s')
        torch.cuda.synchronize(dev)
        del res, canvas_b, canvas_p, pastes

    if not args.no_network:
        net = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=s)
        w = synth.fill_state_dict(net.state_dict(), 0, 'trained')
        net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        net.num_streams = 3
        net = net.to(dev).eval()
        net.time_split = True
        x = torch.from_numpy(synth.synth_input(10, (1, 3, n_img, n_img))).to(dev)
        u8 = (x[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
        lines.append(f'whole call on synthetic weights (time_split; median of {args.repeats} calls after one warm-up): compute / gather / paste-or-blend ms')
        for name, fn, img in (('test_tile', net.test_tile, x), ('test_tile_u8', net.test_tile_u8, u8)):
            for blend in (False, True):
                torch.cuda.synchronize(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                splits = []
                for i in range(args.repeats + 1):
                    y = fn(img, ts, pad, blend=blend)
                    sp = net.last_split_ms
                    del y
                    if i:
                        splits.append(sp)
                med = {k: statistics.median(sp[k] for sp in splits) for k in ('compute', 'gather', 'paste')}
                total = sum(med.values())
                lines.append(f'{name:13s} blend={blend!s:5s}: {med["compute"]:8.2f} / {med["gather"]:5.2f} / {med["paste"]:6.3f}   last step = '
                             f'{100 * med["paste"] / total:.2f} % of {total:.2f} ms   peak device memory {torch.cuda.max_memory_allocated(dev) / 2 ** 20:.0f} MiB')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

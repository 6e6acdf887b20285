"""The final resample of the output image (femasr_amd/resample.py, csrc/resample.hip) on one MI355X box.

    python tools/bench_resample.py [--skip-net] [--repeats 5] [--out profiles/resample_bench.txt]

Content comes from tests/golden/testset_all.npz only: a 1440x1440 input tiled from one of its images and, as the network's 5760x5760 result,
its x4 PIL-bicubic upscale (RGB; RGBA with a synthetic alpha plane).
(a) The kernel on the 5760x5760x3 canvas -> 4320x4320 (x3 of the input) and on 5760x5760x4 -> 1440x1440 (the input's own size), against the
    composition the package offered before: split into float64 planes, femasr_amd.resize.imresize (both cases are one scalar scale with
    ceil(n s) the target, so it can express them), clip, round, interleave in stock torch.  Outputs checked equal first.  Device events
    around back-to-back calls, the two legs alternating in one process, median and (max - min) / median over the repeats; bytes/s on the
    algorithmic traffic (the image read once, the result written once).
(b) Peak device memory of one call of each above what is allocated before it (the input and, for the kernel, nothing else: its output is
    all it allocates).
(c) FeMaSRNet.test_tile_u8 of the 1440x1440 input (synthetic weights, tile 240, pad 16) alone and followed by the resample to 4320x4320,
    alternating, host clock around a synchronised call."""
import argparse
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_channels import synthetic_alpha      # noqa: E402
from bench_png_io import testset                # noqa: E402


def composition(x, scale):
    """The parent commit's way to the same bytes: uint8 (H,W,C) -> float64 planes -> resize.imresize -> clip, round, interleave."""
    import torch
    from femasr_amd import resize
    planes = x.permute(2, 0, 1).to(torch.float64)
    return torch.round(resize.imresize(planes, scale).clamp_(0, 255)).to(torch.uint8).permute(1, 2, 0).contiguous()


def alternating_ms(legs, warmup, steps, repeats):
    """{name: (median ms per call, spread)} of device-event timings, the legs taking turns within every repeat."""
    import torch
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in legs}
    for _ in range(repeats):
        for n, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[n].append(e0.elapsed_time(e1) / steps)
    return {n: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for n, v in ms.items()}


def peak_above(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-net', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from femasr_amd import resample as RS
    lines = [f'# tools/bench_resample.py on {torch.cuda.get_device_name(0)}; content: tests/golden/testset_all.npz, synthetic alpha']

    def say(line):
        lines.append(line)
        print(line, flush=True)

    src = np.array(Image.open(io.BytesIO(testset()['OST_020.png'])).convert('RGB'))
    lr = np.ascontiguousarray(np.tile(src, (4, 4, 1))[:1440, :1440])
    sr = np.array(Image.fromarray(lr, 'RGB').resize((5760, 5760), Image.BICUBIC))
    al = np.array(Image.fromarray(synthetic_alpha(1440, 1440), 'L').resize((5760, 5760), Image.BICUBIC))
    rgb = torch.from_numpy(sr).cuda()
    rgba = torch.from_numpy(np.concatenate([sr, al[..., None]], axis=2)).cuda()
    say(f'(a) kernel against the float64-plane composition, alternating, device events, median of {a.repeats} x 5 calls; (b) peak device memory of one call above its input')
    for name, x, o, scale in (('5760x5760x3 -> 4320x4320', rgb, 4320, 0.75), ('5760x5760x4 -> 1440x1440', rgba, 1440, 0.25)):
        got, ref = RS.resample_u8(x, o, o), composition(x, scale)
        same = torch.equal(got, ref)
        del got, ref
        out = torch.empty((o, o, x.shape[2]), dtype=torch.uint8, device='cuda')
        t = alternating_ms({'kernel': lambda: RS.resample_u8(x, o, o, out=out), 'composition': lambda: composition(x, scale)}, 2, 5, a.repeats)
        del out
        nbytes = x.numel() + o * o * x.shape[2]
        pk, pc = peak_above(lambda: RS.resample_u8(x, o, o)), peak_above(lambda: composition(x, scale))
        (km, ks), (cm, cs) = t['kernel'], t['composition']
        say(f'  {name}: kernel {km:7.3f} ms (spread {100 * ks:4.1f} %), {nbytes / 1e6:6.1f} MB algorithmic, {nbytes / (km * 1e-3) / 1e12:5.2f} TB/s;  '
            f'composition {cm:8.3f} ms (spread {100 * cs:4.1f} %) = {cm / km:5.1f}x the kernel, equal output: {same}')
        say(f'  {"":{len(name)}s}  peak memory above the input ({x.numel() / 2**20:6.1f} MiB): kernel {pk / 2**20:7.1f} MiB (its output: {o * o * x.shape[2] / 2**20:6.1f} MiB), '
            f'composition {pc / 2**20:8.1f} MiB')
    del rgb, rgba
    torch.cuda.empty_cache()

    if not a.skip_net:
        from femasr_amd import synth
        from femasr_amd.archs.femasr_arch import FeMaSRNet
        model = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4)
        w = synth.fill_state_dict(model.state_dict(), 3, 'trained')
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        model.num_streams = 3
        model = model.cuda().eval()
        x = torch.from_numpy(lr).cuda()
        legs = {'test_tile_u8 alone': lambda: model.test_tile_u8(x, 240, 16),
                'test_tile_u8 + resample_u8 to 4320x4320': lambda: RS.resample_u8(model.test_tile_u8(x, 240, 16), 4320, 4320)}
        wall = {n: [] for n in legs}
        for rep in range(a.repeats + 1):                   # (the first round warms up and is not counted)
            for n, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                del r
                if rep:
                    wall[n].append(dt)
        say(f'(c) 1440x1440 RGB through FeMaSRNet.test_tile_u8 (synthetic weights, tile 240, pad 16, 3 streams), alternating, {a.repeats} counted calls each, host clock')
        for n, v in wall.items():
            say(f'  {n:42s}: median {1e3 * statistics.median(v):8.1f} ms (min {1e3 * min(v):8.1f}, max {1e3 * max(v):8.1f})')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

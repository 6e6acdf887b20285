"""Gray / gray + alpha / RGBA through inference (femasr_amd/channels.py, csrc/channels.hip, csrc/png_filter.hip) on one MI355X box.

    python tools/bench_channels.py [--skip-cli] [--repeats 5] [--cli-repeats 2] [--out profiles/channels_bench.txt]

Content comes from tests/golden/testset_all.npz only: a 1440x1440 input tiled from one of its images with a synthetic alpha plane (a soft
disc with a hard-edged hole), and as the network's 5760x5760 result its x4 PIL-bicubic upscale.
(a) The kernels at 5760x5760 from the 1440x1440 input: split (C = 1, 2, 4), merge with both alpha sources (channels 2, 4), the gray and the
    bicubic alpha alone, the row filters for C = 1, 2, 4.  Device events around back-to-back launches, median and (max - min) / median;
    bytes/s on the algorithmic traffic (every input read once, the output written once).  Beside each a stock-torch restatement on the same
    GPU, checked equal first (the bicubic through femasr_amd.resize.imresize: torch has no MATLAB resize).
(b) The CLI over the 38 testset images as RGBA files, --synthetic-seed, every run a fresh child process, alternating: without the flag (the
    parent commit's behaviour: opaque RGB files), --keep-format --alpha bicubic and --keep-format --alpha network; each with --io-threads 0
    and 8.
Thread counts are the arguments above, never derived from the machine."""
import argparse
import io
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_png_io import events_ms, testset      # noqa: E402


def synthetic_alpha(h, w):
    import numpy as np
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot((y - h / 2) / (h / 2), (x - w / 2) / (w / 2))
    a = np.clip((1.0 - r) * 4.0, 0.0, 1.0) * 255.0
    a[(abs(y - h / 2) < h / 8) & (abs(x - w / 2) < w / 8)] = 0.0
    return np.rint(a).astype(np.uint8)


def gray_torch(rgb):
    import torch
    v = rgb.to(torch.int32)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16).to(torch.uint8)


def alpha_torch(alpha, s):
    import torch
    from femasr_amd import resize
    return torch.round(resize.imresize(alpha.to(torch.float64), s).clamp_(0, 255)).to(torch.uint8)


def split_torch(x):
    c = x.shape[-1]
    rgb = x[..., :3].contiguous() if c == 4 else x[..., :1].expand(-1, -1, 3).contiguous()
    return rgb, (x[..., c - 1].contiguous() if c != 1 else None)


def merge_torch(rgb, a_sr, channels):
    import torch
    return torch.cat([rgb if channels == 4 else gray_torch(rgb)[..., None], a_sr[..., None]], dim=2)


def filter_image_torch(u8):
    """pngio.filter_image restated with stock torch ops on the device (int16 planes)."""
    import torch
    H, W, C = u8.shape
    x = u8.reshape(H, C * W).to(torch.int16)
    a, b, c = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :-C]
    p = a + b - c
    pa, pb, pc = (p - a).abs(), (p - b).abs(), (p - c).abs()
    paeth = torch.where((pa <= pb) & (pa <= pc), a, torch.where(pb <= pc, b, c))
    res = torch.stack([x, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth) & 255])
    cost = torch.minimum(res, 256 - res).sum(dim=2, dtype=torch.int32)
    kind = cost.argmin(dim=0)
    out = torch.empty((H, 1 + C * W), dtype=torch.uint8, device=u8.device)
    out[:, 0] = kind.to(torch.uint8)
    out[:, 1:] = res.gather(0, kind.view(1, H, 1).expand(1, H, C * W))[0].to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-cli', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--cli-repeats', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from femasr_amd import channels as CH
    from femasr_amd import pngio
    lines = [f'# tools/bench_channels.py on {torch.cuda.get_device_name(0)}; Pillow {Image.__version__}; content: tests/golden/testset_all.npz, '
             'synthetic alpha']

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def row(name, fn, ref, nbytes, same):
        ms, sp = events_ms(fn, 3, 20, a.repeats)
        tms, tsp = events_ms(ref, 1, 3, 3)
        say(f'  {name:34s}: kernel {ms:7.4f} ms (spread {100 * sp:4.1f} %), {nbytes / 1e6:6.1f} MB algorithmic, {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s;  '
            f'stock torch {tms:8.3f} ms (spread {100 * tsp:4.1f} %) = {tms / ms:6.1f}x the kernel, equal output: {same}')

    files = testset()
    src = np.array(Image.open(io.BytesIO(files['OST_020.png'])).convert('RGB'))
    lr = np.ascontiguousarray(np.tile(src, (4, 4, 1))[:1440, :1440])
    sr = np.array(Image.fromarray(lr, 'RGB').resize((5760, 5760), Image.BICUBIC))
    al = synthetic_alpha(1440, 1440)
    s = 4
    say('(a) kernels, 1440x1440 -> 5760x5760: device events, median of %d x 20 back-to-back launches' % a.repeats)
    rgba = torch.from_numpy(np.concatenate([lr, al[..., None]], axis=2)).cuda()
    big = torch.from_numpy(sr).cuda()
    for c in (1, 2, 4):                                    # split, at the size it runs at (the input) and at the output's for the rate
        for name, x in ((f'split C={c} 1440x1440', rgba[..., 4 - c:].contiguous()),
                        (f'split C={c} 5760x5760', torch.cat([big, big[..., :1]], dim=2)[..., 4 - c:].contiguous())):
            got, ref = CH.split_u8(x), split_torch(x)
            same = torch.equal(got[0], ref[0]) and (c == 1 or torch.equal(got[1], ref[1]))
            row(name, lambda: CH.split_u8(x), lambda: split_torch(x), x.numel() // c * (c + 3 + (c != 1)), same)
            del got, ref
    alpha = torch.from_numpy(al).cuda()
    net_a = torch.from_numpy(np.repeat(np.array(Image.fromarray(al, 'L').resize((5760, 5760), Image.BICUBIC))[..., None], 3, axis=2)).cuda()
    npx = 5760 * 5760
    out1 = torch.empty((5760, 5760), dtype=torch.uint8, device='cuda')
    row('gray_u8 5760x5760', lambda: CH.gray_u8(big, out=out1), lambda: gray_torch(big), npx * 4, torch.equal(CH.gray_u8(big), gray_torch(big)))
    row('alpha_bicubic_u8 x4', lambda: CH.alpha_bicubic_u8(alpha, s, out=out1), lambda: alpha_torch(alpha, s), npx + alpha.numel(),
        torch.equal(CH.alpha_bicubic_u8(alpha, s), alpha_torch(alpha, s)))
    for ch in (2, 4):
        out = torch.empty((5760, 5760, ch), dtype=torch.uint8, device='cuda')
        row(f'merge_u8 channels={ch}, bicubic alpha', lambda: CH.merge_u8(big, alpha, ch, s, out=out), lambda: merge_torch(big, alpha_torch(alpha, s), ch),
            npx * (3 + ch) + alpha.numel(), torch.equal(CH.merge_u8(big, alpha, ch, s), merge_torch(big, alpha_torch(alpha, s), ch)))
        row(f'merge_u8 channels={ch}, network alpha', lambda: CH.merge_u8(big, net_a, ch, out=out), lambda: merge_torch(big, gray_torch(net_a), ch),
            npx * (6 + ch), torch.equal(CH.merge_u8(big, net_a, ch), merge_torch(big, gray_torch(net_a), ch)))
        del out
    full = CH.merge_u8(big, alpha, 4, s)
    del net_a, out1
    torch.cuda.empty_cache()
    for c in (1, 2, 4):
        x = full[..., 4 - c:].contiguous()
        out = pngio.filter_image_gpu(x)
        same = torch.equal(out, filter_image_torch(x))
        row(f'png filter C={c} 5760x5760, adaptive', lambda: pngio.filter_image_gpu(x, out=out), lambda: filter_image_torch(x), x.numel() + out.numel(), same)
        del x, out
        torch.cuda.empty_cache()

    if not a.skip_cli:
        tmp = tempfile.mkdtemp(prefix='channels_bench_')
        try:
            folder = os.path.join(tmp, 'in')
            os.makedirs(folder)
            for n, raw in files.items():
                im = np.array(Image.open(io.BytesIO(raw)).convert('RGB'))
                Image.fromarray(np.concatenate([im, synthetic_alpha(*im.shape[:2])[..., None]], axis=2), 'RGBA').save(os.path.join(folder, os.path.splitext(n)[0] + '.png'))
            runs = [(f'{label}, --io-threads {t}', extra + ['--io-threads', str(t)]) for t in (0, 8)
                    for label, extra in (('without the flag (RGB out)', []), ('--keep-format --alpha bicubic', ['--keep-format']),
                                         ('--keep-format --alpha network', ['--keep-format', '--alpha', 'network']))]
            wall = {r[0]: [] for r in runs}
            for rep in range(a.cli_repeats + 1):                   # (the first round warms the file cache and is not counted)
                for label, extra in runs:
                    dst = os.path.join(tmp, 'out')
                    shutil.rmtree(dst, ignore_errors=True)
                    t0 = time.perf_counter()
                    subprocess.run([sys.executable, '-m', 'femasr_amd.inference', '-i', folder, '-o', dst, '--synthetic-seed', '3'] + extra, cwd=ROOT,
                                   env=dict(os.environ, PYTHONPATH=ROOT), check=True, stdout=subprocess.DEVNULL, timeout=900)
                    dt = time.perf_counter() - t0
                    assert len(os.listdir(dst)) == len(files)
                    if rep:
                        wall[label].append(dt)
            say(f'(b) python -m femasr_amd.inference over the {len(files)} testset images as RGBA PNGs, --synthetic-seed 3, fresh child process each, '
                f'alternating, {a.cli_repeats} counted runs each (process start, weights and model build included)')
            for label, v in wall.items():
                say(f'  {label:46s}: ' + ', '.join(f'{x:6.2f} s' for x in v) + f'   median {statistics.median(v):6.2f} s')
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

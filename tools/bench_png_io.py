"""Fast PNG output (femasr_amd/pngio.py, csrc/png_filter.hip) on one MI355X box: the filter kernel, one image's encode, the CLI.

    python tools/bench_png_io.py [--baseline DIR] [--skip-cli] [--repeats 5] [--cli-repeats 2] [--out profiles/png_io_bench.txt]

Content comes from tests/golden/testset_all.npz only (x4 PIL-bicubic upscales of its images, as the network's outputs are x4 images).
(a) The kernel at 2048x1024 and 5760x5760, adaptive: device events around back-to-back launches, median and (max - min) / median; bytes/s on
    the algorithmic traffic (the image read once, the filtered stream written once); beside it a stock-torch restatement on the GPU and the
    D2H copy of the kernel's own output into pinned memory - the step the kernel has to disappear beside.
(b) One image: wall time of filter + copy + encode_png at threads 1 / 4 / 8 / 16 against Image.save of the same pixels at the same level,
    interleaved, with the file sizes.
(c) The CLI over the 38 testset images with --synthetic-seed, every run a fresh child process: the tree at --baseline (a checkout of the parent
    commit with its library built), this tree with --io-threads 0 and with --io-threads 8, alternating.  The first two run the same code and
    show the spread; the third is the figure.
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


def testset():
    import numpy as np
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'testset_all.npz'), allow_pickle=False)
    return {str(n): g['file_bytes'][int(g['file_off'][i]):int(g['file_off'][i + 1])].tobytes() for i, n in enumerate(g['names'])}


def upscaled(raw, noise=0):
    import numpy as np
    from PIL import Image
    im = Image.open(io.BytesIO(raw)).convert('RGB')
    img = np.array(im.resize((im.width * 4, im.height * 4), Image.BICUBIC))
    if noise:
        img = np.clip(img.astype(np.int16) + np.random.RandomState(0).randint(-noise, noise + 1, img.shape), 0, 255).astype(np.uint8)
    return img


def events_ms(fn, warmup, steps, repeats):
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


def filter_rows_torch(u8):
    """pngio.filter_rows restated with stock torch ops on the device (int16 planes; the yardstick of (a))."""
    import torch
    H, W = u8.shape[:2]
    x = u8.reshape(H, 3 * W).to(torch.int16)
    a, b, c = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b[1:] = x[:-1]
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = (p - a).abs(), (p - b).abs(), (p - c).abs()
    paeth = torch.where((pa <= pb) & (pa <= pc), a, torch.where(pb <= pc, b, c))
    res = torch.stack([x, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth) & 255])
    cost = torch.minimum(res, 256 - res).sum(dim=2, dtype=torch.int32)
    kind = cost.argmin(dim=0)                                      # (ties: checked against the kernel below on this content)
    out = torch.empty((H, 1 + 3 * W), dtype=torch.uint8, device=u8.device)
    out[:, 0] = kind.to(torch.uint8)
    out[:, 1:] = res.gather(0, kind.view(1, H, 1).expand(1, H, 3 * W))[0].to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--baseline', default=None, help="a checkout of the parent commit with its library built: the CLI baseline of (c)")
    ap.add_argument('--skip-cli', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--cli-repeats', type=int, default=2)
    ap.add_argument('--level', type=int, default=6)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from femasr_amd import pngio
    lines = [f'# tools/bench_png_io.py on {torch.cuda.get_device_name(0)}; zlib {__import__("zlib").ZLIB_RUNTIME_VERSION}, Pillow {Image.__version__}, '
             f'level {a.level}; content: x4 PIL-bicubic upscales of tests/golden/testset_all.npz']

    def say(line):
        lines.append(line)
        print(line, flush=True)
    files = testset()
    small = upscaled(files['00003.png'])                           # 1024 x 2048
    big_src = upscaled(files['OST_020.png'])
    big = np.ascontiguousarray(np.tile(big_src, (4, 3, 1))[:5760, :5760])

    say('(a) femasr_png_filter_rgb8, adaptive: device events, median of %d x 20 back-to-back launches' % a.repeats)
    for name, img in (('2048x1024', small), ('5760x5760', big)):
        t = torch.from_numpy(img).cuda()
        out = pngio.filter_rows_gpu(t)
        ref = filter_rows_torch(t)
        same = torch.equal(out, ref)
        pin = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
        ms, sp = events_ms(lambda: pngio.filter_rows_gpu(t, out=out), 3, 20, a.repeats)
        tms, tsp = events_ms(lambda: filter_rows_torch(t), 1, 2, 3)
        cms, csp = events_ms(lambda: pin.copy_(out, non_blocking=True), 2, 5, a.repeats)
        by = t.numel() + out.numel()
        kinds = np.bincount(out[:, 0].cpu().numpy(), minlength=5).tolist()
        say(f'  {name}: kernel {ms:7.4f} ms (spread {100 * sp:4.1f} %), {by / 1e6:6.1f} MB algorithmic, {by / (ms * 1e-3) / 1e12:5.2f} TB/s;  '
            f'stock torch {tms:8.3f} ms (spread {100 * tsp:4.1f} %) = {tms / ms:6.1f}x the kernel, equal output: {same};  D2H of the output '
            f'{cms:7.3f} ms (spread {100 * csp:4.1f} %, {out.numel() / (cms * 1e-3) / 1e9:5.1f} GB/s): the kernel is {100 * ms / cms:5.1f} % of its copy;  '
            f'rows per filter type 0..4: {kinds}')
        del t, out, ref, pin
        torch.cuda.empty_cache()

    say(f'(b) one image, wall time, best and median of {a.repeats}, interleaved; writer = filter kernel + D2H + encode_png(threads), PIL = D2H + Image.save')
    for name, img in (('2048x1024 smooth', small), ('2048x1024 +-2 noise', upscaled(files['00003.png'], 2)), ('2560x1664', big_src)):
        t = torch.from_numpy(img).cuda()
        H, W = img.shape[:2]
        pin = torch.empty((H, 1 + 3 * W), dtype=torch.uint8, pin_memory=True)
        pools = {n: ThreadPoolExecutor(n) for n in (1, 4, 8, 16)}
        times, sizes = {k: [] for k in ('PIL', 1, 4, 8, 16)}, {}
        for _ in range(a.repeats):
            for k in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == 'PIL':
                    buf = io.BytesIO()
                    Image.fromarray(t.cpu().numpy(), 'RGB').save(buf, 'PNG', compress_level=a.level)
                    data = buf.getvalue()
                else:
                    pin.copy_(pngio.filter_rows_gpu(t), non_blocking=True)
                    torch.cuda.synchronize()
                    data = pngio.encode_png(pin.numpy(), W, H, a.level, pools[k])
                times[k].append(time.perf_counter() - t0)
                sizes[k] = len(data)
        assert np.array_equal(np.array(Image.open(io.BytesIO(data)).convert('RGB')), img)
        for p in pools.values():
            p.shutdown()
        base = statistics.median(times['PIL'])
        say(f'  {name}: ' + ';  '.join(f'{k if k == "PIL" else "threads " + str(k)}: best {min(v) * 1e3:7.1f} ms, median {statistics.median(v) * 1e3:7.1f} ms'
                                       f' ({base / statistics.median(v):4.1f}x), {sizes[k]} B' for k, v in times.items()))
        del t, pin

    if not a.skip_cli:
        tmp = tempfile.mkdtemp(prefix='png_io_bench_')
        try:
            src = os.path.join(tmp, 'in')
            os.makedirs(src)
            for n, raw in files.items():
                with open(os.path.join(src, n), 'wb') as f:
                    f.write(raw)
            runs = [('this tree, --io-threads 0', ROOT, ['--io-threads', '0']), ('this tree, --io-threads 8', ROOT, ['--io-threads', '8'])]
            if a.baseline:
                runs.insert(0, ('parent commit', os.path.abspath(a.baseline), []))
            wall = {r[0]: [] for r in runs}
            for rep in range(a.cli_repeats + 1):                   # (the first round warms the file cache and is not counted)
                for label, tree, extra in runs:
                    dst = os.path.join(tmp, 'out')
                    shutil.rmtree(dst, ignore_errors=True)
                    env = dict(os.environ, PYTHONPATH=tree)
                    t0 = time.perf_counter()
                    subprocess.run([sys.executable, '-m', 'femasr_amd.inference', '-i', src, '-o', dst, '--synthetic-seed', '3'] + extra, cwd=tree, env=env,
                                   check=True, stdout=subprocess.DEVNULL, timeout=900)
                    dt = time.perf_counter() - t0
                    assert len(os.listdir(dst)) == len(files)
                    if rep:
                        wall[label].append(dt)
            say(f'(c) python -m femasr_amd.inference over the {len(files)} testset images, --synthetic-seed 3, fresh child process each, alternating, '
                f'{a.cli_repeats} counted runs each (process start, weights and model build included)')
            for label, v in wall.items():
                say(f'  {label:28s}: ' + ', '.join(f'{x:6.2f} s' for x in v) + f'   median {statistics.median(v):6.2f} s')
            first = statistics.median(wall[runs[0][0]])
            say(f'  --io-threads 8 against {runs[0][0]}: {first / statistics.median(wall["this tree, --io-threads 8"]):.2f}x')
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

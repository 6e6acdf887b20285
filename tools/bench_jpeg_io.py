"""Fast JPEG output (femasr_amd/jpegio.py, csrc/jpeg_dct.hip) on one MI355X box: the coefficient kernel, one image's file, the CLI.

    python tools/bench_jpeg_io.py [--quality 90] [--subsampling 420] [--threads 1 4 8 16] [--baseline DIR] [--skip-cli] [--repeats 5]
                                  [--cli-repeats 2] [--out profiles/jpeg_io_bench.txt]

Content comes from tests/golden/testset_all.npz only (x4 PIL-bicubic upscales of its images, as the network's outputs are x4 images).
(a) The kernel at 2048x1024x3 and 5760x5760x3: device events around back-to-back launches, median and (max - min) / median; bytes/s on the
    algorithmic traffic (the image read once, the int16 planes written once); beside it the D2H copy of the kernel's own output into pinned
    memory - the step the kernel has to disappear beside.
(b) One image: wall time of kernel + copy + encode_jpeg at each thread count against D2H + Image.save(quality=Q, subsampling=S) of the same
    bytes at the same settings, interleaved in one process, with the file sizes.
(c) The CLI over the 12 .jpg images of the testset with --synthetic-seed at --io-threads 8, every run a fresh child process: without and with
    --jpeg-quality 90, alternating (and, with --baseline DIR, a checkout of the parent commit with its library built, without the flag: the
    same code as this tree without the flag, so the pair shows the spread).
Thread counts are arguments (capped at 16), never derived from the machine."""
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

from tools.bench_png_io import events_ms, testset, upscaled      # noqa: E402  (the same content and the same timer as the PNG tool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--subsampling', choices=['420', '444'], default='420')
    ap.add_argument('--threads', type=int, nargs='+', default=[1, 4, 8, 16])
    ap.add_argument('--baseline', default=None, help='a checkout of the parent commit with its library built: the CLI baseline of (c)')
    ap.add_argument('--skip-cli', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--cli-repeats', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from femasr_amd import jpegio, pngio
    threads = sorted({pngio.clamp_threads(n) for n in a.threads})
    q, ss = a.quality, a.subsampling
    pil_ss = 0 if ss == '444' else 2
    lines = [f'# tools/bench_jpeg_io.py on {torch.cuda.get_device_name(0)}; Pillow {Image.__version__}; quality {q}, subsampling {ss}; '
             f'content: x4 PIL-bicubic upscales of tests/golden/testset_all.npz']

    def say(line):
        lines.append(line)
        print(line, flush=True)
    files = testset()
    small = upscaled(files['00003.png'])                           # 1024 x 2048
    big_src = upscaled(files['OST_020.png'])
    big = np.ascontiguousarray(np.tile(big_src, (4, 3, 1))[:5760, :5760])

    say('(a) femasr_jpeg_coefficients_u8: device events, median of %d x 20 back-to-back launches' % a.repeats)
    for name, img in (('2048x1024x3', small), ('5760x5760x3', big)):
        t = torch.from_numpy(img).cuda()
        for sub in ('420', '444'):
            flat, views = jpegio.coefficients_flat_gpu(t, q, sub)
            crop = img[:64, :512]
            same = all(np.array_equal(v[:c.shape[0], :c.shape[1]].cpu().numpy(), c) for v, c in zip(views, jpegio.coefficients_ref(crop, q, sub)))
            pin = torch.empty(flat.shape, dtype=torch.int16, pin_memory=True)
            ms, sp = events_ms(lambda: jpegio.coefficients_flat_gpu(t, q, sub), 3, 20, a.repeats)
            cms, csp = events_ms(lambda: pin.copy_(flat, non_blocking=True), 2, 5, a.repeats)
            by = t.numel() + 2 * flat.numel()
            say(f'  {name} {sub}: kernel {ms:7.4f} ms (spread {100 * sp:4.1f} %), {by / 1e6:6.1f} MB algorithmic, {by / (ms * 1e-3) / 1e12:5.2f} TB/s, '
                f'equal to coefficients_ref on the top-left 64x512 crop: {same};  D2H of the output {cms:7.3f} ms (spread {100 * csp:4.1f} %, '
                f'{2 * flat.numel() / (cms * 1e-3) / 1e9:5.1f} GB/s): the kernel is {100 * ms / cms:5.1f} % of its copy')
            del flat, views, pin
        del t
        torch.cuda.empty_cache()

    say(f'(b) one image, wall time, best and median of {a.repeats}, interleaved; writer = kernel + D2H + encode_jpeg(threads), '
        f'PIL = D2H + Image.save(quality={q}, subsampling={pil_ss})')
    for name, img in (('2048x1024', small), ('2560x1664', big_src), ('5760x5760', big)):
        t = torch.from_numpy(img).cuda()
        H, W = img.shape[:2]
        shapes = jpegio.geometry(H, W, 3, ss)[2]
        pin = torch.empty(sum(hb * wb * 64 for hb, wb in shapes), dtype=torch.int16, pin_memory=True)
        pools = {n: ThreadPoolExecutor(n) for n in threads}
        times, sizes, psnr = {k: [] for k in ['PIL'] + threads}, {}, {}
        for _ in range(a.repeats):
            for k in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == 'PIL':
                    buf = io.BytesIO()
                    Image.fromarray(t.cpu().numpy(), 'RGB').save(buf, 'JPEG', quality=q, subsampling=pil_ss)
                    data = buf.getvalue()
                else:
                    pin.copy_(jpegio.coefficients_flat_gpu(t, q, ss)[0], non_blocking=True)
                    torch.cuda.synchronize()
                    host, comps, off = pin.numpy(), [], 0
                    for hb, wb in shapes:
                        comps.append(host[off:off + hb * wb * 64].reshape(hb, wb, 64))
                        off += hb * wb * 64
                    data = jpegio.encode_jpeg(comps, W, H, q, ss, pools[k])
                times[k].append(time.perf_counter() - t0)
                sizes[k] = len(data)
                if k not in psnr:
                    dec = np.array(Image.open(io.BytesIO(data)).convert('RGB')).astype(np.float64)
                    psnr[k] = 10 * np.log10(255.0 ** 2 / np.mean((dec - img) ** 2))
        for p in pools.values():
            p.shutdown()
        base = statistics.median(times['PIL'])
        say(f'  {name}: ' + ';  '.join(f'{k if k == "PIL" else "threads " + str(k)}: best {min(v) * 1e3:7.1f} ms, median {statistics.median(v) * 1e3:7.1f} ms'
                                       f' ({base / statistics.median(v):4.1f}x), {sizes[k]} B, {psnr[k]:.2f} dB' for k, v in times.items()))
        del t, pin

    if not a.skip_cli:
        tmp = tempfile.mkdtemp(prefix='jpeg_io_bench_')
        try:
            src = os.path.join(tmp, 'in')
            os.makedirs(src)
            names = [n for n in files if n.lower().endswith('.jpg')]
            for n in names:
                with open(os.path.join(src, n), 'wb') as f:
                    f.write(files[n])
            runs = [('this tree, --io-threads 8', ROOT, ['--io-threads', '8']),
                    (f'this tree, --io-threads 8 --jpeg-quality {q}', ROOT, ['--io-threads', '8', '--jpeg-quality', str(q), '--jpeg-subsampling', ss])]
            if a.baseline:
                runs.insert(0, ('parent commit, --io-threads 8', os.path.abspath(a.baseline), ['--io-threads', '8']))
            wall, size = {r[0]: [] for r in runs}, {}
            for rep in range(a.cli_repeats + 1):                   # (the first round warms the file cache and is not counted)
                for label, tree, extra in runs:
                    dst = os.path.join(tmp, 'out')
                    shutil.rmtree(dst, ignore_errors=True)
                    env = dict(os.environ, PYTHONPATH=tree)
                    t0 = time.perf_counter()
                    subprocess.run([sys.executable, '-m', 'femasr_amd.inference', '-i', src, '-o', dst, '--synthetic-seed', '3'] + extra, cwd=tree, env=env,
                                   check=True, stdout=subprocess.DEVNULL, timeout=900)
                    dt = time.perf_counter() - t0
                    assert len(os.listdir(dst)) == len(names)
                    size[label] = sum(os.path.getsize(os.path.join(dst, n)) for n in names)
                    if rep:
                        wall[label].append(dt)
            say(f'(c) python -m femasr_amd.inference over the {len(names)} .jpg images of the testset, --synthetic-seed 3, fresh child process each, '
                f'alternating, {a.cli_repeats} counted runs each (process start, weights and model build included)')
            for label, v in wall.items():
                say(f'  {label:46s}: ' + ', '.join(f'{x:6.2f} s' for x in v) + f'   median {statistics.median(v):6.2f} s, {size[label]} B written')
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

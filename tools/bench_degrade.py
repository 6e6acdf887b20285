"""Synthesis of LQ inputs (femasr_amd/degrade.py, csrc/degrade.hip) on one MI355X box: every kernel, one whole recipe, the CLI.

    python tools/bench_degrade.py [--repeats 5] [--skip-cli] [--skip-host] [--out profiles/degrade_bench.txt]

Recorded, not gating.  Content: the x4 PIL-bicubic upscale of a testset image (tests/golden/testset_all.npz) cut to a 2040 x 1356 GT.
(a) Per kernel at that size: device events around back-to-back launches, median and (max - min) / median, beside a stock-torch restatement
    of the same operation on the device (conv2d over a mirror-padded plane; index_select and a weighted sum; torch.randn scaled by the
    factor - the same distribution, not the same numbers; clamp-mul-round; no stock-torch JPEG decoder exists: the decoder stands beside
    the D2H copy of its own output).
(b) One whole degrade_u8 of a fixed sf-4 recipe against degrade_ref of the same recipe on the host (one run: the host takes seconds).
(c) The CLI over the 38 testset images taken as GT, sf 4, a fresh child process: wall time with --io-threads 0 and 8."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png_io import events_ms, testset, upscaled      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--skip-cli', action='store_true')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from femasr_amd import degrade as D, jpegio
    lines = [f'# tools/bench_degrade.py on {torch.cuda.get_device_name(0)}; GT 2040 x 1356 x 3 (x4 upscale of a testset image)']

    def say(line):
        lines.append(line)
        print(line, flush=True)
    files = testset()
    gt = np.ascontiguousarray(np.tile(upscaled(files['00003.png']), (2, 1, 1))[:1356, :2040])
    assert gt.shape == (1356, 2040, 3)
    u8 = torch.from_numpy(gt).cuda()
    x = D.unit_gpu(u8)
    chw = x.permute(2, 0, 1).contiguous()

    def row(name, ours, theirs, note=''):
        ms, sp = events_ms(ours, 3, 10, a.repeats)
        if theirs is None:
            say(f'  {name:34s} {ms:8.3f} ms (spread {sp:.2f}){note}')
            return
        tms, tsp = events_ms(theirs, 3, 10, a.repeats)
        say(f'  {name:34s} {ms:8.3f} ms (spread {sp:.2f})   stock torch {tms:8.3f} ms (spread {tsp:.2f})   x{tms / ms:.2f}{note}')

    say('(a) kernels: device events, median of %d x 10 back-to-back launches' % a.repeats)
    for k, s in ((7, 1), (25, 1), (25, 4)):
        kern = D.fspecial_gaussian(k, 0.3 * k).astype(np.float32) if s == 1 else D.shifted_gaussian(s, 1.8).astype(np.float32)
        kt = torch.from_numpy(np.ascontiguousarray(kern[::-1, ::-1])).cuda()[None, None].repeat(3, 1, 1, 1)

        def torch_blur():
            p = F.pad(chw[None], (k // 2,) * 4, mode='reflect')
            return F.conv2d(p, kt, stride=s, groups=3)
        row(f'blur k={k} stride={s}', lambda: D.blur_gpu(x, kern, s), torch_blur)
    for filt, oh, ow in (('bicubic', 339, 510), ('area', 339, 510), ('area', 172, 259), ('matlab', 678, 1020), ('bilinear', 2712, 4080)):
        th, tw = D.op_tables({'op': 'resize', 'filter': filt, 'out_h': oh, 'out_w': ow}, 1356, 2040)
        dev = [torch.from_numpy(t).cuda() for t in (th[0], th[1].astype(np.int64), tw[0], tw[1].astype(np.int64))]

        def torch_resize():
            h1 = (x[dev[1].reshape(-1)].reshape(oh, -1, 2040, 3) * dev[0][:, :, None, None]).sum(1)
            return (h1[:, dev[3].reshape(-1)].reshape(oh, ow, -1, 3) * dev[2][None, :, :, None]).sum(2).clamp_(0, 1)
        row(f'resize {filt} -> {ow}x{oh} ({th[0].shape[1]}/{tw[0].shape[1]} taps)', lambda: D.resize_gpu(x, th, tw), torch_resize)
    m = np.random.RandomState(4).uniform(-1, 1, (3, 3))
    fac = {'color': np.eye(3) * 0.05, 'gray': np.eye(3) * 0.05, 'correlated': D.factor_of_covariance((25 / 255.0) ** 2 * (m @ m.T))}
    for mode, f in fac.items():
        ft = torch.from_numpy(f.astype(np.float32)).cuda()

        def torch_noise():
            n = torch.randn((1356, 2040, 1 if mode == 'gray' else 3), device='cuda')
            return (x + (n * ft[0, 0] if mode != 'correlated' else n @ ft.T)).clamp_(0, 1)
        row(f'noise {mode}', lambda: D.noise_gpu(x, mode, f.reshape(-1), 5), torch_noise)
    row('quantize', lambda: D.quantize_gpu(x), lambda: (x.clamp(0, 1) * 255.0).round().to(torch.uint8))
    row('unit', lambda: D.unit_gpu(u8), lambda: u8.to(torch.float32) / 255.0)
    for ss in ('420', '444'):
        planes = jpegio.coefficients_gpu(u8, 75, ss)
        out = jpegio.decode_gpu(planes, 75, ss, 1356, 2040)
        pin = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
        cms, _ = events_ms(lambda: pin.copy_(out, non_blocking=True), 3, 10, a.repeats)
        row(f'jpeg decode {ss} -> u8', lambda: jpegio.decode_gpu(planes, 75, ss, 1356, 2040), None, f'   (D2H copy of its output: {cms:.3f} ms)')
        row(f'jpeg decode {ss} -> f32', lambda: jpegio.decode_gpu(planes, 75, ss, 1356, 2040, float32=True), None)
    row('jpeg op (quantize, coefficients, decode)', lambda: D.jpeg_gpu(x, 75), None)

    say('(b) one whole recipe (sf 4)')
    rec = D.sample_recipe(5, 'fixed.png', 1356, 2040, 4)
    say('  ops: ' + ', '.join(o['op'] + (f"[{o.get('kind') or o.get('filter') or o.get('mode') or o.get('quality')}]" if len(o) > 1 else '') for o in rec['ops']))
    ms, sp = events_ms(lambda: D.degrade_u8(u8, rec), 2, 5, a.repeats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        D.degrade_u8(u8, rec)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / 5
    say(f'  degrade_u8: {ms:.3f} ms by device events (spread {sp:.2f}), {wall * 1e3:.3f} ms wall with the host work of the tables (cached)')
    if not a.skip_host:
        t0 = time.perf_counter()
        want = D.degrade_ref(gt, rec)
        host = time.perf_counter() - t0
        got = D.degrade_u8(u8, rec).cpu().numpy()
        diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
        say(f'  degrade_ref on the host: {host:.2f} s; GPU result differs on {int((diff > 0).sum())} of {diff.size} bytes (max {int(diff.max())}): '
            'float32 kernels against float64 definitions')

    if not a.skip_cli:
        say('(c) the CLI over the 38 testset images as GT, sf 4, fresh child processes')
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, 'gt')
            os.makedirs(src)
            for name, raw in files.items():
                with open(os.path.join(src, name), 'wb') as f:
                    f.write(raw)
            env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
            for threads in (0, 8):
                t0 = time.perf_counter()
                p = subprocess.run([sys.executable, '-m', 'femasr_amd.degrade_folder', '-i', src, '-o', os.path.join(tmp, f'lq{threads}'), '-s', '4',
                                    '--io-threads', str(threads)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, p.stderr[-2000:]
                say(f'  --io-threads {threads}: {time.perf_counter() - t0:.2f} s wall for {len(files)} images (process start and torch import included)')
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

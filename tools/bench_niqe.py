"""NIQE throughput on one MI355X: one 2040x1356 image and 16 images at 512x512, crop 0; the host definition on the same 2040x1356 image
beside them.

    python tools/bench_niqe.py [--warmup 3] [--steps 20] [--profile] [--out profiles/FILE.txt]

Seeded synthetic images (a smooth sinusoid plus Gaussian noise) and synthetic parameters (no real niqe_pris_params.npz is needed for
timing); reads neither the reference nor the oracle.  Timing: device events around `steps` back-to-back femasr_niqe_features calls
(workspace, tables and outputs allocated before) after `warmup` calls on the current stream; the median of `--repeats` such measurements.
Beside it the whole femasr_amd.niqe.niqe call (tables uploaded, features copied back, the host tail) by the wall clock.  CPU:
calculate_niqe of femasr_amd.models.femasr_model (numpy, fp64) once on the host: the only comparison made.  --profile: per workload a
separate child process runs the same calls under `rocprofv3 --kernel-trace --stats`; the mean time of each kernel per call (calls after
the first) is the per-kernel split.
"""
import argparse
import ctypes
import glob
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (('1x2040x1356', 1, 1356, 2040), ('16x512x512', 16, 512, 512))
KERNELS = ('niqe_y_kernel', 'niqe_mscn_kernel', 'imresize_h_kernel', 'imresize_w_kernel', 'niqe_block_kernel')


def _params():
    import numpy as np
    rng = np.random.RandomState(2024)
    mu = rng.rand(36)
    a = rng.normal(size=(36, 36))
    r = np.arange(7) - 3.0
    win = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2 * (7.0 / 6.0) ** 2))
    return mu, a @ a.T / 36 + 0.1 * np.eye(36), win / win.sum()


def _images(B, H, W):
    import numpy as np
    rng = np.random.RandomState(B * 7 + H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 128 + 70 * np.sin(y / 23.0) * np.cos(x / 31.0)
    noise = rng.normal(size=(B, H, W, 1)) * 12.0 + rng.normal(size=(B, H, W, 3)) * 2.0
    return np.clip(np.rint(base[None, ..., None] + np.arange(3) * 6.0 + noise), 0, 255).astype(np.uint8)


class Call:
    """One femasr_niqe_features call with everything allocated up front."""

    def __init__(self, B, H, W):
        import numpy as np
        import torch
        from femasr_amd import _lib, resize
        from femasr_amd.models.femasr_model import aggd_tables
        self.lib, self.check = _lib.load(), _lib.check
        self.img = torch.from_numpy(_images(B, H, W)).cuda()
        nh, nw = H // 96, W // 96
        n = ctypes.c_size_t()
        _lib.check(self.lib.femasr_niqe_workspace_bytes(B, H, W, 0, ctypes.byref(n)))
        self.nbytes = n.value
        dev = self.img.device
        wh, ih, self.ph = resize.device_tables(nh * 96, nh * 48, 0.5, True, dev)
        ww, iw, self.pw = resize.device_tables(nw * 96, nw * 48, 0.5, True, dev)
        self.keep = [torch.from_numpy(_params()[2]).cuda(), torch.from_numpy(np.concatenate(aggd_tables())).cuda(), wh, ih, ww, iw,
                     torch.empty((B, nh * nw, 36), dtype=torch.float64, device=dev), torch.empty((B, nh * nw, 10), dtype=torch.int32, device=dev),
                     torch.empty(n.value, dtype=torch.uint8, device=dev)]
        self.feat = self.keep[6]
        self.shape = (B, H, W)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ptrs = [_lib.ptr(t) for t in [self.img] + self.keep]

    def __call__(self):
        img, win, tab, wh, ih, ww, iw, feat, pos, ws = self.ptrs
        B, H, W = self.shape
        self.check(self.lib.femasr_niqe_features(self.stream, img, B, H, W, 0, win, tab, wh, ih, self.ph, ww, iw, self.pw, feat, pos, ws,
                                                 self.nbytes))


def time_calls(B, H, W, warmup, steps, repeats):
    import torch
    from femasr_amd import niqe
    call = Call(B, H, W)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    assert bool(torch.isfinite(call.feat).all())
    params = _params()
    niqe.niqe(call.img, params)
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = niqe.niqe(call.img, params)
        wall.append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(score).all())
    return statistics.median(ms), statistics.median(wall), call.nbytes


def child(B, H, W, n):
    import torch
    call = Call(B, H, W)
    for _ in range(n):
        call()
    torch.cuda.synchronize()


def profile(B, H, W, n, timeout):
    """{kernel: mean ms per call} over the calls after the first, from a rocprofv3 kernel trace of a child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['timeout', '-k', '10', str(timeout), 'rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'nq', '--',
               sys.executable, os.path.abspath(__file__), '--child', str(B), str(H), str(W), str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'rocprofv3 child failed ({r.returncode}): {r.stderr[-2000:]}')
        dbs = glob.glob(os.path.join(d, '**', '*.db'), recursive=True)
        if not dbs:
            raise RuntimeError('rocprofv3 wrote no .db')
        rows = sqlite3.connect(dbs[0]).execute('select name, start, end from kernels order by start').fetchall()
    rows = [r for r in rows if any(k in r[0] for k in KERNELS)]
    if len(rows) != 6 * n:
        raise RuntimeError(f'expected {6 * n} niqe dispatches, found {len(rows)}')
    out = dict.fromkeys(KERNELS, 0.0)
    for name, s, e in rows[6:]:
        out[next(k for k in KERNELS if k in name)] += (e - s) / 1e6 / (n - 1)
    return out


def cpu_time(H, W):
    from femasr_amd.models.femasr_model import calculate_niqe
    img = _images(1, H, W)[0]
    t0 = time.perf_counter()
    score = calculate_niqe(img, 0, _params())
    return (time.perf_counter() - t0) * 1e3, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--profile-calls', type=int, default=6)
    ap.add_argument('--no-cpu', action='store_true', help='skip the host timing of the definition')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs=4, type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return
    import torch
    lines = [f'# tools/bench_niqe.py on {torch.cuda.get_device_name(0)}: crop 0, warmup {a.warmup}, steps {a.steps}, median of {a.repeats} '
             '(device events); seeded synthetic images and parameters',
             '# features call = femasr_niqe_features (six launches: y, mscn, imresize h + w, mscn, blocks); niqe() = the whole Python call by '
             'the wall clock (table upload, features to the host, the host tail)']
    for label, B, H, W in WORKLOADS:
        ms, wall, nbytes = time_calls(B, H, W, a.warmup, a.steps, a.repeats)
        px = B * (H // 96) * (W // 96) * 9216
        lines.append(f'{label:12s} features call {ms * 1e3:9.1f} us   {ms * 1e3 / B:9.1f} us/image   {px / (ms * 1e-3) / 1e9:6.2f} Gpixel/s scored   '
                     f'workspace {nbytes / 1e6:6.1f} MB   niqe() {wall:8.2f} ms')
        print(lines[-1], flush=True)
        if a.profile:
            prof = profile(B, H, W, a.profile_calls, 600)
            total = sum(prof.values())
            lines.append(f'    rocprofv3 kernel time per call (mean of {a.profile_calls - 1} calls), total {total * 1e3:8.1f} us: ' +
                         ', '.join(f'{k} {v * 1e3:.1f} us' for k, v in prof.items()))
            print(lines[-1], flush=True)
    if not a.no_cpu:
        t, score = cpu_time(1356, 2040)
        lines.append(f'CPU (host, numpy fp64) 1x2040x1356  calculate_niqe {t:9.1f} ms   (score {score:.6f} with the synthetic parameters)')
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

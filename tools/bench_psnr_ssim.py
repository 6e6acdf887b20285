"""PSNR + SSIM throughput on one MI355X: one 2040x1356 pair and 16 pairs at 512x512, Y and RGB mode, crop 4; the CPU definitions on the
same 2040x1356 pair beside them.

    python tools/bench_psnr_ssim.py [--warmup 5] [--steps 50] [--profile] [--out profiles/FILE.txt]

Seeded synthetic images (smooth content plus noise); reads neither the reference nor the oracle.  Timing: device events around `steps`
back-to-back femasr_psnr_ssim calls (all three outputs, workspace and outputs allocated before) after `warmup` calls on the current stream.
CPU: calculate_psnr / calculate_ssim of femasr_amd.models.femasr_model (numpy / scipy, fp64) once each on the host.  --profile: per workload
a separate child process runs the same calls under `rocprofv3 --kernel-trace --stats`; the kernel time of the two launches (mean over the
calls after the first) gives achieved fp64 GFLOP/s and HBM GB/s from the shapes (below).  No fp64 peak is quoted for the chip, so no share
of peak is reported.
"""
import argparse
import ctypes
import glob
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROP = 4
WORKLOADS = (('1x2040x1356', 1, 1356, 2040), ('16x512x512', 16, 512, 512))


def work(B, H, W, ty):
    """(fp64 FLOPs, HBM bytes) of one call.  FLOPs, per plane: every valid SSIM position sums 5 moments over 121 products (mul + add each:
    1210) and evaluates the map (13, the division counted once); every cropped pixel forms a², b², ab (3) and its PSNR term (3), and in Y mode
    the luma of both images (2 x 9).  Bytes: both uint8 images once, one fp64 partial per block written and read back, the outputs."""
    P = 1 if ty else 3
    hc, wc = H - 2 * CROP, W - 2 * CROP
    ho, wo = hc - 10, wc - 10
    per_plane = ho * wo * (1210 + 13) + hc * wc * (3 + 3 + (18 if ty else 0))
    blocks = -(-ho // 16) * -(-wo // 32) + -(-hc * wc // 4096)
    return B * P * per_plane, 2 * B * H * W * 3 + 2 * 8 * B * P * blocks + 3 * 8 * B


def _inputs(B, H, W):
    import numpy as np
    import torch
    rng = np.random.RandomState(B * 7 + H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 128 + 90 * np.sin(y / 300.0)[..., None] * np.cos(x / 450.0)[..., None] + np.arange(3) * 5
    mk = lambda: np.clip(np.rint(base[None] + rng.uniform(-8, 8, (B, H, W, 3))), 0, 255).astype(np.uint8)
    return torch.from_numpy(mk()).cuda(), torch.from_numpy(mk()).cuda()


class Call:
    """One femasr_psnr_ssim call with everything allocated up front."""

    def __init__(self, B, H, W, ty):
        import torch
        from femasr_amd import _lib
        self.lib, self.args = _lib.load(), (B, H, W, CROP, int(ty))
        self.a, self.b = _inputs(B, H, W)
        self.out = [torch.empty(B, dtype=torch.float64, device='cuda') for _ in range(3)]
        n = ctypes.c_size_t()
        _lib.check(self.lib.femasr_psnr_ssim_workspace_bytes(B, H, W, CROP, int(ty), ctypes.byref(n)))
        self.ws, self.nbytes = torch.empty(n.value, dtype=torch.uint8, device='cuda'), n.value
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.check = _lib.check
        self.ptrs = [_lib.ptr(t) for t in (self.a, self.b, *self.out, self.ws)]

    def __call__(self):
        a, b, p, s, m, ws = self.ptrs
        self.check(self.lib.femasr_psnr_ssim(self.stream, a, b, *self.args, p, s, m, ws, self.nbytes))


def time_calls(B, H, W, ty, warmup, steps):
    import torch
    call = Call(B, H, W, ty)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(call.out[0]).all()) and bool(((call.out[1] > 0) & (call.out[1] < 1)).all())
    return e0.elapsed_time(e1) / steps, call


def child(B, H, W, ty, n):
    import torch
    call = Call(B, H, W, ty)
    for _ in range(n):
        call()
    torch.cuda.synchronize()


def profile(B, H, W, ty, n, timeout):
    """{kernel name: mean ms per call} over the calls after the first, from a rocprofv3 kernel trace of a child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['timeout', '-k', '10', str(timeout), 'rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'ps', '--',
               sys.executable, os.path.abspath(__file__), '--child', str(B), str(H), str(W), str(int(ty)), str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'rocprofv3 child failed ({r.returncode}): {r.stderr[-2000:]}')
        dbs = glob.glob(os.path.join(d, '**', '*.db'), recursive=True)
        if not dbs:
            raise RuntimeError('rocprofv3 wrote no .db')
        rows = sqlite3.connect(dbs[0]).execute('select name, start, end from kernels order by start').fetchall()
    rows = [r for r in rows if 'psnr_ssim' in r[0]]
    if len(rows) != 2 * n:
        raise RuntimeError(f'expected {2 * n} psnr_ssim dispatches, found {len(rows)}')
    out = {}
    for name, s, e in rows[2:]:
        key = 'finalize' if 'finalize' in name else 'psnr_ssim_kernel'
        out[key] = out.get(key, 0.0) + (e - s) / 1e6 / (n - 1)
    return out


def cpu_times(H, W):
    import numpy as np
    from femasr_amd.models.femasr_model import calculate_psnr, calculate_ssim
    a, b = (t[0].cpu().numpy() for t in _inputs(1, H, W))
    out = []
    for ty in (True, False):
        t0 = time.perf_counter()
        calculate_psnr(a, b, crop_border=CROP, test_y_channel=ty)
        t1 = time.perf_counter()
        calculate_ssim(a, b, crop_border=CROP, test_y_channel=ty)
        t2 = time.perf_counter()
        out.append((ty, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--profile-calls', type=int, default=6)
    ap.add_argument('--no-cpu', action='store_true', help='skip the host timing of the CPU functions')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs=5, type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        B, H, W, ty, n = a.child
        child(B, H, W, bool(ty), n)
        return
    import torch
    lines = [f'# tools/bench_psnr_ssim.py on {torch.cuda.get_device_name(0)}: crop {CROP}, warmup {a.warmup}, steps {a.steps} (device events); '
             'seeded synthetic images',
             '# one call = femasr_psnr_ssim with psnr, ssim and mse (two launches); GFLOP = fp64 operations from the shapes (bench docstring), '
             'GB = both uint8 images + partials + outputs']
    for label, B, H, W in WORKLOADS:
        for ty in (True, False):
            ms, _ = time_calls(B, H, W, ty, a.warmup, a.steps)
            fl, by = work(B, H, W, ty)
            lines.append(f'{label:12s} {"Y  " if ty else "RGB"}  call {ms * 1e3:9.1f} us   {ms * 1e3 / B:9.1f} us/pair   '
                         f'{fl / 1e9:7.3f} GFLOP {fl / (ms * 1e-3) / 1e9:8.0f} GFLOP/s   {by / 1e6:7.1f} MB {by / (ms * 1e-3) / 1e9:7.1f} GB/s')
            print(lines[-1], flush=True)
            if a.profile:
                prof = profile(B, H, W, ty, a.profile_calls, 600)
                k = prof['psnr_ssim_kernel']
                lines.append(f'    rocprofv3 kernel time (mean of {a.profile_calls - 1} calls): psnr_ssim_kernel {k * 1e3:8.1f} us '
                             f'({fl / (k * 1e-3) / 1e9:.0f} GFLOP/s fp64, {by / (k * 1e-3) / 1e9:.1f} GB/s), finalize {prof["finalize"] * 1e3:6.1f} us')
                print(lines[-1], flush=True)
    if not a.no_cpu:
        for ty, tp, ts in cpu_times(1356, 2040):
            lines.append(f'CPU (host, numpy / scipy fp64) 1x2040x1356 {"Y  " if ty else "RGB"}  calculate_psnr {tp:8.1f} ms   '
                         f'calculate_ssim {ts:9.1f} ms')
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""LPIPS throughput on one MI355X: ms per pair for one 2040x1356 pair and for 16 pairs at 512x512, both backbones.

    python tools/bench_lpips.py [--nets alex,vgg] [--warmup 3] [--steps 10] [--profile] [--out profiles/FILE.txt]

Synthetic weights (femasr_amd.synth.lpips_state) and inputs; reads neither the reference nor the oracle.  Timing: device events
around `steps` forwards after `warmup` forwards on the current stream.  --profile: for every (net, workload) a separate child
process runs the same forwards under `rocprofv3 --kernel-trace --stats`; its dispatches are mapped back to the layers (one forward
is a fixed sequence: input, then per conv the conv and, after a tapped conv, the tap kernel, then finalize), giving the per-layer
time and, for the dominant conv, the achieved fraction of the 157.3 TFLOP/s fp32 matrix peak (FLOPs from the shapes, below).
"""
import argparse
import glob
import os
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK = 157.3e12
WORKLOADS = (('1x2040x1356', 1, 1356, 2040), ('16x512x512', 16, 512, 512))


def layer_plan(net, H, W):
    """[(layer name, kind, FLOPs per pair)] in launch order; FLOPs = 2 * Ho * Wo * Cout * Cin * k * k per image, two images."""
    from femasr_amd.lpips import _CONVS, _pool_out
    out, y, x, t = [('input', 'input', 0.0)], H, W, 0
    for k, i, cin, cout, ksz, stride, pad, tap, pool in _CONVS[net]:
        y, x = (y + 2 * pad - ksz) // stride + 1, (x + 2 * pad - ksz) // stride + 1
        out.append((f'conv{i} {cin}->{cout} {ksz}x{ksz}/s{stride} @{y}x{x}', 'conv', 2.0 * 2 * y * x * cout * cin * ksz * ksz))
        if tap:
            out.append((f'tap{t + 1} C{cout} @{y}x{x}' + (' + pool' if pool else ''), 'tap', 0.0))
            t += 1
        if pool:
            y, x = _pool_out(y, pool), _pool_out(x, pool)
    out.append(('finalize', 'finalize', 0.0))
    return out


def _setup(net, B, H, W):
    import torch
    from femasr_amd import lpips as L
    from femasr_amd import synth
    m = L.LPIPS(net, state_dict={k: torch.from_numpy(v) for k, v in synth.lpips_state(L.expected_shapes(net), 1).items()}).cuda()
    x0 = torch.from_numpy(synth.synth_input(1, (B, 3, H, W))).cuda()
    x1 = torch.from_numpy(synth.synth_input(2, (B, 3, H, W))).cuda()
    return m, x0, x1


def time_forward(net, B, H, W, warmup, steps):
    import torch
    m, x0, x1 = _setup(net, B, H, W)
    for _ in range(warmup):
        m(x0, x1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = m(x0, x1)
    e1.record()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return e0.elapsed_time(e1) / steps


def child(net, B, H, W, n):
    import torch
    m, x0, x1 = _setup(net, B, H, W)
    for _ in range(n):
        m(x0, x1)
    torch.cuda.synchronize()


def profile(net, B, H, W, n, timeout):
    """Per-layer device time (ms per forward, averaged over the forwards after the first) from a rocprofv3 kernel trace."""
    plan = layer_plan(net, H, W)
    with tempfile.TemporaryDirectory() as d:
        cmd = ['timeout', '-k', '10', str(timeout), 'rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'lp', '--',
               sys.executable, os.path.abspath(__file__), '--child', net, str(B), str(H), str(W), str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'rocprofv3 child failed ({r.returncode}): {r.stderr[-2000:]}')
        dbs = glob.glob(os.path.join(d, '**', '*.db'), recursive=True)
        if not dbs:
            raise RuntimeError('rocprofv3 wrote no .db')
        rows = sqlite3.connect(dbs[0]).execute('select name, start, end from kernels order by start').fetchall()
    names = ('lpips_', 'conv_igemm', 'conv3x3_halo')
    rows = [r for r in rows if any(s in r[0] for s in names) and 'repack' not in r[0]]
    per = len(plan)
    if len(rows) != per * n:
        raise RuntimeError(f'expected {per * n} LPIPS dispatches, found {len(rows)}')
    acc = [0.0] * per
    kern = [''] * per
    for f in range(1, n):
        for j in range(per):
            name, s, e = rows[f * per + j]
            acc[j] += (e - s) / 1e6
            kern[j] = name
    return [(plan[j][0], plan[j][1], plan[j][2], acc[j] / (n - 1), kern[j]) for j in range(per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nets', default='alex,vgg')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--profile-forwards', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs=5, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        net, B, H, W, n = a.child
        child(net, int(B), int(H), int(W), int(n))
        return
    import torch
    lines = [f'# tools/bench_lpips.py on {torch.cuda.get_device_name(0)}: warmup {a.warmup}, steps {a.steps} (device events); synthetic weights',
             '# "ms/pair" = forward time / pairs; "TFLOP/s" = conv FLOPs from the shapes (2 images per pair) / forward time']
    for net in a.nets.split(','):
        for label, B, H, W in WORKLOADS:
            ms = time_forward(net, B, H, W, a.warmup, a.steps)
            flops = B * sum(p[2] for p in layer_plan(net, H, W))
            lines.append(f'{net:5s} {label:12s} forward {ms:9.3f} ms   {ms / B:9.3f} ms/pair   conv GFLOP/pair {flops / B / 1e9:9.2f}   '
                         f'{flops / (ms * 1e-3) / 1e12:6.1f} TFLOP/s = {flops / (ms * 1e-3) / FP32_MATRIX_PEAK:5.1%} of the fp32 matrix peak')
            print(lines[-1], flush=True)
            if a.profile:
                prof = profile(net, B, H, W, a.profile_forwards, 600)
                tot = sum(p[3] for p in prof)
                lines.append(f'  per-layer device time (rocprofv3 kernel trace, mean of {a.profile_forwards - 1} forwards; sum {tot:.3f} ms):')
                for name, kind, fl, t, kn in prof:
                    frac = f'   {fl * B / (t * 1e-3) / 1e12:6.1f} TFLOP/s = {fl * B / (t * 1e-3) / FP32_MATRIX_PEAK:5.1%} of peak' if fl else ''
                    lines.append(f'    {name:44s} {t:9.3f} ms {100 * t / tot:5.1f} %{frac}   [{kn[:60]}]')
                dom = max((p for p in prof if p[1] == 'conv'), key=lambda p: p[3])
                lines.append(f'  dominant conv launch: {dom[0]}: {dom[3]:.3f} ms, achieved fp32-matrix fraction '
                             f'{dom[2] * B / (dom[3] * 1e-3) / FP32_MATRIX_PEAK:.1%}')
                print('\n'.join(lines[-len(prof) - 2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

"""DISTS throughput on one MI355X beside its natural yardsticks: ms per call for one 2040x1356 pair and for 16 pairs at 512x512.

    python tools/bench_dists.py [--warmup 2] [--steps 5] [--rounds 3] [--trace] [--out profiles/dists_bench.txt]

Three legs in ONE process, alternating in rounds so that clock drift hits all of them; device events around `steps` back-to-back calls
after `warmup` calls; the median of the rounds with the round-to-round spread:
  dists      femasr_amd.dists.DISTS (csrc/dists.hip)
  lpips-vgg  femasr_amd.lpips.LPIPS('vgg'): the same 13 convs on the same kernels, max-pool and a fused head instead of the L2 pool and moments
  torch      the float32 stock-torch restatement of DISTS on the device (F.conv2d, grouped conv2d pool, fp64 statistics)
and the workspace femasr_dists_workspace_bytes asks for beside femasr_lpips_workspace_bytes.  No bar is fixed: what is expected is
DISTS = LPIPS-VGG's conv time plus a bandwidth-bound pass or two over each stage map.  --trace: a child process runs DISTS forwards
under `rocprofv3 --kernel-trace --stats`; the device time per kernel family (convs, L2 pool, moments, reduce, finalize, input).
Synthetic weights and inputs; reads neither the reference nor the oracle.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (('1x2040x1356', 1, 1356, 2040), ('16x512x512', 16, 512, 512))


def _setup(B, H, W):
    import torch
    from femasr_amd import dists as D
    from femasr_amd import lpips as L
    from femasr_amd import synth
    sd = synth.dists_state(1)
    md = D.DISTS(state_dict={k: torch.from_numpy(v) for k, v in sd.items()}).cuda()
    ml = L.LPIPS('vgg', state_dict={k: torch.from_numpy(v) for k, v in synth.lpips_state(L.expected_shapes('vgg'), 1).items()}).cuda()
    x = torch.from_numpy(synth.synth_input(1, (B, 3, H, W))).cuda()
    y = torch.from_numpy(synth.synth_input(2, (B, 3, H, W))).cuda()
    return md, ml, {k: torch.from_numpy(v).cuda() for k, v in sd.items()}, x, y


def torch_dists(sd, x, y):
    """The float32 stock-torch restatement on the device: float32 features, fp64 statistics."""
    import torch
    import torch.nn.functional as F
    mean = torch.tensor((0.485, 0.456, 0.406), device=x.device).view(1, 3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), device=x.device).view(1, 3, 1, 1)
    hann = torch.tensor([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=torch.float32, device=x.device) / 16
    stages = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
    B = x.shape[0]
    h = (torch.cat([x, y]) - mean) / std
    maps = [torch.cat([x, y])]
    for k, idx in enumerate(stages):
        if k:
            c = h.shape[1]
            # (clamp: the library's conv algorithm may return a small negative sum of non-negative products, and the sqrt a NaN)
            h = torch.sqrt(F.conv2d(h * h, hann[None, None].repeat(c, 1, 1, 1), stride=2, padding=1, groups=c).clamp_min(0) + 1e-12)
        for i in idx:
            h = F.relu(F.conv2d(h, sd[f'stage{k + 1}.{i}.weight'], sd[f'stage{k + 1}.{i}.bias'], padding=1))
        maps.append(h)
    alpha, beta = sd['alpha'].double().view(-1), sd['beta'].double().view(-1)
    total, off = torch.zeros(B, dtype=torch.float64, device=x.device), 0
    for f in maps:
        c = f.shape[1]
        fx, fy = f[:B].double(), f[B:].double()
        mx, my = fx.mean((2, 3)), fy.mean((2, 3))
        vx, vy = (fx * fx).mean((2, 3)) - mx * mx, (fy * fy).mean((2, 3)) - my * my
        cov = (fx * fy).mean((2, 3)) - mx * my
        s1 = (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)
        s2 = (2 * cov + 1e-6) / (vx + vy + 1e-6)
        total = total + (alpha[off:off + c] * s1 + beta[off:off + c] * s2).sum(1)
        off += c
    return 1 - total / (alpha.sum() + beta.sum())


def _timed(fn, warmup, steps, what=''):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    if not bool(torch.isfinite(out).all()):
        raise RuntimeError(f'{what}: non-finite result {out.flatten()[:8].tolist()}')
    return e0.elapsed_time(e1) / steps


def child(B, H, W, n):
    import torch
    md, _, _, x, y = _setup(B, H, W)
    for _ in range(n):
        md(x, y)
    torch.cuda.synchronize()


FAMILIES = (('dists_l2pool', 'l2pool'), ('dists_moments_input', 'moments (input)'), ('dists_moments', 'moments'), ('dists_reduce', 'reduce'),
            ('dists_finalize', 'finalize'), ('dists_input', 'input'), ('conv', 'convs'))


def trace(B, H, W, n, timeout):
    """Device ms per forward and kernel family (mean over the forwards after the first) from a rocprofv3 kernel trace of a child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ['timeout', '-k', '10', str(timeout), 'rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'ds', '--',
               sys.executable, os.path.abspath(__file__), '--child', str(B), str(H), str(W), str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'rocprofv3 child failed ({r.returncode}): {r.stderr[-2000:]}')
        dbs = glob.glob(os.path.join(d, '**', '*.db'), recursive=True)
        if not dbs:
            raise RuntimeError('rocprofv3 wrote no .db')
        rows = sqlite3.connect(dbs[0]).execute('select name, start, end from kernels order by start').fetchall()
    rows = [r for r in rows if 'repack' not in r[0]]
    first = [i for i, r in enumerate(rows) if 'dists_input_kernel' in r[0]]
    if len(first) != n:
        raise RuntimeError(f'expected {n} forwards in the trace, found {len(first)}')
    acc = {}
    for name, s, e in rows[first[1]:]:
        fam = next((label for key, label in FAMILIES if key in name), None)
        if fam:
            acc[fam] = acc.get(fam, 0.0) + (e - s) / 1e6 / (n - 1)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(*(int(v) for v in a.child))
        return
    import torch
    from femasr_amd import _lib
    lines = [f'# tools/bench_dists.py on {torch.cuda.get_device_name(0)}: warmup {a.warmup}, steps {a.steps}, rounds {a.rounds} '
             '(device events, legs alternating); synthetic weights',
             '# ms per call: median of the rounds [min .. max]']
    for label, B, H, W in WORKLOADS:
        md, ml, sd, x, y = _setup(B, H, W)
        legs = (('dists', lambda: md(x, y)), ('lpips-vgg', lambda: ml(x, y)), ('torch', lambda: torch_dists(sd, x, y)))
        got = {name: [] for name, _ in legs}
        for _ in range(a.rounds):
            for name, fn in legs:
                got[name].append(_timed(fn, a.warmup, a.steps, f'{label} {name}'))
        dev = float((md(x, y) - torch_dists(sd, x, y)).abs().max())
        for name, _ in legs:
            v = got[name]
            lines.append(f'{label:12s} {name:10s} {statistics.median(v):10.3f} ms  [{min(v):.3f} .. {max(v):.3f}]   '
                         f'{statistics.median(v) / B:9.3f} ms/pair')
        d, l = statistics.median(got['dists']), statistics.median(got['lpips-vgg'])
        lines.append(f'{label:12s} dists - lpips-vgg = {d - l:.3f} ms ({d / l:.3f}x); max |dists - torch restatement| = {dev:.3e}')
        lib = _lib.load()
        nb = ctypes.c_size_t()
        _lib.check(lib.femasr_dists_workspace_bytes(md._native(x.device)[1], B, H, W, ctypes.byref(nb)))
        nl = ctypes.c_size_t()
        _lib.check(lib.femasr_lpips_workspace_bytes(ml._native(x.device)[1], B, H, W, ctypes.byref(nl)))
        lines.append(f'{label:12s} workspace: dists {nb.value / 2 ** 20:.1f} MiB, lpips-vgg {nl.value / 2 ** 20:.1f} MiB')
        print('\n'.join(lines[-5:]), flush=True)
        del md, ml, sd, x, y
        torch.cuda.empty_cache()
        if a.trace:
            acc = trace(B, H, W, 3, 600)
            tot = sum(acc.values())
            lines.append(f'{label:12s} kernel trace (rocprofv3, mean of 2 forwards; sum {tot:.3f} ms): ' +
                         ', '.join(f'{k} {v:.3f} ms ({100 * v / tot:.1f} %)' for k, v in sorted(acc.items(), key=lambda kv: -kv[1])))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

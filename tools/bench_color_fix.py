"""Wavelet colour fix (femasr_amd/colorfix.py, csrc/colorfix.hip) on one MI355X: a 1440x1440 input and its x4 canvas (5760x5760, three
planes), float32 and uint8, levels = 5.

    python tools/bench_color_fix.py [--lr 1440] [--levels 5] [--warmup 2] [--steps 5] [--repeats 5] [--no-tile] [--out profiles/color_fix_bench.txt]

Timing: device events around `steps` back-to-back femasr_color_fix / femasr_color_fix_u8 calls (tables, workspace and tensors allocated
before, in place over the canvas) after `warmup` calls; the median of `repeats` such measurements.  The workspace is what
femasr_amd.colorfix.wavelet_color_fix would allocate (WORKSPACE_CAP: planes in groups).  Reported beside the time:
  * achieved bytes/s on the ALGORITHMIC traffic computed from the shapes (every kernel reads its inputs and writes its outputs once: the
    nine loads per element of a level count as one read of the plane);
  * the same canvas through a stock-torch restatement on the same GPU: up from femasr_amd.resize.imresize (torch has no MATLAB resize),
    then replicate pad + dilated depthwise conv2d per pass, and the largest difference between the two results;
  * the fix's share of a whole test_tile_u8 call (synthetic weights, tiles of 240 / 16, default arithmetic), color_fix off and on.
Seeded synthetic images; reads neither the reference nor the oracle.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def traffic_bytes(planes, h, w, s, levels, u8):
    """Algorithmic bytes of one call: H pass (lq in, fp64 intermediate out), W pass + difference (intermediate and sr in, d out), `levels`
    levels (d in, d out), store (sr and d in, canvas out)."""
    e = 1 if u8 else 4
    p, q = s * h * s * w, s * h * w
    return planes * ((h * w * e + q * 8) + (q * 8 + p * e + p * 4) + levels * (p * 8) + (p * e + p * 4 + p * e))


class Call:
    def __init__(self, lr, s, levels, u8):
        import torch
        from femasr_amd import _lib, colorfix
        g = torch.Generator().manual_seed(lr + u8)
        self.lib, self.check, self.levels, self.u8 = _lib.load(), _lib.check, levels, u8
        if u8:
            self.lq = torch.randint(0, 256, (1, lr, lr, 3), generator=g, dtype=torch.uint8).cuda()
            self.sr = torch.randint(0, 256, (1, lr * s, lr * s, 3), generator=g, dtype=torch.uint8).cuda()
        else:
            self.lq = torch.rand((1, 3, lr, lr), generator=g).cuda()
            self.sr = torch.rand((1, 3, lr * s, lr * s), generator=g).cuda()
        self.tables = colorfix._tables(lr, lr, s, self.lq.device)
        per, n = ctypes.c_size_t(), ctypes.c_size_t()
        self.units = 1 if u8 else 3                          # femasr_color_fix_u8 counts images, femasr_color_fix planes
        _lib.check(self.lib.femasr_color_fix_workspace_bytes(1, lr, lr, lr * s, lr * s, s, ctypes.byref(per)))
        group = max(1, min(3, colorfix.WORKSPACE_CAP // per.value))
        _lib.check(self.lib.femasr_color_fix_workspace_bytes(group, lr, lr, lr * s, lr * s, s, ctypes.byref(n)))
        self.nbytes = n.value
        self.ws = torch.empty(n.value, dtype=torch.uint8, device=self.lq.device)
        self.fn = self.lib.femasr_color_fix_u8 if u8 else self.lib.femasr_color_fix
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.dims = (self.units, lr, lr, lr * s, lr * s, s, levels)
        self.ptr = _lib.ptr

    def __call__(self, out=None):
        wh, ih, ph, ww, iw, pw = self.tables
        p = self.ptr
        self.check(self.fn(self.stream, p(self.sr), p(self.lq), *self.dims, p(wh), p(ih), ph, p(ww), p(iw), pw, p(self.sr if out is None else out),
                           p(self.ws), self.nbytes))


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
    return statistics.median(ms)


def torch_fix(sr, lq, s, levels):
    """The restatement in stock torch ops (the resize excepted): replicate pad + dilated depthwise conv2d, horizontal then vertical."""
    import torch
    import torch.nn.functional as F
    from femasr_amd import resize
    c = sr.shape[1]
    kh = torch.tensor([0.25, 0.5, 0.25], device=sr.device).view(1, 1, 1, 3).repeat(c, 1, 1, 1)
    kv = kh.view(c, 1, 3, 1)
    d = resize.imresize(lq, s) - sr
    for i in range(levels):
        r = 1 << i
        d = F.conv2d(F.pad(d, (r, r, 0, 0), mode='replicate'), kh, dilation=(1, r), groups=c)
        d = F.conv2d(F.pad(d, (0, 0, r, r), mode='replicate'), kv, dilation=(r, 1), groups=c)
    return sr + d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lr', type=int, default=1440)
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-tile', action='store_true', help='skip the whole test_tile_u8 call')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    lr, s, L = a.lr, a.scale, a.levels
    lines = [f'# tools/bench_color_fix.py on {torch.cuda.get_device_name(0)}: input {lr}x{lr}, canvas {lr * s}x{lr * s} x 3 planes, levels {L}, warmup '
             f'{a.warmup}, steps {a.steps}, median of {a.repeats} (device events, back-to-back calls, in place)',
             '# traffic: algorithmic bytes from the shapes (each kernel reads its inputs and writes its outputs once)']
    for u8 in (False, True):
        call = Call(lr, s, L, u8)
        ms = events_ms(call, a.warmup, a.steps, a.repeats)
        by = traffic_bytes(3, lr, lr, s, L, u8)
        lines.append(f'{"uint8 " if u8 else "float32"}  femasr_color_fix{"_u8" if u8 else "   "} {ms:8.3f} ms   {by / 1e9:6.2f} GB algorithmic   '
                     f'{by / (ms * 1e-3) / 1e12:5.2f} TB/s   workspace {call.nbytes / 1e6:7.1f} MB ({L + 3} launches per group)')
        print(lines[-1], flush=True)
        if not u8:
            sr0 = call.sr.clone()
            ref = torch_fix(sr0, call.lq, s, L)
            got = torch.empty_like(sr0)
            call.sr.copy_(sr0)
            call(out=got)
            torch.cuda.synchronize()
            diff = float((got - ref).abs().max())
            del ref, got
            tms = events_ms(lambda: torch_fix(sr0, call.lq, s, L), 1, max(1, a.steps // 2), a.repeats)
            lines.append(f'float32  stock torch (imresize + replicate pad + dilated depthwise conv2d) {tms:8.3f} ms   ({tms / ms:.1f}x the kernels; '
                         f'largest difference between the two results {diff:.3g})')
            print(lines[-1], flush=True)
            del sr0
        del call
        torch.cuda.empty_cache()
    if not a.no_tile:
        from femasr_amd import synth
        from femasr_amd.archs.femasr_arch import FeMaSRNet
        net = FeMaSRNet(codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=s)
        w = synth.fill_state_dict(net.state_dict(), 0, 'trained')
        net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        net = net.cuda().eval()
        net.color_fix_levels = L
        g = torch.Generator().manual_seed(1)
        img = torch.randint(0, 256, (lr, lr, 3), generator=g, dtype=torch.uint8).cuda()
        off = events_ms(lambda: net.test_tile_u8(img, 240, 16), 1, 1, 3)
        on = events_ms(lambda: net.test_tile_u8(img, 240, 16, color_fix=True), 1, 1, 3)
        lines.append(f'test_tile_u8 {lr}x{lr} (240 / 16, synthetic weights): {off:9.2f} ms off, {on:9.2f} ms with color_fix=True: '
                     f'the fix is {100 * (on - off) / on:.2f} % of the call')
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

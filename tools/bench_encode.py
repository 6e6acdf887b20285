"""`encode_indices` against the whole forward as a way to get VQ indices, and `codebook.usage` against torch.bincount, in ONE process.

    python tools/bench_encode.py [--steps 40] [--warmup 5] [--rounds 4] [--streams 3] [--out profiles/encode_bench.txt]

Network shapes: the HQ net on 8 images of 256x256 through `forward` geometry (the frozen net that turns a GT batch into gt_indices), and
the x4 net on 16 tiles of 128x128 with test()'s mirror pad (bench.py's headline shape).  Synthetic weights (seed 0), inputs resident in
HBM, `--streams` sub-batch streams for both legs.  Legs per shape: 'forward' - what a caller had to run for indices before (`forward` /
`test_with_all_indices`, image thrown away) - and 'encode' (`encode_indices`).  The two legs use ONE network, so the same weights and
workspace.
Histogram shapes: 82 944 tokens (81 maps of 32x32) and 10^7 tokens, codes uniform in [0, 1024); legs `codebook.usage` (with its range
check, which reads one number back) and `torch.bincount(minlength=1024)` followed by the same one-number read-back.
Timing: every leg is warmed up; then `--rounds` rounds in which the legs of a shape run `steps / rounds` calls one after the other
(A, B, A, B, ...), each block timed by the host clock between two device synchronisations.  ms per call = mean of the blocks, spread =
max - min of the blocks.  No ratio is asked for: the condition printed is that 'encode' is not slower than 'forward' by more than the larger
of the two spreads.  Untimed afterwards: the maps of the two legs are compared bit for bit.  Needs a GPU and fails without one."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _interleaved(legs, per, rounds, sync):
    blocks = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            sync()
            t0 = time.perf_counter()
            for _ in range(per):
                fn()
            sync()
            blocks[name].append((time.perf_counter() - t0) / per * 1e3)
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--streams', type=int, default=3)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.steps % args.rounds:
        raise SystemExit('--steps must be a multiple of --rounds')

    import ctypes

    import torch
    from femasr_amd import _lib, codebook, synth
    from femasr_amd.archs import build_network
    if not torch.cuda.is_available():
        raise SystemExit('bench_encode needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)

    def sync():
        torch.cuda.synchronize(dev)

    per = args.steps // args.rounds
    lines = [f'{torch.cuda.get_device_name(dev)}; warm-up {args.warmup} calls per leg, {args.steps} timed calls per leg in {args.rounds} interleaved rounds, '
             f'host clock between device synchronisations; {args.streams} sub-batch streams']
    shapes = [('HQ forward geometry, 8 x 256x256', dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=False), (8, 3, 256, 256), False),
              ('x4 test() geometry, 16 x 128x128', dict(type='FeMaSRNet', codebook_params=[[32, 1024, 512]], LQ_stage=True, scale_factor=4), (16, 3, 128, 128), True)]
    with torch.no_grad():
        for title, cfg, shape, pad in shapes:
            net = build_network(dict(cfg))
            sd = synth.fill_state_dict(net.state_dict(), seed=0, codebook='trained')
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
            net = net.to(dev).eval()
            net.num_streams = args.streams
            x = torch.from_numpy(synth.synth_input(1000, shape)).to(dev)
            full = (lambda: net.test_with_all_indices(x)[1]) if pad else (lambda: net(x)[3])
            legs = [('forward', full), ('encode', lambda: net.encode_indices(x, pad=pad))]
            for _, fn in legs:
                for _ in range(args.warmup):
                    fn()
            blocks = _interleaved(legs, per, args.rounds, sync)
            ms = {k: sum(v) / len(v) for k, v in blocks.items()}
            spread = {k: max(v) - min(v) for k, v in blocks.items()}
            lines.append(f'{title} (decoder_math {net.decoder_math}, linear_math {net.linear_math}):')
            for k in ('forward', 'encode'):
                lines.append(f'  {k:8s} {ms[k]:8.3f} ms per call   spread {spread[k]:.3f}   rounds: ' + ' '.join(f'{b:.3f}' for b in blocks[k]))
            noise = max(spread.values())
            lines.append(f'  encode against forward: {ms["encode"] - ms["forward"]:+.3f} ms per call ({ms["encode"] / ms["forward"]:.4f}), spread {noise:.3f}: '
                         f'not slower beyond the spread: {ms["encode"] <= ms["forward"] + noise}')
            a, b = full(), net.encode_indices(x, pad=pad)
            same = all(torch.equal(p, q) for p, q in zip(a, b))
            lines.append(f'  index maps of the two legs bit-identical: {same} ({sum(p.numel() for p in a)} tokens)')
            lib_ws = [0, 0]
            lib, h = net._native(dev)
            for i, q in enumerate((lib.femasr_workspace_bytes, lib.femasr_encode_workspace_bytes)):
                n = ctypes.c_size_t()
                _lib.check(q(h, shape[0], shape[2], shape[3], int(pad), ctypes.byref(n)))
                lib_ws[i] = n.value
            lines.append(f'  workspace: forward {lib_ws[0] / 2**20:.1f} MiB, encode {lib_ws[1] / 2**20:.1f} MiB')
            del net
        for title, shape in (('82 944 tokens (81 x 32x32)', (81, 1, 32, 32)), ('10^7 tokens', (10 ** 7,))):
            idx = torch.randint(0, 1024, shape, dtype=torch.int64, device=dev, generator=torch.Generator(dev).manual_seed(3))
            legs = [('bincount', lambda: int(torch.bincount(idx.flatten(), minlength=1024).sum())),
                    ('usage', lambda: codebook.usage(idx, 1024))]
            for _, fn in legs:
                for _ in range(args.warmup):
                    fn()
            blocks = _interleaved(legs, per, args.rounds, sync)
            lines.append(f'code usage, {title}, n_e 1024:')
            for k in ('bincount', 'usage'):
                v = blocks[k]
                lines.append(f'  {k:8s} {sum(v) / len(v) * 1e3:9.1f} us per call   spread {(max(v) - min(v)) * 1e3:.1f}   rounds: ' + ' '.join(f'{b * 1e3:.1f}' for b in v))
            lines.append(f'  counts identical: {torch.equal(codebook.usage(idx, 1024), torch.bincount(idx.flatten(), minlength=1024))}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

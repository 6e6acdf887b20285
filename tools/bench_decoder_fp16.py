"""decoder_math 'fp32' against 'bf16x3' against 'fp16' on bench.py's headline workload, in ONE process, on one MI355X.

    python tools/bench_decoder_fp16.py [--steps 20] [--warmup 5] [--rounds 4] [--batch 16] [--streams 3] [--out profiles/decoder_fp16_bench.txt]

Workload: bench.py's defaults (its config, weights and inputs are imported / rebuilt from the same seeds): x4, 16 tiles of 128x128 per
step through FeMaSRNet.test, three sub-batch streams, synthetic weights (seed 0), inputs resident in HBM.  bench.py is not touched and
stays the bench of record; the MPix/s printed here are THIS tool's figures.

Timing: one network per leg (same weights), each warmed up `--warmup` steps; then `--rounds` rounds, in each of which the legs run
`steps / rounds` steps one after the other (A, B, C, A, B, C, ...), so clock and power drift hit all three alike.  A block is timed by
the host clock between two device synchronisations; a leg's ms per step is its blocks' total over its steps, the per-round figures
show the spread.  Engine clock and package power are sampled by bench.PowerWatch (sysfs reads on a host thread) over the timed part
where the files exist.
Separate untimed passes afterwards: the built-in profiler's per-slot times of the fp16 leg (and the bf16x3 leg's conv slots beside
them) at one stream, and the fp16 / bf16x3 images against the fp32 image (max abs, PSNR at peak 1) with the VQ indices compared.
Reads neither the reference nor the oracle; needs a GPU and fails without one."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ('fp32', 'bf16x3', 'fp16')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--streams', type=int, default=3)
    ap.add_argument('--profile-steps', type=int, default=2)
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.steps % args.rounds:
        raise SystemExit('--steps must be a multiple of --rounds')

    import numpy as np
    import torch
    from bench import X4_CFG, PowerWatch
    from femasr_amd import synth
    from femasr_amd.archs import build_network
    if not torch.cuda.is_available():
        raise SystemExit('bench_decoder_fp16 needs a GPU: nothing is measured without one')
    dev = torch.device('cuda', 0)
    B = args.batch
    x = torch.from_numpy(synth.synth_input(1000, (B, 3, 128, 128))).to(dev)
    nets = {}
    sd = None
    for leg in LEGS:
        net = build_network(dict(X4_CFG))
        if sd is None:
            sd = synth.fill_state_dict(net.state_dict(), seed=0, codebook='trained')
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        net = net.to(dev).eval()
        net.num_streams, net.decoder_math = args.streams, leg
        nets[leg] = net
    out_mpix = B * 512 * 512 / 1e6
    lines = [f'decoder_math legs on x4 FeMaSRNet.test, batch {B} of 128x128 LR tiles -> 512x512, {args.streams} streams, synthetic weights (seed 0)',
             f'{torch.cuda.get_device_name(dev)}; warm-up {args.warmup} steps per leg, {args.steps} timed steps per leg in {args.rounds} interleaved rounds '
             f'({", ".join(LEGS)}, repeated), host clock between device synchronisations']

    with torch.no_grad():
        for leg in LEGS:
            for _ in range(args.warmup):
                nets[leg].test(x)
        torch.cuda.synchronize(dev)
        pr = torch.cuda.get_device_properties(dev)
        watch = PowerWatch((pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id) if hasattr(pr, 'pci_bus_id') else None)
        if watch.dir:
            watch.start()
        per = args.steps // args.rounds
        blocks = {leg: [] for leg in LEGS}
        for _ in range(args.rounds):
            for leg in LEGS:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(per):
                    nets[leg].test(x)
                torch.cuda.synchronize(dev)
                blocks[leg].append((time.perf_counter() - t0) / per * 1e3)
        power = watch.stop() if watch.dir else None
        ms = {leg: sum(blocks[leg]) / len(blocks[leg]) for leg in LEGS}
        for leg in LEGS:
            lines.append(f'{leg:7s} {ms[leg]:8.3f} ms per step   {out_mpix / ms[leg] * 1e3:8.2f} MPix/s (this tool)   rounds: ' +
                         ' '.join(f'{b:.3f}' for b in blocks[leg]))
        lines.append(f"fp16 / fp32 = {ms['fp16'] / ms['fp32']:.4f}, fp16 / bf16x3 = {ms['fp16'] / ms['bf16x3']:.4f}; "
                     f"ordering fp16 < bf16x3 and fp16 < fp32: {ms['fp16'] < ms['bf16x3'] and ms['fp16'] < ms['fp32']}")
        if power:
            lines.append(f"over the timed part ({power['samples']} samples of the amdgpu hwmon files): package power mean {power['package_w_mean']} W, max "
                         f"{power['package_w_max']} W, cap {power['cap_w']} W; engine clock median {power['sclk_mhz_median']} MHz, min / max {power['sclk_mhz_min_max']}")
        else:
            lines.append('engine clock / package power: not read (no amdgpu hwmon files for this device)')

        # untimed: per-slot times at one stream
        prof = {}
        for leg in ('fp16', 'bf16x3'):
            net = nets[leg]
            net.num_streams = 1
            net.test(x)
            net.enable_profile(True)
            for _ in range(args.profile_steps):
                net.test(x)
            torch.cuda.synchronize(dev)
            prof[leg] = net.profile()
            net.enable_profile(False)
            net.num_streams = args.streams
        lines.append(f'built-in profiler, separate pass at 1 stream, {args.profile_steps} steps (ms per step, launches per step, TFLOP/s, TB/s of algorithmic bytes):')
        for leg, prefix in (('fp16', 'conv3x3_halo_f16<'), ('bf16x3', 'conv3x3_halo_bf16x3<')):
            tot = 0.0
            for s, (t, n, fl, by) in sorted(prof[leg].items()):
                if s.startswith(prefix):
                    tot += t / args.profile_steps
                    lines.append(f'  {s:78s} {t / args.profile_steps:8.3f} ms  {n // args.profile_steps:3d}  {fl / t / 1e9 if t else 0:7.1f}  {by / t / 1e9 if t else 0:5.2f}')
            lines.append(f'  {leg} conv slots together {tot:8.3f} ms per step; every slot of the step {sum(v[0] for v in prof[leg].values()) / args.profile_steps:8.3f} ms')

        # untimed: the images
        ys = {}
        for leg in LEGS:
            y, idx = nets[leg].test_with_indices(x)
            ys[leg] = (y.double().cpu().numpy(), idx.cpu().numpy())
        ref = ys['fp32'][0]
        lines.append(f'fp32 image range [{ref.min():.3f}, {ref.max():.3f}]')
        for leg in ('bf16x3', 'fp16'):
            d = np.abs(ys[leg][0] - ref)
            mse = float(np.mean(d * d))
            lines.append(f'{leg:7s} against fp32: max abs {d.max():.3e}, PSNR (peak 1) {10 * np.log10(1.0 / mse) if mse else float("inf"):.1f} dB, '
                         f'VQ indices equal: {bool(np.array_equal(ys[leg][1], ys["fp32"][1]))}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

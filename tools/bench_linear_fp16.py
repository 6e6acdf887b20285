"""linear_math 'bf16_split' against 'fp16', each with decoder_math 'fp32' and 'fp16', on bench.py's headline workload, in ONE process, on one MI355X.

    python tools/bench_linear_fp16.py [--steps 20] [--warmup 5] [--rounds 4] [--batch 16] [--streams 3] [--out profiles/linear_fp16_bench.txt]

Workload: bench.py's defaults (its config, weights and inputs are imported / rebuilt from the same seeds): x4, 16 tiles of 128x128 per
step through FeMaSRNet.test, three sub-batch streams, synthetic weights (seed 0), inputs resident in HBM.  bench.py is not touched and
stays the bench of record; the MPix/s printed here are THIS tool's figures.

Legs, as (linear_math, decoder_math): (bf16_split, fp32), (bf16_split, fp16), (fp16, fp32), (fp16, fp16).
Timing: one network per leg (same weights), each warmed up `--warmup` steps; then `--rounds` rounds, in each of which the legs run
`steps / rounds` steps one after the other (A, B, C, D, A, ...), so clock and power drift hit all alike.  A block is timed by the host
clock between two device synchronisations; a leg's ms per step is the mean of its blocks, its spread the max - min of the blocks.
A new leg counts as faster only if it beats the leg with the same decoder_math and 'bf16_split' by more than the larger of the two spreads.
Separate untimed passes afterwards, for the two new legs: the built-in profiler's per-slot times of the gemm_f16 and conv3x3_halo_f16
launches at one stream (serialized), and the image against the (bf16_split, fp32) leg's (max abs, PSNR at peak 1) with the flipped
tokens counted.  Reads neither the reference nor the oracle; needs a GPU and fails without one."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = (('bf16_split', 'fp32'), ('bf16_split', 'fp16'), ('fp16', 'fp32'), ('fp16', 'fp16'))


def _name(leg):
    return f'({leg[0]}, {leg[1]})'


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
        raise SystemExit('bench_linear_fp16 needs a GPU: nothing is measured without one')
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
        net.num_streams, net.linear_math, net.decoder_math = args.streams, leg[0], leg[1]
        nets[leg] = net
    out_mpix = B * 512 * 512 / 1e6
    lines = [f'(linear_math, decoder_math) legs on x4 FeMaSRNet.test, batch {B} of 128x128 LR tiles -> 512x512, {args.streams} streams, synthetic weights (seed 0)',
             f'{torch.cuda.get_device_name(dev)}; warm-up {args.warmup} steps per leg, {args.steps} timed steps per leg in {args.rounds} interleaved rounds, '
             'host clock between device synchronisations']

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
        spread = {leg: max(blocks[leg]) - min(blocks[leg]) for leg in LEGS}
        for leg in LEGS:
            lines.append(f'{_name(leg):20s} {ms[leg]:8.3f} ms per step   {out_mpix / ms[leg] * 1e3:8.2f} MPix/s (this tool)   spread {spread[leg]:.3f}   rounds: ' +
                         ' '.join(f'{b:.3f}' for b in blocks[leg]))
        for dm in ('fp32', 'fp16'):
            new, old = ('fp16', dm), ('bf16_split', dm)
            gain, noise = ms[old] - ms[new], max(spread[new], spread[old])
            lines.append(f'{_name(new)} against {_name(old)}: {gain:+.3f} ms per step ({ms[new] / ms[old]:.4f}), round-to-round spread {noise:.3f}: '
                         f'faster by more than the spread: {gain > noise}')
        if power:
            lines.append(f"over the timed part ({power['samples']} samples of the amdgpu hwmon files): package power mean {power['package_w_mean']} W, max "
                         f"{power['package_w_max']} W, cap {power['cap_w']} W; engine clock median {power['sclk_mhz_median']} MHz, min / max {power['sclk_mhz_min_max']}")
        else:
            lines.append('engine clock / package power: not read (no amdgpu hwmon files for this device)')

        # untimed: per-slot times of the new legs at one stream (every launch serialized between its two events)
        lines.append(f'built-in profiler, separate pass at 1 stream, {args.profile_steps} steps (ms per step, launches per step, TFLOP/s, TB/s of algorithmic bytes):')
        for leg in LEGS:
            net = nets[leg]
            net.num_streams = 1
            net.test(x)
            net.enable_profile(True)
            for _ in range(args.profile_steps):
                net.test(x)
            torch.cuda.synchronize(dev)
            prof = net.profile()
            net.enable_profile(False)
            net.num_streams = args.streams
            lines.append(f' {_name(leg)}: every slot of the step {sum(v[0] for v in prof.values()) / args.profile_steps:8.3f} ms')
            prefixes = ('gemm_f16<', 'conv3x3_halo_f16<') if leg[0] == 'fp16' else ('gemm_bf16s<', 'conv3x3_bf16s<')
            if leg[1] == 'fp16' and leg != ('fp16', 'fp16'):
                continue                    # (the old legs' front slots are listed once, from the (bf16_split, fp32) leg)
            for prefix in prefixes:
                tot = 0.0
                for s, (t, n, fl, by) in sorted(prof.items()):
                    if s.startswith(prefix) and n:
                        tot += t / args.profile_steps
                        lines.append(f'  {s:78s} {t / args.profile_steps:8.3f} ms  {n // args.profile_steps:3d}  {fl / t / 1e9 if t else 0:7.1f}  {by / t / 1e9 if t else 0:5.2f}')
                lines.append(f'  {prefix}...> slots together {tot:8.3f} ms per step')

        # untimed: the images and the index maps
        ys = {}
        for leg in LEGS:
            y, idx = nets[leg].test_with_indices(x)
            ys[leg] = (y.double().cpu().numpy(), idx.cpu().numpy())
        ref, iref = ys[LEGS[0]]
        lines.append(f'{_name(LEGS[0])} image range [{ref.min():.3f}, {ref.max():.3f}], {iref.size} tokens')
        for leg in LEGS[1:]:
            d = np.abs(ys[leg][0] - ref)
            mse = float(np.mean(d * d))
            flips = int((ys[leg][1] != iref).sum())
            lines.append(f'{_name(leg):20s} against {_name(LEGS[0])}: flipped tokens {flips} of {iref.size} ({100.0 * flips / iref.size:.3f} %), max abs {d.max():.3e}, '
                         f'PSNR (peak 1) {10 * np.log10(1.0 / mse) if mse else float("inf"):.1f} dB')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

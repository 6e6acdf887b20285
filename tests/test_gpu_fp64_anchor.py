"""-m gpu: every kernel launch the benchmarked workloads make, at its real shape, against an fp64 restatement of the plain definition.

The unit parity tests compare each kernel bit for bit with the CPU oracle at small shapes, and the oracle restates the kernels' own
arithmetic; this module anchors the kernels to an INDEPENDENT reference (tests/fp64_ref.py, no oracle) where the grid size, the batch
per launch, the last partial tile and the 32-bit offset ranges are the benchmark's.  Workloads (bench.py, 3 sub-batch streams): x4
batch 16 of 128^2, x2 batch 32 of 256^2, HQ forward batch 8 of 512^2; decoder_math 'fp32' (timed) and 'fp32_strict', the default
linear_math.  The launch list comes from the architecture's weight shapes and the resolution schedule (fp64_ref.workload_layers),
each conv's instantiation from the library itself (femasr_debug_conv_variant_name), and test_inventory_covers_every_profiled_slot
fails on any profile slot a real forward fills that no case maps to.

Each case fills its output with a NaN sentinel, checks the whole output on the GPU (no sentinel left, all finite), and compares
sampled positions with fp64: image corners, border rows / columns, the seams of the 8x16 halo tiles and 16x16 Winograd sub-blocks,
the last partial tile, the last image, every output channel (so every 32 / 64 / 128-column block and GroupNorm group boundary).
Per-element bounds and their calibration: tests/fp64_ref.py.
"""
import pytest
import torch

import fp64_ref as R
from anchor_cases import WORST, _gen, inventory, run_conv_case, run_small_case
from femasr_amd import _lib

pytestmark = pytest.mark.gpu

# (the launch inventory and the case runners are shared with tests/test_gpu_product_anchor.py: tests/anchor_cases.py)
WL = list(R.WORKLOADS)


@pytest.mark.parametrize('wl_name', WL)
def test_conv_launches_match_fp64(cuda_device, wl_name):
    convs, _ = inventory(wl_name)
    assert convs
    for i, case in enumerate(sorted(convs.values(), key=lambda c: (c['slot'], c['L']['B'], c['L']['H']))):
        run_conv_case(case, 1000 + i)


@pytest.mark.parametrize('wl_name', WL)
def test_small_kernel_launches_match_fp64(cuda_device, wl_name):
    _, small = inventory(wl_name)
    for i, L in enumerate(small.values()):
        run_small_case(L, 2000 + i)


def test_concat_resize_matches_definition(cuda_device):
    """CombineQuantBlock's nearest resize + concat (multi-codebook configs) at the x4 workload's 72^2 code grid, batch 6: exact."""
    lib = _lib.load()
    g = _gen(7)
    B, H, W, Ca, Hb, Cb = 6, 72, 72, 512, 36, 256
    a = torch.randn((B, H, W, Ca), generator=g, device='cuda')
    b = torch.randn((B, Hb, Hb, Cb), generator=g, device='cuda')
    out = torch.full((B, H, W, Ca + Cb), float('nan'), device='cuda')
    _lib.check(lib.femasr_concat_resize(None, _lib.ptr(a), Ca, _lib.ptr(b), Hb, Hb, Cb, B, H, W, _lib.ptr(out)))
    torch.cuda.synchronize()
    ys = (torch.arange(H, device='cuda') * Hb) // H
    ref = torch.cat([a, b[:, ys][:, :, ys]], -1)
    assert torch.equal(out, ref)


@pytest.mark.parametrize('wl_name', WL)
def test_inventory_covers_every_profiled_slot(cuda_device, wl_name):
    """One bench-shaped forward per mode with the profiler on: every slot it fills maps to a case of the inventory."""
    from femasr_amd.archs import build_network
    from helpers import weights_from_arch
    wl = R.WORKLOADS[wl_name]
    convs, small = inventory(wl_name)
    have = {c['slot'] for c in convs.values()}
    small_slot = {'gn': 'gn_moments', 'ln': 'layernorm', 'attn': 'window_attention', 'vq': 'vq(codebook lookup)',
                  'pad': 'pad/crop/gather layout', 'crop': 'pad/crop/gather layout'}
    have |= {small_slot[L['kind']] for L in small.values()}
    have.add('gn_moments')        # also covered by the fused-partials path of the conv cases
    net = build_network(dict(type='FeMaSRNet', **wl['cfg']))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights_from_arch(wl['cfg'], 3, 'trained').items()}, strict=False)
    net = net.to(cuda_device).eval()
    net.num_streams = R.BENCH_STREAMS
    x = torch.rand((wl['batch'], 3, wl['hw'], wl['hw']), generator=_gen(11), device='cuda')
    missing = {}
    for dm in ('fp32', 'fp32_strict'):
        net.decoder_math = dm
        net.linear_math = 'bf16_split'
        with torch.no_grad():
            net.test(x) if wl['fn'] == 'test' else net(x)
            net.enable_profile(True)
            net.test(x) if wl['fn'] == 'test' else net(x)
            torch.cuda.synchronize()
            prof = net.profile()
            net.enable_profile(False)
        miss = sorted(s for s, v in prof.items() if v[1] > 0 and s not in have)
        if miss:
            missing[dm] = miss
    assert not missing, f'{wl_name}: profile slots with launches but no fp64 case: {missing}'


def test_report_worst_ratios(cuda_device):
    """Prints the worst err / bound per instantiation / kernel of the cases run in this session (-s)."""
    print('\nworst err/bound: ' + ', '.join(f'{k}: {v:.3g}' for k, v in sorted(WORST.items())))

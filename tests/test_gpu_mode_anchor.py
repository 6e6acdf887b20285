"""-m gpu: the launches of the NON-DEFAULT arithmetic modes against fp64, at the benchmark's and the product's shapes.

tests/test_gpu_fp64_anchor.py and tests/test_gpu_product_anchor.py anchor decoder_math 'fp32' / 'fp32_strict' with linear_math
'bf16_split'.  The library ships three more combinations, documented in include/femasr_hip.h and timed by bench.py --full:
  decoder_math 'bf16x3'        every conv behind the lookup (but out_conv) on the bf16 matrix cores, 3-term split: kernels_conv_bf16.hip.
                               No oracle restates it; its bound is C_FORM['bf16x3'], calibrated on the CPU against a model of the
                               SPECIFIED arithmetic (tests/test_fp64_anchor_host.py) and capped at the arithmetic's analytic worst case.
  decoder_math 'fp32_direct'   the direct halo form with GN prologue, fused partials, one or two residuals, and the x2 phase filters at
                               every decoder shape (the default modes meet them only past a Winograd limit).
  linear_math 'fp32'           the LDS-DMA GEMM at the Swin layers' K = 256 / 1024 and real row counts, the direct / conv_igemm forms of
                               every 3x3 conv in front of the lookup.

Sections:
  A  the three benchmarked workloads at the bench's 3 streams: the cases of each mode's inventory that the default inventories do
     not hold (anchor_cases.mode_inventory), and the five bf16x3 instantiations no workload reaches at unit shapes of the same size.
  B  product shapes: the 272^2 window class of a 1440x1440 image at sub-batches 16 and 6 and the whole-image branch at 599x599, with
     the wrap-aware positions, and the B = 1 batch check on the 272^2 cases (the bf16x3 kernel holds its patch offsets as 32-bit
     element offsets: a wrapped one shows there).
  C  the bf16x3 size limit at natural size: B = 2 of 4094 x 4096 x 64 (2 146 435 072 input elements, 1 048 576 under 2^31) against
     fp64; B = 2 of 4096 x 4096 x 64 (exactly 2^31) refused before any launch; and the planner's side: test() on (2, 3, 1020, 1020)
     in bf16x3 mode launches bf16x3 slots below the limit and direct-form slots for the 4096^2 x 64 layers - the conv launches per
     profile slot equal the Python restatement of the planner - within the mode's network contract of the 'fp32' image.
  D  test_mode_inventories_cover_every_profiled_slot: one real forward per mode and bench workload with the profiler on; every slot
     with launches has a case.  This pins fp64_ref.conv_form / the skip schedule of workload_layers to model.hip.

require_memory is the only skip in this module (a device with less free memory than a case needs).
"""
import collections
import ctypes
import time

import pytest
import torch

import fp64_ref as R
from anchor_cases import (MODES, MODE_PRODUCT, WORST, _conv_args, _gen, _slot, bf16x3_unit_cases, conv_case_bytes, inventory,
                          make_case, mode_inventory, require_memory, run_conv_case)
from femasr_amd import _lib

pytestmark = pytest.mark.gpu

MODE_IDS = [f'{dm}-{lm}' for dm, lm in MODES]
PEAK = {}
_DONE = set()
NETWORK_TOL = 1e-3          # max abs on images in [0, 1], as tests/test_gpu_product_anchor.py applies it (tests/test_gpu_network_r2.py holds
                            # bf16x3 against the exact mode at 1e-3 of the output RANGE, about the same number here)


def _free():
    torch.cuda.synchronize()
    PEAK['bytes'] = max(PEAK.get('bytes', 0), torch.cuda.max_memory_allocated())
    torch.cuda.empty_cache()


def _run(convs, seed0, what, **kw):
    t0 = time.time()
    todo = {k: c for k, c in convs.items() if k not in _DONE}
    _DONE.update(todo)
    for i, case in enumerate(sorted(todo.values(), key=lambda c: (c['slot'], c['L']['B'], c['L']['H'], c['L']['W'], c['L']['nres']))):
        L = case['L']
        require_memory(conv_case_bytes(case), f"{case['slot']} B{L['B']} {L['H']}x{L['W']} {L['cin']}->{L['cout']} nres {L['nres']}")
        run_conv_case(case, seed0 + i, **kw)
        _free()
    print(f'{what}: {len(todo)} conv cases ({len(convs) - len(todo)} already run) in {time.time() - t0:.1f} s')


# ---------------------------------------------------------------- A: the benchmarked workloads
@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('wl_name', list(R.WORKLOADS))
def test_mode_conv_launches_match_fp64(cuda_device, wl_name, mode):
    convs, small = mode_inventory([wl_name], *mode)
    assert convs
    assert not small          # (workload_layers lists every GroupNorm's moments pass in every mode: the default inventories hold them all)
    _run(convs, 8000, f'{wl_name} {mode}')


def test_bf16x3_unit_shapes_of_the_unreached_instantiations(cuda_device):
    cases = bf16x3_unit_cases()
    assert len({c['slot'] for c in cases}) == 5
    _run({('unit', i): c for i, c in enumerate(cases)}, 8600, 'bf16x3 unit shapes', wrap=True, batch_check=True)


# ---------------------------------------------------------------- B: product shapes
@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('wl_name', list(MODE_PRODUCT))
def test_mode_product_launches_match_fp64(cuda_device, wl_name, mode):
    convs, small = mode_inventory({wl_name: MODE_PRODUCT[wl_name]}, *mode)
    assert convs
    assert not small
    _run(convs, 9000, f'{wl_name} {mode}', wrap=True, batch_check=wl_name.startswith('tiled'))


# ---------------------------------------------------------------- C: the bf16x3 size limit
def test_bf16x3_just_under_its_size_limit(cuda_device):
    """B = 2 of 4094 x 4096 x 64 -> 64 with the GN prologue: 2 146 435 072 input and output elements, 8.6 GB each (a multiple of 2^31
    bytes falls into both images).  About 55 GiB with the fp64 moments of the prologue's GroupNorm."""
    case = make_case('bf16x3', 2, 4094, 4096, 64, 64, pro=True, key='limit bf16x3')
    assert case['slot'] == 'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_GN_SILU,up2=false,waves=2x2>'
    assert 2 * 4094 * 4096 * 64 == 2146435072 == 2 ** 31 - 2 ** 20
    require_memory(conv_case_bytes(case) + 2 * 4 * 2146435072, case['slot'] + ' B2 4094x4096')
    run_conv_case(case, 9601, wrap=True)
    _free()


def test_bf16x3_refuses_at_its_size_limit(cuda_device):
    """B = 2 of 4096 x 4096 x 64 = 2^31 elements exactly: FEMASR_ERR_INVALID before any launch, the output's sentinel untouched."""
    lib = _lib.load()
    case = make_case('bf16x3', 2, 4096, 4096, 64, 64, pro=True, key='limit bf16x3')
    a = _conv_args(case['L'], 'bf16x3', False)
    require_memory(2 * 4 * 2 ** 31 + (1 << 28), 'bf16x3 refusal 2 x 4096^2 x 64')
    x = torch.zeros((2, 4096, 4096, 64), device='cuda')
    out = torch.full((2, 4096, 4096, 64), float('nan'), device='cuda')
    w = torch.zeros((1 << 20,), device='cuda')
    a.in_, a.w, a.w_bf16x3, a.bias, a.out, a.pro_a, a.pro_b = (x.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), out.data_ptr(),
                                                               w.data_ptr(), w.data_ptr())
    rc = lib.femasr_conv2d(None, ctypes.byref(a))
    torch.cuda.synchronize()
    assert rc == -1, rc          # FEMASR_ERR_INVALID
    assert b'bf16x3' in lib.femasr_last_error()
    assert bool(torch.isnan(out).all())
    del x, out, w
    _free()


def test_phase_filter_form_with_2_to_31_output_elements(cuda_device):
    """The x2 conv in front of those layers: 2 x 2048^2 x 128 -> 2 x 4096^2 x 64, input 2^30 and output exactly 2^31 elements, beyond
    the bf16x3 and the Winograd-type forms, so every mode runs it as four phase filters (32-bit input patch offsets, 64-bit output
    base).  Against fp64 with the wrap-aware positions, fused GroupNorm partials included.  About 45 GiB."""
    case = make_case('direct', 2, 2048, 2048, 128, 64, up2=True, gn_out=True, key='limit x2 phase filters')
    assert case['slot'].startswith('conv3x3_halo<') and 'up2=true' in case['slot'], case['slot']
    assert R.conv_form(case['L'], 'bf16x3', 'bf16_split') == 'direct' and R.conv_form(case['L'], 'fp32', 'bf16_split') == 'direct'
    require_memory(conv_case_bytes(case), case['slot'] + ' B2 2048^2 -> 4096^2')
    run_conv_case(case, 9602, wrap=True)
    _free()


def _net(cfg, device, seed=3):
    from femasr_amd.archs import build_network
    from helpers import weights_from_arch
    net = build_network(dict(type='FeMaSRNet', **cfg))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights_from_arch(cfg, seed, 'trained').items()}, strict=False)
    return net.to(device).eval()


def _expected_conv_slots(cfg, B, hw, fn, dm, lm):
    """{slot: launches} of the conv layers of one call, by the Python restatement of the planner."""
    from anchor_cases import _weight_shapes
    want = collections.Counter()
    for L in R.workload_layers(cfg, B, hw, fn, _weight_shapes(cfg), dm):
        if L['kind'] == 'conv':
            form = R.conv_form(L, dm, lm)
            want[_slot(_conv_args(L, form, dm == 'fp32' and form in ('wino4', 'wino_up2')))] += 1
    return want


def test_planner_leaves_bf16x3_at_the_limit(cuda_device):
    """test() on (2, 3, 1020, 1020), x4: the padded 1024^2 input makes 64-channel decoder tensors of 2 x 4096^2 x 64 = 2^31 elements.
    In bf16x3 mode the planner keeps the 256- and 128-channel stages on the matrix cores and sends the 64-channel ResBlock convs to
    the direct form (64-bit generic kernel); the x2 conv in front of them (input 2^30, output 2^31 elements) too.  Conv launches per
    profile slot == the Python planner's; image within the mode's network contract of the 'fp32' mode's, indices equal.  Two workspaces of
    about 40 GiB each."""
    require_memory(100 * 2 ** 30, 'test() on (2, 3, 1020, 1020), bf16x3 and fp32')
    net = _net(R._X4, cuda_device)
    net.num_streams = 1
    x = torch.rand((2, 3, 1020, 1020), generator=_gen(21), device='cuda')
    want = _expected_conv_slots(R._X4, 2, (1020, 1020), 'test', 'bf16x3', 'bf16_split')
    b16 = {s: n for s, n in want.items() if s.startswith('conv3x3_halo_bf16x3<')}
    assert len(b16) >= 5 and sum(b16.values()) >= 20
    assert sum(n for s, n in want.items() if s.startswith('conv_igemm<') and 'GN_SILU' in s) == 4, sorted(want)      # the 4096^2 x 64 ResBlock convs
    assert sum(n for s, n in want.items() if s.startswith('conv3x3_halo<') and 'up2=true' in s) == 1, sorted(want)    # the x2 conv in front of them
    out = {}
    with torch.no_grad():
        for dm in ('bf16x3', 'fp32'):
            net.decoder_math = dm
            net.test_with_indices(x)
            net.enable_profile(True)
            y, idx = net.test_with_indices(x)
            torch.cuda.synchronize()
            prof = net.profile()
            net.enable_profile(False)
            assert bool(torch.isfinite(y).all())
            out[dm] = (y, idx)
            if dm == 'bf16x3':
                conv_slots = {s: v[1] for s, v in prof.items() if s.startswith(('conv', 'gemm'))}
                assert conv_slots == dict(want), f'profile {sorted(conv_slots.items())} != planner {sorted(want.items())}'
    assert torch.equal(out['bf16x3'][1], out['fp32'][1]), 'indices differ between bf16x3 and fp32'
    d = float((out['bf16x3'][0] - out['fp32'][0]).abs().max())
    print(f'test() on (2, 3, 1020, 1020): bf16x3 against fp32 max abs {d:.3g}')
    assert d <= NETWORK_TOL, d
    del net, x, out
    _free()


# ---------------------------------------------------------------- D: the inventories against the real planner
@pytest.mark.parametrize('mode', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('wl_name', list(R.WORKLOADS))
def test_mode_inventories_cover_every_profiled_slot(cuda_device, wl_name, mode):
    """One bench-shaped forward in the mode with the profiler on: every slot it fills maps to a case of the mode's inventory (the unit
    shapes of section A are NOT counted: what the network launches has to be in a workload's inventory)."""
    dm, lm = mode
    wl = R.WORKLOADS[wl_name]
    convs, small = inventory(wl_name, modes=(dm,), linear_math=lm, split_res2=True)
    have = {c['slot'] for c in convs.values()}
    small_slot = {'gn': 'gn_moments', 'ln': 'layernorm', 'attn': 'window_attention', 'vq': 'vq(codebook lookup)',
                  'pad': 'pad/crop/gather layout', 'crop': 'pad/crop/gather layout'}
    have |= {small_slot[L['kind']] for L in small.values()}
    net = _net(wl['cfg'], cuda_device)
    net.num_streams = R.BENCH_STREAMS
    net.decoder_math, net.linear_math = dm, lm
    x = torch.rand((wl['batch'], 3, wl['hw'], wl['hw']), generator=_gen(11), device='cuda')
    with torch.no_grad():
        net.test(x) if wl['fn'] == 'test' else net(x)
        net.enable_profile(True)
        net.test(x) if wl['fn'] == 'test' else net(x)
        torch.cuda.synchronize()
        prof = net.profile()
        net.enable_profile(False)
    miss = sorted(s for s, v in prof.items() if v[1] > 0 and s not in have)
    # and the other way round for the convs: a slot the Python planner lists for this mode is one the forward launched
    ghost = sorted(c['slot'] for c in convs.values() if c['slot'] not in prof)
    del net, x
    _free()
    assert not miss, f'{wl_name} {mode}: profile slots with launches but no fp64 case: {miss}'
    assert not ghost, f'{wl_name} {mode}: cases of slots the forward never launched: {ghost}'


def test_report_mode_worst_ratios(cuda_device):
    """Prints the worst err / bound per instantiation / kernel of the cases run in this session and the peak device memory (-s)."""
    print('\nmode anchor worst err/bound: ' + ', '.join(f'{k}: {v:.3g}' for k, v in sorted(WORST.items())))
    print(f"mode anchor peak torch.cuda.max_memory_allocated: {PEAK.get('bytes', 0) / 2 ** 30:.2f} GiB")

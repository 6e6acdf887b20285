"""-m gpu: the launches the CLI and the Python API make BY DEFAULT, and the kernels' offset limits, against fp64.

tests/test_gpu_fp64_anchor.py anchors the three benchmarked workloads: square inputs, at most 0.2 G elements per tensor.  The product's
defaults (tile 240, pad 16, max_tile_batch 16; 1 stream in the module, 3 in the CLI) launch larger and rectangular tensors: the tiled
branch runs batches of 16 / 8 / 6 windows of 272^2 (padded to 288^2), whose 64-channel decoder tensors are 5.4 GB (past 2^32 bytes),
2.7 GB (between 2^31 and 2^32) and 2.04 GB (5 % under 2^31), and half of the window classes are rectangular; the whole-image branch
(h*w < 600^2) runs a mixed plan at 599x599 - Winograd at 256 channels, the direct and phase-filter forms at 128 and 64 channels, whose
images are over the Winograd forms' 2^27-element limit.  The launch tables (fp64_ref.PRODUCT_WORKLOADS) are derived from
femasr_amd.tiling, and tests/test_fp64_anchor_host.py holds them to those conditions on the CPU.

Sections:
  B  every distinct launch of ANCHORED (below) through the unit ABI: NaN sentinel, whole-output finite check, fp64 at the structured
     positions of tests/fp64_ref.py with the unchanged per-element bounds, PLUS structured positions on the images in which a 32-bit
     byte offset into any tensor of the case wraps (and the image after), PLUS the whole-tensor batch check: the same instantiation
     at B = 1 on views of image 0, the last and each straddling image must reproduce out[n] and gn_part[n] bit for bit.  Small
     kernels (GroupNorm, LayerNorm, attention, VQ + gather, pad, crop, the uint8 pad / crop pair) at the same shapes.
  C  the network at the same sizes: test_tile on a 1440x1440 image with all defaults == the one-crop-at-a-time reference loop, bit
     for bit, in both fp32 modes, index maps included; streams 2 and 3 == streams 1; test_tile_u8 == output_to_u8(test_tile(.)).
  D  the offset limits at natural size: the Winograd forms 28 672 elements under their per-image limit and refused above it, a batch
     of 16 just under their 2^31-element total limit, window attention below and at its limit, and the direct form past 2^31 and
     2^32 input elements, where the halo kernels' 32-bit element offset would wrap and the launcher uses the 64-bit generic form
     (tests/test_fp64_anchor_host.py pins that shape rule on the CPU), and one test() on 256 tiles in a single call, whose decoder
     tensors pass 2^32 elements, against calls of 16.

ANCHORED is the part of PRODUCT_WORKLOADS this module launches: every window class of the 1440x1440 and the 1356x2040 image (the
ragged 172- and 136-wide ones included) at the batches test_tile launches with one stream (16, 12, 8, 7, 4, 1), the 272^2 class also
at the largest sub-batch of two and three streams (8, 6) - the three size regimes above - and the four whole-image cases.  The smaller
sub-batches of two and three streams (5, 4, 3, 2, 1 windows) are the same instantiations on fewer images; the host test lists them,
this module does not launch them (about 820 further launches; profiles/r09_product_anchor.txt has the cost).

Every case prints the device memory it needs and skips only if the device reports less free; tensors are freed between cases.
Every 'outside the limit' case is a refusal before any launch.
"""
import ctypes
import time

import pytest
import torch

import fp64_ref as R
from anchor_cases import (WORST, _conv_args, _gen, _slot, conv_case_bytes, inventory, product_inventory, require_memory, run_conv_case,
                          run_small_case)
from femasr_amd import _lib, imgproc, tiling

pytestmark = pytest.mark.gpu

ANCHORED = {name: tuple(wl['calls']) for name, wl in R.PRODUCT_WORKLOADS.items()}          # the batches of one stream, whole images
ANCHORED['tiled1440x1440_win272x272'] = (16, 8, 6)                                         # + the largest sub-batch of 2 and 3 streams
PEAK = {}
_DONE = set()          # case keys launched in this session


def _free():
    torch.cuda.synchronize()
    PEAK['bytes'] = max(PEAK.get('bytes', 0), torch.cuda.max_memory_allocated())
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- B: every launch at its product shape
@pytest.mark.parametrize('wl_name', list(ANCHORED))
def test_product_conv_launches_match_fp64(cuda_device, wl_name):
    convs, _ = product_inventory({wl_name: ANCHORED[wl_name]})
    assert convs
    t0 = time.time()
    todo = {k: c for k, c in convs.items() if k not in _DONE}          # (equal launches of another image's workload ran there)
    _DONE.update(todo)
    for i, case in enumerate(sorted(todo.values(), key=lambda c: (c['slot'], c['L']['B'], c['L']['H'], c['L']['W']))):
        L = case['L']
        require_memory(conv_case_bytes(case), f"{case['slot']} B{L['B']} {L['H']}x{L['W']} {L['cin']}->{L['cout']}")
        run_conv_case(case, 5000 + i, wrap=True, batch_check=True)
        _free()
    print(f'{wl_name}: {len(todo)} conv cases ({len(convs) - len(todo)} already run) in {time.time() - t0:.1f} s')


def _small_bytes(L):
    k = L['kind']
    if k == 'gn':
        n = L['B'] * L['H'] * L['W'] * L['c']
        return 4 * n + 8 * 3 * (n // L['B'] if (L['B'] > 1 and n > 2 ** 28) else n) + (1 << 28)
    if k == 'ln':
        return 4 * 3 * L['rows'] * L['c'] + (1 << 28)
    if k == 'attn':
        return 4 * 5 * L['B'] * L['H'] * L['W'] * L['c'] + (1 << 28)
    if k == 'vq':
        return 4 * L['M'] * (5 * L['d'] + 2 * 1024) + (1 << 28)
    return 4 * 4 * L['B'] * L['H'] * L['W'] * L['c'] + (1 << 28)


@pytest.mark.parametrize('wl_name', list(ANCHORED))
def test_product_small_kernel_launches_match_fp64(cuda_device, wl_name):
    """gn, ln (331 776 rows at B = 16), attn, vq (both lookups and the gather) against fp64; pad and crop exact against the torch
    expression at rectangular and ragged Hp, Wp."""
    _, small = product_inventory({wl_name: ANCHORED[wl_name]})
    assert small
    todo = {k: L for k, L in small.items() if k not in _DONE}
    _DONE.update(todo)
    for i, L in enumerate(todo.values()):
        require_memory(_small_bytes(L), f"{L['kind']} {({k: v for k, v in L.items() if k not in ('kind', 'key')})}")
        run_small_case(L, 6000 + i)
        _free()


@pytest.mark.parametrize('B,h,w,scale', [(16, 272, 272, 4), (8, 256, 272, 4), (1, 599, 599, 4), (1, 339, 510, 4)])
@pytest.mark.parametrize('bgr', [0, 1])
def test_u8_pad_and_crop_match_the_fp32_kernels(cuda_device, B, h, w, scale, bgr):
    """femasr_pad_u8hwc_to_nhwc == femasr_pad_nchw_to_nhwc of u8 / 255 (imgproc.u8_to_input), femasr_crop_nhwc_to_u8hwc ==
    imgproc.output_to_u8 of femasr_crop_nhwc_to_nchw: exact, at the tiled and the whole-image shapes."""
    lib = _lib.load()
    g = _gen(31 + B + bgr)
    Hp, Wp = tiling.padded_hw(h, w, scale)
    require_memory(4 * B * (2 * 3 * Hp * Wp + 3 * h * w + 3 * 3 * Hp * Wp * scale * scale) + (1 << 28), f'u8 pad / crop B{B} {h}x{w}')
    u8 = torch.randint(0, 256, (B, h, w, 3), generator=g, device='cuda', dtype=torch.uint8)
    got = torch.full((B, Hp, Wp, 3), float('nan'), device='cuda')
    _lib.check(lib.femasr_pad_u8hwc_to_nhwc(None, _lib.ptr(u8), B, h, w, bgr, Hp, Wp, _lib.ptr(got)))
    x = torch.stack([imgproc.u8_to_input(u8[n], bgr=bool(bgr))[0] for n in range(B)]).contiguous()
    assert x.shape == (B, 3, h, w)
    want = torch.full((B, Hp, Wp, 3), float('nan'), device='cuda')
    _lib.check(lib.femasr_pad_nchw_to_nhwc(None, _lib.ptr(x), B, 3, h, w, Hp, Wp, _lib.ptr(want)))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    Hs, Ws, Hc, Wc = Hp * scale, Wp * scale, h * scale, w * scale
    y = torch.rand((B, Hs, Ws, 3), generator=g, device='cuda') * 1.2 - 0.1          # some values outside [0, 1]: the clamp
    y[:, ::7, ::5] = (torch.randint(0, 256, (B, (Hs + 6) // 7, (Ws + 4) // 5, 3), generator=g, device='cuda').float() + 0.5) / 255.0     # ties
    got8 = torch.full((B, Hc, Wc, 3), 77, device='cuda', dtype=torch.uint8)
    _lib.check(lib.femasr_crop_nhwc_to_u8hwc(None, _lib.ptr(y), B, Hs, Ws, Hc, Wc, bgr, _lib.ptr(got8)))
    f = torch.full((B, 3, Hc, Wc), float('nan'), device='cuda')
    _lib.check(lib.femasr_crop_nhwc_to_nchw(None, _lib.ptr(y), B, Hs, Ws, 3, Hc, Wc, _lib.ptr(f)))
    torch.cuda.synchronize()
    want8 = torch.stack([imgproc.output_to_u8(f[n:n + 1], bgr=bool(bgr)) for n in range(B)]).reshape(B, Hc, Wc, 3)
    assert torch.equal(got8, want8)
    del u8, got, want, x, y, got8, f, want8
    _free()


def _net(cfg, device, seed=3):
    from femasr_amd.archs import build_network
    from helpers import weights_from_arch
    net = build_network(dict(type='FeMaSRNet', **cfg))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights_from_arch(cfg, seed, 'trained').items()}, strict=False)
    return net.to(device).eval()


@pytest.mark.parametrize('which', ['test_tile_1440_streams1', 'test_whole_599'])
def test_product_inventory_covers_every_profiled_slot(cuda_device, which):
    """One real test_tile on the 1440^2 image at num_streams = 1 and one whole-image test() at 599x599, with the profiler on: every
    slot with launches maps to a case of the bench or the product inventory."""
    names = ({k: R.PRODUCT_WORKLOADS[k]['calls'] for k in ANCHORED if k.startswith('tiled1440x1440_')} if which.startswith('test_tile')
             else {'whole599x599_x4': None})
    have, small = set(), {}
    for n, subs in names.items():
        c, s = inventory(n, sub_batches=subs)
        have |= {v['slot'] for v in c.values()}
        small.update(s)
    small_slot = {'gn': 'gn_moments', 'ln': 'layernorm', 'attn': 'window_attention', 'vq': 'vq(codebook lookup)',
                  'pad': 'pad/crop/gather layout', 'crop': 'pad/crop/gather layout'}
    have |= {small_slot[L['kind']] for L in small.values()}
    have.add('gn_moments')        # also covered by the fused-partials path of the conv cases
    net = _net(R._X4, cuda_device)
    net.num_streams = 1
    side = 1440 if which.startswith('test_tile') else 599
    require_memory(60 * 2 ** 30 if side == 1440 else 30 * 2 ** 30, which)
    x = torch.rand((1, 3, side, side), generator=_gen(12), device='cuda')
    missing = {}
    for dm in ('fp32', 'fp32_strict'):
        net.decoder_math = dm
        run = (lambda: net.test_tile(x)) if side == 1440 else (lambda: net.test(x))
        with torch.no_grad():
            run()
            net.enable_profile(True)
            run()
            torch.cuda.synchronize()
            prof = net.profile()
            net.enable_profile(False)
        miss = sorted(s for s, v in prof.items() if v[1] > 0 and s not in have)
        if miss:
            missing[dm] = miss
    del net, x
    _free()
    assert not missing, f'{which}: profile slots with launches but no fp64 case: {missing}'


# ---------------------------------------------------------------- C: the network at the same sizes
@pytest.fixture(scope='module')
def image1440(cuda_device):
    return torch.rand((1, 3, 1440, 1440), generator=_gen(77), device='cuda')


@pytest.mark.parametrize('dm', ['fp32_strict', 'fp32'])
def test_tile_defaults_equal_the_one_crop_loop(cuda_device, image1440, dm):
    """test_tile(x) with all defaults (one stream: the 272^2 class is ONE B = 16 call, 5.4 GB activations) == test() on each of the 36
    crops one at a time, pasted with Tile.out_src / out_dst; the index maps of the batched calls == the single calls'; streams 2 and
    3 == streams 1.  Same kernels, deterministic: equality.  Needs about 60 GiB."""
    require_memory(60 * 2 ** 30, f'test_tile 1440x1440 {dm}')
    net = _net(R._X4, cuda_device)
    net.decoder_math = dm
    x = image1440
    assert (net.num_streams, net.max_tile_batch) == (1, 16)
    with torch.no_grad():
        got = net.test_tile(x)
        tiles = tiling.enumerate_tiles(1440, 1440, 240, 16)
        assert len(tiles) == 36
        want = torch.zeros_like(got)
        single_idx = {}
        for t in tiles:
            crop = x[:, :, t.y0p:t.y1p, t.x0p:t.x1p].contiguous()
            y, idx = net.test_with_indices(crop)
            single_idx[t.index] = idx
            ys, ye, xs, xe = t.out_src(4)
            dy, dye, dx, dxe = t.out_dst(4)
            want[:, :, dy:dye, dx:dxe] = y[:, :, ys:ye, xs:xe]
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, want), f'{dm}: test_tile differs from the one-crop loop in {int((got != want).sum())} values'
        for hw, tl in tiling.shape_classes(tiles).items():          # the batched calls test_tile made, with their index maps
            crops = torch.cat([x[:, :, t.y0p:t.y1p, t.x0p:t.x1p] for t in tl], 0).contiguous()
            yb, ib = net.test_with_indices(crops)
            for k, t in enumerate(tl):
                assert torch.equal(ib[k:k + 1], single_idx[t.index]), f'{dm}: index map of tile {t.index} (class {hw}, B {len(tl)})'
            del crops, yb, ib
        for s in (2, 3):
            net.num_streams = s
            assert torch.equal(net.test_tile(x), got), f'{dm}: num_streams {s} differs from 1'
    del net, got, want
    _free()


def test_tile_u8_equals_the_fp32_path(cuda_device, image1440):
    require_memory(60 * 2 ** 30, 'test_tile_u8 1440x1440')
    net = _net(R._X4, cuda_device)
    u8 = (image1440[0].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    with torch.no_grad():
        got = net.test_tile_u8(u8)
        want = imgproc.output_to_u8(net.test_tile(imgproc.u8_to_input(u8)))
    assert got.shape == (5760, 5760, 3) and torch.equal(got, want.reshape(got.shape))
    del net, got, want
    _free()


# ---------------------------------------------------------------- D: the offset limits at natural size
def _limit_case(form, B, H, W, cin, cout, up2=False, pro=False, nres=0, gn_out=False, fast=False):
    L = dict(kind='conv', key=f'limit {form}', B=B, H=H, W=W, cin=cin, cout=cout, ksz=3, stride=1, pad=1, up2=up2, pro=pro, nres=nres,
             act=0, behind=True, gn_out=gn_out, in_add=False)
    return dict(L=L, form=form, fast=fast, slot=_slot(_conv_args(L, form, fast)))


def test_wino_forms_just_under_their_per_image_limit(cuda_device):
    """64 -> 64 channels, B = 1, 1448^2 = 134 189 056 elements per image: 28 672 under 2^27, not a multiple of 16 (partial sub-blocks).
    wino4 with GN prologue, one residual and gn_part; wino_up2 from 724^2.  About 3 GiB each."""
    for case in (_limit_case('wino4', 1, 1448, 1448, 64, 64, pro=True, nres=1, gn_out=True),
                 _limit_case('wino4', 1, 1448, 1448, 64, 64, pro=True, nres=1, gn_out=True, fast=True),
                 _limit_case('wino_up2', 1, 724, 724, 64, 64, up2=True, gn_out=True)):
        assert case['slot'].startswith('conv3x3_wino'), case['slot']
        assert 2 ** 27 - 1448 * 1448 * 64 == 28672
        require_memory(conv_case_bytes(case), case['slot'] + ' 1448^2')
        run_conv_case(case, 7001, wrap=True)
        _free()


@pytest.mark.parametrize('up2', [False, True])
def test_wino_forms_refuse_above_their_per_image_limit(cuda_device, up2):
    """1456^2 x 64 = 135 675 904 > 2^27: FEMASR_ERR_INVALID, the output sentinel untouched (no launch)."""
    lib = _lib.load()
    H = 728 if up2 else 1456
    case = _limit_case('wino_up2' if up2 else 'wino4', 1, H, H, 64, 64, up2=up2)
    a = _conv_args(case['L'], case['form'], False)
    require_memory(4 * (1456 * 1456 * 64 * 2) + (1 << 28), 'wino refusal 1456^2')
    x = torch.zeros((1, H, H, 64), device='cuda')
    out = torch.full((1, 1456, 1456, 64), float('nan'), device='cuda')
    w = torch.zeros((1 << 20,), device='cuda')
    a.in_, a.w, a.w_wino, a.bias, a.out = x.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), out.data_ptr()
    rc = lib.femasr_conv2d(None, ctypes.byref(a))
    torch.cuda.synchronize()
    assert rc == -1, rc          # FEMASR_ERR_INVALID
    assert bool(torch.isnan(out).all())
    del x, out, w
    _free()


def test_wino4_batch_just_under_the_total_limit(cuda_device):
    """16 x 1440^2 x 64 = 2 123 366 400 elements (2^31 = 2 147 483 648), 8.5 GB per tensor, three held (input, residual, output):
    wrap-aware sampling (a multiple of 2^31 bytes falls into images 4, 8 and 12) and the B = 1 batch check.  About 36 GiB."""
    case = _limit_case('wino4', 16, 1440, 1440, 64, 64, pro=True, nres=1)
    assert case['slot'].startswith('conv3x3_wino4<')
    assert R.straddle_images(16, 1440 * 1440 * 64 * 4)[0] == 4
    require_memory(conv_case_bytes(case), case['slot'] + ' B16 1440^2')
    run_conv_case(case, 7002, wrap=True, batch_check=True)
    _free()


def test_attention_below_and_at_its_limit(cuda_device):
    """window_attention indexes one image's qkv with 32-bit byte offsets: H*W*3C < 2^30.  1176^2 x 768 (4.2 GB of qkv, B = 1) is the
    last 8-aligned square below it and is anchored to fp64; 1184^2 is refused before any launch.  About 7 GiB."""
    lib = _lib.load()
    assert 1176 * 1176 * 768 < 2 ** 30 <= 1184 * 1184 * 768
    assert lib.femasr_window_attention(None, 1, 1, 1184, 1184, 256, 8, 0, 1, 1) == -1          # FEMASR_ERR_INVALID
    assert b'32-bit' in lib.femasr_last_error()
    for i, shift in enumerate((0, 4)):
        L = dict(kind='attn', B=1, H=1176, W=1176, c=256, shift=shift, key='limit attn')
        require_memory(_small_bytes(L), f'window_attention 1176^2 shift {shift}')
        run_small_case(L, 7100 + i)
        _free()


def test_direct_form_past_2_to_32_input_elements(cuda_device):
    """out_conv's shape (64 -> 3, 3x3) at B = 18 of 2048^2: 4 831 838 208 input elements = 18 GiB, past 2^32 elements, where the 32-bit
    ELEMENT offset of the halo / out_conv kernels would wrap: the launcher's shape rule (B*H*W*Cin < 2^31) has sent the layer to the
    generic implicit-GEMM form, whose offsets are 64-bit.  Anchored on every image, those behind the wrap (16, 17) included; 0.9 GiB
    of output.  The same at 2^31 < elements < 2^32 (B = 9, 9 GiB), with a GN prologue at 64 -> 64, and a nearest-x2 conv.
    About 20 / 10 / 33 / 28 GiB."""
    for B, H, cin, cout, pro, up2 in ((18, 2048, 64, 3, False, False), (9, 2048, 64, 3, False, False), (9, 2048, 64, 64, True, False),
                                      (17, 1024, 128, 32, False, True)):          # the last: nearest-x2 in the generic form, 2.28 G in and out
        case = _limit_case('direct', B, H, H, cin, cout, pro=pro, up2=up2)
        assert case['slot'].startswith('conv_igemm<'), case['slot']
        require_memory(conv_case_bytes(case), f"{case['slot']} B{B} {H}^2 {cin}->{cout}{' x2' if up2 else ''}")
        run_conv_case(case, 7200 + B, wrap=True)
        _free()


NETWORK_TOL = 1e-3          # the suite's network-level bound (max abs, fp32 output; tests/test_gpu_network_r3.py, test_oracle_golden_r2.py)


@pytest.mark.parametrize('dm', ['fp32_strict', 'fp32'])
def test_forward_with_a_batch_past_2_to_32_elements(cuda_device, dm):
    """max_tile_batch is a public knob: test() on 256 tiles of 128^2 in ONE call makes 64-channel decoder tensors of 256 x 576^2 x 64 =
    5.4 G elements (past 2^32: image 202 holds element 2^32), where the planner's shape rules send every conv behind the lookup to the
    generic 64-bit form.  Against calls of 16 tiles (Winograd / halo forms, so not bit for bit): the index maps are equal and the
    image agrees within the suite's network-level bound on the first images, the one the wrap falls into and the last ones.
    Needs about 86 GiB."""
    require_memory(90 * 2 ** 30, f'test() on 256 tiles of 128^2, {dm}')
    assert 2 ** 32 // (576 * 576 * 64) == 202
    net = _net(R._X4, cuda_device)
    net.decoder_math = dm
    x = torch.rand((256, 3, 128, 128), generator=_gen(5), device='cuda')
    with torch.no_grad():
        big, ibig = net.test_with_indices(x)
        assert bool(torch.isfinite(big).all())
        for i in (0, 96, 192, 208, 240):          # images 101 (2^31 elements) and 202 (2^32) are inside
            y, idx = net.test_with_indices(x[i:i + 16])
            assert torch.equal(ibig[i:i + 16], idx), f'{dm}: index maps of images {i}..{i + 15}'
            d = float((big[i:i + 16] - y).abs().max())
            print(f'{dm}: images {i}..{i + 15}: max abs difference to the call of 16: {d:.3g}')
            assert d <= NETWORK_TOL, (dm, i, d)
    del net, x, big, ibig
    _free()


def test_report_product_worst_ratios(cuda_device):
    """Prints the worst err / bound per instantiation / kernel of the cases run in this session and the peak device memory (-s)."""
    print('\nproduct anchor worst err/bound: ' + ', '.join(f'{k}: {v:.3g}' for k, v in sorted(WORST.items())))
    print(f"product anchor peak torch.cuda.max_memory_allocated: {PEAK.get('bytes', 0) / 2 ** 30:.2f} GiB")

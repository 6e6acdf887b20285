"""-m gpu: every HIP kernel, called through the C ABI, against the CPU oracle on the same seeded inputs.
Bar: BIT-EXACT (the kernels implement the oracle's arithmetic specification: fmaf chains in ascending
k on the fp32 matrix cores, fixed-order moments, explicit exp/erf) — asserted with array_equal; the
message reports max-abs so a regression is quantified."""
import numpy as np
import pytest
import torch

from femasr_amd import _lib, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        raise AssertionError(f'{what}: not bit-identical: max-abs {np.nanmax(d):.3e}, mismatching {np.sum(got != ref)} '
                             f'of {got.size}, nan {np.isnan(got).sum()}')


def test_native_library_is_loaded(cuda_device):
    lib = _lib.load()
    assert lib.femasr_version() >= 100
    with open('/proc/self/maps') as f:
        assert 'libfemasr_hip.so' in f.read()


def test_pad_crop_exact(cuda_device):
    import gpu_utils as G
    lib = _lib.load()
    x = synth.uniform(0, 'px', (3, 3, 21, 30), 0, 1)
    tx = G.dev(x)
    out = torch.empty((3, 32, 32, 3), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_pad_nchw_to_nhwc(None, _lib.ptr(tx), 3, 3, 21, 30, 32, 32, _lib.ptr(out)))
    _same(out.cpu().numpy(), orc.pad_nchw_to_nhwc(x, 32, 32), 'pad')
    y = synth.uniform(1, 'cy', (2, 40, 48, 3), -1, 1)
    ty = G.dev(y)
    o2 = torch.empty((2, 3, 33, 47), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_crop_nhwc_to_nchw(None, _lib.ptr(ty), 2, 40, 48, 3, 33, 47, _lib.ptr(o2)))
    _same(o2.cpu().numpy(), orc.crop_nhwc_to_nchw(y, 33, 47), 'crop')
    # error behaviour: pad larger than the image is refused (the reference would mis-slice silently)
    assert lib.femasr_pad_nchw_to_nhwc(None, _lib.ptr(tx), 3, 3, 21, 30, 64, 32, _lib.ptr(out)) != 0


def test_unit_float_to_byte_rule_at_ties_and_non_finite(cuda_device):
    """The one float -> byte rule (csrc/pixel.h: clamp to [0,1], NaN -> 0, x255, round half to even) through both kernels that end in it,
    femasr_crop_nhwc_to_u8hwc (both channel orders) and femasr_image_f32_to_u8: NaN, +-inf, -0.0, values outside [0,1], and for every k in
    0..254 the fp32 value nearest (k + 0.5)/255 with its two neighbours, where x255 lands on, just below or just above a tie.  These are
    775 values and a 13x17 RGB image holds 663, so they fill two such images (the rest: uniform in [-0.5, 1.5])."""
    import gpu_utils as G
    lib = _lib.load()
    tie = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1e-3, -7.0, 1.0, 1.0 + 2.0 ** -23, 3.5], dtype=np.float32)
    vals = np.concatenate([special, np.nextafter(tie, np.float32(0)), tie, np.nextafter(tie, np.float32(2))])
    B, H, W = 2, 13, 17
    v = synth.uniform(2, 'ties', (B * H * W * 3,), -0.5, 1.5).astype(np.float32)
    v[:vals.size] = vals
    v = np.random.default_rng(0).permutation(v).reshape(B, H, W, 3)
    with np.errstate(invalid='ignore'):
        ref = np.rint(np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))) * np.float32(255))
    assert ref.dtype == np.float32
    ref = ref.astype(np.uint8)
    assert len(np.unique(ref)) == 256
    tv = G.dev(v)
    chw = [G.dev(np.ascontiguousarray(v[b].transpose(2, 0, 1))) for b in range(B)]
    for swap in (0, 1):
        want = ref[..., ::-1] if swap else ref
        crop = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda')
        _lib.check(lib.femasr_crop_nhwc_to_u8hwc(None, _lib.ptr(tv), B, H, W, H, W, swap, _lib.ptr(crop)))
        _same(crop.cpu().numpy(), want, f'crop_nhwc_to_u8hwc swap {swap}')
        img = torch.empty((B, H, W, 3), dtype=torch.uint8, device='cuda')
        for b in range(B):
            _lib.check(lib.femasr_image_f32_to_u8(None, _lib.ptr(chw[b]), H, W, swap, _lib.ptr(img[b])))
        _same(img.cpu().numpy(), want, f'image_f32_to_u8 swap {swap}')
        _same(img.cpu().numpy(), crop.cpu().numpy(), f'image_f32_to_u8 against crop_nhwc_to_u8hwc, swap {swap}')


CONV_CASES = [
    # name, (B,H,W,Cin), Cout, k, s, p, up2
    ('in_conv_k4_cin3', (2, 31, 33, 3), 256, 4, 1, 1, False),
    ('in_conv_k4_cin3_c64', (1, 17, 16, 3), 64, 4, 1, 1, False),
    ('down_s2_odd', (2, 31, 29, 256), 256, 3, 2, 1, False),
    ('k3_256', (1, 16, 24, 256), 256, 3, 1, 1, False),
    ('up2_256_128', (2, 9, 12, 256), 128, 3, 1, 1, True),
    ('k1_256_512', (1, 16, 16, 256), 512, 1, 1, 0, False),
    ('k3_512_256', (1, 8, 8, 512), 256, 3, 1, 1, False),
    ('cout64', (1, 20, 24, 128), 64, 3, 1, 1, True),
    ('cout3', (2, 24, 20, 64), 3, 3, 1, 1, False),
    ('tiny_m', (1, 3, 5, 32), 96, 3, 1, 1, False),
    ('halo_edges_17x23', (2, 17, 23, 64), 128, 3, 1, 1, False),      # tiles overhang both edges
    ('halo_up2_odd', (1, 7, 9, 128), 64, 3, 1, 1, True),              # fused x2, 14x18 output
    ('halo_up2_cout3', (1, 5, 6, 32), 3, 3, 1, 1, True),
    ('k3_no_pad', (1, 12, 12, 64), 64, 3, 1, 0, False),               # pad 0 -> im2col kernel
]


@pytest.fixture
def conv_small(request):
    """Threshold of the small-launch rule of the convs (femasr_conv_small_launch_blocks): 0 = 128-column blocks as for the big
    launches, -1 = the default (small launches take 64-column blocks)."""
    lib = _lib.load()
    prev = lib.femasr_conv_small_launch_blocks(request.param)
    yield request.param
    lib.femasr_conv_small_launch_blocks(prev)


CONV_SMALL = pytest.mark.parametrize('conv_small', [0, -1], indirect=True, ids=['bn128', 'small_launch_bn64'])


@CONV_SMALL
@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_bit_exact(cuda_device, case, conv_small):
    import gpu_utils as G
    name, shp, cout, k, s, p, up = case
    x = synth.uniform(1, name + 'x', shp, -1.5, 1.5)
    w = synth.uniform(1, name + 'w', (k, k, shp[3], cout), -0.1, 0.1)
    b = synth.uniform(1, name + 'b', (cout,), -0.5, 0.5)
    _same(G.conv2d(x, w, b, k, s, p, up), orc.conv2d(x, w, b, k, s, p, up), name)


@CONV_SMALL
@pytest.mark.parametrize('cin,cout', [(256, 256), (128, 128), (64, 64), (64, 3), (128, 64)])
def test_conv_gn_silu_prologue_and_residuals(cuda_device, cin, cout, conv_small):
    """ResBlock conv: GroupNorm-apply + SiLU fused on load, bias + two residual adds fused on store."""
    import gpu_utils as G
    x = synth.uniform(2, 'gx', (2, 13, 10, cin), -3, 4)
    gamma = synth.uniform(2, 'gg', (cin,), 0.5, 1.5)
    beta = synth.uniform(2, 'gb', (cin,), -0.5, 0.5)
    a_ref, b_ref = orc.gn_coeffs(x, gamma, beta)
    a, bb = G.gn_coeffs(x, gamma, beta)
    _same(a, a_ref, 'gn a')
    _same(bb, b_ref, 'gn b')
    w = synth.uniform(2, 'gw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(2, 'gbias', (cout,), -0.5, 0.5)
    r1 = synth.uniform(2, 'r1', (2, 13, 10, cout), -1, 1)
    r2 = synth.uniform(2, 'r2', (2, 13, 10, cout), -1, 1)
    ref = orc.conv2d(orc.scale_shift_silu(x, a_ref, b_ref), w, bias, 3, 1, 1, res1=r1, res2=r2)
    got = G.conv2d(x, w, bias, 3, 1, 1, prologue=_lib.PRO_GN_SILU, pro=(a_ref, b_ref, None), res1=r1, res2=r2)
    _same(got, ref, f'conv gn_silu {cin}->{cout}')


def test_gn_moments_large_and_offset(cuda_device):
    """Cancellation-prone case: large mean, small variance, H*W big enough for many rows."""
    import gpu_utils as G
    x = synth.uniform(3, 'big', (1, 96, 80, 64), 99.0, 101.0)
    g = synth.uniform(3, 'g', (64,), 0.5, 1.5)
    b = synth.uniform(3, 'b', (64,), -0.5, 0.5)
    a_ref, b_ref = orc.gn_coeffs(x, g, b)
    a, bb = G.gn_coeffs(x, g, b)
    _same(a, a_ref, 'gn a (offset)')
    _same(bb, b_ref, 'gn b (offset)')


@pytest.fixture
def gemm_cfg(request):
    """Force one block configuration of the LDS-DMA GEMM (femasr_gemm_force_config); -1 = the automatic choice."""
    lib = _lib.load()
    prev = lib.femasr_gemm_force_config(request.param)
    yield request.param
    lib.femasr_gemm_force_config(prev)


GEMM_CFGS = pytest.mark.parametrize('gemm_cfg', [-1, 0, 1, 2], indirect=True, ids=['auto', '128x128_k32', '128x128_k16', '64x64'])


@GEMM_CFGS
@pytest.mark.parametrize('cout,act', [(768, 0), (1024, 1), (256, 0)])
def test_linear_ln_prologue_gelu(cuda_device, cout, act, gemm_cfg):
    """Swin linears: LayerNorm pass (norm1 / norm2) -> LDS-DMA GEMM (qkv / fc1), exact-erf GELU + residual on store."""
    import gpu_utils as G
    rows = 300
    x = synth.uniform(4, 'lx', (rows, 256), -4, 6)
    gamma = synth.uniform(4, 'lg', (256,), 0.5, 1.5)
    beta = synth.uniform(4, 'lb', (256,), -0.5, 0.5)
    w = synth.uniform(4, 'lw', (256, cout), -0.1, 0.1)
    bias = synth.uniform(4, 'lbias', (cout,), -0.5, 0.5)
    res = synth.uniform(4, 'lres', (rows, cout), -1, 1) if cout == 256 else None
    xn_ref = orc.layernorm(x, gamma, beta)
    xn = G.layernorm(x, gamma, beta)
    _same(xn, xn_ref, 'layernorm')
    ref = orc.linear(xn_ref, w, bias, act=act, res=res)
    got = G.conv2d(xn.reshape(1, rows, 1, 256), w.reshape(1, 1, 256, cout), bias, 1, act=act,
                   res1=None if res is None else res.reshape(1, rows, 1, cout))
    _same(got.reshape(rows, cout), ref, f'linear ln cout={cout} act={act}')


@GEMM_CFGS
def test_linear_k1024(cuda_device, gemm_cfg):
    import gpu_utils as G
    rows = 200
    x = synth.uniform(5, 'fx', (rows, 1024), -1, 1)
    w = synth.uniform(5, 'fw', (1024, 256), -0.05, 0.05)
    bias = synth.uniform(5, 'fb', (256,), -0.5, 0.5)
    res = synth.uniform(5, 'fr', (rows, 256), -1, 1)
    got = G.conv2d(x.reshape(1, rows, 1, 1024), w.reshape(1, 1, 1024, 256), bias, 1, res1=res.reshape(1, rows, 1, 256))
    _same(got.reshape(rows, 256), orc.linear(x, w, bias, res=res), 'fc2')


@GEMM_CFGS
@pytest.mark.parametrize('n,k', [(96, 64), (160, 32)])
def test_linear_ragged_columns_all_configs(cuda_device, n, k, gemm_cfg):
    """N not a multiple of the block tile (64 / 128) nor of the packed 32-column tiles' pair; M with a ragged last row tile."""
    import gpu_utils as G
    rows = 77 + 64 * 3
    x = synth.uniform(8, 'rx', (rows, k), -1, 1)
    w = synth.uniform(8, 'rw', (k, n), -0.2, 0.2)
    bias = synth.uniform(8, 'rb', (n,), -0.5, 0.5)
    r1 = synth.uniform(8, 'rr1', (rows, n), -1, 1)
    r2 = synth.uniform(8, 'rr2', (rows, n), -1, 1)
    got = G.conv2d(x.reshape(1, rows, 1, k), w.reshape(1, 1, k, n), bias, 1, res1=r1.reshape(1, rows, 1, n), res2=r2.reshape(1, rows, 1, n))
    ref = orc.linear(x, w, bias, res=r1) + r2
    _same(got.reshape(rows, n), ref, f'ragged linear n={n} k={k}')


@pytest.mark.parametrize('shift', [0, 4])
def test_window_attention_bit_exact(cuda_device, shift):
    import gpu_utils as G
    b, h, w, c = 2, 16, 24, 256
    qkv = synth.uniform(6 + shift, 'qkv', (b, h * w, 3 * c), -2, 2)
    table = synth.uniform(6, 'tab', (225, 8), -0.5, 0.5)
    _same(G.window_attention(qkv, b, h, w, c, 8, shift, table),
          orc.window_attention(qkv, b, h, w, c, 8, shift, table), f'window attention shift={shift}')


def test_vq_bit_exact_and_first_min_tie(cuda_device):
    import gpu_utils as G
    cb = synth.uniform(5, 'vq.codebook', (1024, 512), -1.0, 1.0)
    cb[700] = cb[13]
    cb[901] = cb[13]                       # exact ties across n-blocks (cols 13, 700, 901 -> blocks 0, 5, 7)
    cb[14] = cb[13]                        # and inside one 32-column MFMA tile
    z = synth.uniform(6, 'vq.rows', (333, 512), -1.0, 1.0)
    z[0] = cb[13] * 0.97
    z[200] = cb[700] * 1.02
    idx_ref, zq_ref = orc.vq(z, cb)
    idx, zq, cbt, ee = G.vq(z, cb)
    assert idx[0] == 13 and idx[200] == 13
    assert np.array_equal(cbt, G.lib_weight_layout(cb.T.reshape(1, 1, 512, 1024)))
    _same(idx, idx_ref, 'vq indices')
    _same(zq, zq_ref, 'vq z_q')
    # reference init regime: codes tiny against |z|^2 -> distances quantised to the ulp of |z|^2, many exact ties
    cb2 = synth.uniform(7, 'vq.cb.init', (1024, 512), -1.0 / 1024, 1.0 / 1024)
    z2 = synth.uniform(7, 'vq.rows2', (257, 512), -1.0, 1.0)
    idx_ref2, zq_ref2 = orc.vq(z2, cb2)
    idx2, zq2, _, _ = G.vq(z2, cb2)
    _same(idx2, idx_ref2, 'vq indices (init codebook)')
    _same(zq2, zq_ref2, 'vq z_q (init codebook)')


BF16_CASES = [
    # name, (B,H,W,Cin), Cout, up2, gn
    ('b16_256_256', (1, 16, 24, 256), 256, False, False),
    ('b16_up2_256_128', (2, 9, 12, 256), 128, True, False),
    ('b16_gn_64_64', (1, 20, 33, 64), 64, False, True),
    ('b16_gn_128_128_edges', (2, 13, 10, 128), 128, False, True),
    ('b16_cout3', (1, 24, 20, 64), 3, False, False),
    ('b16_up2_128_64', (1, 7, 9, 128), 64, True, False),
    ('b16_gn_256_256_edges', (2, 13, 21, 256), 256, False, True),     # 256-wide block: 128 px x 64 ch per wave
    ('b16_up2_256_256', (1, 9, 12, 256), 256, True, False),
    ('b16_gn_64_256', (1, 17, 16, 64), 256, False, True),
    ('b16_gn_32_64_one_block', (2, 11, 19, 32), 64, False, True),     # single channel block, single-buffered patch
    ('b16_32_3', (1, 9, 40, 32), 3, False, False),
    ('b16_gn_128_64', (1, 24, 16, 128), 64, False, True),             # 4 channel blocks through the single buffer
]


@pytest.mark.parametrize('case', BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_conv_bf16x3_within_tolerance(cuda_device, case):
    """Opt-in split-bf16 3x3 conv (decoder side): NOT bit-exact by design; bound 1e-4 of the output scale
    (the network-level bar is the north-star's 1e-3 max-abs)."""
    import gpu_utils as G
    name, shp, cout, up, gn = case
    x = synth.uniform(3, name + 'x', shp, -2.0, 3.0)
    w = synth.uniform(3, name + 'w', (3, 3, shp[3], cout), -0.1, 0.1)
    b = synth.uniform(3, name + 'b', (cout,), -0.5, 0.5)
    ho, wo = (2 * shp[1], 2 * shp[2]) if up else (shp[1], shp[2])
    r1 = synth.uniform(3, name + 'r', (shp[0], ho, wo, cout), -1, 1)
    if gn:
        gamma = synth.uniform(3, name + 'g', (shp[3],), 0.5, 1.5)
        beta = synth.uniform(3, name + 'be', (shp[3],), -0.5, 0.5)
        a_, b_ = orc.gn_coeffs(x, gamma, beta)
        ref = orc.conv2d(orc.scale_shift_silu(x, a_, b_), w, b, 3, 1, 1, up, res1=r1)
        got = G.conv2d(x, w, b, 3, 1, 1, up, prologue=_lib.PRO_GN_SILU, pro=(a_, b_, None), res1=r1, bf16x3=True)
    else:
        ref = orc.conv2d(x, w, b, 3, 1, 1, up, res1=r1)
        got = G.conv2d(x, w, b, 3, 1, 1, up, res1=r1, bf16x3=True)
    assert got.shape == ref.shape and not np.isnan(got).any()
    err = float(np.abs(got - ref).max())
    scale = float(np.abs(ref).max())
    assert err <= 1e-4 * scale, f'{name}: max-abs {err:.3e} vs scale {scale:.3e}'
    # and every element within the per-element fp64 bound of the form (tests/fp64_ref.py; Cout = 3 is outside the planner's use of
    # the kernel but inside the unit ABI's)
    import fp64_ref as R
    worst = R.check_whole_conv3x3(x, w, b, got, 'bf16x3', up2=up, pro=(a_, b_) if gn else None, res=[r1], what=name)
    print(f'{name}: worst err / fp64 bound {worst:.3g}')


@pytest.mark.parametrize('cin,cout,shape,up', [(64, 64, (2, 20, 33), False), (128, 128, (1, 13, 10), False),
                                               (256, 256, (1, 9, 12), True), (128, 64, (1, 7, 9), True)])
def test_conv_bf16x3_fused_gn_moments(cuda_device, cin, cout, shape, up):
    """bf16x3 conv epilogue emits per-tile GroupNorm partial moments of its output; finalising them must give the same
    (a, b) as the oracle's moments of that output (tolerance: fp32 partials, 1e-5 relative)."""
    import gpu_utils as G
    b, h, w = shape
    x = synth.uniform(8, 'fgx', (b, h, w, cin), -2.0, 3.0)
    wt = synth.uniform(8, 'fgw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(8, 'fgb', (cout,), 0.5, 1.5)          # non-zero mean: exercises the cancellation in var
    gamma = synth.uniform(8, 'fgg', (cout,), 0.5, 1.5)
    beta = synth.uniform(8, 'fgbe', (cout,), -0.5, 0.5)
    y, part = G.conv2d(x, wt, bias, 3, 1, 1, up, bf16x3=True, gn_part=True)
    assert not torch.isnan(part).any()
    a, bb = G.gn_coeffs_from_partials(part, y.shape[1], y.shape[2], cout, gamma, beta)
    a_ref, b_ref = orc.gn_coeffs(y, gamma, beta)
    assert np.abs(a - a_ref).max() <= 1e-5 * np.abs(a_ref).max()
    assert np.abs(bb - b_ref).max() <= 2e-5 * max(1.0, np.abs(b_ref).max())


@pytest.mark.parametrize('cin,cout,shape,up,nres', [(64, 64, (2, 20, 33), False, 1), (128, 128, (1, 13, 10), False, 2),
                                                    (256, 256, (1, 9, 12), True, 0), (128, 64, (1, 7, 9), True, 0),
                                                    (64, 32, (1, 17, 40), False, 0), (32, 512, (1, 8, 16), False, 1)])
@CONV_SMALL
def test_conv_fp32_fused_gn_moments_bit_exact(cuda_device, cin, cout, shape, up, nres, conv_small):
    """The exact-fp32 halo conv emits per-tile GroupNorm partial moments of its output in the specified summation order:
    finalising them gives bit-for-bit the oracle's (a, b) of that output, and so does the standalone moments kernel."""
    import gpu_utils as G
    b, h, w = shape
    x = synth.uniform(18, 'egx', (b, h, w, cin), -2.0, 3.0)
    wt = synth.uniform(18, 'egw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(18, 'egb', (cout,), 0.5, 1.5)
    gamma = synth.uniform(18, 'egg', (cout,), 0.5, 1.5)
    beta = synth.uniform(18, 'egbe', (cout,), -0.5, 0.5)
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    res = [synth.uniform(18, f'egr{k}', (b, ho, wo, cout), -1, 1) for k in range(nres)]
    r1, r2 = (res + [None, None])[:2]
    y_ref = orc.conv2d(x, wt, bias, 3, 1, 1, up, res1=r1, res2=r2)
    a_ref, b_ref = orc.gn_coeffs(y_ref, gamma, beta)
    y, part = G.conv2d(x, wt, bias, 3, 1, 1, up, res1=r1, res2=r2, gn_part=True)
    assert not torch.isnan(part).any()
    _same(y, y_ref, 'conv output')
    a, bb = G.gn_coeffs_from_partials(part, ho, wo, cout, gamma, beta)
    # nearest-x2 convs run as four phase filters: their partials are per half-resolution tile and phase (another ORDER of the
    # same fp64 sums, restated by the oracle with phases=True)
    a_f, b_f = orc.gn_coeffs(y_ref, gamma, beta, phases=True) if up else (a_ref, b_ref)
    _same(a, a_f, 'fused gn a')
    _same(bb, b_f, 'fused gn b')
    if up:
        assert np.abs(a_f - a_ref).max() <= 1e-6 * np.abs(a_ref).max() and np.abs(b_f - b_ref).max() <= 1e-6 * max(1.0, np.abs(b_ref).max())
    a2, b2 = G.gn_coeffs(y_ref, gamma, beta)
    _same(a2, a_ref, 'standalone gn a')
    _same(b2, b_ref, 'standalone gn b')


@pytest.mark.parametrize('cin,cout,shape,nres', [(32, 64, (1, 8, 16), 0), (64, 96, (2, 11, 19), 1), (128, 40, (1, 5, 33), 2),
                                                 (256, 128, (1, 16, 16), 0), (64, 3, (1, 9, 7), 0)])
@CONV_SMALL
def test_conv_up2_phase_filters_bit_exact(cuda_device, cin, cout, shape, nres, conv_small):
    """nn.Upsample(x2, nearest) + 3x3 conv as four 2x2-tap phase filters with pre-summed fp32 weights: bit-identical to the
    oracle's restatement of the same form, and within fp32 rounding of the 9-tap definition on the upsampled image."""
    import gpu_utils as G
    b, h, w = shape
    x = synth.uniform(19, 'upx', (b, h, w, cin), -2.0, 2.0)
    wt = synth.uniform(19, 'upw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(19, 'upb', (cout,), -0.5, 0.5)
    res = [synth.uniform(19, f'upr{k}', (b, 2 * h, 2 * w, cout), -1, 1) for k in range(nres)]
    r1, r2 = (res + [None, None])[:2]
    y = G.conv2d(x, wt, bias, 3, 1, 1, True, res1=r1, res2=r2)
    _same(y, orc.conv2d(x, wt, bias, 3, 1, 1, True, res1=r1, res2=r2), 'up2 conv (phase form)')
    xu = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)                 # the definition: upsample, then the ordinary conv
    y_def = orc.conv2d(xu, wt, bias, 3, 1, 1, False, res1=r1, res2=r2)
    assert np.abs(y - y_def).max() <= 1e-5 * max(1.0, np.abs(y_def).max()), np.abs(y - y_def).max()


@pytest.mark.parametrize('cin,cout,shape,gn,nres,part', [
    (32, 128, (1, 8, 16), False, 0, False), (64, 128, (2, 16, 32), True, 1, True), (128, 256, (1, 13, 21), True, 2, True),
    (256, 128, (1, 9, 7), False, 1, False), (64, 64, (1, 24, 40), True, 1, True), (32, 192, (2, 5, 33), False, 0, False),
    (512, 256, (1, 8, 8), False, 0, False)])
def test_conv_winograd_bit_exact(cuda_device, cin, cout, shape, gn, nres, part):
    """3x3 convs in the Winograd F(4x4,3x3) form: bit-identical to the oracle's restatement of the same form (including the
    fused GroupNorm partial moments of the output, summed in the sub-block order), and within fp32 rounding of the direct form."""
    import gpu_utils as G
    b, h, w = shape
    x = synth.uniform(21, 'wix', (b, h, w, cin), -2.0, 2.0)
    wt = synth.uniform(21, 'wiw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(21, 'wib', (cout,), -0.5, 0.5)
    res = [synth.uniform(21, f'wir{k}', (b, h, w, cout), -1, 1) for k in range(nres)]
    r1, r2 = (res + [None, None])[:2]
    pro, xin = (None, None, None), x
    if gn:
        ga = synth.uniform(21, 'wiga', (b, cin), 0.5, 1.5)
        gb = synth.uniform(21, 'wigb', (b, cin), -0.5, 0.5)
        pro, xin = (ga, gb, None), orc.scale_shift_silu(x, ga, gb)
    got = G.conv2d(x, wt, bias, 3, 1, 1, prologue=_lib.PRO_GN_SILU if gn else 0, pro=pro, res1=r1, res2=r2, wino=True, gn_part=part)
    y_ref = orc.conv2d(xin, wt, bias, 3, 1, 1, res1=r1, res2=r2, wino=True)
    y = got[0] if part else got
    _same(y, y_ref, 'winograd conv')
    y_dir = orc.conv2d(xin, wt, bias, 3, 1, 1, res1=r1, res2=r2)
    err = np.abs(y - y_dir).max()
    assert err <= 1e-4 * max(1.0, np.abs(y_dir).max()), err
    if part:
        gamma = synth.uniform(21, 'wigg', (cout,), 0.5, 1.5)
        beta = synth.uniform(21, 'wigbe', (cout,), -0.5, 0.5)
        a_ref, b_ref = orc.gn_coeffs(y_ref, gamma, beta, phases=2)
        a, bb = G.gn_coeffs_from_partials(got[1], h, w, cout, gamma, beta)
        _same(a, a_ref, 'fused gn a (winograd)')
        _same(bb, b_ref, 'fused gn b (winograd)')


def test_conv_winograd_largest_lds_after_small(cuda_device):
    """The F(4x4) kernel's dynamic-LDS cap is set once per device to the kernel's maximum, not grown per launch: on ONE instantiation
    (GroupNorm prologue, exact SiLU, no residual) a Cin = 32 launch and then the largest request - Cin = 1024 (the shape rule's cap: 128
    k-steps, a 141 952-byte main-loop image with its GroupNorm table) on 1 x 8 x 20 (one sub-block pair, a border block) - both match the
    oracle's restatement bit for bit."""
    import gpu_utils as G
    for cin, (b, h, w) in ((32, (1, 16, 16)), (1024, (1, 8, 20))):
        x = synth.uniform(27, f'wlx{cin}', (b, h, w, cin), -2.0, 2.0)
        wt = synth.uniform(27, f'wlw{cin}', (3, 3, cin, 64), -0.1, 0.1)
        bias = synth.uniform(27, f'wlb{cin}', (64,), -0.5, 0.5)
        ga = synth.uniform(27, f'wlga{cin}', (b, cin), 0.5, 1.5)
        gb = synth.uniform(27, f'wlgb{cin}', (b, cin), -0.5, 0.5)
        y = G.conv2d(x, wt, bias, 3, 1, 1, prologue=_lib.PRO_GN_SILU, pro=(ga, gb, None), wino=True)
        _same(y, orc.conv2d(orc.scale_shift_silu(x, ga, gb), wt, bias, 3, 1, 1, wino=True), f'winograd conv, Cin = {cin}')


@pytest.mark.parametrize('cin,cout,shape,nres,part', [(32, 64, (1, 8, 8), 0, False), (64, 128, (2, 9, 13), 1, True), (256, 128, (1, 12, 20), 0, True),
                                                      (128, 64, (3, 5, 7), 2, True), (32, 192, (1, 1, 3), 0, False), (512, 256, (1, 4, 4), 0, True)])
def test_conv_up2_winograd_bit_exact(cuda_device, cin, cout, shape, nres, part):
    """nn.Upsample(x2) + 3x3 conv in the 25-product Winograd-type form (kernels_wino_up2.hip): bit-identical to the oracle's
    restatement (orc_conv_up2_winograd), within fp32 rounding of the definition, fused GroupNorm moments per 16x16 output sub-block."""
    import gpu_utils as G
    b, h, w = shape
    x = synth.uniform(23, 'wux', (b, h, w, cin), -2.0, 2.0)
    wt = synth.uniform(23, 'wuw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(23, 'wub', (cout,), -0.5, 0.5)
    res = [synth.uniform(23, f'wur{k}', (b, 2 * h, 2 * w, cout), -1, 1) for k in range(nres)]
    r1, r2 = (res + [None, None])[:2]
    ref = orc.conv2d(x, wt, bias, 3, 1, 1, True, res1=r1, res2=r2, wino=True)
    got = G.conv2d(x, wt, bias, 3, 1, 1, True, res1=r1, res2=r2, wino=True, gn_part=part)
    y = got[0] if part else got
    _same(y, ref, 'up2 conv (Winograd-type form)')
    xu = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)                 # the definition: upsample, then the ordinary conv
    y_def = orc.conv2d(xu, wt, bias, 3, 1, 1, False, res1=r1, res2=r2)
    assert np.abs(y - y_def).max() <= 1e-4 * max(1.0, np.abs(y_def).max()), np.abs(y - y_def).max()
    if part:
        gamma = synth.uniform(23, 'wug', (cout,), 0.5, 1.5)
        beta = synth.uniform(23, 'wube', (cout,), -0.5, 0.5)
        a_ref, b_ref = orc.gn_coeffs(ref, gamma, beta, phases=2)
        a, bb = G.gn_coeffs_from_partials(got[1], 2 * h, 2 * w, cout, gamma, beta)
        _same(a, a_ref, 'fused gn a (up2 winograd)')
        _same(bb, b_ref, 'fused gn b (up2 winograd)')


@pytest.mark.parametrize('in_add', [False, True])
@pytest.mark.parametrize('nres', [0, 1, 2])
def test_conv_up2_winograd_border_block_every_instantiation(cuda_device, nres, in_add):
    """Each of the six instantiations of the x2 Winograd-type kernel (residual operands x second input) on a border block with
    GroupNorm partials: 2 x 5 x 7 -> 10 x 14 outputs is one 16x16 sub-block per image, so the two sub-blocks of the only block lie in
    different images and neither is full.  Reference: the oracle's Winograd restatement on x + in_add; image and GroupNorm
    coefficients bit for bit."""
    import gpu_utils as G
    cin, cout, (b, h, w) = 64, 64, (2, 5, 7)
    x = synth.uniform(29, 'wbx', (b, h, w, cin), -2.0, 2.0)
    sk = synth.uniform(29, 'wbs', (b, h, w, cin), -1.0, 1.0) if in_add else None
    wt = synth.uniform(29, 'wbw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(29, 'wbb', (cout,), -0.5, 0.5)
    res = [synth.uniform(29, f'wbr{k}', (b, 2 * h, 2 * w, cout), -1, 1) for k in range(nres)]
    r1, r2 = (res + [None, None])[:2]
    ref = orc.conv2d((x + sk).astype(np.float32) if in_add else x, wt, bias, 3, 1, 1, True, res1=r1, res2=r2, wino=True)
    y, part = G.conv2d(x, wt, bias, 3, 1, 1, True, res1=r1, res2=r2, wino=True, gn_part=True, in_add=sk)
    _same(y, ref, 'up2 conv (Winograd-type form), border block')
    gamma = synth.uniform(29, 'wbg', (cout,), 0.5, 1.5)
    beta = synth.uniform(29, 'wbbe', (cout,), -0.5, 0.5)
    a_ref, b_ref = orc.gn_coeffs(ref, gamma, beta, phases=2)
    a, bb = G.gn_coeffs_from_partials(part, 2 * h, 2 * w, cout, gamma, beta)
    _same(a, a_ref, 'fused gn a (up2 winograd, border block)')
    _same(bb, b_ref, 'fused gn b (up2 winograd, border block)')


@pytest.mark.parametrize('cin,cout,shape,nres', [(64, 128, (2, 16, 32), 1), (128, 64, (1, 13, 21), 2), (256, 256, (1, 20, 9), 0)])
def test_conv_winograd_fast_act_close(cuda_device, cin, cout, shape, nres):
    """The model's default for the convs behind the codebook lookup: Winograd form with the SiLU of the GroupNorm prologue on the
    hardware exp2 / rcp units (femasr_conv_args.fast_act).  Not bit-identical to the oracle by construction (v_exp_f32 / v_rcp_f32
    are 1-ulp approximations): within 1e-5 of the output scale of the exact kernel (the same class as the rounding noise of the F(4x4) transforms, which amplify a 1-ulp input change ~10x), and the fused GroupNorm coefficients of the
    output within 1e-5 relative."""
    import gpu_utils as G
    b, h, w = shape
    x = synth.uniform(23, 'fax', (b, h, w, cin), -3.0, 3.0)
    wt = synth.uniform(23, 'faw', (3, 3, cin, cout), -0.1, 0.1)
    bias = synth.uniform(23, 'fab', (cout,), -0.5, 0.5)
    res = [synth.uniform(23, f'far{k}', (b, h, w, cout), -1, 1) for k in range(nres)]
    r1, r2 = (res + [None, None])[:2]
    ga = synth.uniform(23, 'faga', (b, cin), 0.5, 1.5)
    gb = synth.uniform(23, 'fagb', (b, cin), -0.5, 0.5)
    kw = dict(prologue=_lib.PRO_GN_SILU, pro=(ga, gb, None), res1=r1, res2=r2, wino=True, gn_part=True)
    y_exact, p_exact = G.conv2d(x, wt, bias, 3, 1, 1, **kw)
    y_fast, p_fast = G.conv2d(x, wt, bias, 3, 1, 1, fast_act=True, **kw)
    scale = max(1.0, float(np.abs(y_exact).max()))
    err = float(np.abs(y_fast - y_exact).max())
    assert 0.0 < err <= 1e-5 * scale, (err, scale)
    gamma = synth.uniform(23, 'fagg', (cout,), 0.5, 1.5)
    beta = synth.uniform(23, 'fagbe', (cout,), -0.5, 0.5)
    a0, b0 = G.gn_coeffs_from_partials(p_exact, h, w, cout, gamma, beta)
    a1, b1 = G.gn_coeffs_from_partials(p_fast, h, w, cout, gamma, beta)
    assert np.abs(a1 - a0).max() <= 1e-5 * np.abs(a0).max() and np.abs(b1 - b0).max() <= 1e-5 * max(1.0, np.abs(b0).max())


def test_repack_oihw_layout(cuda_device):
    """femasr_repack_oihw (what set_weight runs) == the documented K-major layout."""
    import gpu_utils as G
    lib = _lib.load()
    for (o, i, k) in ((40, 64, 3), (8, 3, 4), (16, 96, 1), (16, 24, 1), (300, 256, 1)):
        w = synth.uniform(9, f'rw{o}{i}{k}', (o, i, k, k), -1, 1)
        tw = G.dev(w)
        out = torch.empty(int(lib.femasr_packed_weight_floats(o, i, k, k)), dtype=torch.float32, device='cuda')
        _lib.check(lib.femasr_repack_oihw(None, _lib.ptr(tw), o, i, k, k, _lib.ptr(out)))
        ref = G.lib_weight_layout(orc.repack_conv_weight(w)).reshape(-1)
        _same(out.cpu().numpy(), ref, f'repack {o}x{i}x{k}')


def test_bad_arguments_are_refused(cuda_device):
    import ctypes
    lib = _lib.load()
    x = torch.zeros((1, 8, 8, 32), device='cuda')
    assert lib.femasr_window_attention(None, _lib.ptr(x), 1, 9, 8, 256, 8, 0, _lib.ptr(x), _lib.ptr(x)) != 0
    assert b'multiples of 8' in lib.femasr_last_error()
    assert lib.femasr_ln_stats(None, _lib.ptr(x), 4, 128, 1e-5, _lib.ptr(x)) != 0
    a = _lib.ConvArgs()
    assert lib.femasr_conv2d(None, ctypes.byref(a)) != 0

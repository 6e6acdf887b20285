"""-m gpu: exp, erf, SiLU, GELU and the softmax of the kernels against the oracle across all of fp32.

  * the device functions themselves (csrc/detmath.h through femasr_debug_math_eval) on the 27 million points of tests/math_range.py
    - every exponent, the active range densely, the neighbourhoods of every breakpoint, subnormals, +-0, +-inf, NaN - bit for bit
    against the oracle, the packed two-at-a-time forms bit for bit against the scalar ones in both slots, and the hardware SiLU of the
    default mode (fast_silu) against fp64 with a derived bound;
  * the call sites: the same extremes through every kernel that applies SiLU or GELU, with identity weights so that no sum overflows;
  * the softmax of the window attention at its extremes (dominant keys at every accumulator slot, logit gaps far beyond exp's clamp,
    large biases, subnormal products, large values, a mask that loses, the shifts nothing else runs);
  * a magnitude ladder: the reductions with inputs and weights scaled by 2^-70 (subnormal products) and 2^55 (sums near 2^120).

Everything except fast_silu is bit-exact; NaNs are compared by position (x86's default NaN is 0xffc00000, the GPU's 0x7fc00000), zeros
with their sign.  The host side of the same set - oracle against fp64, the set's witnesses, the softmax cases' premises - is
tests/test_math_range_host.py.  Measured figures: profiles/math_range_report.txt.
"""
import numpy as np
import pytest
import torch

import fp64_ref as R
import gpu_utils as G
import math_range as M
from femasr_amd import _lib, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GN = _lib.PRO_GN_SILU


def _u(tag, shape, lo=-1.0, hi=1.0):
    return synth.uniform(67, tag, tuple(shape), lo, hi)


@pytest.fixture(scope='module')
def padded_sweep():
    """The sweep set with one value repeated, so that its length is even (the packed forms take pairs)."""
    x = M.sweep_set()
    return np.concatenate([x, x[:x.size % 2]])


_SCALAR = {}


def _scalar(fn, x):
    """Selector 0-3 on the padded sweep set, computed once per session and shared (left unchanged) between the tests."""
    if fn not in _SCALAR:
        _SCALAR[fn] = G.math_eval(fn, x)
    return _SCALAR[fn]


# ---------------------------------------------------------------- the functions themselves
@pytest.mark.parametrize('fn', ['exp', 'erf', 'silu', 'gelu'])
def test_function_equals_the_oracle_on_the_whole_set(cuda_device, padded_sweep, fn):
    x = padded_sweep
    M.assert_same(_scalar(fn, x), orc.math_eval(fn, x), f'det_{fn}f vs orc_{fn}', x)


@pytest.mark.parametrize('fn', ['exp', 'erf', 'silu', 'gelu'])
def test_packed_form_equals_the_scalar_one(cuda_device, padded_sweep, fn):
    """As laid out (neighbours of the sorted set share a pair) and reversed (every value in the other slot); then with the two ends of
    the set interleaved, (x[0], x[n-1]), (x[1], x[n-2]) ..., and that reversed: every value in both slots next to a partner from the
    other end of the range."""
    x = padded_sweep
    M.assert_same(G.math_eval(fn + '2', x), _scalar(fn, x), f'det_{fn}2 vs det_{fn}, as laid out', x)
    # interleave the two ends: (x[0], x[-1]), (x[1], x[-2]) ...: a partner from the other end of the range, each value in slot 0 and 1
    n = x.size
    mixed = np.empty(n, np.float32)
    mixed[0::2], mixed[1::2] = x[:n // 2], x[::-1][:n // 2]
    for lay, what in ((np.ascontiguousarray(x[::-1]), 'reversed'), (mixed, 'ends interleaved'), (np.ascontiguousarray(mixed[::-1]), 'ends interleaved, reversed')):
        M.assert_same(G.math_eval(fn + '2', lay), G.math_eval(fn, lay), f'det_{fn}2 vs det_{fn}, {what}', lay)


def test_fast_silu_against_fp64(cuda_device, padded_sweep):
    """fast_silu(t) = t * rcp(1 + exp2(t * -log2e)) on the hardware units, against fp64 t sigma(t):
      |err| <= u |silu(t)| (4.5 + (1 - sigma(t)) (1.3 |t| + 2))  for t >= -80 (derivation: math_range.fast_silu_bound), plus one quantum
                2^-149 of the subnormal range (the relative model of a rounding does not hold below 2^-126);
      -2^-100 <= y <= 0  for t < -80 (the hardware may flush there);  NaN exactly where fp64 t sigma(t) is NaN (NaN, and -inf * 0).
    Also prints the largest error in ulp of |silu| (the unit of fp64_ref.PRO_ERR) per unit interval of t."""
    x = padded_sweep
    y = G.math_eval('fast_silu', x)
    t = x.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        ref = t * (1.0 / (1.0 + np.exp(-t)))
    assert np.array_equal(np.isnan(y), np.isnan(ref)), f'NaN at {x[np.isnan(y) != np.isnan(ref)][:8]}'
    ok = ~np.isnan(ref)
    low = ok & (x < np.float32(-80.0))
    assert np.all((y[low] <= 0) & (y[low] >= np.float32(-2.0 ** -100))), x[low][~((y[low] <= 0) & (y[low] >= np.float32(-2.0 ** -100)))][:8]
    hi = ok & ~low & np.isfinite(x)
    err = np.abs(y[hi].astype(np.float64) - ref[hi])
    bound = M.fast_silu_bound(t[hi]) + 2.0 ** -149
    ratio = err / bound
    i = int(np.argmax(ratio))
    print(f'fast_silu: worst err / bound {ratio[i]:.3f} at t = {x[hi][i]!r}')
    inf = x == np.inf
    assert np.all(y[inf] == np.inf)
    # the error in ulp of |silu| per unit interval of t (normal results only)
    th, sil = t[hi], np.abs(ref[hi])
    norm = sil >= 2.0 ** -126
    ulps = err[norm] / (R.U * sil[norm])
    k = (np.floor(np.clip(th[norm], -80.0, 21.0)) + 80).astype(np.int64)          # 0..100: [-80, -79) .. [20, 21); 101: t >= 21
    worst = np.zeros(102)
    np.maximum.at(worst, k, ulps)
    print('fast_silu: max error in ulp of |silu| per interval [k, k+1) of t:')
    for row in range(0, 101, 10):
        print('  ' + '  '.join(f'{kk - 80}: {worst[kk]:.2f}' for kk in range(row, min(row + 10, 101))))
    print(f'  t >= 21: {worst[101]:.2f}')
    over = np.flatnonzero(worst > R.PRO_ERR[True])
    print(f'fast_silu: PRO_ERR[True] = {R.PRO_ERR[True]} ulp of |silu| holds for t >= {int(over.max()) - 79 if over.size else -80} (largest there: '
          f'{worst[(int(over.max()) + 1 if over.size else 0):].max():.2f})')
    assert ratio[i] <= 1.0, f'fast_silu: err / bound = {ratio[i]:.3f} at t = {x[hi][i]!r}: got {y[hi][i]!r}, fp64 {ref[hi][i]!r}'
    # what the comment at fp64_ref.PRO_ERR and DESIGN section 4 state: 8 ulp of |silu| from the interval [-5, -4) upwards
    assert worst[75:].max() <= R.PRO_ERR[True], f'PRO_ERR[True] no longer holds for t >= -5: {worst[75:].max():.2f} ulp of |silu|'


# ---------------------------------------------------------------- the call sites
def _identity(cin, cout, ksz):
    w = np.zeros((ksz, ksz, cin, cout), np.float32)
    for c in range(min(cin, cout)):
        w[ksz // 2, ksz // 2, c, c] = 1.0
    return w


ONE = np.ones((1, 32), np.float32)
ZERO = np.zeros((1, 32), np.float32)
HW = 56                  # 56 * 56 * 32 = 100 352 values: the whole call-site set (99 726), tiled from its start


def test_call_site_gn_silu_apply(cuda_device):
    x = M.call_site_set(HW * HW * 32).reshape(1, HW, HW, 32)            # NaN and +-inf included: the kernel is element-wise
    y = G.gn_silu_apply(x, ONE, ZERO)
    M.assert_same(y, orc.scale_shift_silu(x, ONE, ZERO), 'gn_silu_apply vs orc_scale_shift_silu', x)
    M.assert_same(y, orc.math_eval('silu', x + np.float32(0.0)), 'gn_silu_apply vs silu(x + 0)', x)      # fmaf(x, 1, +0): -0 becomes +0


def test_call_site_direct_conv_scalar_silu(cuda_device):
    """The GN + SiLU prologue that calls scalar det_silu: the implicit-GEMM kernel, here as a 3x3 stride-2 conv.  Output (y, x) takes
    its centre tap from input (2y, 2x): the set sits there, the other pixels hold it rolled (weight 0)."""
    shape = (1, 2 * HW, 2 * HW, 32)
    name = G.conv_variant_name(shape, 32, 3, 2, 1, prologue=GN)
    assert name == 'conv_igemm<128x32,FEMASR_PRO_GN_SILU,cinvec=true,waves=4x1>', name
    vals = M.call_site_set(HW * HW * 32, finite=True).reshape(1, HW, HW, 32)
    x = np.roll(M.call_site_set(4 * HW * HW * 32, finite=True), 12345).reshape(shape).copy()
    x[:, ::2, ::2] = vals
    w, bias = _identity(32, 32, 3), np.zeros(32, np.float32)
    y = G.conv2d(x, w, bias, 3, 2, 1, prologue=GN, pro=(ONE, ZERO, None))
    M.assert_same(y, orc.conv2d(orc.scale_shift_silu(x, ONE, ZERO), w, bias, 3, 2, 1), name, vals)
    # exact: one product with 1, the others +-0, added to a chain that starts from +0
    M.assert_same(y, orc.math_eval('silu', vals + np.float32(0.0)) + np.float32(0.0), name + ' vs silu(x + 0)', vals)


def test_call_site_halo_conv_packed_silu(cuda_device):
    """The GN + SiLU prologue of the halo kernel: det_silu2 on the packed ALU."""
    shape = (1, HW, HW, 32)
    name = G.conv_variant_name(shape, 32, 3, 1, 1, prologue=GN)
    assert name == 'conv3x3_halo<8x16x32,FEMASR_PRO_GN_SILU,up2=false,waves=4x1>', name
    x = M.call_site_set(HW * HW * 32, finite=True).reshape(shape)
    w, bias = _identity(32, 32, 3), np.zeros(32, np.float32)
    y = G.conv2d(x, w, bias, 3, 1, 1, prologue=GN, pro=(ONE, ZERO, None))
    M.assert_same(y, orc.conv2d(orc.scale_shift_silu(x, ONE, ZERO), w, bias, 3, 1, 1), name, x)
    M.assert_same(y, orc.math_eval('silu', x + np.float32(0.0)) + np.float32(0.0), name + ' vs silu(x + 0)', x)


def test_call_site_winograd_exact_silu(cuda_device):
    """The GN + SiLU prologue of the exact Winograd form (fast_act = 0); |x| <= 2^100 so that the input transform stays finite.  The
    transforms round, so the comparison is with the oracle's Winograd conv only."""
    shape = (1, HW, HW, 32)
    name = G.conv_variant_name(shape, 64, 3, 1, 1, prologue=GN, wino=True)
    assert name == 'conv3x3_wino4<2x16x16px x64,FEMASR_PRO_GN_SILU,false,res=0,waves=8>', name
    x = M.call_site_set(HW * HW * 32, finite=True, cap=2.0 ** 100).reshape(shape)
    w, bias = _identity(32, 64, 3), np.zeros(64, np.float32)
    y = G.conv2d(x, w, bias, 3, 1, 1, prologue=GN, pro=(ONE, ZERO, None), wino=True)
    ref = orc.conv2d(orc.scale_shift_silu(x, ONE, ZERO), w, bias, 3, 1, 1, wino=True)
    assert np.isfinite(ref).all()
    M.assert_same(y, ref, name)


def _in_live_columns(s, cin, cout, row_multiple=1):
    """(rows, cin) input of an identity-weight layer with `cout` outputs: the first `cout` columns - the only ones the weight passes on -
    hold the WHOLE set s in order (tiled from its start to fill the last rows), the other columns hold the set rolled (their weight is
    0).  rows = the least multiple of row_multiple that takes the set."""
    rows = -(-s.size // cout)
    rows = -(-rows // row_multiple) * row_multiple
    x = np.roll(np.resize(s, rows * cin), 4321).reshape(rows, cin).copy()
    x[:, :cout] = np.resize(s, rows * cout).reshape(rows, cout)
    assert np.array_equal(np.unique(x[:, :cout].view(np.uint32)), np.unique(s.view(np.uint32))), 'every value of the set reaches an output'
    return x


@pytest.mark.parametrize('cout', [32, 30], ids=['float4', 'scalar'])
def test_call_site_gelu_fp32_gemm(cuda_device, cout):
    xr = _in_live_columns(M.call_site_set(finite=True), 32, cout)
    rows = xr.shape[0]
    x = xr.reshape(1, rows, 1, 32)
    name = G.conv_variant_name(x.shape, cout, 1, 1, 0, act=1)
    assert name == 'gemm_dma<tile=64*1,k=8*4,stages=2,act=1,nres=0,vq=false>', name
    w, bias = _identity(32, cout, 1), np.zeros(cout, np.float32)
    y = G.conv2d(x, w, bias, 1, act=1)
    M.assert_same(y, orc.conv2d(x, w, bias, 1, act=1), name, x[..., :cout])
    M.assert_same(y, orc.math_eval('gelu', x[..., :cout] + np.float32(0.0)), name + ' vs gelu(x + 0)', x[..., :cout])


@pytest.mark.parametrize('cout', [32, 30], ids=['float4', 'scalar'])
def test_call_site_gelu_general_conv(cuda_device, cout):
    xr = _in_live_columns(M.call_site_set(finite=True), 32, cout, row_multiple=HW)
    x = xr.reshape(1, xr.shape[0] // HW, HW, 32)
    name = G.conv_variant_name(x.shape, cout, 3, 1, 1, act=1)
    assert name == 'conv_igemm<128x32,FEMASR_PRO_NONE,cinvec=true,waves=4x1>', name
    w, bias = _identity(32, cout, 3), np.zeros(cout, np.float32)
    y = G.conv2d(x, w, bias, 3, 1, 1, act=1)
    M.assert_same(y, orc.conv2d(x, w, bias, 3, 1, 1, act=1), name, x[..., :cout])
    M.assert_same(y, orc.math_eval('gelu', x[..., :cout] + np.float32(0.0)), name + ' vs gelu(x + 0)', x[..., :cout])


def _split_gemm_set():
    """What the split-bf16 GEMM's call-site test feeds: the finite call-site set with 2^-100 <= |x| <= 2^126, or 0."""
    s = M.call_site_set(finite=True, cap=2.0 ** 126)
    return s[(np.abs(s) >= np.float32(2.0 ** -100)) | (s == 0)]


@pytest.mark.parametrize('cout', [32, 30], ids=['float4', 'scalar'])
def test_call_site_gelu_split_gemm(cuda_device, cout):
    """The split-bf16 GEMM (its own copy of the epilogue: kernels_gemm_bf16.hip): 2^-100 <= |x| <= 2^126 or 0 (DESIGN section 2 documents
    the last-place differences of the three-term split below that); against the oracle's restatement of the instruction.  Cin = 64 (the
    form's least), of which an identity weight passes on the first Cout columns: the whole admitted set sits in those."""
    xr = _in_live_columns(_split_gemm_set(), 64, cout)
    rows = xr.shape[0]
    name = G.conv_variant_name((1, rows, 1, 64), cout, 1, 1, 0, act=1, bf16s=True)
    assert name == 'gemm_bf16s<act=1,nres=0>', name
    w, bias = _identity(64, cout, 1), np.zeros(cout, np.float32)
    y = G.conv2d(xr.reshape(1, rows, 1, 64), w, bias, 1, act=1, bf16s=True)
    ref = orc.linear_bf16s(xr, np.ascontiguousarray(w.reshape(64, cout).T), bias, 1)
    M.assert_same(y.reshape(rows, cout), ref, name, xr[:, :cout])


# ---------------------------------------------------------------- softmax extremes
@pytest.mark.parametrize('name', M.ATTENTION_CASES + ('nan_key',))
def test_softmax_extremes(cuda_device, name):
    """Bit-exact against orc.window_attention, and against fp64_ref.attention_ref on ALL windows with that reference's own bound
    (the premises of 'dominant' and 'mask_loses' are checked on fp64 alone in tests/test_math_range_host.py).  'nan_key': one key per
    window is NaN - it loses the softmax (weight exp(-87)); its own value row is finite, so the output is; oracle only."""
    c = M.attention_case(name)
    got = G.window_attention(c['qkv'], c['b'], c['h'], c['w'], c['c'], c['heads'], c['shift'], c['table'])
    want = orc.window_attention(c['qkv'], c['b'], c['h'], c['w'], c['c'], c['heads'], c['shift'], c['table'])
    assert np.isfinite(want).all()
    M.assert_same(got, want, f'window attention, case {name}')
    if name == 'nan_key':
        return
    rows, ref, bound = R.attention_ref(torch.from_numpy(c['qkv'].reshape(-1, 3 * c['c'])), c['b'], c['h'], c['w'], c['c'], c['heads'],
                                       c['shift'], c['table'], c['wins'])
    assert len(rows) == c['b'] * c['h'] * c['w']
    R.check(got.reshape(-1, c['c'])[rows], ref, bound, f'window attention vs fp64, case {name}')


# ---------------------------------------------------------------- magnitude ladder
LADDER = [2.0 ** -70, 2.0 ** 55]


@pytest.mark.parametrize('scale', LADDER, ids=['2^-70', '2^55'])
def test_magnitude_ladder(cuda_device, scale):
    """Random weights at the smallest fuzz-sized shapes, inputs - and the conv / GEMM weights - scaled by 2^-70 (products subnormal) and
    2^55 (sums near 2^120, no overflow): fp32 MFMA and the VALU keep subnormals in the default mode, so everything stays bit-exact."""
    s = np.float32(scale)
    x = _u('lx', (1, 5, 7, 32), -2.0, 3.0) * s
    # direct 3x3 conv (halo kernel)
    w, bias = _u('lw', (3, 3, 32, 24), -0.1, 0.1) * s, _u('lb', (24,), -0.5, 0.5) * s * s
    ref = orc.conv2d(x, w, bias, 3, 1, 1)
    assert np.isfinite(ref).all() and np.count_nonzero(ref) > ref.size // 2
    if scale < 1:
        assert np.abs(ref).max() < 2.0 ** -126, 'the outputs are meant to be subnormal'
    M.assert_same(G.conv2d(x, w, bias, 3, 1, 1), ref, f'direct conv at {scale}')
    # fp32 GEMM
    xr = _u('lgx', (1, 37, 1, 32), -2.0, 3.0) * s
    wg, bg = _u('lgw', (1, 1, 32, 32), -0.1, 0.1) * s, _u('lgb', (32,), -0.5, 0.5) * s * s
    ref = orc.conv2d(xr, wg, bg, 1)
    assert np.isfinite(ref).all() and np.count_nonzero(ref) > ref.size // 2
    M.assert_same(G.conv2d(xr, wg, bg, 1), ref, f'fp32 GEMM at {scale}')
    # exact Winograd conv (smaller amplitudes: the three transforms grow the values by up to ~100 each)
    xw = _u('lwx', (1, 5, 7, 32), -1.0, 1.0) * s
    ww, bw = _u('lww', (3, 3, 32, 64), -0.05, 0.05) * s, _u('lwb', (64,), -0.5, 0.5) * s * s
    ref = orc.conv2d(xw, ww, bw, 3, 1, 1, wino=True)
    assert np.isfinite(ref).all() and np.count_nonzero(ref) > ref.size // 2
    M.assert_same(G.conv2d(xw, ww, bw, 3, 1, 1, wino=True), ref, f'Winograd conv at {scale}')
    # GroupNorm coefficients and LayerNorm
    gamma, beta = _u('lg', (32,), 0.5, 1.5), _u('lbe', (32,), -0.5, 0.5)
    a, b = G.gn_coeffs(x, gamma, beta)
    a_ref, b_ref = orc.gn_coeffs(x, gamma, beta)
    assert np.isfinite(a_ref).all() and np.isfinite(b_ref).all()
    M.assert_same(a, a_ref, f'gn_coeffs a at {scale}')
    M.assert_same(b, b_ref, f'gn_coeffs b at {scale}')
    xl = _u('ll', (3, 256), -4.0, 6.0) * s
    g2, b2 = _u('llg', (256,), 0.5, 1.5), _u('llb', (256,), -0.5, 0.5)
    ref = orc.layernorm(xl, g2, b2)
    assert np.isfinite(ref).all()
    M.assert_same(G.layernorm(xl, g2, b2), ref, f'layernorm at {scale}')
    # window attention: q, k and v scaled
    qkv = _u('lq', (1, 64, 96), -3.0, 3.0) * s
    table = _u('lt', (225, 1))
    ref = orc.window_attention(qkv, 1, 8, 8, 32, 1, 0, table)
    assert np.isfinite(ref).all()
    M.assert_same(G.window_attention(qkv, 1, 8, 8, 32, 1, 0, table), ref, f'window attention at {scale}')

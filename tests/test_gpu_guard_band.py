"""-m gpu: every kernel family between guard bands and under two poisons (tests/guard_arena.py).

Each case places ALL operands of the call in one arena at their exact sizes (the library's own size queries, through the wrappers of
tests/gpu_utils.py), runs once per poison, and requires: no byte outside the writable regions changed, every output region
bit-identical between the two poisons (nothing unwritten, nothing computed from bytes outside the inputs), and the usual comparison
with the reference the unit tests already use for that kernel - the oracle bit for bit, or tests/fp64_ref.py / fp16_ref.py with
their bounds for the bf16x3, fp16 and hardware-SiLU forms.  No tolerance is introduced here.

Shapes are the smallest at which each kernel's edge logic runs; the tile sizes are written next to each table.  The closing test
holds the conv table against the library's list of conv instantiations: a new instantiation without a guard case fails it.
"""
import ctypes

import numpy as np
import pytest
import torch

import fp16_front_ref as FR
import fp16_ref as F16
import fp64_ref as R
import guard_arena as GA
import gpu_utils as G
from femasr_amd import _lib, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SEEN = set()        # instantiation names of the conv cases that ran


def _u(tag, shape, lo=-1.0, hi=1.0):
    return synth.uniform(31, tag, tuple(shape), lo, hi)


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        raise AssertionError(f'{what}: not bit-identical: max-abs {np.nanmax(d):.3e}, mismatching {np.sum(got != ref)} of {got.size}, '
                             f'nan {np.isnan(got.astype(np.float64)).sum()}')


# ---------------------------------------------------------------- conv forms through femasr_conv2d
# Tiles (csrc): halo kernels (direct fp32, bf16x3, fp16; halo_mma.h, kernels_conv.hip) 8 x 16 pixels per block, an x2 conv 8 x 16 of the
# HALF-resolution image per block and phase; implicit GEMM (kernels_conv.hip) 128 output pixels x 128 / 64 / 32 channels; cout3 VALU kernel
# 8 x 32 pixels; Winograd forms (kernels_wino*.hip) 4 x 4 output tiles in 16 x 16 sub-blocks, two sub-blocks per block; column classes of
# the pick_variant functions: Cout <= 32, 33..64, 65..128, > 128.
HALO_HW = [(1, 1), (7, 17), (9, 15), (17, 33)]                   # one pixel; one short / one past the 8 x 16 tile in either axis; two tiles + 1
HALO_UP2_HW = [(1, 1), (7, 17), (9, 15)]                         # the same on the half-resolution input of an x2 conv
WINO_HW = [(1, 1), (3, 17), (5, 15), (15, 5), (17, 3), (17, 33)]  # 4 x 4 tiles and 16 x 16 sub-blocks: one short / one past, either axis
WINO_UP2_HW = [(1, 1), (2, 9), (7, 8), (9, 7), (8, 17)]          # input sizes: outputs 2x2, 4x18, 14x16, 18x14, 16x34


def C(form, hw, cin, cout, B=2, k=3, s=1, p=1, up2=False, pro=False, nres=0, in_add=False, part=False, small=-1, fast=False, act=0,
      cfg=-1):
    return dict(form=form, hw=hw, cin=cin, cout=cout, B=B, k=k, s=s, p=p, up2=up2, pro=pro, nres=nres, in_add=in_add, part=part,
                small=small, fast=fast, act=act, cfg=cfg)


def _conv_cases():
    cs = []
    # direct fp32 halo kernels: every column class (ragged 3 / 24, 40, 72, 136) x {plain, GN prologue, x2 phase filters}; the 128-column
    # blocks need the small-launch rule off (small = 0), the 64-column blocks of a small launch are its default
    for i, hw in enumerate(HALO_HW):
        cs += [C('direct', hw, 32, 24, nres=i % 3), C('direct', hw, 32, 40, pro=True, nres=(i + 1) % 3),
               C('direct', hw, 32, 72, small=0, nres=(i + 2) % 3), C('direct', hw, 32, 136, small=-1, pro=True),
               C('direct', hw, 64, 64, part=True, nres=i % 3), C('direct', hw, 32, 128, small=0, part=True, pro=True)]
    cs += [C('direct', (7, 17), 32, 32, pro=True, part=True), C('direct', (9, 15), 32, 136, small=0, pro=True, nres=2),
           C('direct', (7, 17), 32, 72, small=0, nres=2), C('direct', (9, 15), 32, 40, nres=2), C('direct', (9, 15), 32, 24, pro=True)]
    for i, hw in enumerate(HALO_UP2_HW):        # the phase-filter x2 form: three column classes, partials per half-resolution tile and phase
        cs += [C('direct', hw, 32, 24, up2=True, nres=i % 3), C('direct', hw, 32, 64, up2=True, part=True, nres=(i + 1) % 3),
               C('direct', hw, 32, 136, up2=True, small=0, nres=(i + 2) % 3), C('direct', hw, 32, 128, up2=True, part=True)]
    # the cout3 VALU kernel (8 x 32 pixels) and Cout = 3 with a prologue / x2 (32-column halo kernel)
    cs += [C('direct', hw, 32, 3) for hw in [(1, 1), (7, 33), (9, 31), (17, 33)]]
    cs += [C('direct', (9, 15), 64, 3, pro=True), C('direct', (7, 17), 32, 3, up2=True)]
    # generic implicit GEMM: Cin = 3 k = 4 (in_conv), stride 2, pad 0, GN prologue in front of a stride-2 conv; 128 output pixels per block:
    # 11 x 12 = 132 pixels per image (one past), 127 = one short over the batch (B = 1), ragged columns per class
    cs += [C('direct', (12, 13), 3, 136, k=4), C('direct', (12, 13), 3, 40, k=4), C('direct', (12, 13), 3, 24, k=4), C('direct', (2, 2), 3, 64, k=4),
           C('direct', (23, 21), 32, 136, s=2, small=0), C('direct', (23, 21), 32, 136, s=2, small=0, pro=True, nres=1),
           C('direct', (23, 21), 32, 40, s=2, nres=2), C('direct', (23, 21), 32, 40, s=2, pro=True),
           C('direct', (1, 1), 32, 24, s=2), C('direct', (23, 21), 32, 24, s=2, pro=True, nres=1),
           C('direct', (13, 14), 32, 40, p=0), C('direct', (3, 3), 32, 24, p=0, nres=1), C('direct', (18, 9), 64, 72, p=0, B=1, small=0),
           C('direct', (9, 15), 32, 72, up2=True, s=2)]
    # Winograd F(4x4,3x3): Cout % 64 == 0; prologue form x residual operands; partials per 16 x 16 sub-block
    for i, hw in enumerate(WINO_HW):
        cs += [C('wino', hw, 32, 64, nres=i % 3, part=True), C('wino', hw, 32, 64, pro=True, nres=(i + 1) % 3, part=i % 2 == 0),
               C('wino', hw, 32, 128, pro=True, fast=True, nres=(i + 2) % 3, part=i % 2 == 1)]
    # an odd TOTAL number of sub-blocks (blocks take two): B = 1 at 16 x 16, B = 3 at 16 x 16, B = 1 at 17 x 33 (2 x 3 - even - and 1 x 3)
    cs += [C('wino', (16, 16), 32, 64, B=1, part=True), C('wino', (16, 16), 32, 64, B=3, pro=True, nres=1, part=True),
           C('wino', (16, 33), 32, 64, B=1, nres=2), C('wino', (16, 16), 32, 192, B=1, pro=True, fast=True, part=False)]
    for i, hw in enumerate(WINO_UP2_HW):
        cs += [C('wino', hw, 32, 64, up2=True, nres=i % 3, part=True, in_add=i % 2 == 0),
               C('wino', hw, 32, 128, up2=True, nres=(i + 1) % 3, in_add=i % 2 == 1)]
    cs += [C('wino', (8, 8), 32, 64, up2=True, B=1, part=True, in_add=True), C('wino', (8, 8), 32, 64, up2=True, B=3, nres=1, part=True)]
    # bf16x3 and fp16 halo forms: four column classes x {plain, GN prologue, x2}; partials while Cout / 32 is a power of two <= 8.
    # Their partials are fp32 sums, and the coefficients come from E[y^2] - E[y]^2: a group of ONE pixel with 1 - 8 channels has a variance
    # of the order of the cancellation error (exactly 0 at Cout = 32), where fp64_ref.gn_coeffs_ref's bound - written for moments over
    # thousands of elements - does not describe an fp32 moment pass.  The partials are asked for from the next size up (119 pixels).
    for form in ('bf16x3', 'f16'):
        for i, hw in enumerate(HALO_HW):
            part = hw != (1, 1)
            cs += [C(form, hw, 32, 24, nres=i % 3), C(form, hw, 32, 32, pro=True, part=part, nres=(i + 1) % 3),
                   C(form, hw, 32, 40, pro=True, nres=(i + 2) % 3), C(form, hw, 32, 64, part=part),
                   C(form, hw, 32, 72, nres=(i + 1) % 3), C(form, hw, 32, 128, pro=True, part=part),
                   C(form, hw, 32, 136, pro=True, nres=i % 3), C(form, hw, 32, 256, part=part)]
        for i, hw in enumerate(HALO_UP2_HW):
            part = hw != (1, 1)
            cs += [C(form, hw, 32, 24, up2=True, nres=i % 3), C(form, hw, 32, 64, up2=True, part=part), C(form, hw, 32, 72, up2=True, nres=(i + 1) % 3),
                   C(form, hw, 32, 256, up2=True, part=part, nres=(i + 2) % 3)]
    return cs


CONV_CASES = _conv_cases()


def _conv_id(c):
    h, w = c['hw']
    return (f"{c['form']}_B{c['B']}_{h}x{w}_{c['cin']}to{c['cout']}_k{c['k']}s{c['s']}p{c['p']}" + ('_up2' if c['up2'] else '') + ('_gn' if c['pro'] else '') +
            ('_fast' if c['fast'] else '') + f"_res{c['nres']}" + ('_add' if c['in_add'] else '') + ('_part' if c['part'] else '') +
            ('_bn128' if c['small'] == 0 else '') + (f"_act{c['act']}" if c['act'] else '') + (f"_cfg{c['cfg']}" if c['cfg'] >= 0 else ''))


def _whole(B, ho, wo):
    return F16.all_positions(B, ho, wo)


def _run_conv(c):
    lib = _lib.load()
    form, (h, w), cin, cout, B, k, s, p, up2 = c['form'], c['hw'], c['cin'], c['cout'], c['B'], c['k'], c['s'], c['p'], c['up2']
    tag = _conv_id(c)
    x = _u(tag + 'x', (B, h, w, cin), -2.0, 2.0)
    wt = _u(tag + 'w', (k, k, cin, cout), -0.1, 0.1)
    bias = _u(tag + 'b', (cout,), -0.5, 0.5)
    hv, wv = (2 * h, 2 * w) if up2 else (h, w)
    ho, wo = (hv + 2 * p - k) // s + 1, (wv + 2 * p - k) // s + 1
    res = [_u(tag + f'r{i}', (B, ho, wo, cout)) for i in range(c['nres'])]
    r1, r2 = (res + [None, None])[:2]
    pro = (_u(tag + 'ga', (B, cin), 0.5, 1.5), _u(tag + 'gb', (B, cin), -0.5, 0.5)) if c['pro'] else None
    sk = _u(tag + 'sk', (B, h, w, cin)) if c['in_add'] else None
    gamma, beta = _u(tag + 'gg', (cout,), 0.5, 1.5), _u(tag + 'gbe', (cout,), -0.5, 0.5)
    flags = dict(bf16x3=form == 'bf16x3', wino=form == 'wino', bf16s=form == 'bf16s', f16=form in ('f16', 'gemm_f16'))

    def launch():
        got = G.conv2d(x, wt, bias, k, s, p, up2, prologue=_lib.PRO_GN_SILU if pro else 0, pro=(pro + (None,)) if pro else (None, None, None),
                       act=c['act'], res1=r1, res2=r2, gn_part=c['part'], fast_act=c['fast'], in_add=sk, **flags)
        if not c['part']:
            return got, None
        return got[0], G.gn_coeffs_from_partials(got[1], ho, wo, cout, gamma, beta)

    prev_small = lib.femasr_conv_small_launch_blocks(c['small'])
    prev_cfg = lib.femasr_gemm_force_config(c['cfg'])
    try:
        name = G.conv_variant_name(x.shape, cout, k, s, p, up2, prologue=1 if pro else 0, act=c['act'], nres=c['nres'], fast_act=c['fast'],
                                   in_add=c['in_add'], **flags)
        y, ab = GA.run_twice(launch, f'{tag} [{name}]')
    finally:
        lib.femasr_conv_small_launch_blocks(prev_small)
        lib.femasr_gemm_force_config(prev_cfg)
    what = f'{tag} [{name}]'
    assert y.shape == (B, ho, wo, cout) and np.isfinite(y).all(), f'{what}: poison or a non-finite value in the output'
    xin = x if sk is None else (x + sk).astype(np.float32)
    xact = orc.scale_shift_silu(xin, pro[0], pro[1]) if pro else xin
    w_oihw = np.ascontiguousarray(wt.transpose(3, 2, 0, 1))
    exact = True
    if form == 'direct' or (form == 'wino' and not c['fast']):
        y_ref = orc.conv2d(xact, wt, bias, k, s, p, up2, act=c['act'], res1=r1, res2=r2, wino=form == 'wino')
        _same(y, y_ref, what)
    elif form == 'bf16s':
        if k == 1:
            y_ref = orc.linear_bf16s(x.reshape(-1, cin), np.ascontiguousarray(wt.reshape(cin, cout).T), bias, c['act'],
                                     None if r1 is None else r1.reshape(-1, cout), None if r2 is None else r2.reshape(-1, cout)).reshape(y.shape)
        else:
            y_ref = orc.conv3x3_bf16s(x, wt, bias, r1, r2, stride=s)
        _same(y.view(np.uint32), y_ref.view(np.uint32), what)
    elif form == 'gemm_f16':
        rows = B * h * w
        ref, mag, rest = FR.gemm_ref(torch.from_numpy(x.reshape(rows, cin)), torch.from_numpy(w_oihw.reshape(cout, cin)), torch.from_numpy(bias),
                                     None if r1 is None else torch.from_numpy(r1.reshape(rows, cout)))
        if c['act'] == 1:       # the GELU epilogue == the oracle's GELU of the same launch without it, bit for bit (as test_gpu_linear_fp16.py)
            plain = G.conv2d(x, wt, bias, 1, act=0, f16=True)
            R.check(plain.reshape(rows, cout), ref, FR.gemm_bound(mag, rest), what + ' (plain)')
            _same(y, orc.math_eval('gelu', plain), what)
        else:
            R.check(y.reshape(rows, cout), ref, FR.gemm_bound(mag, rest), what)
        exact = False
    else:
        exact = False
        pos = _whole(B, ho, wo)
        rs = [torch.from_numpy(r) for r in res]
        if form == 'f16':
            ref, mag, near, rest = F16.conv_ref(torch.from_numpy(x), w_oihw, bias, pos, up2=up2, pro=pro, res=rs)
            bound = F16.conv_bound(mag, near, rest)
        else:                   # bf16x3, and the Winograd form with the hardware SiLU
            ref, mag, pt, rest = R.conv_ref(torch.from_numpy(x), w_oihw, bias, pos, 3, 1, 1, up2, pro=pro, fast_act=True, res=rs)
            bound = R.conv_bound(mag, pt, rest, 'bf16x3' if form == 'bf16x3' else 'wino4')
        R.check(torch.from_numpy(y).reshape(len(pos), cout), ref, bound, what)
    if ab is not None:
        if exact:               # the specified summation order: phases per half-resolution tile (x2 phase filters) / per sub-block (Winograd)
            a_ref, b_ref = orc.gn_coeffs(y_ref, gamma, beta, phases=2 if form == 'wino' else bool(up2))
            _same(ab[0], a_ref, what + ' fused gn a')
            _same(ab[1], b_ref, what + ' fused gn b')
        else:                   # against fp64 moments of the kernel's own output (anchor_cases.run_conv_case)
            ra, rb, ba, bb = R.gn_coeffs_ref(torch.from_numpy(y), gamma, beta)
            R.check(torch.from_numpy(ab[0]), ra, ba, what + ' gn a')
            R.check(torch.from_numpy(ab[1]), rb, bb, what + ' gn b')
    SEEN.add(name)


@pytest.mark.parametrize('case', CONV_CASES, ids=[_conv_id(c) for c in CONV_CASES])
def test_conv_forms(cuda_device, case):
    _run_conv(case)


# ---------------------------------------------------------------- row kernels
# Row tiles (csrc): LDS-DMA GEMM 128 x 128 (configs 0, 1) and 64 x 64 (config 2; the automatic choice at these sizes), split-bf16 GEMM and
# its 3x3 form 128 rows x 128 columns, fp16 GEMM 128 rows; ln_stats / layernorm / codebook_gather / vq_finalize 4 rows per block;
# row_sqsum 64; femasr_vq's GEMM 128 rows; two-pass search VQ_R = 128 rows; ragged N as test_linear_ragged_columns_all_configs (96, 160).
def _row_conv_cases():
    cs = []
    for cfg, tile in ((0, 128), (1, 128), (2, 64), (-1, 64)):
        for i, m in enumerate((1, tile - 1, tile + 1)):
            cs += [C('direct', (m, 1), 64, 96, B=1, k=1, p=0, cfg=cfg, nres=i), C('direct', (m, 1), 32, 160, B=1, k=1, p=0, cfg=cfg, act=1, nres=(i + 1) % 3)]
        cs += [C('direct', (tile + 1, 1), 32, 96, B=2, k=1, p=0, cfg=cfg, act=1, nres=2), C('direct', (3, 43), 32, 160, B=1, k=1, p=0, cfg=cfg, act=0, nres=0),
               C('direct', (5, 13), 32, 24, B=2, k=1, p=0, cfg=cfg, act=1, nres=0), C('direct', (5, 13), 32, 24, B=2, k=1, p=0, cfg=cfg, act=0, nres=1),
               C('direct', (5, 13), 32, 24, B=2, k=1, p=0, cfg=cfg, act=0, nres=2), C('direct', (5, 13), 32, 24, B=2, k=1, p=0, cfg=cfg, act=1, nres=1)]
    for i, m in enumerate((1, 127, 129)):
        cs += [C('bf16s', (m, 1), 64, 96, B=1, k=1, p=0, nres=i), C('bf16s', (m, 1), 64, 160, B=1, k=1, p=0, act=1, nres=(i + 1) % 3),
               C('bf16s', (m, 1), 64, 3, B=1, k=1, p=0, act=1, nres=(i + 2) % 3), C('bf16s', (m, 1), 64, 40, B=1, k=1, p=0, act=0, nres=(i + 2) % 3)]
        cs += [C('gemm_f16', (m, 1), 64, 96, B=1, k=1, p=0), C('gemm_f16', (m, 1), 64, 160, B=1, k=1, p=0, act=1), C('gemm_f16', (m, 1), 64, 40, B=1, k=1, p=0, nres=1)]
    # the 3x3 form of the split GEMM: 128 output pixels per block over the batch, stride 1 and 2
    cs += [C('bf16s', (1, 1), 64, 40, nres=0), C('bf16s', (7, 9), 64, 96, nres=1), C('bf16s', (5, 13), 64, 136, nres=2),
           C('bf16s', (15, 17), 64, 40, s=2, nres=1), C('bf16s', (16, 16), 64, 96, s=2, B=1, nres=0), C('bf16s', (23, 11), 64, 24, s=2, B=1, nres=2)]
    return cs


ROW_CONV_CASES = _row_conv_cases()


@pytest.mark.parametrize('case', ROW_CONV_CASES, ids=[_conv_id(c) for c in ROW_CONV_CASES])
def test_linear_forms(cuda_device, case):
    _run_conv(case)


@pytest.mark.parametrize('rows', [1, 3, 5, 63, 65])
def test_ln_stats_layernorm_row_sqsum(cuda_device, rows):
    x = _u(f'ln{rows}', (rows, 256), -4, 6)
    gamma, beta = _u('lng', (256,), 0.5, 1.5), _u('lnb', (256,), -0.5, 0.5)
    y = GA.run_twice(lambda: G.layernorm(x, gamma, beta), f'layernorm rows {rows}')
    _same(y, orc.layernorm(x, gamma, beta), f'layernorm rows {rows}')
    st = GA.run_twice(lambda: G.ln_stats(x), f'ln_stats rows {rows}')
    assert st.shape == (rows, 2) and np.isfinite(st).all()
    # femasr_layernorm is "the same moments, then fmaf((x - mean) * rstd, gamma, beta)": with gamma = 1, beta = 0 the oracle's LayerNorm IS
    # (x - mean) * rstd of its own moments, one fp32 subtraction and one fp32 multiplication per element
    one, zero = np.ones(256, np.float32), np.zeros(256, np.float32)
    _same(((x - st[:, :1]).astype(np.float32) * st[:, 1:]).astype(np.float32), orc.layernorm(x, one, zero), f'ln_stats rows {rows}: (x - mean) * rstd')
    lib = _lib.load()

    def sq():
        ops = G.Operands(f'row_sqsum rows {rows}').inp('x', x).out('out', 4 * rows).build()
        _lib.check(lib.femasr_row_sqsum(None, ops.p('x'), rows, 256, ops.p('out')))
        ops.check()
        return ops.get('out', torch.float32).cpu().numpy()
    ee = GA.run_twice(sq, f'row_sqsum rows {rows}')
    # (no oracle entry returns |x|^2 alone: an fp32 sum of D = 256 non-negative terms, in any order and with or without fma, is within
    # D * 2^-24 of the exact sum, relative)
    ref64 = (x.astype(np.float64) ** 2).sum(1)
    assert (np.abs(ee - ref64) <= 256 * 2.0 ** -24 * ref64).all(), f'row_sqsum rows {rows}'


@pytest.mark.parametrize('shape', [(1, 1, 1, 32), (2, 3, 5, 64), (1, 17, 15, 36), (3, 9, 29, 128)])
def test_gn_silu_apply_and_gn_coeffs(cuda_device, shape):
    """gn_silu_apply: grid-stride over float4s, 256 threads (C % 4 == 0).  gn_coeffs: both branches - the fused-moments layout
    (C / 32 a power of two: 8 x 16 tiles, scratch per tile) and the generic per-row one (C = 36 does not exist for 32 groups: C = 96)."""
    b, h, w, c = shape
    x = _u(f'gs{shape}', shape, -3, 4)
    a, bb = _u(f'gsa{shape}', (b, c), 0.5, 1.5), _u(f'gsb{shape}', (b, c), -0.5, 0.5)
    y = GA.run_twice(lambda: G.gn_silu_apply(x, a, bb), f'gn_silu_apply {shape}')
    _same(y.view(np.uint32), orc.scale_shift_silu(x, a, bb).view(np.uint32), f'gn_silu_apply {shape}')
    for cc in ({32: 32, 64: 64, 36: 96, 128: 128}[c], ):
        xx = _u(f'gc{shape}', (b, h, w, cc), -3, 4)
        gamma, beta = _u(f'gcg{cc}', (cc,), 0.5, 1.5), _u(f'gcb{cc}', (cc,), -0.5, 0.5)
        ga, gb = GA.run_twice(lambda: G.gn_coeffs(xx, gamma, beta), f'gn_coeffs {xx.shape}')
        a_ref, b_ref = orc.gn_coeffs(xx, gamma, beta)
        _same(ga, a_ref, f'gn_coeffs a {xx.shape}')
        _same(gb, b_ref, f'gn_coeffs b {xx.shape}')


@pytest.mark.parametrize('m', [1, 127, 129])
def test_vq_family(cuda_device, m):
    """n_e = 1024 at the smallest e_dim the two-pass search accepts (64): femasr_vq, femasr_vq_twopass, femasr_vq_candidates and
    femasr_codebook_gather, with the codebook images (repack, row_sqsum, vq_prepare) written into exact-size regions."""
    d = 64
    cb = _u('vqcb', (1024, d))
    z = (cb[(np.arange(m) * 37) % 1024] + 0.3 * _u(f'vqz{m}', (m, d))).astype(np.float32)
    idx_ref, zq_ref = orc.vq(z, cb)
    for mode in ('gemm', 'twopass'):
        idx, zq, cbt, ee = GA.run_twice(lambda: G.vq(z, cb, mode), f'vq {mode} M {m}')
        _same(idx, idx_ref, f'vq {mode} M {m} indices')
        _same(zq, zq_ref, f'vq {mode} M {m} z_q')
        assert np.array_equal(cbt, G.lib_weight_layout(cb.T.reshape(1, 1, d, 1024)))
    cand, cnt = GA.run_twice(lambda: G.vq_candidates(z, cb), f'vq_candidates M {m}')
    every = cnt == 0xFFFF
    n = np.where(every, 0, cnt).astype(np.int64)
    hit = every.copy()
    for k in range(32):
        hit |= (k < n) & (cand[:, k].astype(np.int64) == idx_ref)
    assert (n <= 32).all() and hit.all(), f'vq_candidates M {m}: {int((~hit).sum())} rows lost their first-min'
    for r in range(m):          # include/femasr_hip.h: a row's codes ascending, zeros behind them (no slot keeps poison or stale LDS)
        assert (np.diff(cand[r, :n[r]].astype(np.int64)) > 0).all() and not cand[r, n[r]:].any(), f'vq_candidates M {m}: row {r} {cand[r]} cnt {cnt[r]}'
    lib = _lib.load()

    def gather():
        ops = G.Operands(f'codebook_gather M {m}').inp('idx', idx_ref.astype(np.int64)).inp('cb', cb).out('zq', 4 * m * d).build()
        _lib.check(lib.femasr_codebook_gather(None, ops.p('idx'), m, d, ops.p('cb'), 1024, ops.p('zq')))
        ops.check()
        return ops.get('zq', torch.float32, (m, d)).cpu().numpy()
    _same(GA.run_twice(gather, f'codebook_gather M {m}'), cb[idx_ref], f'codebook_gather M {m}')


def _math_inputs(n):
    """n values spread over the whole call-site set (specials, subnormals and both clamps' neighbourhoods at n = 63, 65)."""
    import math_range as MR
    s = MR.call_site_set()
    return np.ascontiguousarray(s[np.linspace(0, s.size - 1, n).astype(np.int64)])


@pytest.mark.parametrize('n', [1, 2, 63, 65])
def test_debug_math_eval(cuda_device, n):
    """femasr_debug_math_eval: one value (or pair) per thread, grid-stride over blocks of 256.  The scalar selectors at every n, the
    packed ones (float2 accesses) at the even n."""
    import math_range as MR
    x = _math_inputs(n)
    assert x.size == n
    for fn, code in G.MATH_FN.items():
        if fn.endswith('2') and n % 2:
            continue                    # refused: test_debug_math_eval_refusals
        what = f'debug_math_eval {fn} n {n}'
        y = GA.run_twice(lambda: G.math_eval(fn, x), what)
        if code < 8:
            MR.assert_same(y, orc.math_eval(fn.rstrip('2'), x), what, x)


@pytest.mark.parametrize('n', [1, 2, 63, 65])
def test_debug_math_eval_refusals(cuda_device, n):
    """A bad fn, a null pointer, n <= 0 and - for the packed selectors - an odd n return FEMASR_ERR_INVALID and write nothing: y keeps
    its poison and no guard byte changes."""
    lib = _lib.load()
    x = _math_inputs(n)
    ops = G.Operands(f'debug_math_eval refusals n {n}').inp('x', x).out('y', 4 * n).build()
    poison = ops.get('y', torch.int32)
    px, py = ops.p('x'), ops.p('y')
    calls = [(9, px, n, py), (-1, px, n, py), (0, None, n, py), (0, px, n, None), (4, None, 2, py), (0, px, 0, py), (0, px, -2, py),
             (7, px, 0, py)]
    if n % 2:
        calls += [(code, px, n, py) for code in (4, 5, 6, 7)]
    for args in calls:
        assert lib.femasr_debug_math_eval(None, *args) == -1, args          # FEMASR_ERR_INVALID
    ops.check()
    assert torch.equal(ops.get('y', torch.int32), poison), 'a refused call wrote to y'


# ---------------------------------------------------------------- window attention: one (window, head) per wave, 8 x 8 windows
@pytest.mark.parametrize('b,h,w', [(1, 8, 8), (2, 8, 8), (1, 16, 16), (2, 16, 16)])
@pytest.mark.parametrize('shift', [0, 4])
def test_window_attention(cuda_device, b, h, w, shift):
    c = 256
    qkv = _u(f'qkv{b}{h}{shift}', (b, h * w, 3 * c), -2, 2)
    table = _u('tab', (225, 8), -0.5, 0.5)
    got = GA.run_twice(lambda: G.window_attention(qkv, b, h, w, c, 8, shift, table), f'window_attention B{b} {h}x{w} shift {shift}')
    _same(got, orc.window_attention(qkv, b, h, w, c, 8, shift, table), f'window attention B{b} {h}x{w} shift={shift}')


# ---------------------------------------------------------------- layout and image kernels: one odd-sized case each
def _raw(what, inputs, outs, call):
    """One library call on exact-size regions: inputs {name: array}, outs {name: (dtype, shape)}; call(lib, ops).  Returns the outputs."""
    lib = _lib.load()

    def go():
        ops = G.Operands(what)
        for n, a in inputs.items():
            ops.inp(n, a)
        for n, (dt, shp) in outs.items():
            ops.out(n, int(np.prod(shp)) * torch.empty(0, dtype=dt).element_size())
        ops.build()
        _lib.check(call(lib, ops))
        ops.check()
        return {n: ops.get(n, dt, shp).cpu() for n, (dt, shp) in outs.items()}
    return GA.run_twice(go, what)


def test_pad_and_crop(cuda_device):
    x = _u('padx', (2, 3, 21, 29), 0, 1)
    out = _raw('pad_nchw_to_nhwc', {'x': x}, {'y': (torch.float32, (2, 32, 40, 3))},
               lambda lib, o: lib.femasr_pad_nchw_to_nhwc(None, o.p('x'), 2, 3, 21, 29, 32, 40, o.p('y')))['y'].numpy()
    _same(out, orc.pad_nchw_to_nhwc(x, 32, 40), 'pad')
    y = _u('cropy', (2, 19, 23, 3), -1, 1)
    out = _raw('crop_nhwc_to_nchw', {'x': y}, {'y': (torch.float32, (2, 3, 13, 17))},
               lambda lib, o: lib.femasr_crop_nhwc_to_nchw(None, o.p('x'), 2, 19, 23, 3, 13, 17, o.p('y')))['y'].numpy()
    _same(out, orc.crop_nhwc_to_nchw(y, 13, 17), 'crop')
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (2, 21, 29, 3), dtype=np.uint8)
    yf = (rng.random((2, 19, 23, 3)) * 1.2 - 0.1).astype(np.float32)
    for swap in (0, 1):
        out = _raw(f'pad_u8hwc_to_nhwc swap {swap}', {'x': u8}, {'y': (torch.float32, (2, 32, 40, 3))},
                   lambda lib, o: lib.femasr_pad_u8hwc_to_nhwc(None, o.p('x'), 2, 21, 29, swap, 32, 40, o.p('y')))['y'].numpy()
        src = (u8[..., ::-1] if swap else u8).astype(np.float32) / np.float32(255.0)
        _same(out, orc.pad_nchw_to_nhwc(np.ascontiguousarray(src.transpose(0, 3, 1, 2)), 32, 40), f'pad u8 swap {swap}')
        out = _raw(f'crop_nhwc_to_u8hwc swap {swap}', {'x': yf}, {'y': (torch.uint8, (2, 13, 17, 3))},
                   lambda lib, o: lib.femasr_crop_nhwc_to_u8hwc(None, o.p('x'), 2, 19, 23, 13, 17, swap, o.p('y')))['y'].numpy()
        want = np.rint(np.clip(yf[:, :13, :17], 0, 1) * np.float32(255.0)).astype(np.uint8)
        _same(out, want[..., ::-1] if swap else want, f'crop u8 swap {swap}')


def test_concat_resize(cuda_device):
    a, b = _u('cra', (2, 6, 10, 4)), _u('crb', (2, 3, 5, 12))        # (channel counts: multiples of 4)
    out = _raw('concat_resize', {'a': a, 'b': b}, {'y': (torch.float32, (2, 6, 10, 16))},
               lambda lib, o: lib.femasr_concat_resize(None, o.p('a'), 4, o.p('b'), 3, 5, 12, 2, 6, 10, o.p('y')))['y'].numpy()
    _same(out, np.concatenate([a, np.repeat(np.repeat(b, 2, 1), 2, 2)], -1), 'concat_resize')


@pytest.mark.parametrize('u8', [False, True])
def test_extract_paste_blend_tiles(cuda_device, u8):
    """Odd sizes: a 2 x 3 x 21 x 27 image, two 9 x 11 windows; pasted bodies of odd size; a 1 x 2 blend grid with an overlap of 4."""
    rng = np.random.default_rng(7)
    B, Cc, H, W, th, tw, n = 2, 3, 21, 27, 9, 11, 2
    dt, tdt = (np.uint8, torch.uint8) if u8 else (np.float32, torch.float32)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if u8 else rng.random((B, Cc, H, W)).astype(np.float32)
    yx = np.array([[0, 0], [12, 16]], np.int32)
    if u8:
        tiles = _raw('extract_tiles_u8', {'img': img, 'yx': yx}, {'t': (tdt, (n * B, th, tw, 3))},
                     lambda lib, o: lib.femasr_extract_tiles_u8(None, o.p('img'), B, H, W, o.p('yx'), n, th, tw, o.p('t')))['t'].numpy()
        want = np.concatenate([img[:, y:y + th, x:x + tw] for y, x in yx])
    else:
        tiles = _raw('extract_tiles', {'img': img, 'yx': yx}, {'t': (tdt, (n * B, Cc, th, tw))},
                     lambda lib, o: lib.femasr_extract_tiles(None, o.p('img'), B, Cc, H, W, o.p('yx'), n, th, tw, o.p('t')))['t'].numpy()
        want = np.concatenate([img[:, :, y:y + th, x:x + tw] for y, x in yx])
    _same(tiles, want, 'extract_tiles')
    # paste: bodies (src_y, src_x, dst_y, dst_x, h, w) that cover a 7 x 17 canvas exactly: every canvas byte is written
    Ho, Wo = 7, 17
    rects = np.array([[1, 1, 0, 0, 7, 8], [2, 2, 0, 8, 7, 9]], np.int32)
    canvas_shape = (B, Ho, Wo, 3) if u8 else (B, Cc, Ho, Wo)
    if u8:
        got = _raw('paste_tiles_u8', {'t': tiles, 'r': rects}, {'c': (tdt, canvas_shape)},
                   lambda lib, o: lib.femasr_paste_tiles_u8(None, o.p('t'), B, n, th, tw, o.p('r'), 7, Ho, Wo, o.p('c')))['c'].numpy()
    else:
        got = _raw('paste_tiles', {'t': tiles, 'r': rects}, {'c': (tdt, canvas_shape)},
                   lambda lib, o: lib.femasr_paste_tiles(None, o.p('t'), B, Cc, n, th, tw, o.p('r'), 7, Ho, Wo, o.p('c')))['c'].numpy()
    want = np.zeros(canvas_shape, dt)
    for kk, (sy, sx, dy, dx, hh, ww) in enumerate(rects):
        t = tiles[kk * B:(kk + 1) * B]
        if u8:
            want[:, dy:dy + hh, dx:dx + ww] = t[:, sy:sy + hh, sx:sx + ww]
        else:
            want[:, :, dy:dy + hh, dx:dx + ww] = t[:, :, sy:sy + hh, sx:sx + ww]
    _same(got, want, 'paste_tiles')
    # blend: two 9 x 11 windows side by side on a 9 x 18 canvas, bodies of 9 columns (pitch 9), an overlap of 4 columns (margin 2 either
    # side of the body edge); the reference restates include/femasr_hip.h: w = (float)num / (float)(4 margin), acc and den summed from 0
    # in tile order, out = acc / den, the uint8 form on (float)byte with rintf and a clamp
    Hc, Wc, pitch = 9, 18, 9
    geom = np.array([[0, 0, th, tw, 0, 0, 0, 2], [0, 7, th, tw, 0, 0, 2, 0]], np.int32)
    acc = np.zeros((B, Cc, Hc, Wc), np.float32)
    den = np.zeros((Hc, Wc), np.float32)
    for kk, (ay, ax, hh, ww, ly, ry, lx, rx) in enumerate(geom):
        i = np.arange(ww)
        wl = np.ones(ww, np.float32) if lx == 0 else np.minimum(np.float32(1), (2 * i + 1).astype(np.float32) / np.float32(4 * lx))
        wr = np.ones(ww, np.float32) if rx == 0 else np.minimum(np.float32(1), (2 * (ww - 1 - i) + 1).astype(np.float32) / np.float32(4 * rx))
        wgt = np.minimum(wl, wr)[None, :] * np.ones((hh, 1), np.float32)
        t = tiles[kk * B:(kk + 1) * B]
        v = t.transpose(0, 3, 1, 2).astype(np.float32) if u8 else t
        acc[:, :, ay:ay + hh, ax:ax + ww] += wgt * v
        den[ay:ay + hh, ax:ax + ww] += wgt
    ref = acc / den
    if u8:
        ref = np.ascontiguousarray(np.rint(np.clip(ref, 0, 255)).astype(np.uint8).transpose(0, 2, 3, 1))
    lib = _lib.load()

    def blend():
        ops = G.Operands('blend_tiles' + ('_u8' if u8 else '')).inp('t', tiles).inp('geom', geom)
        ops.scratch('ptrs', 8 * n).out('c', ref.size * ref.itemsize).build()        # (addresses: they differ between the arenas)
        per = tiles[0:B].size * tiles.itemsize
        ops.r['ptrs'].as_(torch.int64)[:] = torch.tensor([ops.r['t'].ptr + kk * per for kk in range(n)], dtype=torch.int64)
        ops.arena.freeze(ops.r['ptrs'])
        if u8:
            rc = lib.femasr_blend_tiles_u8(None, ops.p('ptrs'), ops.p('geom'), n, 1, 2, pitch, B, Hc, Wc, ops.p('c'))
        else:
            rc = lib.femasr_blend_tiles(None, ops.p('ptrs'), ops.p('geom'), n, 1, 2, pitch, B, Cc, Hc, Wc, ops.p('c'))
        _lib.check(rc)
        ops.check()
        return ops.get('c', tdt, ref.shape).cpu().numpy()
    _same(GA.run_twice(blend, 'blend_tiles'), ref, 'blend_tiles')


def _dihedral(x, k):
    """Variant k of an (..., H, W) array: rows flipped (k & 1), columns flipped (k & 2), then transposed (k & 4)."""
    y = x[..., ::-1, :] if k & 1 else x
    y = y[..., :, ::-1] if k & 2 else y
    return np.swapaxes(y, -1, -2) if k & 4 else y


@pytest.mark.parametrize('u8', [False, True])
def test_dihedral_expand_merge(cuda_device, u8):
    """64 x 64 tiles: 67 x 35 has a ragged tile in either axis and differs between the axes (the transposed buffers are 35 x 67)."""
    rng = np.random.default_rng(9)
    B, Cc, H, W = 2, 3, 67, 35
    tdt = torch.uint8 if u8 else torch.float32
    if u8:
        x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        planes = x.transpose(0, 3, 1, 2)
        sshape, tshape = (4, B, H, W, 3), (4, B, W, H, 3)
        back = lambda v: np.ascontiguousarray(v.transpose(0, 2, 3, 1))
        out = _raw('dihedral_expand_u8', {'x': x}, {'s': (tdt, sshape), 't': (tdt, tshape)},
                   lambda lib, o: lib.femasr_dihedral_expand_u8(None, o.p('x'), B, H, W, o.p('s'), o.p('t')))
    else:
        x = rng.random((B, Cc, H, W)).astype(np.float32)
        planes = x
        sshape, tshape = (4, B, Cc, H, W), (4, B, Cc, W, H)
        back = lambda v: np.ascontiguousarray(v)
        out = _raw('dihedral_expand', {'x': x}, {'s': (tdt, sshape), 't': (tdt, tshape)},
                   lambda lib, o: lib.femasr_dihedral_expand(None, o.p('x'), B, Cc, H, W, o.p('s'), o.p('t')))
    st, tr = out['s'].numpy(), out['t'].numpy()
    for k in range(8):
        _same((st if k < 4 else tr)[k & 3], back(_dihedral(planes, k)), f'dihedral_expand variant {k}')
    # merge: eight independent results y_k laid out like the variants; z_k undoes the variant; fp32 sum in order, x 0.125 / bytes: half to even
    ys = [rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8) if u8 else rng.random((B, Cc, H, W)).astype(np.float32) for _ in range(8)]
    sbuf = np.stack([back(_dihedral(ys[k], k)) for k in range(4)])
    tbuf = np.stack([back(_dihedral(ys[k], k)) for k in range(4, 8)])
    if u8:
        S = sum(y.astype(np.int64) for y in ys)
        want = back(((S + 3 + ((S >> 3) & 1)) >> 3).astype(np.uint8))
        got = _raw('dihedral_merge_u8', {'s': sbuf, 't': tbuf}, {'o': (tdt, (B, H, W, 3))},
                   lambda lib, o: lib.femasr_dihedral_merge_u8(None, o.p('s'), o.p('t'), B, H, W, o.p('o')))['o'].numpy()
    else:
        acc = ys[0]
        for y in ys[1:]:
            acc = (acc + y).astype(np.float32)
        want = (np.float32(0.125) * acc).astype(np.float32)
        got = _raw('dihedral_merge', {'s': sbuf, 't': tbuf}, {'o': (tdt, (B, Cc, H, W))},
                   lambda lib, o: lib.femasr_dihedral_merge(None, o.p('s'), o.p('t'), B, Cc, H, W, o.p('o')))['o'].numpy()
    _same(got, want, 'dihedral_merge')


# ---------------------------------------------------------------- whole-network entries: exact-size workspace, two poisons
# The smallest input each config accepts through test()'s mirror pad (plan_geometry, csrc/model.hip: the pad may not exceed the image in
# the LQ configs, whose Swin stage needs a feature map divisible by 8: x4 pads to multiples of 16, x2 of 32; HQ pads to at most 2 H) and one
# odd size that needs the mirror pad in both axes.
NET_SIZES = {'x4': [(8, 8), (13, 19)], 'x2': [(16, 16), (21, 27)], 'hq': [(4, 4), (13, 19)]}
_NETS = {}


def _net(cn):
    from helpers import synth_weights
    if cn not in _NETS:
        _NETS[cn] = G.build_net(cn, synth_weights(cn, 3, 'trained'))
    return _NETS[cn]


def _shapes(lib, h, hh, ww):
    oh, ow, nq = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    qh, qw = (ctypes.c_int * _lib.MAX_CODEBOOKS)(), (ctypes.c_int * _lib.MAX_CODEBOOKS)()
    _lib.check(lib.femasr_forward_shapes(h, hh, ww, 1, ctypes.byref(oh), ctypes.byref(ow), ctypes.byref(nq), ctypes.byref(qh), ctypes.byref(qw)))
    return oh.value, ow.value, [(qh[k], qw[k]) for k in range(nq.value)]


def _guarded_forward(net, x, u8):
    """femasr_forward / femasr_forward_u8 with the image, the indices and a workspace of EXACTLY femasr_workspace_bytes in one arena."""
    lib, h = net._native(x.device)
    b, hh, ww = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    oh, ow, qhw = _shapes(lib, h, hh, ww)
    nidx = sum(b * a * c for a, c in qhw)
    what = f'femasr_forward{"_u8" if u8 else ""} B{b} {hh}x{ww} {net.decoder_math}/{net.linear_math} streams {net.num_streams}'

    def go():
        ops = G.Operands(what).inp('x', x).out('out', b * 3 * oh * ow * (1 if u8 else 4)).out('idx', 8 * nidx)
        ops.scratch('ws', G.qp('femasr_workspace_bytes', h, b, hh, ww, 1)).build()
        st = net._stream(x.device)
        if u8:
            rc = lib.femasr_forward_u8(h, st, ops.p('x'), b, hh, ww, 0, 1, ops.p('out'), ops.p('idx'), ops.p('ws'), ops.r['ws'].nbytes)
        else:
            rc = lib.femasr_forward(h, st, ops.p('x'), b, hh, ww, 1, ops.p('out'), ops.p('idx'), ops.p('ws'), ops.r['ws'].nbytes)
        _lib.check(rc)
        ops.check()
        return (ops.get('out', torch.uint8, (b, oh, ow, 3)) if u8 else ops.get('out', torch.float32, (b, 3, oh, ow))), ops.get('idx', torch.int64)
    return GA.run_twice(go, what) + (qhw,)


def _guarded_decode(net, idx, b, qh, qw):
    lib, h = net._native(idx.device)
    up = 2 ** net.max_depth
    what = f'femasr_decode_indices B{b} {qh}x{qw} {net.decoder_math}'

    def go():
        ops = G.Operands(what).inp('idx', idx).out('out', 4 * b * 3 * qh * up * qw * up)
        ops.scratch('ws', G.qp('femasr_decode_workspace_bytes', h, b, qh, qw)).build()
        _lib.check(lib.femasr_decode_indices(h, net._stream(idx.device), ops.p('idx'), b, qh, qw, ops.p('out'), ops.p('ws'), ops.r['ws'].nbytes))
        ops.check()
        return ops.get('out', torch.float32, (b, 3, qh * up, qw * up))
    return GA.run_twice(go, what)


def _network_case(cn, dm, lm, streams=1, B=2):
    net = _net(cn)
    net.decoder_math, net.linear_math, net.num_streams = dm, lm, streams
    try:
        for hh, ww in NET_SIZES[cn]:
            g = torch.Generator().manual_seed(hh * 100 + ww)
            u = torch.randint(0, 256, (B, hh, ww, 3), generator=g, dtype=torch.uint8).cuda()
            x = (u.float() / 255.0).permute(0, 3, 1, 2).contiguous()
            y0, idx0 = net.test_with_all_indices(x)                           # the ordinary call: torch's own allocations
            flat0 = torch.cat([i.reshape(-1) for i in idx0])
            y, idx, qhw = _guarded_forward(net, x, False)
            assert torch.equal(y, y0) and torch.equal(idx, flat0), f'{cn} {dm}/{lm} {hh}x{ww}: guarded forward differs from the ordinary call'
            yu, idxu, _ = _guarded_forward(net, u, True)
            assert torch.equal(yu, net.test_u8(u)) and torch.equal(idxu, flat0), f'{cn} {dm}/{lm} {hh}x{ww}: guarded uint8 forward differs'
            (qh, qw) = qhw[0]
            if len(qhw) == 1:
                d = _guarded_decode(net, idx0[0].contiguous(), B, qh, qw)
                assert torch.equal(d, net.decode_indices(idx0[0])), f'{cn} {dm} {hh}x{ww}: guarded decode_indices differs'
    finally:
        net.decoder_math, net.linear_math, net.num_streams = 'fp32_strict', 'bf16_split', 1


@pytest.mark.parametrize('lm', ['bf16_split', 'fp32'])
@pytest.mark.parametrize('dm', ['fp32', 'bf16x3', 'fp16'])
@pytest.mark.parametrize('cn', ['x4', 'x2', 'hq'])
def test_network_entries_exact_workspace(cuda_device, cn, dm, lm):
    _network_case(cn, dm, lm)


@pytest.mark.parametrize('streams', [1, 2])
def test_network_entries_streams(cuda_device, streams):
    _network_case('x4', 'fp32', 'bf16_split', streams=streams, B=3)


# ---------------------------------------------------------------- metric entries: a workspace of exactly *_workspace_bytes, two poisons
@pytest.mark.parametrize('crop,ty', [(0, 0), (3, 1)])
def test_psnr_ssim_exact_workspace(cuda_device, crop, ty):
    """femasr_psnr_ssim on three 23 x 37 pairs (SSIM's 11 x 11 window: a 13 x 27 valid area after the crop): every result bit-identical
    to femasr_amd.psnr_ssim's, whose workspace is a torch allocation."""
    from femasr_amd import psnr_ssim as PS
    g = torch.Generator().manual_seed(41)
    x = torch.randint(0, 256, (3, 23, 37, 3), generator=g, dtype=torch.uint8).cuda()
    y = (x.int() + torch.randint(-9, 10, x.shape, generator=g).cuda()).clamp(0, 255).to(torch.uint8)
    B, H, W, _ = x.shape
    lib = _lib.load()

    def go():
        ops = G.Operands(f'psnr_ssim crop {crop} y {ty}').inp('x', x).inp('y', y).out('psnr', 8 * B).out('ssim', 8 * B).out('mse', 8 * B)
        ops.scratch('ws', G.qp('femasr_psnr_ssim_workspace_bytes', B, H, W, crop, ty)).build()
        _lib.check(lib.femasr_psnr_ssim(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ops.p('x'), ops.p('y'), B, H, W, crop, ty,
                                        ops.p('psnr'), ops.p('ssim'), ops.p('mse'), ops.p('ws'), ops.r['ws'].nbytes))
        ops.check()
        return [ops.get(n, torch.float64) for n in ('psnr', 'ssim', 'mse')]
    got = GA.run_twice(go, f'psnr_ssim crop {crop} y {ty}')
    want = PS._scores(x, y, crop, ty, True, True, True)
    for gq, wq, n in zip(got, want, ('psnr', 'ssim', 'mse')):
        assert torch.equal(gq, wq), f'{n}: {gq.tolist()} != {wq.tolist()}'


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_imresize_exact_workspace(cuda_device, dtype):
    """femasr_imresize, three 23 x 37 planes to half size (antialiased bicubic: 12 x 19): bit-identical to femasr_amd.resize.imresize."""
    from femasr_amd import resize
    g = torch.Generator().manual_seed(43)
    x = torch.rand((3, 23, 37), generator=g, dtype=torch.float64).to(dtype).cuda()
    N, H, W = x.shape
    Ho, Wo = 12, 19
    wh, ih, ph = resize.device_tables(H, Ho, 0.5, True, x.device)
    ww, iw, pw = resize.device_tables(W, Wo, 0.5, True, x.device)
    lib = _lib.load()
    esz = x.element_size()

    def go():
        ops = G.Operands(f'imresize {dtype}').inp('x', x).inp('wh', wh).inp('ih', ih).inp('ww', ww).inp('iw', iw).out('out', N * Ho * Wo * esz)
        ops.scratch('ws', G.qp('femasr_imresize_workspace_bytes', N, H, W, Ho, Wo)).build()
        _lib.check(lib.femasr_imresize(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ops.p('x'), int(dtype == torch.float64), N, H, W, Ho, Wo,
                                       ops.p('wh'), ops.p('ih'), ph, ops.p('ww'), ops.p('iw'), pw, ops.p('out'), ops.p('ws'), ops.r['ws'].nbytes))
        ops.check()
        return ops.get('out', dtype, (N, Ho, Wo))
    got = GA.run_twice(go, f'imresize {dtype}')
    assert torch.equal(got, resize.imresize(x, 0.5)), 'imresize differs from the Python entry'


@pytest.mark.parametrize('u8', [False, True])
def test_color_fix_exact_workspace(cuda_device, u8):
    """femasr_color_fix / _u8: two images of 7 x 9 against their x3 results (21 x 27), 3 levels; bit-identical to colorfix.wavelet_color_fix."""
    from femasr_amd import colorfix as CF
    g = torch.Generator().manual_seed(47)
    B, h, w, sc, levels = 2, 7, 9, 3, 3
    if u8:
        lq = torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8).cuda()
        sr = torch.randint(0, 256, (B, sc * h, sc * w, 3), generator=g, dtype=torch.uint8).cuda()
    else:
        lq = torch.rand((B, 3, h, w), generator=g).cuda()
        sr = torch.rand((B, 3, sc * h, sc * w), generator=g).cuda()
    planes = 3 * B
    wh, ih, ph, ww, iw, pw = CF._tables(h, w, sc, sr.device)
    lib = _lib.load()
    fn = lib.femasr_color_fix_u8 if u8 else lib.femasr_color_fix
    what = 'color_fix' + ('_u8' if u8 else '')

    def go():
        ops = G.Operands(what).inp('sr', sr).inp('lq', lq).inp('wh', wh).inp('ih', ih).inp('ww', ww).inp('iw', iw).out('out', sr.numel() * sr.element_size())
        ops.scratch('ws', G.qp('femasr_color_fix_workspace_bytes', planes, h, w, sc * h, sc * w, sc)).build()
        _lib.check(fn(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ops.p('sr'), ops.p('lq'), B if u8 else planes, h, w, sc * h, sc * w, sc,
                      levels, ops.p('wh'), ops.p('ih'), ph, ops.p('ww'), ops.p('iw'), pw, ops.p('out'), ops.p('ws'), ops.r['ws'].nbytes))
        ops.check()
        return ops.get('out', sr.dtype, tuple(sr.shape))
    got = GA.run_twice(go, what)
    assert torch.equal(got, CF.wavelet_color_fix(sr, lq, levels)), f'{what} differs from the Python entry'


def test_niqe_features_exact_workspace(cuda_device):
    """femasr_niqe_features on the smallest image with two blocks (96 x 192) plus a crop border of 4: features and alpha positions
    bit-identical to femasr_amd.niqe.features."""
    import niqe_cases as NC
    from femasr_amd import niqe as N
    from femasr_amd import resize
    from femasr_amd.models.femasr_model import aggd_tables
    g = torch.Generator().manual_seed(53)
    x = torch.randint(0, 256, (2, 104, 200, 3), generator=g, dtype=torch.uint8).cuda()
    B, H, W, _ = x.shape
    crop = 4
    params = N.check_params(NC.params())
    nh, nw = (H - 2 * crop) // 96, (W - 2 * crop) // 96
    Hb, Wb = nh * 96, nw * 96
    window = torch.from_numpy(params.window).cuda()
    tables = torch.from_numpy(np.concatenate(aggd_tables())).cuda()
    wh, ih, ph = resize.device_tables(Hb, Hb // 2, 0.5, True, x.device)
    ww, iw, pw = resize.device_tables(Wb, Wb // 2, 0.5, True, x.device)
    lib = _lib.load()

    def go():
        ops = G.Operands('niqe_features').inp('x', x).inp('window', window).inp('tables', tables).inp('wh', wh).inp('ih', ih).inp('ww', ww).inp('iw', iw)
        ops.out('feat', 8 * B * nh * nw * 36).out('pos', 4 * B * nh * nw * 10).scratch('ws', G.qp('femasr_niqe_workspace_bytes', B, H, W, crop)).build()
        _lib.check(lib.femasr_niqe_features(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ops.p('x'), B, H, W, crop, ops.p('window'), ops.p('tables'),
                                            ops.p('wh'), ops.p('ih'), ph, ops.p('ww'), ops.p('iw'), pw, ops.p('feat'), ops.p('pos'), ops.p('ws'),
                                            ops.r['ws'].nbytes))
        ops.check()
        return ops.get('feat', torch.float64, (B, nh * nw, 36)), ops.get('pos', torch.int32, (B, nh * nw, 10))
    feat, pos = GA.run_twice(go, 'niqe_features')
    want = N.features(x, NC.params(), crop)
    assert torch.equal(feat.view(torch.int64), want.features.view(torch.int64)) and torch.equal(pos, want.positions), 'niqe_features differs from the Python entry'


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_lpips_forward_exact_workspace(cuda_device, net):
    """femasr_lpips_forward on two pairs at the smallest size both backbones take with a ragged tile (33 x 37): scores and per-layer
    terms bit-identical to the LPIPS module's."""
    from femasr_amd import lpips as L
    m = L.LPIPS(net, state_dict={k: torch.from_numpy(v) for k, v in synth.lpips_state(L.expected_shapes(net), 7).items()}).cuda()
    shape = (2, 3, 33, 37)
    x0, x1 = torch.from_numpy(synth.synth_input(11, shape)).cuda(), torch.from_numpy(synth.synth_input(12, shape)).cuda()
    lib, h = m._native(x0.device)
    B, _, H, W = shape

    def go():
        ops = G.Operands(f'lpips_forward {net}').inp('x0', x0).inp('x1', x1).out('out', 4 * B).out('terms', 4 * B * 5)
        ops.scratch('ws', G.qp('femasr_lpips_workspace_bytes', h, B, H, W)).build()
        _lib.check(lib.femasr_lpips_forward(h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ops.p('x0'), ops.p('x1'), B, H, W, ops.p('out'),
                                            ops.p('terms'), ops.p('ws'), ops.r['ws'].nbytes))
        ops.check()
        return ops.get('out', torch.float32), ops.get('terms', torch.float32, (B, 5))
    out, terms = GA.run_twice(go, f'lpips_forward {net}')
    want, wterms = m(x0, x1, per_layer=True)
    assert torch.equal(out, want.reshape(-1)) and torch.equal(terms, wterms), f'lpips {net} differs from the module'


@pytest.mark.parametrize('c,pool,h,w', [(64, 1, 23, 37), (128, 2, 21, 33), (192, 0, 11, 7)])
def test_lpips_tap_and_finalize(cuda_device, c, pool, h, w):
    """femasr_lpips_tap with femasr_lpips_tap_partials(h, w) partials per pair and its fused max-pool (3x3 stride 2 / 2x2), then
    femasr_lpips_finalize: the pooled map bit for bit, the terms within the bar of tests/test_gpu_lpips.py::test_tap_unit."""
    import lpips_ref
    rng = np.random.RandomState(c + h)
    b = 2
    f = np.maximum(rng.randn(2 * b, h, w, c), 0).astype(np.float32)
    wl = (rng.rand(c) / c).astype(np.float32)
    hp, wp = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if pool == 1 else (h // 2, w // 2)
    lib = _lib.load()
    hw = (ctypes.c_int32 * 2)(h, w)

    def go():
        ops = G.Operands(f'lpips_tap {h}x{w}x{c} pool {pool}').inp('f', f).inp('w', wl)
        ops.out('part', 8 * b * G.q('femasr_lpips_tap_partials', h, w))
        if pool:
            ops.out('pooled', 4 * 2 * b * hp * wp * c)
        ops.out('out', 4 * b).out('terms', 4 * b).build()
        _lib.check(lib.femasr_lpips_tap(None, ops.p('f'), 2 * b, h, w, c, ops.p('w'), pool, ops.p('pooled'), ops.p('part')))
        ops.check('tap')
        _lib.check(lib.femasr_lpips_finalize(None, ops.p('part'), b, 1, hw, ops.p('out'), ops.p('terms')))
        ops.check('finalize')
        return (ops.get('terms', torch.float32).cpu().numpy(), ops.get('out', torch.float32).cpu().numpy(),
                ops.get('pooled', torch.float32, (2 * b, hp, wp, c)).cpu().numpy() if pool else None)
    terms, out, pooled = GA.run_twice(go, f'lpips_tap {h}x{w}x{c} pool {pool}')
    if pool:
        k = 3 if pool == 1 else 2
        want = np.full((2 * b, hp, wp, c), -np.inf, np.float32)
        for ky in range(k):
            for kx in range(k):
                want = np.maximum(want, f[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :][:, :hp, :wp])
        _same(pooled, want, 'lpips_tap pooled map')
    ref = lpips_ref.head(torch.from_numpy(f[:b].astype(np.float64)).permute(0, 3, 1, 2),
                         torch.from_numpy(f[b:].astype(np.float64)).permute(0, 3, 1, 2), wl.astype(np.float64)).numpy()
    assert np.all(np.abs(terms - ref) <= 2e-6 * ref + 1e-9), (terms, ref)
    _same(out, terms, 'lpips_finalize: one layer')


def test_clock_probe_stays_inside_its_entries(cuda_device):
    """femasr_clock_probe writes femasr_clock_probe_entries() 64-bit tick counts (times: a scratch region, only the guards are checked)."""
    lib = _lib.load()
    ops = G.Operands('clock_probe').scratch('ticks', 8 * G.q('femasr_clock_probe_entries')).build()
    _lib.check(lib.femasr_clock_probe(None, 64, ops.p('ticks')))
    ops.check()
    assert int((ops.get('ticks', torch.int64) > 0).sum()) == G.q('femasr_clock_probe_entries')


# ---------------------------------------------------------------- coverage: every conv instantiation has a guard case
# Rows of the variant tables that no shape femasr_conv2d accepts can select:
UNREACHABLE = {
    # femasr_conv_bf16x3_pick_variant sends Cout 33..64 to rows 15-17 (64 px x 32 ch per wave); the older 64-column tilings stay in the
    # table for the micro-benchmarks: rows 3-5 (8 waves, x2 with 4) and rows 12-14 (32 px x 64 ch per wave) - anchor_cases.bf16x3_unit_cases
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_NONE,up2=false,waves=4x2>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_GN_SILU,up2=false,waves=4x2>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_NONE,up2=true,waves=4x1>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_NONE,up2=false,waves=4x1>',
    'conv3x3_halo_bf16x3<8x16x64,FEMASR_PRO_GN_SILU,up2=false,waves=4x1>',
    # the VQ epilogue of the LDS-DMA GEMM is not a femasr_conv2d launch: femasr_vq runs it (test_vq_family, mode 'gemm')
    'gemm_dma<tile=64*2,k=8*4,stages=2,act=0,nres=0,vq=true>',
    'gemm_dma<tile=64*2,k=8*2,stages=3,act=0,nres=0,vq=true>',
}


def test_every_conv_instantiation_has_a_guard_case(cuda_device):
    """Runs last: the names the conv cases of this module launched (femasr_debug_conv_variant_name) against every conv instantiation the
    library lists (the profile slots of a handle whose names are conv instantiations: they carry template arguments)."""
    import helpers
    from helpers import synth_weights
    have = set()           # (from the tables, so that a deselected case still counts)
    lib = _lib.load()
    for c in CONV_CASES + ROW_CONV_CASES:
        prev_small, prev_cfg = lib.femasr_conv_small_launch_blocks(c['small']), lib.femasr_gemm_force_config(c['cfg'])
        try:
            h, w = c['hw']
            have.add(G.conv_variant_name((c['B'], h, w, c['cin']), c['cout'], c['k'], c['s'], c['p'], c['up2'], prologue=1 if c['pro'] else 0,
                                         act=c['act'], nres=c['nres'], fast_act=c['fast'], in_add=c['in_add'], bf16x3=c['form'] == 'bf16x3',
                                         wino=c['form'] == 'wino', bf16s=c['form'] == 'bf16s', f16=c['form'] in ('f16', 'gemm_f16')))
        finally:
            lib.femasr_conv_small_launch_blocks(prev_small)
            lib.femasr_gemm_force_config(prev_cfg)
    cn = sorted(helpers.CONFIGS)[0]
    net = G.build_net(cn, synth_weights(cn, 3, 'trained'))
    _, hnd = net._native(next(net.parameters()).device)
    listed = set()
    for i in range(lib.femasr_profile_slots(hnd)):
        nm = lib.femasr_profile_name(hnd, i).decode()
        if '<' in nm:
            listed.add(nm)
    assert listed, 'the library listed no conv instantiation'
    assert UNREACHABLE <= listed, f'UNREACHABLE names the library does not list: {sorted(UNREACHABLE - listed)}'
    want = listed - UNREACHABLE
    assert have == want, f'conv instantiations without a guard case: {sorted(want - have)}; cases of unknown instantiations: {sorted(have - want)}'
    ran = SEEN - have
    assert not ran, f'cases ran under names the table does not give: {sorted(ran)}'

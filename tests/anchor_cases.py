"""Shared machinery of the fp64-anchor GPU tests (tests/test_gpu_fp64_anchor.py: the benchmarked workloads;
tests/test_gpu_product_anchor.py: the launches the CLI and the Python API make by default, and the kernels' offset limits;
tests/test_gpu_mode_anchor.py: the non-default arithmetic modes - MODES, mode_inventory, BF16X3_UNIT - at both sets of shapes).

inventory() lists the distinct (instantiation, launch shape) cases of a workload table - the instantiation name comes from the library
itself (femasr_debug_conv_variant_name, which needs no GPU) - and run_conv_case / run_small_case launch one case through the public
unit ABI and hold it to tests/fp64_ref.py.
"""
import ctypes
import math

import numpy as np
import torch

import fp64_ref as R
from femasr_amd import _lib, synth


WORST = {}          # form -> worst err / bound seen (printed by the last test)


def _note(form, r):
    WORST[form] = max(WORST.get(form, 0.0), r)


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _weight_shapes(cfg):
    from femasr_amd.archs import build_network
    net = build_network(dict(type='FeMaSRNet', **cfg))
    return {k: tuple(v.shape) for k, v in net.state_dict().items()}


_SHAPES = {}


def _workload(wl_name):
    return R.WORKLOADS[wl_name] if wl_name in R.WORKLOADS else R.PRODUCT_WORKLOADS[wl_name]


def _layers(wl_name, sub_b, decoder_math='fp32'):
    wl = _workload(wl_name)
    key = repr(sorted(wl['cfg'].items()))
    if key not in _SHAPES:
        _SHAPES[key] = _weight_shapes(wl['cfg'])
    return R.workload_layers(wl['cfg'], sub_b, wl['hw'], wl['fn'], _SHAPES[key], decoder_math)


def _conv_args(L, form, fast_act):
    """ConvArgs of the launch as the network makes it (weight images set to a non-null marker: the hook reads no pointer)."""
    a = _lib.ConvArgs()
    a.B, a.H, a.W, a.Cin, a.Cout = L['B'], L['H'], L['W'], L['cin'], L['cout']
    a.ksz, a.stride, a.pad, a.up2 = L['ksz'], L['stride'], L['pad'], int(L['up2'])
    hv, wv = (2 * L['H'], 2 * L['W']) if L['up2'] else (L['H'], L['W'])
    a.Ho, a.Wo = (hv + 2 * L['pad'] - L['ksz']) // L['stride'] + 1, (wv + 2 * L['pad'] - L['ksz']) // L['stride'] + 1
    a.prologue = 1 if (L['pro'] and form != 'split3x3') else 0
    a.act = L['act']
    a.res1 = 1 if L['nres'] >= 1 else None
    a.res2 = 1 if L['nres'] >= 2 else None
    a.w = 1
    if form in ('wino4', 'wino_up2'):
        a.w_wino = 1
        a.fast_act = int(fast_act)
    if form in ('split3x3', 'split1x1'):
        a.w_bf16s = 1
    if form == 'bf16x3':
        a.w_bf16x3 = 1
    if L['up2'] and form == 'direct':
        a.w_up2 = 1
    if form == 'wino_up2' and L['in_add']:
        a.in_add = 1
    return a


def _slot(a):
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().femasr_debug_conv_variant_name(ctypes.byref(a), buf, len(buf)))
    return buf.value.decode()


def _gn_tiles(form, a):
    """The forms' gn_tiles rules (csrc/conv_forms.hip kConvForms): fused GroupNorm partials per sample of this form, 0 = none."""
    c = a.Cout
    fus = c % 32 == 0 and (c // 32) & (c // 32 - 1) == 0 and c // 32 <= 32
    halo = a.ksz == 3 and a.stride == 1 and a.pad == 1 and a.Cin % 32 == 0 and a.act in (0, 2) and not (a.up2 and a.prologue)
    if form in ('split3x3', 'split1x1') or not fus:
        return 0
    if form == 'bf16x3':          # per 8x16 tile of the output (full resolution for an x2 conv), at most 8 channels per group
        return ((a.Ho + 7) // 8) * ((a.Wo + 15) // 16) if c <= 256 else 0
    if form in ('wino4', 'wino_up2'):
        return ((a.Ho + 15) // 16) * ((a.Wo + 15) // 16) if halo else 0
    if not halo:
        return 0
    return 4 * ((a.H + 7) // 8) * ((a.W + 15) // 16) if a.up2 else ((a.Ho + 7) // 8) * ((a.Wo + 15) // 16)


def inventory(wl_name, modes=('fp32', 'fp32_strict'), linear_math='bf16_split', sub_batches=None, split_res2=False):
    """Distinct (instantiation, launch shape) conv cases and the small-kernel cases of one workload: {key: case}.
    sub_batches: only these of the workload's sub-batch sizes.  split_res2: a conv with two residuals is a case of its own (the
    names of the halo, bf16x3 and GEMM instantiations do not tell the residual count; the mode inventories ask for it)."""
    wl = _workload(wl_name)
    convs, small = {}, {}
    subs = wl.get('sub_batches') or R.sub_batches(wl['batch'], R.BENCH_STREAMS)
    assert sub_batches is None or set(sub_batches) <= set(subs), (wl_name, sub_batches, subs)
    for sub_b in (subs if sub_batches is None else sorted(sub_batches)):
        per_mode = [_layers(wl_name, sub_b, dm) for dm in modes]          # (the skip schedule follows the mode; same layers, same order)
        for Ls in zip(*per_mode):
            if Ls[0]['kind'] != 'conv':
                L = Ls[0]
                small.setdefault((L['kind'],) + tuple(sorted((k, v) for k, v in L.items() if k not in ('kind', 'key'))), L)
                continue
            for dm, L in zip(modes, Ls):
                form = R.conv_form(L, dm, linear_math)
                fast = dm == 'fp32' and form in ('wino4', 'wino_up2')
                a = _conv_args(L, form, fast)
                name = _slot(a)
                key = (name, L['B'], L['H'], L['W'], L['cin'], L['cout'], L['ksz'], L['stride'], L['in_add'], L['gn_out'])
                if split_res2 and L['nres'] == 2:
                    key += ('res2',)
                convs.setdefault(key, dict(L=L, form=form, fast=fast, slot=name))
    return convs, small


def product_inventory(names=None):
    """The cases of fp64_ref.PRODUCT_WORKLOADS (or of `names`: a list, or {name: sub-batch sizes or None}) that the benchmarked
    workloads' inventories do not hold."""
    bench = set()
    for wl in R.WORKLOADS:
        bench |= set(inventory(wl)[0])
    convs, small = {}, {}
    for n in (names if names is not None else R.PRODUCT_WORKLOADS):
        c, s = inventory(n, sub_batches=names[n] if isinstance(names, dict) else None)
        for k, v in c.items():
            if k not in bench:
                convs.setdefault(k, v)
        for k, v in s.items():
            small.setdefault(k, v)
    return convs, small


# ---------------------------------------------------------------- the non-default arithmetic modes
MODES = (('bf16x3', 'bf16_split'), ('fp32_direct', 'bf16_split'), ('fp32', 'fp32'))          # (decoder_math, linear_math)
MODE_PRODUCT = {'tiled1440x1440_win272x272': (16, 6), 'whole599x599_x4': None}                 # the product shapes the mode module launches


def mode_inventory(names, decoder_math, linear_math):
    """The cases of the workloads `names` (a list, or {name: sub-batch sizes or None}) under one non-default mode that neither the
    benchmarked workloads' default inventories nor the default inventories of `names` hold (those run in the other two modules)."""
    default, default_small = set(), set()
    for wl in R.WORKLOADS:
        c, s = inventory(wl)
        default |= set(c)
        default_small |= set(s)
    convs, small = {}, {}
    for n in names:
        subs = names[n] if isinstance(names, dict) else None
        if n not in R.WORKLOADS:
            c, s = inventory(n, sub_batches=subs)
            default |= set(c)
            default_small |= set(s)
        c, s = inventory(n, modes=(decoder_math,), linear_math=linear_math, sub_batches=subs, split_res2=True)
        for k, v in c.items():
            if k not in default:
                convs.setdefault(k, v)
        for k, v in s.items():
            if k not in default_small:
                small.setdefault(k, v)
    return convs, small


def make_case(form, B, H, W, cin, cout, up2=False, pro=False, nres=0, gn_out=False, fast=False, key=None):
    """A 3x3 stride-1 conv case outside the workload tables (unit shapes, limit shapes)."""
    L = dict(kind='conv', key=key or f'unit {form}', B=B, H=H, W=W, cin=cin, cout=cout, ksz=3, stride=1, pad=1, up2=up2, pro=pro, nres=nres,
             act=0, behind=True, gn_out=gn_out, in_add=False)
    return dict(L=L, form=form, fast=fast, slot=_slot(_conv_args(L, form, fast)))


# The 12 instantiations femasr_conv_bf16x3_pick_variant can return (g_v16 rows 0-2, 6-11, 15-17).  The network's layers behind the
# lookup reach seven of them; no conv there has Cout <= 32, and none with 33 .. 128 output channels is without both a prologue and x2
# (tests/test_fp64_anchor_host.py::test_bf16x3_instantiations_are_all_launched derives that).  Those five get unit shapes at the
# bench workload's grid sizes, B = 6: ragged last tiles, one or two residuals, fused GroupNorm partials.
def bf16x3_unit_cases():
    return [make_case('bf16x3', 6, 288, 288, 128, 128, nres=1, gn_out=True, key='unit bf16x3 128 plain'),
            make_case('bf16x3', 6, 570, 566, 64, 64, nres=2, key='unit bf16x3 64 plain'),
            make_case('bf16x3', 6, 570, 566, 64, 32, nres=1, gn_out=True, key='unit bf16x3 32 plain'),
            make_case('bf16x3', 6, 576, 576, 64, 32, pro=True, nres=2, gn_out=True, key='unit bf16x3 32 gn'),
            make_case('bf16x3', 6, 285, 283, 64, 32, up2=True, gn_out=True, key='unit bf16x3 32 x2')]


# ---------------------------------------------------------------- launches through the public unit ABI
def _pack(form, L, w_oihw):
    lib = _lib.load()
    o, i, kh, kw = w_oihw.shape
    packed = {}
    wd = torch.empty(int(lib.femasr_packed_weight_floats(o, i, kh, kw)), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_repack_oihw(None, _lib.ptr(w_oihw), o, i, kh, kw, _lib.ptr(wd)))
    packed['w'] = wd
    if form == 'direct' and L['up2'] and i % 32 == 0:
        t = torch.empty(int(lib.femasr_up2_weight_floats(o, i)), dtype=torch.float32, device='cuda')
        _lib.check(lib.femasr_repack_oihw_up2(None, _lib.ptr(w_oihw), o, i, _lib.ptr(t)))
        packed['w_up2'] = t
    if form == 'wino4':
        t = torch.empty(int(lib.femasr_wino_weight_floats(o, i)), dtype=torch.float32, device='cuda')
        _lib.check(lib.femasr_repack_oihw_wino(None, _lib.ptr(w_oihw), o, i, _lib.ptr(t)))
        packed['w_wino'] = t
    if form == 'wino_up2':
        t = torch.empty(int(lib.femasr_wino_up2_weight_floats(o, i)), dtype=torch.float32, device='cuda')
        _lib.check(lib.femasr_repack_oihw_wino_up2(None, _lib.ptr(w_oihw), o, i, _lib.ptr(t)))
        packed['w_wino'] = t
    if form == 'split1x1':
        t = torch.empty(int(lib.femasr_packed_weight_bf16s_bytes(o, i)), dtype=torch.uint8, device='cuda')
        _lib.check(lib.femasr_repack_k1_bf16s(None, _lib.ptr(w_oihw.reshape(o, i)), o, i, _lib.ptr(t)))
        packed['w_bf16s'] = t
    if form == 'bf16x3':
        t = torch.empty(int(lib.femasr_packed_weight_bf16x3_bytes(o, i, kh, kw)), dtype=torch.uint8, device='cuda')
        _lib.check(lib.femasr_repack_oihw_bf16x3(None, _lib.ptr(w_oihw), o, i, kh, kw, _lib.ptr(t)))
        packed['w_bf16x3'] = t
    if form == 'split3x3':
        t = torch.empty(int(lib.femasr_packed_weight_conv3x3_bf16s_bytes(o, i)), dtype=torch.uint8, device='cuda')
        _lib.check(lib.femasr_repack_oihw_bf16s(None, _lib.ptr(w_oihw), o, i, _lib.ptr(t)))
        packed['w_bf16s'] = t
    return packed


def _gn_ab(x, seed):
    """GroupNorm(32) coefficients of x with network-like affine parameters (fp64 moments): a, b (B, C) float32."""
    c = x.shape[-1]
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = rng.uniform(-0.3, 0.3, c).astype(np.float32)
    a, b, _, _ = R.gn_coeffs_ref(x, gamma, beta)
    return a.to(torch.float32).numpy(), b.to(torch.float32).numpy()


def conv_case_bytes(case):
    """Device memory one conv case needs: its tensors, the finite / equality masks and the fp64 moments of the GroupNorm references."""
    L = case['L']
    a = _conv_args(L, case['form'], case['fast'])
    nin, nout = L['B'] * L['H'] * L['W'] * L['cin'], L['B'] * a.Ho * a.Wo * L['cout']
    fp32 = nin * (1 + (1 if (L['pro'] and case['form'] == 'split3x3') else 0) + (1 if L['in_add'] else 0)) + nout * (2 + L['nres'])
    per = lambda n: n // L['B'] if (L['B'] > 1 and n > 2 ** 28) else n          # (gn_coeffs_ref goes image by image on large tensors)
    fp64 = max(3 * per(nin) if L['pro'] else 0, 3 * per(nout) if L['gn_out'] else 0)
    return 4 * fp32 + 8 * fp64 + (1 << 28)


def require_memory(need, what):
    """Prints the case's need; skips only when the device reports less free memory than that."""
    import pytest
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    print(f'{what}: needs {need / 2 ** 30:.2f} GiB, {free / 2 ** 30:.1f} GiB free')
    if free < need:
        pytest.skip(f'{what}: needs {need / 2 ** 30:.2f} GiB of device memory, {free / 2 ** 30:.2f} GiB free')


def run_conv_case(case, seed, wrap=False, batch_check=False):
    """Launch one conv case at its network shape and check it against fp64; returns the worst err / bound.
    wrap: structured positions also on the images in which a 32-bit byte offset into any tensor of the case wraps, and on the image
    after (fp64_ref.straddle_images).  batch_check (B > 1): the same instantiation launched at B = 1 on views of image 0, the last
    and each straddling image - input, residuals, per-sample GroupNorm coefficients - must give out[n] and gn_part[n] bit for bit
    (per-sample independence and the fixed summation order: a store that wrapped into an unsampled part of another image shows)."""
    lib = _lib.load()
    L, form, fast = case['L'], case['form'], case['fast']
    B, H, W, cin, cout = L['B'], L['H'], L['W'], L['cin'], L['cout']
    g = _gen(seed)
    # input: raw activations with a per-channel offset / scale where a GroupNorm prologue normalises them, N(0,1) otherwise
    x = torch.randn((B, H, W, cin), generator=g, device='cuda')
    if L['pro']:
        x = x * (0.5 + torch.rand(cin, generator=g, device='cuda')) + (torch.rand(cin, generator=g, device='cuda') - 0.5)
    K = L['ksz'] * L['ksz'] * cin
    w = torch.randn((cout, cin, L['ksz'], L['ksz']), generator=g, device='cuda') * (1.0 / math.sqrt(K))
    bias = (torch.rand(cout, generator=g, device='cuda') - 0.5) * 0.2
    a = _conv_args(L, form, fast)
    ho, wo = a.Ho, a.Wo
    res = [torch.randn((B, ho, wo, cout), generator=g, device='cuda') for _ in range(L['nres'])]
    in_add = torch.randn((B, H, W, cin), generator=g, device='cuda') if (form == 'wino_up2' and L['in_add']) else None
    pro = _gn_ab(x, seed) if L['pro'] else None
    packed = _pack(form, L, w)
    out = torch.full((B, ho, wo, cout), float('nan'), dtype=torch.float32, device='cuda')
    keep = [x, w, bias, out, in_add] + res + list(packed.values())
    xin = x
    if pro is not None and form == 'split3x3':     # the split 3x3 form takes plain rows: the network's GN + SiLU pass in front
        pa, pb = torch.from_numpy(pro[0]).cuda(), torch.from_numpy(pro[1]).cuda()
        xin = torch.full_like(x, float('nan'))
        _lib.check(lib.femasr_gn_silu_apply(None, _lib.ptr(x), B, H, W, cin, _lib.ptr(pa), _lib.ptr(pb), _lib.ptr(xin)))
        keep += [pa, pb, xin]
    elif pro is not None:
        pa, pb = torch.from_numpy(pro[0]).cuda(), torch.from_numpy(pro[1]).cuda()
        a.pro_a, a.pro_b = pa.data_ptr(), pb.data_ptr()
        keep += [pa, pb]
    a.in_ = xin.data_ptr()
    a.w = packed['w'].data_ptr()
    a.bias = bias.data_ptr()
    a.out = out.data_ptr()
    a.res1 = res[0].data_ptr() if len(res) >= 1 else None
    a.res2 = res[1].data_ptr() if len(res) >= 2 else None
    a.w_up2 = packed['w_up2'].data_ptr() if 'w_up2' in packed else None
    a.w_wino = packed['w_wino'].data_ptr() if 'w_wino' in packed else None
    a.w_bf16s = packed['w_bf16s'].data_ptr() if 'w_bf16s' in packed else None
    a.w_bf16x3 = packed['w_bf16x3'].data_ptr() if 'w_bf16x3' in packed else None
    a.in_add = in_add.data_ptr() if in_add is not None else None
    tiles = _gn_tiles(form, a) if L['gn_out'] else 0
    part = None
    if tiles:
        part = torch.full((B, tiles, 32, 2), float('nan'), dtype=torch.float64, device='cuda')
        a.gn_part = part.data_ptr()
    assert _slot(a) == case['slot'], (_slot(a), case['slot'])
    _lib.check(lib.femasr_conv2d(None, ctypes.byref(a)))
    torch.cuda.synchronize()
    what = f"{case['slot']} B{B} {H}x{W} {cin}->{cout} k{L['ksz']}s{L['stride']}{' up2' if L['up2'] else ''} ({L['key']})"
    assert bool(torch.isfinite(out).all()), f'{what}: NaN sentinel left or non-finite output'
    images = set()
    if wrap:
        for t in [x, out, in_add] + res:
            if t is not None and t.numel() * 4 > 2 ** 31:
                images |= set(R.straddle_images(B, t[0].numel() * 4))
    pos = R.conv_positions(B, ho, wo, seed, tiles_y=(8, 16), tiles_x=(16,), images=images)
    ref, mag, pro_t, rest = R.conv_ref(x, w.cpu().numpy(), bias.cpu().numpy(), pos, L['ksz'], L['stride'], L['pad'], L['up2'],
                                       pro=pro, fast_act=fast or form == 'bf16x3', in_add=in_add, res=res, act=L['act'])
    p = torch.as_tensor(pos, device='cuda')
    got = out[p[:, 0], p[:, 1], p[:, 2]].cpu()
    # the fp32 GEMM kernels: the generic implicit GEMM of a Cin % 32 != 0 layer (in_conv) and the LDS-DMA GEMM of the 1x1 layers
    cform = 'gemm_fp32' if (form == 'direct' and (L['cin'] % 32 or R.gemm_fp32_layer(L))) else form
    worst = R.check(got, ref, R.conv_bound(mag, pro_t, rest, cform), what)
    _note(case['slot'], worst)
    if part is not None:        # fused GroupNorm partials -> coefficients, against fp64 moments of the kernel's own output
        rng = np.random.default_rng(seed + 1)
        gamma = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        beta = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
        ga, gb = G_coeffs_from_partials(part, ho, wo, cout, gamma, beta)
        ra, rb, ba, bb = R.gn_coeffs_ref(out, gamma, beta)
        _note('gn_coeffs_from_partials', R.check(ga, ra, ba, what + ' gn a'))
        _note('gn_coeffs_from_partials', R.check(gb, rb, bb, what + ' gn b'))
    if batch_check and B > 1:
        L1 = dict(L, B=1)
        for n in sorted({0, B - 1} | images):
            a1 = _conv_args(L1, form, fast)
            out1 = torch.full((1, ho, wo, cout), float('nan'), dtype=torch.float32, device='cuda')
            a1.in_, a1.w, a1.bias, a1.out = xin[n].data_ptr(), a.w, a.bias, out1.data_ptr()
            a1.w_up2, a1.w_wino, a1.w_bf16s, a1.w_bf16x3 = a.w_up2, a.w_wino, a.w_bf16s, a.w_bf16x3
            a1.res1 = res[0][n].data_ptr() if len(res) >= 1 else None
            a1.res2 = res[1][n].data_ptr() if len(res) >= 2 else None
            a1.in_add = in_add[n].data_ptr() if in_add is not None else None
            if a.prologue:
                a1.pro_a, a1.pro_b = pa[n].data_ptr(), pb[n].data_ptr()
            part1 = None
            if part is not None:
                part1 = torch.full((1, tiles, 32, 2), float('nan'), dtype=torch.float64, device='cuda')
                a1.gn_part = part1.data_ptr()
            _lib.check(lib.femasr_conv2d(None, ctypes.byref(a1)))
            torch.cuda.synchronize()
            names = f"batched {case['slot']}, single {_slot(a1)}"
            assert torch.equal(out1[0], out[n]), f'{what}: image {n} of the batched launch differs from its own B = 1 launch ({names})'
            assert part1 is None or torch.equal(part1[0], part[n]), f'{what}: gn_part of image {n} differs from its B = 1 launch ({names})'
            del out1, part1
    del keep
    return worst


def G_coeffs_from_partials(part, h, w, c, gamma, beta):
    lib = _lib.load()
    b, tiles = part.shape[0], part.shape[1]
    tg, tb = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    a = torch.full((b, c), float('nan'), dtype=torch.float32, device='cuda')
    bb = torch.full((b, c), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_gn_coeffs_from_partials(None, _lib.ptr(part), b, tiles, h, w, c, 32, _lib.ptr(tg), _lib.ptr(tb), 1e-6,
                                                  _lib.ptr(a), _lib.ptr(bb)))
    torch.cuda.synchronize()
    return a.cpu(), bb.cpu()


# ---------------------------------------------------------------- small kernels
def run_small_case(L, seed):
    lib = _lib.load()
    g = _gen(seed)
    kind = L['kind']
    if kind == 'gn':
        B, H, W, C = L['B'], L['H'], L['W'], L['c']
        x = torch.randn((B, H, W, C), generator=g, device='cuda') * 2.0 + (torch.rand(C, generator=g, device='cuda') - 0.5)
        rng = np.random.default_rng(seed)
        gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.3, 0.3, C).astype(np.float32)
        tg, tb = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        a = torch.full((B, C), float('nan'), device='cuda')
        b = torch.full((B, C), float('nan'), device='cuda')
        scratch = torch.empty(int(lib.femasr_gn_scratch_bytes(B, H, W, C, 32)), dtype=torch.uint8, device='cuda')
        _lib.check(lib.femasr_gn_coeffs(None, _lib.ptr(x), B, H, W, C, 32, _lib.ptr(tg), _lib.ptr(tb), 1e-6, _lib.ptr(a), _lib.ptr(b),
                                        _lib.ptr(scratch)))
        torch.cuda.synchronize()
        ra, rb, ba, bb = R.gn_coeffs_ref(x, gamma, beta)
        what = f'gn_coeffs B{B} {H}x{W}x{C}'
        _note('gn_coeffs', R.check(a.cpu(), ra, ba, what + ' a'))
        _note('gn_coeffs', R.check(b.cpu(), rb, bb, what + ' b'))
        return 'gn_moments'
    if kind == 'ln':
        rows, C = L['rows'], L['c']
        x = torch.randn((rows, C), generator=g, device='cuda') * 1.5 + 0.3
        rng = np.random.default_rng(seed)
        gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.3, 0.3, C).astype(np.float32)
        tg, tb = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
        y = torch.full((rows, C), float('nan'), device='cuda')
        _lib.check(lib.femasr_layernorm(None, _lib.ptr(x), rows, C, _lib.ptr(tg), _lib.ptr(tb), 1e-5, _lib.ptr(y)))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()), f'layernorm rows {rows}: NaN sentinel left'
        rr = np.unique(np.concatenate([R.axis_samples(rows, (64, 128, 256), rng=rng, nrand=256)]))
        ref, bnd = R.layernorm_ref(x[torch.as_tensor(rr, device='cuda')].to('cpu', torch.float64), gamma, beta)
        _note('layernorm', R.check(y[torch.as_tensor(rr, device='cuda')].cpu(), ref, bnd, f'layernorm rows {rows}'))
        return 'layernorm'
    if kind == 'attn':
        B, H, W, C, shift = L['B'], L['H'], L['W'], L['c'], L['shift']
        qkv = torch.randn((B * H * W, 3 * C), generator=g, device='cuda')
        table = (np.random.default_rng(seed).standard_normal((225, 8)) * 0.5).astype(np.float32)
        tt = torch.from_numpy(table).cuda()
        out = torch.full((B * H * W, C), float('nan'), device='cuda')
        _lib.check(lib.femasr_window_attention(None, _lib.ptr(qkv), B, H, W, C, 8, shift, _lib.ptr(tt), _lib.ptr(out)))
        torch.cuda.synchronize()
        what = f'window_attention B{B} {H}x{W} shift {shift}'
        assert bool(torch.isfinite(out).all()), f'{what}: NaN sentinel left'
        rows, ref, bnd = R.attention_ref(qkv, B, H, W, C, 8, shift, table, R.attention_windows(B, H, W, 8, seed))
        _note('window_attention', R.check(out[torch.as_tensor(rows, device='cuda')].cpu(), ref, bnd, what))
        return 'window_attention'
    if kind == 'vq':
        M, D = L['M'], L['d']
        cb = synth.synth_tensor(seed, L['key'], (1024, D), 'trained').astype(np.float32)
        tcb = torch.from_numpy(cb).cuda()
        j = torch.randint(0, 1024, (M,), generator=g, device='cuda')
        z = tcb[j] + 0.5 * tcb.std() * torch.randn((M, D), generator=g, device='cuda')
        cbt = torch.empty(int(lib.femasr_packed_weight_floats(1024, D, 1, 1)), dtype=torch.float32, device='cuda')
        ee = torch.empty((1024,), dtype=torch.float32, device='cuda')
        _lib.check(lib.femasr_repack_oihw(None, _lib.ptr(tcb), 1024, D, 1, 1, _lib.ptr(cbt)))
        _lib.check(lib.femasr_row_sqsum(None, _lib.ptr(tcb), 1024, D, _lib.ptr(ee)))
        scratch = torch.empty(int(lib.femasr_vq_scratch_bytes(M, 1024)), dtype=torch.uint8, device='cuda')
        rows = R.vq_rows(z, cb, seed)
        for mode in ('twopass', 'gemm'):
            idx = torch.full((M,), -1, dtype=torch.int64, device='cuda')
            zq = torch.full((M, D), float('nan'), device='cuda')
            if mode == 'gemm':
                _lib.check(lib.femasr_vq(None, _lib.ptr(z), M, D, _lib.ptr(tcb), _lib.ptr(cbt), _lib.ptr(ee), 1024, _lib.ptr(idx),
                                         _lib.ptr(zq), _lib.ptr(scratch)))
            else:
                assert lib.femasr_vq_twopass_ok(1024, D)
                aux = torch.empty(int(lib.femasr_vq_aux_bytes(1024, D)), dtype=torch.uint8, device='cuda')
                _lib.check(lib.femasr_vq_prepare(None, _lib.ptr(tcb), _lib.ptr(ee), 1024, D, _lib.ptr(aux)))
                _lib.check(lib.femasr_vq_twopass(None, _lib.ptr(z), M, D, _lib.ptr(tcb), _lib.ptr(aux), _lib.ptr(ee), 1024,
                                                 _lib.ptr(idx), _lib.ptr(zq), _lib.ptr(scratch)))
            torch.cuda.synchronize()
            what = f'vq {mode} M {M}'
            assert bool(((idx >= 0) & (idx < 1024)).all()) and bool(torch.isfinite(zq).all()), f'{what}: sentinel left'
            R.vq_check(z, cb, idx, zq, rows, what)
            # every row's zq is its codebook row (whole tensor, on the GPU)
            assert torch.equal(zq, tcb[idx]), f'{what}: zq differs from the chosen rows'
            if mode == 'twopass':        # the gather kernel (decode_indices) at the same M: exact rows
                gq = torch.full((M, D), float('nan'), device='cuda')
                _lib.check(lib.femasr_codebook_gather(None, _lib.ptr(idx), M, D, _lib.ptr(tcb), 1024, _lib.ptr(gq)))
                torch.cuda.synchronize()
                assert torch.equal(gq, zq), f'codebook_gather M {M}'
        return 'vq(codebook lookup)'
    if kind == 'pad':
        B, Hp, Wp, hi, wi = L['B'], L['Hp'], L['Wp'], L['h_in'], L['w_in']
        x = torch.rand((B, 3, hi, wi), generator=g, device='cuda')
        out = torch.full((B, Hp, Wp, 3), float('nan'), device='cuda')
        _lib.check(lib.femasr_pad_nchw_to_nhwc(None, _lib.ptr(x), B, 3, hi, wi, Hp, Wp, _lib.ptr(out)))
        torch.cuda.synchronize()
        # test()'s mirror pad: cat([x, flip(x)])[:, :, :Hp] along each axis (femasr_arch.py:459-460)
        xe = torch.cat([x, x.flip(2)], 2)[:, :, :Hp]
        xe = torch.cat([xe, xe.flip(3)], 3)[:, :, :, :Wp]
        assert torch.equal(out, xe.permute(0, 2, 3, 1)), f'pad B{B} {hi}x{wi}->{Hp}x{Wp}'
        return 'pad/crop/gather layout'
    if kind == 'crop':
        B, H, W, C = L['B'], L['H'], L['W'], L['c']
        x = torch.randn((B, H, W, C), generator=g, device='cuda')
        hc, wc = H - 3, W - 5
        out = torch.full((B, C, hc, wc), float('nan'), device='cuda')
        _lib.check(lib.femasr_crop_nhwc_to_nchw(None, _lib.ptr(x), B, H, W, C, hc, wc, _lib.ptr(out)))
        torch.cuda.synchronize()
        assert torch.equal(out, x[:, :hc, :wc].permute(0, 3, 1, 2)), f'crop B{B} {H}x{W}'
        return 'pad/crop/gather layout'
    raise AssertionError(kind)

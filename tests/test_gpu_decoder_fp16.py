"""-m gpu: decoder_math='fp16' - the one-pass fp16 halo convs behind the codebook lookup (csrc/kernels_conv_f16.hip).

Kernel cases run through femasr_conv2d with w_f16 and are held against tests/fp16_ref.py's restatement of the specification with its
per-element bound (C_F16 = 128; tests/test_decoder_fp16_host.py exercises that checker on the CPU first).  Every instantiation of the
variant table runs; the last test asserts that from the variant names and prints the worst err / bound per instantiation, the module's
run time and its peak device memory (-s).

Network cases hold the mode's contract: VQ indices bit-identical to 'fp32', the image within 2 x E of the 'fp32' image - E the CPU
emulation's max abs on the same case (one rounding of both operands to fp16, float64 accumulation); bf16 grade sits above 2 E
(host test) -, the same launches as 'bf16x3' with the slot names mapped, and bit identity within the mode across graph replay, streams,
`out=`, mode switches, weight reloads, the uint8 tile path and the CLI.
"""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import fp16_ref as F
import fp64_ref as R
from anchor_cases import G_coeffs_from_partials, _gen, _gn_ab, _slot
from femasr_amd import _lib

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()


def _pack_f16(w_oihw):
    lib = _lib.load()
    o, i = w_oihw.shape[:2]
    t = torch.empty(int(lib.femasr_packed_weight_f16_bytes(o, i, 3, 3)), dtype=torch.uint8, device='cuda')
    _lib.check(lib.femasr_repack_oihw_f16(None, _lib.ptr(w_oihw), o, i, 3, 3, _lib.ptr(t)))
    return t


def _args(x, wf, bias, out, up2=False, pro=None, res=(), part=None):
    B, H, W, cin = x.shape
    a = _lib.ConvArgs()
    a.in_, a.B, a.H, a.W, a.Cin = x.data_ptr(), B, H, W, cin
    a.bias, a.Cout, a.ksz, a.stride, a.pad, a.up2 = bias.data_ptr(), out.shape[-1], 3, 1, 1, int(up2)
    a.out, a.Ho, a.Wo = out.data_ptr(), out.shape[1], out.shape[2]
    a.w_f16 = wf.data_ptr()
    if pro is not None:
        a.prologue, a.pro_a, a.pro_b = 1, pro[0].data_ptr(), pro[1].data_ptr()
    a.res1 = res[0].data_ptr() if len(res) >= 1 else None
    a.res2 = res[1].data_ptr() if len(res) >= 2 else None
    a.gn_part = part.data_ptr() if part is not None else None
    return a


def _launch(a):
    _lib.check(_lib.load().femasr_conv2d(None, ctypes.byref(a)))
    torch.cuda.synchronize()


def run_case(seed, B, H, W, cin, cout, up2=False, pro=False, nres=0, gn=False, x=None, w=None):
    """One launch, every output element against the specification.  Returns (out, slot)."""
    g = _gen(seed)
    if x is None:
        x = torch.randn((B, H, W, cin), generator=g, device='cuda')
        if pro:
            x = x * (0.5 + torch.rand(cin, generator=g, device='cuda')) + (torch.rand(cin, generator=g, device='cuda') - 0.5)
    if w is None:
        w = torch.randn((cout, cin, 3, 3), generator=g, device='cuda') * (1.0 / math.sqrt(9 * cin))
    bias = (torch.rand(cout, generator=g, device='cuda') - 0.5) * 0.2
    ho, wo = (2 * H, 2 * W) if up2 else (H, W)
    res = [torch.randn((B, ho, wo, cout), generator=g, device='cuda') for _ in range(nres)]
    ab = _gn_ab(x, seed) if pro else None                       # per-sample coefficients (B, C)
    abt = None if ab is None else (torch.from_numpy(ab[0]).cuda(), torch.from_numpy(ab[1]).cuda())
    wf = _pack_f16(w)
    out = torch.full((B, ho, wo, cout), float('nan'), device='cuda')
    tiles = ((ho + 7) // 8) * ((wo + 15) // 16)
    part = torch.full((B, tiles, 32, 2), float('nan'), dtype=torch.float64, device='cuda') if gn else None
    a = _args(x, wf, bias, out, up2, abt, res, part)
    slot = _slot(a)
    assert slot.startswith('conv3x3_halo_f16<'), slot
    _launch(a)
    what = f'{slot} B{B} {H}x{W} {cin}->{cout}{" up2" if up2 else ""}{" pro" if pro else ""} nres {nres}'
    assert bool(torch.isfinite(out).all()), f'{what}: NaN sentinel left or non-finite output'
    pos = F.all_positions(B, ho, wo)
    ref, mag, near, rest = F.conv_ref(x, w.cpu().numpy(), bias.cpu().numpy(), pos, up2=up2, pro=ab, res=res)
    worst = R.check(out.reshape(len(pos), cout).cpu(), ref, F.conv_bound(mag, near, rest), what)
    WORST[slot] = max(WORST.get(slot, 0.0), worst)
    print(f'{what}: worst err/bound {worst:.3g}')
    if gn:          # fused partials -> coefficients, against fp64 moments of the kernel's own output, within C_GN
        rng = np.random.default_rng(seed + 1)
        gamma, beta = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.uniform(-0.3, 0.3, cout).astype(np.float32)
        ga, gb = G_coeffs_from_partials(part, ho, wo, cout, gamma, beta)
        ra, rb, ba, bb = R.gn_coeffs_ref(out, gamma, beta)
        R.check(ga, ra, ba, what + ' gn a')
        R.check(gb, rb, bb, what + ' gn b')
        import gpu_utils as G                                  # and == the stand-alone moments kernel's coefficients within the same bound
        sa, sb = G.gn_coeffs(out.cpu().numpy(), gamma, beta)
        R.check(torch.from_numpy(sa), ra, ba, what + ' stand-alone gn a')
        assert bool(((ga.double() - torch.from_numpy(sa).double()).abs() <= 2 * ba).all()) and \
            bool(((gb.double() - torch.from_numpy(sb).double()).abs() <= 2 * bb).all())
    return out, slot


# (cin, cout, pro, up2, nres, gn): every tiling class x {none, GN+SiLU, x2}, Cin 32 / 64 / 96 / 512, 0 / 1 / 2 residuals, fused partials,
# and Cout = 48 (not a multiple of its 64-wide block: the second 32-column tile is half empty)
KERNEL_CASES = [
    (32, 32, False, False, 0, True), (64, 32, True, False, 1, True), (96, 32, False, True, 0, False),
    (64, 64, False, False, 2, False), (96, 64, True, False, 0, True), (32, 64, False, True, 1, True),
    (96, 128, False, False, 1, True), (64, 128, True, False, 2, True), (64, 128, False, True, 0, True),
    (512, 256, False, False, 0, True), (64, 256, True, False, 1, True), (96, 256, False, True, 2, False),
    (64, 48, True, False, 1, False), (32, 48, False, False, 0, False),
]


@pytest.mark.parametrize('case', KERNEL_CASES, ids=[f'{c[0]}to{c[1]}{"_pro" if c[2] else ""}{"_up2" if c[3] else ""}_res{c[4]}{"_gn" if c[5] else ""}' for c in KERNEL_CASES])
def test_kernel_against_the_specification(cuda_device, case):
    cin, cout, pro, up2, nres, gn = case
    seed = 100 + KERNEL_CASES.index(case)
    if up2:
        run_case(seed, 2, 7, 11, cin, cout, up2=True, nres=nres, gn=gn)           # 7x11 -> 14x22: two tiles each way, both ragged
        run_case(seed + 50, 2, 4, 8, cin, cout, up2=True, nres=nres, gn=gn)       # -> 8x16: exactly one tile
    else:
        run_case(seed, 2, 13, 21, cin, cout, pro=pro, nres=nres, gn=gn)
        run_case(seed + 50, 2, 8, 16, cin, cout, pro=pro, nres=nres, gn=gn)


# ---------------------------------------------------------------- the frame the fp16 and bf16x3 kernels share (csrc/halo_mma.h), exactly
EXACT_SHAPES = [(13, 21, False), (8, 16, False), (7, 11, True), (4, 8, True)]       # two ragged tiles each way / exactly one tile, plain and x2


def _int_conv_ref(x, w, up2):
    """int64 3x3 pad-1 convolution (nearest x2 first if up2) of integer arrays x (B, H, W, Cin) and w (Cout, Cin, 3, 3): (B, Ho, Wo, Cout)."""
    if up2:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, W, w.shape[0]), np.int64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].T
    return out


@pytest.mark.parametrize('cout', [32, 48, 64, 128, 256, 3])
def test_both_forms_are_exact_on_small_integers(cuda_device, cout):
    """Integer inputs and weights in [-2, 2], integer bias and residuals in [-8, 8], Cin = 64: every operand is exact in fp16 and in bf16
    (the bf16x3 lo terms are zero) and every partial sum is an integer below 2^24, so BOTH matrix-core halo forms must return the int64
    convolution exactly - block decode, patch addressing, masks, residual and bias passes, both store paths (Cout = 3 takes the scalar
    one) - and their fused GroupNorm partials, computed by the same code from identical accumulators, must agree bit for bit."""
    lib = _lib.load()
    rng = np.random.default_rng(1000 + cout)
    cin = 64
    w = rng.integers(-2, 3, (cout, cin, 3, 3))
    bias = rng.integers(-8, 9, cout)
    wt, bt = torch.from_numpy(w.astype(np.float32)).cuda(), torch.from_numpy(bias.astype(np.float32)).cuda()
    wb = torch.empty(int(lib.femasr_packed_weight_bf16x3_bytes(cout, cin, 3, 3)), dtype=torch.uint8, device='cuda')
    _lib.check(lib.femasr_repack_oihw_bf16x3(None, _lib.ptr(wt), cout, cin, 3, 3, _lib.ptr(wb)))
    images = {'f16': _pack_f16(wt), 'bf16x3': wb}
    gn = cout // 32 in (1, 2, 4, 8) and cout % 32 == 0
    for H, W, up2 in EXACT_SHAPES:
        x = rng.integers(-2, 3, (2, H, W, cin))
        ho, wo = (2 * H, 2 * W) if up2 else (H, W)
        res = [rng.integers(-8, 9, (2, ho, wo, cout)) for _ in range(2)]
        conv = _int_conv_ref(x, w, up2)
        # before anything is launched: no partial sum of any accumulation order leaves the integers fp32 holds exactly
        assert int((_int_conv_ref(np.abs(x), np.abs(w), up2) + np.abs(bias) + np.abs(res[0]) + np.abs(res[1])).max()) < 2 ** 24
        xt = torch.from_numpy(x.astype(np.float32)).cuda()
        rt = [torch.from_numpy(r.astype(np.float32)).cuda() for r in res]
        tiles = ((ho + 7) // 8) * ((wo + 15) // 16)
        for nres in (0, 1, 2):
            ref = conv + bias + sum(res[:nres])
            parts = {}
            for form, image in images.items():
                out = torch.full((2, ho, wo, cout), float('nan'), device='cuda')
                part = torch.full((2, tiles, 32, 2), float('nan'), dtype=torch.float64, device='cuda') if gn else None
                a = _args(xt, image, bt, out, up2, None, rt[:nres], part)
                if form == 'bf16x3':
                    a.w_f16, a.w_bf16x3 = None, image.data_ptr()
                slot = _slot(a)
                assert slot.startswith(f'conv3x3_halo_{form}<'), slot
                _launch(a)
                what = f'{slot} {H}x{W}{" up2" if up2 else ""} ->{cout} nres {nres}'
                assert np.array_equal(out.cpu().numpy().astype(np.float64), ref.astype(np.float64)), what
                if gn:
                    assert bool(torch.isfinite(part).all()), what
                    parts[form] = part
            if gn:
                assert torch.equal(parts['f16'], parts['bf16x3']), f'GroupNorm partials differ between the forms: {H}x{W} up2={up2} ->{cout} nres {nres}'


def test_subnormal_weights_take_part_with_their_value(cuda_device):
    """Every weight an fp16 SUBNORMAL, |w| in [2^-24, 2^-15], inputs N(0,1) * 64 so the sums are far above the fp32 accumulation's noise:
    the specification says they multiply with their value.  A flush to zero would give bias exactly."""
    g = _gen(7)
    cin, cout = 64, 64
    mag = torch.exp2(-24.0 + 9.0 * torch.rand((cout, cin, 3, 3), generator=g, device='cuda'))
    w = mag * (torch.randint(0, 2, mag.shape, generator=g, device='cuda') * 2.0 - 1.0)
    x = torch.randn((2, 13, 21, cin), generator=g, device='cuda') * 64.0
    h = w.cpu().numpy().astype(np.float16)
    assert bool(((np.abs(h) < 2.0 ** -14) & (h != 0)).mean() > 0.99)
    out, _ = run_case(7, 2, 13, 21, cin, cout, x=x, w=w)
    assert float((out - out.mean((0, 1, 2))).abs().max()) > 1e-4          # the products are there (a flushed run is constant per channel)


def test_inputs_beyond_the_fp16_range_are_clamped(cuda_device):
    g = _gen(8)
    x = torch.randn((2, 13, 21, 64), generator=g, device='cuda')
    idx = torch.randint(0, x.numel(), (64,), generator=g, device='cuda')
    x.view(-1)[idx[:32]] = 1e5
    x.view(-1)[idx[32:]] = -1e5
    out, _ = run_case(8, 2, 13, 21, 64, 128, x=x)          # finite, and == the model with +-65504 (fp16_ref.fp16_rne clamps)
    assert float(out.abs().max()) > 100.0                  # the clamped values did take part


def test_batch_independence(cuda_device):
    g = _gen(9)
    x = torch.randn((3, 13, 21, 64), generator=g, device='cuda') * (0.5 + torch.rand(64, generator=g, device='cuda'))
    w = torch.randn((128, 64, 3, 3), generator=g, device='cuda') / 24.0
    bias = torch.rand(128, generator=g, device='cuda')
    res = [torch.randn((3, 13, 21, 128), generator=g, device='cuda')]
    ab = _gn_ab(x, 9)
    pa, pb = torch.from_numpy(ab[0]).cuda(), torch.from_numpy(ab[1]).cuda()
    wf = _pack_f16(w)
    out3 = torch.full((3, 13, 21, 128), float('nan'), device='cuda')
    part3 = torch.full((3, 4, 32, 2), float('nan'), dtype=torch.float64, device='cuda')
    _launch(_args(x, wf, bias, out3, False, (pa, pb), res, part3))
    out1 = torch.full((1, 13, 21, 128), float('nan'), device='cuda')
    part1 = torch.full((1, 4, 32, 2), float('nan'), dtype=torch.float64, device='cuda')
    _launch(_args(x[1:2], wf, bias, out1, False, (pa[1:2], pb[1:2]), [res[0][1:2]], part1))
    assert torch.equal(out1[0], out3[1]) and torch.equal(part1[0], part3[1])


def test_refusals(cuda_device):
    lib = _lib.load()
    z = torch.zeros(1 << 16, device='cuda')
    out = torch.full((1, 8, 16, 64), float('nan'), device='cuda')
    a = _args(torch.zeros((1, 8, 16, 48), device='cuda'), z, z, out)          # Cin % 32 != 0: outside the shape rule
    assert lib.femasr_conv2d(None, ctypes.byref(a)) == -1 and b'w_f16' in lib.femasr_last_error()
    assert bool(torch.isnan(out).all())
    assert int(lib.femasr_packed_weight_f16_bytes(64, 48, 3, 3)) == 0
    assert int(lib.femasr_packed_weight_f16_bytes(48, 64, 3, 3)) == 18 * 2 * 2048


# ---------------------------------------------------------------- network
NET_CASES = ['x4_small_trained', 'x2_small_trained', 'hq_small_trained']
_NETS = {}


def _net_case(name):
    if name not in _NETS:
        import gpu_utils as G
        from femasr_amd import synth
        from helpers import cfg_name_of, load_golden, synth_weights
        g = load_golden(name)
        cn = cfg_name_of(g)
        w = synth_weights(cn, int(g['seed']), str(g['codebook']))
        x = torch.from_numpy(synth.synth_input(int(g['input_seed']), tuple(g['in_shape']))).cuda()
        _NETS[name] = (cn, w, x, G.build_net(cn, w, decoder_math='fp32'))
    return _NETS[name]


def _run_net(net, cn, x):
    if cn == 'hq':
        o = net(x)
        return o[0], o[3][0]
    return net.test_with_indices(x)


def _profiled(net, cn, x):
    net.enable_profile(True)
    _run_net(net, cn, x)
    torch.cuda.synchronize()
    prof = {s: v[1] for s, v in net.profile().items() if v[1] > 0}
    net.enable_profile(False)
    return prof


@pytest.mark.parametrize('name', NET_CASES)
def test_network_contract(cuda_device, name):
    cn, w, x, net = _net_case(name)
    net.decoder_math, net.num_streams, net.use_graph = 'fp32', 1, False
    y32, i32 = _run_net(net, cn, x)
    net.decoder_math = 'fp16'
    y16, i16 = _run_net(net, cn, x)
    assert torch.equal(i16, i32), 'VQ indices differ between fp16 and fp32'
    e = F.emulated_images(name)
    E = float(np.abs(e['fp16'][0] - e[None][0]).max())
    d = float((y16 - y32).abs().max())
    print(f'{name}: fp16 against fp32 max abs {d:.3g} ({F.psnr(y16.cpu().numpy(), y32.cpu().numpy(), 1.0):.1f} dB), CPU emulation E = {E:.3g}, d / E = {d / E:.2f}')
    assert 0.0 < d <= 2.0 * E, (d, E)
    # the same launches as bf16x3, slot names mapped; out_conv's slot as it was
    p16 = _profiled(net, cn, x)
    net.decoder_math = 'bf16x3'
    pb = _profiled(net, cn, x)
    f16 = {s: n for s, n in p16.items() if s.startswith('conv3x3_halo_f16<')}
    b16 = {s: n for s, n in pb.items() if s.startswith('conv3x3_halo_bf16x3<')}
    assert f16 and sum(f16.values()) == sum(b16.values())

    def cls(s):             # (block-width class, prologue, up2): the tilings inside a class differ between the two kernels
        body = s[s.index('<') + 1:]
        bn = int(body.split(',')[0].split('x')[2])
        return (bn, 'GN_SILU' in body, 'up2=true' in body)
    agg16, aggb = {}, {}
    for s, n in f16.items():
        agg16[cls(s)] = agg16.get(cls(s), 0) + n
    for s, n in b16.items():
        aggb[cls(s)] = aggb.get(cls(s), 0) + n
    assert agg16 == aggb, (agg16, aggb)
    rest16 = {s: n for s, n in p16.items() if s not in f16}
    restb = {s: n for s, n in pb.items() if s not in b16}
    assert rest16 == restb, (rest16, restb)                  # out_conv and everything in front of the lookup: the same slots
    # back to fp32: the first call's bits
    net.decoder_math = 'fp32'
    y32b, i32b = _run_net(net, cn, x)
    assert torch.equal(y32b, y32) and torch.equal(i32b, i32)


def test_bit_identity_within_the_mode(cuda_device):
    cn, w, x, net = _net_case('x4_small_trained')
    net.decoder_math, net.num_streams, net.use_graph = 'fp16', 1, False
    xb = torch.cat([x, x.flip(-1), x.flip(-2)])               # B = 3: three sub-batches at three streams
    y = net.test(xb)
    assert not torch.equal(y[0], y[1])
    net.num_streams = 3
    assert torch.equal(net.test(xb), y)
    net.num_streams = 1
    net.use_graph = True
    assert torch.equal(net.test(xb), y) and torch.equal(net.test(xb), y)          # capture, then replay
    net.use_graph = False
    buf = torch.full((5,) + tuple(y.shape[1:]), -7.0, device='cuda')
    r = net.test(xb, out=buf[1:4])
    assert r.data_ptr() == buf[1:4].data_ptr() and torch.equal(buf[1:4], y) and float(buf[0].max()) == -7.0 and float(buf[4].min()) == -7.0
    net.decoder_math = 'fp32'


def test_weights_are_repacked_while_in_the_mode(cuda_device):
    import gpu_utils as G
    from helpers import synth_weights
    cn, w, x, _ = _net_case('x4_small_trained')
    w2 = synth_weights('x4', 23, 'trained')
    net = G.build_net('x4', w, decoder_math='fp16')
    y1 = net.test(x)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w2.items()}, strict=False)
    y2 = net.test(x)
    fresh = G.build_net('x4', w2, decoder_math='fp16')
    assert torch.equal(y2, fresh.test(x)) and not torch.equal(y2, y1)
    # ... and the images built on the first selection (from the packed fp32 weights) equal those built by set_weight (from OIHW)
    late = G.build_net('x4', w2, decoder_math='fp32')
    late.test(x)
    late.decoder_math = 'fp16'
    assert torch.equal(late.test(x), y2)


def test_tile_paths_and_cli(cuda_device, tmp_path):
    from PIL import Image
    from femasr_amd import imgproc, inference, synth
    import gpu_utils as G
    from helpers import synth_weights
    net = G.build_net('x4', synth_weights('x4', 1, 'trained'), decoder_math='fp16')
    u8 = (synth.synth_input(11, (1, 3, 40, 56), tag='fp16.png')[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    img = torch.from_numpy(u8).cuda()
    want = imgproc.output_to_u8(net.test_tile(imgproc.u8_to_input(img), 24, 4))
    got = net.test_tile_u8(img, 24, 4)
    assert got.shape == (160, 224, 3) and torch.equal(got, want), int((got != want).sum())
    net.decoder_math = 'fp32'
    assert not torch.equal(net.test_tile_u8(img, 24, 4), got)                    # the mode is really another arithmetic, down to the bytes
    net.decoder_math = 'fp16'
    # blend=True goes through the same forwards: without overlap it is the paste, with overlap every byte stays within the tiles' own spread
    assert torch.equal(net.test_tile_u8(img, 24, 0, blend=True), net.test_tile_u8(img, 24, 0))
    x32 = imgproc.u8_to_input(img)
    assert torch.equal(net.test_tile(x32, 24, 0, blend=True), net.test_tile(x32, 24, 0))
    blend = net.test_tile_u8(img, 24, 4, blend=True)
    assert blend.shape == got.shape and blend.dtype == torch.uint8 and not torch.equal(blend, got)
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    Image.fromarray(u8, 'RGB').save(src / 'fp16.png')
    inference.main(['-i', str(src), '-o', str(dst), '-s', '4', '--synthetic-seed', '1', '--max_size', '30', '--tile_size', '24', '--tile_pad', '4',
                    '--streams', '1', '--decoder-math', 'fp16'])
    assert np.array_equal(np.asarray(Image.open(dst / 'fp16.png').convert('RGB')), want.cpu().numpy())


def test_decode_indices_in_the_mode(cuda_device):
    cn, w, x, net = _net_case('hq_small_trained')
    net.decoder_math = 'fp32'
    idx = net(x)[3][0]
    y32 = net.decode_indices(idx)
    net.decoder_math = 'fp16'
    y16 = net.decode_indices(idx)
    E = float(np.abs(F.emulated_images('hq_small_trained')['fp16'][0] - F.emulated_images('hq_small_trained')[None][0]).max())
    d = float((y16 - y32).abs().max())
    assert 0.0 < d <= 2.0 * E, (d, E)
    net.decoder_math = 'fp32'


def test_every_instantiation_ran_and_report(cuda_device):
    names = set()
    a = _lib.ConvArgs()
    a.B, a.H, a.W, a.ksz, a.stride, a.pad, a.w_f16 = 1, 8, 16, 3, 1, 1, 1
    for cout in (32, 64, 128, 256):
        for pro, up2 in ((0, 0), (1, 0), (0, 1)):
            a.Cin, a.Cout, a.prologue, a.up2, a.Ho, a.Wo = 64, cout, pro, up2, 8 << up2, 16 << up2
            names.add(_slot(a))
    assert len(names) == 12                                     # the whole variant table: 4 tilings x {none, GN+SiLU, x2}
    missing = sorted(names - set(WORST))
    assert not missing, f'instantiations that no kernel case ran: {missing}'
    print('\nfp16 conv worst err/bound per instantiation: ' + ', '.join(f'{k}: {v:.3g}' for k, v in sorted(WORST.items())))
    print(f'fp16 module: {time.time() - T0:.1f} s, peak torch.cuda.max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB')

"""-m gpu: linear_math='fp16' - the layers in FRONT of the codebook lookup in one fp16 pass (csrc/kernels_gemm_f16.hip for the 1x1 layers,
the existing fp16 halo kernels for the stride-1 3x3 convs).

Kernel cases run through femasr_conv2d with ksz = 1 and w_f16 from femasr_repack_k1_f16; every output element is held against
tests/fp16_front_ref.py's restatement of the specification with its per-element bound (C = 128; tests/test_linear_fp16_host.py exercises
that checker on the CPU first).  The GELU epilogue is held bit-identical to the oracle's GELU of the same launch without activation.

Network cases hold the mode's contract: the launches the rule names, few flipped tokens and every one a near tie of the reference
arithmetic's own distances, the image within 2 E + D of the fp32 CPU net run with the GPU's own indices, and bit identity within the mode
across graph replay, streams, `out=`, mode switches, weight reloads, the uint8 tile path and the CLI.
"""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import fp16_front_ref as FR
import fp16_ref as F16
import fp64_ref as R
from anchor_cases import _gen, _slot
from femasr_amd import _lib

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()
EPI = ('plain', 'gelu', 'res')            # the three instantiations


def _pack(w):
    lib = _lib.load()
    n, k = w.shape
    t = torch.empty(int(lib.femasr_packed_weight_k1_f16_bytes(n, k)), dtype=torch.uint8, device='cuda')
    _lib.check(lib.femasr_repack_k1_f16(None, _lib.ptr(w), n, k, _lib.ptr(t)))
    return t


def _args(x, wf, bias, out, act=0, res=None):
    B, H, W, cin = x.shape
    a = _lib.ConvArgs()
    a.in_, a.B, a.H, a.W, a.Cin = x.data_ptr(), B, H, W, cin
    a.bias = bias.data_ptr() if bias is not None else None
    a.Cout, a.ksz, a.stride, a.pad, a.up2 = out.shape[-1], 1, 1, 0, 0
    a.out, a.Ho, a.Wo = out.data_ptr(), H, W
    a.w_f16 = wf.data_ptr()
    a.act = act
    a.res1 = res.data_ptr() if res is not None else None
    return a


def _launch(a):
    _lib.check(_lib.load().femasr_conv2d(None, ctypes.byref(a)))
    torch.cuda.synchronize()


def run_case(seed, shape, k, n, epi, with_bias, x=None, w=None):
    """One launch (two for GELU), every output element against the specification.  Returns the output."""
    from oracle import oracle as orc
    g = _gen(seed)
    B, H, W = shape
    if x is None:
        x = torch.randn((B, H, W, k), generator=g, device='cuda') * (0.5 + torch.rand(k, generator=g, device='cuda'))
    if w is None:
        w = torch.randn((n, k), generator=g, device='cuda') / math.sqrt(k)
    bias = (torch.rand(n, generator=g, device='cuda') - 0.5) * 0.2 if with_bias else None
    res = torch.randn((B, H, W, n), generator=g, device='cuda') if epi == 'res' else None
    wf = _pack(w)
    out = torch.full((B, H, W, n), float('nan'), device='cuda')
    a = _args(x, wf, bias, out, act=0, res=res)
    slot = _slot(a)
    assert slot == ('gemm_f16<act=0,nres=1>' if epi == 'res' else 'gemm_f16<act=0,nres=0>'), slot
    _launch(a)
    what = f'{slot} {B}x{H}x{W} rows, K {k}, N {n}, {epi}{", bias" if with_bias else ""}'
    assert bool(torch.isfinite(out).all()), f'{what}: NaN sentinel left or non-finite output'
    rows = B * H * W
    ref, mag, rest = FR.gemm_ref(x.reshape(rows, k), w, bias, None if res is None else res.reshape(rows, n))
    worst = R.check(out.reshape(rows, n).cpu(), ref, FR.gemm_bound(mag, rest), what)
    if epi == 'gelu':           # the same launch with the activation == the oracle's GELU of the launch without it, bit for bit
        outg = torch.full_like(out, float('nan'))
        ag = _args(x, wf, bias, outg, act=1)
        slot = _slot(ag)
        assert slot == 'gemm_f16<act=1,nres=0>', slot
        _launch(ag)
        want = orc.math_eval('gelu', out.cpu().numpy())
        assert np.array_equal(outg.cpu().numpy(), want), f'{what}: GELU epilogue differs from the oracle GELU of the plain launch'
        out = outg
    WORST[slot] = max(WORST.get(slot, 0.0), worst)
    print(f'{what}: worst err/bound {worst:.3g}')
    return out


ROWS = [1, 63, 64, 65, 127, 128, 129, 192, 257]           # 257: two 128-row tiles plus one
KS = [64, 128, 256, 1024]                                 # 64: a single k chunk (the prologue of the pipeline is also its epilogue)
NS = [256, 512, 768, 1024, 1]                             # 1: the smallest the rule admits (scalar stores; 31 padded columns)
CASES = []
for _i, _r in enumerate(ROWS):                            # every row count as (1, 1, rows), K / N / epilogue / bias cycling
    CASES.append(((1, 1, _r), KS[_i % 4], NS[_i % 5], EPI[_i % 3], _i % 2 == 0))
for _e in EPI:                                            # a real (B, H, W)
    CASES.append(((3, 5, 7), 256, 768, _e, True))
for _k in KS:                                             # every K x epilogue x bias
    for _e in EPI:
        for _b in (True, False):
            CASES.append(((1, 1, 129), _k, 256, _e, _b))
for _n in NS + [36, 130, 132]:                            # every N x epilogue (36: one ragged tile, float4 stores; 130: scalar stores, 2 blocks)
    for _e in EPI:
        CASES.append(((1, 1, 65), 128, _n, _e, True))


@pytest.mark.parametrize('case', CASES, ids=[f'{c[0][0]}x{c[0][1]}x{c[0][2]}_K{c[1]}_N{c[2]}_{c[3]}{"_bias" if c[4] else ""}' for c in CASES])
def test_kernel_against_the_specification(cuda_device, case):
    shape, k, n, epi, with_bias = case
    run_case(1000 + CASES.index(case), shape, k, n, epi, with_bias)


@pytest.mark.parametrize('k', [64, 1024])
def test_small_integers_are_exact(cuda_device, k):
    """A and W small integers (exact in fp16), every sum below 2^24: the output is the integer result bit for bit - any fragment-layout or
    K-order error shows outright.  W is asymmetric in (n, k)."""
    g = _gen(31 + k)
    rows, n = 129, 160
    x = torch.randint(-8, 9, (1, 1, rows, k), generator=g, device='cuda').float()
    w = torch.randint(-8, 9, (n, k), generator=g, device='cuda').float()
    w[:, 0] = torch.arange(n, device='cuda').float() % 7 - 3            # (a column that tells the output channels apart)
    bias = torch.randint(-100, 101, (n,), generator=g, device='cuda').float()
    res = torch.randint(-100, 101, (1, 1, rows, n), generator=g, device='cuda').float()
    want = (x.reshape(rows, k).double() @ w.double().t() + bias.double()[None, :]).reshape(1, 1, rows, n)
    assert float(want.abs().max()) + 100 < 2.0 ** 24
    for epi in ('plain', 'res'):
        out = torch.full((1, 1, rows, n), float('nan'), device='cuda')
        _launch(_args(x, _pack(w), bias, out, res=res if epi == 'res' else None))
        assert torch.equal(out.double(), want + (res.double() if epi == 'res' else 0.0)), epi


def _through_identity(vals):
    """The values as inputs of a K = N = 64 layer with the identity as weight: out[m][n] = fp16_rne(clamp(in[m][n])) exactly."""
    x = torch.zeros((1, 1, 2, 64), device='cuda')
    x.view(-1)[:len(vals)] = torch.tensor(vals, device='cuda')
    out = torch.full((1, 1, 2, 64), float('nan'), device='cuda')
    _launch(_args(x, _pack(torch.eye(64, device='cuda')), None, out))
    return out.view(-1)[:len(vals)].cpu().double().tolist()


def test_rounding_midpoints_go_to_even(cuda_device):
    got = _through_identity([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20])
    assert got == [1.0, 1 + 2.0 ** -9, -1.0, -(1 + 2.0 ** -9), 1 + 2.0 ** -10], got      # neither truncation nor rounding away from zero


def test_inputs_beyond_the_fp16_range_are_clamped(cuda_device):
    assert _through_identity([1e5, -1e5, 65504.0, 65519.0, 3e38]) == [65504.0, -65504.0, 65504.0, 65504.0, 65504.0]
    g = _gen(8)                     # ... and inside a real product: finite, within the bound of the model with +-65504
    x = torch.randn((1, 1, 129, 128), generator=g, device='cuda')
    idx = torch.randint(0, x.numel(), (64,), generator=g, device='cuda')
    x.view(-1)[idx[:32]] = 1e5
    x.view(-1)[idx[32:]] = -1e5
    out = run_case(8, (1, 1, 129), 128, 256, 'plain', True, x=x)
    assert float(out.abs().max()) > 100.0                  # the clamped values did take part


def test_subnormal_weights_take_part_with_their_value(cuda_device):
    """Every weight an fp16 SUBNORMAL, |w| in [2^-24, 2^-15], inputs N(0,1) * 64: the specification says they multiply with their value.
    A flush to zero would give the bias exactly."""
    g = _gen(7)
    k, n = 256, 256
    mag = torch.exp2(-24.0 + 9.0 * torch.rand((n, k), generator=g, device='cuda'))
    w = mag * (torch.randint(0, 2, mag.shape, generator=g, device='cuda') * 2.0 - 1.0)
    h = w.cpu().numpy().astype(np.float16)
    assert bool(((np.abs(h) < 2.0 ** -14) & (h != 0)).mean() > 0.99)
    x = torch.randn((1, 1, 129, k), generator=g, device='cuda') * 64.0
    out = run_case(7, (1, 1, 129), k, n, 'plain', True, x=x, w=w)
    assert float((out - out.mean((0, 1, 2))).abs().max()) > 1e-4          # the products are there (a flushed run is constant per channel)


def test_batch_independence(cuda_device):
    g = _gen(9)
    x = torch.randn((3, 5, 7, 256), generator=g, device='cuda')
    w = torch.randn((768, 256), generator=g, device='cuda') / 16.0
    bias = torch.rand(768, generator=g, device='cuda')
    res = torch.randn((3, 5, 7, 768), generator=g, device='cuda')
    wf = _pack(w)
    for act, r in ((0, None), (1, None), (0, res)):
        out3 = torch.full((3, 5, 7, 768), float('nan'), device='cuda')
        _launch(_args(x, wf, bias, out3, act=act, res=r))
        out1 = torch.full((1, 5, 7, 768), float('nan'), device='cuda')
        _launch(_args(x[1:2], wf, bias, out1, act=act, res=None if r is None else r[1:2]))
        assert torch.equal(out1[0], out3[1])


def test_refusals(cuda_device):
    lib = _lib.load()
    z = torch.zeros(1 << 16, device='cuda')
    out = torch.full((1, 1, 8, 64), float('nan'), device='cuda')
    a = _args(torch.zeros((1, 1, 8, 96), device='cuda'), z, z, out)           # Cin % 64 != 0: outside the k1 shape rule
    assert lib.femasr_conv2d(None, ctypes.byref(a)) == -1 and b'w_f16' in lib.femasr_last_error()
    a = _args(torch.zeros((1, 1, 8, 64), device='cuda'), z, z, out, act=1, res=z)      # GELU with a residual: not one of the three epilogues
    assert lib.femasr_conv2d(None, ctypes.byref(a)) == -1 and b'three epilogues' in lib.femasr_last_error()
    a = _args(torch.zeros((1, 1, 8, 64), device='cuda'), z, z, out, res=z)
    a.res2 = z.data_ptr()                                                       # two residuals
    assert lib.femasr_conv2d(None, ctypes.byref(a)) == -1
    assert bool(torch.isnan(out).all())
    assert int(lib.femasr_packed_weight_k1_f16_bytes(64, 96)) == 0
    assert int(lib.femasr_packed_weight_k1_f16_bytes(48, 128)) == 8 * 2 * 1024


# ---------------------------------------------------------------- network
NET_CASES = ['x4_small_trained', 'x2_small_trained', 'hq_small_trained']
_NETS = {}


def _net_case(name):
    if name not in _NETS:
        import gpu_utils as G
        cn, w, x, _ = FR.golden_case(name)
        _NETS[name] = (cn, w, torch.from_numpy(x).cuda(), G.build_net(cn, w, decoder_math='fp32'))
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


def _reset(net):
    net.decoder_math, net.linear_math, net.num_streams, net.use_graph = 'fp32', 'bf16_split', 1, False


@pytest.mark.parametrize('name', NET_CASES)
def test_network_launches(cuda_device, name):
    cn, w, x, net = _net_case(name)
    _reset(net)
    before = _profiled(net, cn, x)
    assert not any(s.startswith(('gemm_f16<', 'conv3x3_halo_f16<')) for s in before)
    net.linear_math = 'fp16'
    p16 = _profiled(net, cn, x)
    lq = cn != 'hq'
    depth = {'x4': 1, 'x2': 2, 'hq': 3}[cn]                  # stride-2 stages of the encoder
    gemm = {s: n for s, n in p16.items() if s.startswith('gemm_f16<')}
    conv = {s: n for s, n in p16.items() if s.startswith('conv3x3_halo_f16<')}
    # the layers the rule names: 4 RSTB x 6 blocks x (qkv | fc1 | proj, fc2) and before_quant; 2 ResBlocks x 2 convs per stage and the 4 RSTB tail convs
    want_gemm = {'gemm_f16<act=0,nres=0>': (24 if lq else 0) + 1}
    if lq:
        want_gemm.update({'gemm_f16<act=1,nres=0>': 24, 'gemm_f16<act=0,nres=1>': 48})
    assert gemm == want_gemm, gemm
    assert sum(conv.values()) == 4 * depth + (4 if lq else 0), conv
    assert sum(n for s, n in conv.items() if 'FEMASR_PRO_GN_SILU' in s) == 4 * depth       # the ResBlock convs carry their GN + SiLU prologue
    assert not any(s.startswith('gemm_bf16s<') for s in p16), p16
    split3 = {s: n for s, n in p16.items() if s.startswith('conv3x3_bf16s<')}
    assert sum(split3.values()) == depth and all('nres=0' in s for s in split3), split3     # only the stride-2 convs are left on the split GEMM
    assert p16['gn_moments'] < before['gn_moments']          # the stand-alone apply / moments passes around the ResBlock convs are gone
    net.linear_math = 'bf16_split'
    assert _profiled(net, cn, x) == before


def _tag(idx):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(idx).tobytes()).hexdigest()


@pytest.mark.parametrize('name', NET_CASES)
def test_network_indices_and_image(cuda_device, name):
    cn, w, x, net = _net_case(name)
    _reset(net)
    ys, i_s = _run_net(net, cn, x)
    net.linear_math = 'fp16'
    y16, i16 = _run_net(net, cn, x)
    ref, emu = FR.emulated(name, None), FR.emulated(name, 'fp16')
    tokens = i_s.numel()
    delta = FR.token_delta(emu['z0'], ref['z0'])
    flips, bad = FR.near_tie_failures(i_s.cpu().numpy(), i16.cpu().numpy(), ref['d0'], FR.codebook0(name), delta)
    print(f'{name}: {flips} of {tokens} tokens flipped against bf16_split (emulation: {int((emu["idx"] != ref["idx"]).sum())}), Delta {delta:.3g}')
    assert flips <= FR.FLIP_CAP * tokens, (flips, tokens)
    assert not bad, bad
    # the image, with the GPU's own indices forced into the CPU nets
    D = float(np.abs(ys.cpu().numpy() - ref['y']).max())
    for dm in ('fp32', 'fp16'):
        net.decoder_math = dm
        y, idx = _run_net(net, cn, x)
        assert torch.equal(idx, i16)                          # decoder_math cannot move an index
        forced = idx.cpu().numpy()
        dop = 'fp16' if dm == 'fp16' else None
        y32f = FR.emulated(name, None, forced=forced, tag=_tag(forced))['y']
        yemf = FR.emulated(name, 'fp16', forced=forced, decoder_operand=dop, tag=_tag(forced))['y']
        E = float(np.abs(yemf - y32f).max())
        d = float(np.abs(y.cpu().numpy() - y32f).max())
        print(f'{name} decoder_math={dm}: max|gpu - fp32 forced| {d:.3g} ({F16.psnr(y.cpu().numpy(), y32f, 1.0):.1f} dB), E {E:.3g}, D {D:.3g}, d / (2E + D) = {d / (2 * E + D):.2f}')
        assert 0.0 < d <= 2.0 * E + D, (d, E, D)
    _reset(net)
    yb, ib = _run_net(net, cn, x)
    assert torch.equal(yb, ys) and torch.equal(ib, i_s)      # bf16_split -> fp16 -> bf16_split: the first run's bits


def test_bit_identity_within_the_mode(cuda_device):
    cn, w, x, net = _net_case('x4_small_trained')
    _reset(net)
    net.linear_math = 'fp16'
    xb = torch.cat([x, x.flip(-1), x.flip(-2)])               # B = 3: three sub-batches at three streams
    y, idx = net.test_with_indices(xb)
    y1, idx1 = net.test_with_indices(xb[1:2])
    assert torch.equal(y1[0], y[1]) and torch.equal(idx1[0], idx[1]) and not torch.equal(y[0], y[1])      # batch independence
    net.num_streams = 3
    y3, idx3 = net.test_with_indices(xb)
    assert torch.equal(y3, y) and torch.equal(idx3, idx)
    net.num_streams = 1
    net.use_graph = True
    for _ in range(2):                                        # capture, then replay
        yg, idxg = net.test_with_indices(xb)
        assert torch.equal(yg, y) and torch.equal(idxg, idx)
    net.use_graph = False
    buf = torch.full((5,) + tuple(y.shape[1:]), -7.0, device='cuda')
    r = net.test(xb, out=buf[1:4])
    assert r.data_ptr() == buf[1:4].data_ptr() and torch.equal(buf[1:4], y) and float(buf[0].max()) == -7.0 and float(buf[4].min()) == -7.0
    _reset(net)


def test_weights_are_repacked_while_in_the_mode(cuda_device):
    import gpu_utils as G
    from helpers import synth_weights
    cn, w, x, _ = _net_case('x4_small_trained')
    w2 = synth_weights('x4', 23, 'trained')
    for dm in ('fp32', 'fp16'):                               # also with both fp16 modes on: each layer's image is built once, by one of them
        net = G.build_net('x4', w, decoder_math=dm, linear_math='fp16')
        y1, i1 = net.test_with_indices(x)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in w2.items()}, strict=False)
        y2, i2 = net.test_with_indices(x)
        fy, fi = G.build_net('x4', w2, decoder_math=dm, linear_math='fp16').test_with_indices(x)
        assert torch.equal(y2, fy) and torch.equal(i2, fi) and not torch.equal(y2, y1)
        # ... and the images built on the first selection (from the packed fp32 weights) equal those built by set_weight (from the torch tensors)
        late = G.build_net('x4', w2, decoder_math='fp32', linear_math='bf16_split')
        late.test(x)
        late.decoder_math, late.linear_math = dm, 'fp16'
        ly, li = late.test_with_indices(x)
        assert torch.equal(ly, y2) and torch.equal(li, i2)


def test_tile_paths_and_cli(cuda_device, tmp_path):
    from PIL import Image
    from femasr_amd import imgproc, inference, synth
    import gpu_utils as G
    from helpers import synth_weights
    net = G.build_net('x4', synth_weights('x4', 1, 'trained'), decoder_math='fp16', linear_math='fp16')
    u8 = (synth.synth_input(11, (1, 3, 40, 56), tag='half.png')[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    img = torch.from_numpy(u8).cuda()
    want = imgproc.output_to_u8(net.test_tile(imgproc.u8_to_input(img), 24, 4))
    got = net.test_tile_u8(img, 24, 4)
    assert got.shape == (160, 224, 3) and torch.equal(got, want), int((got != want).sum())
    whole = net.test_u8(img)
    net.linear_math = 'bf16_split'
    assert not torch.equal(net.test_u8(img), whole)           # the mode is really another arithmetic, down to the bytes
    src = tmp_path / 'in'
    src.mkdir()
    Image.fromarray(u8, 'RGB').save(src / 'half.png')
    common = ['-i', str(src), '-s', '4', '--synthetic-seed', '1', '--streams', '1']
    inference.main(common + ['-o', str(tmp_path / 'whole'), '--half'])
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'whole' / 'half.png').convert('RGB')), whole.cpu().numpy())
    inference.main(common + ['-o', str(tmp_path / 'tiled'), '--max_size', '30', '--tile_size', '24', '--tile_pad', '4', '--half'])
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'tiled' / 'half.png').convert('RGB')), want.cpu().numpy())


def test_two_codebook_network_runs_in_the_mode(cuda_device):
    from femasr_amd.archs import build_network
    _, w, x, cfg = FR.golden_case('x4mc_small_trained')
    net = build_network(dict(type='FeMaSRNet', **cfg))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    net = net.cuda().eval()
    xt = torch.from_numpy(x).cuda()
    ys, idxs = net.test_with_all_indices(xt)
    net.linear_math = 'fp16'
    y16, idx16 = net.test_with_all_indices(xt)
    assert bool(torch.isfinite(y16).all()) and len(idx16) == len(idxs) == 2
    for q, (a, b) in enumerate(zip(idxs, idx16)):
        flips = int((a != b).sum())
        print(f'x4mc_small_trained lookup {q}: {flips} of {a.numel()} tokens flipped')
        assert flips <= FR.FLIP_CAP * a.numel()
    assert not torch.equal(y16, ys)


def test_every_instantiation_ran_and_report(cuda_device):
    assert set(WORST) == {'gemm_f16<act=0,nres=0>', 'gemm_f16<act=1,nres=0>', 'gemm_f16<act=0,nres=1>'}, sorted(WORST)
    print('\nfp16 GEMM worst err/bound per instantiation: ' + ', '.join(f'{k}: {v:.3g}' for k, v in sorted(WORST.items())))
    print(f'linear fp16 module: {time.time() - T0:.1f} s, peak torch.cuda.max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB')

"""LPIPS on the GPU: the ReLU conv epilogue bit for bit against the oracle, the tap / finalize units, the whole metric against the fp64
restatement (tests/lpips_ref.py), the schedule pinned as a composition of the public units, bitwise properties, and the
validation / CLI surfaces."""
import ctypes

import numpy as np
import pytest
import torch
import yaml

import lpips_ref
from femasr_amd import _lib, synth
from femasr_amd import lpips as L

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _state(net, seed=7):
    return {k: torch.from_numpy(v) for k, v in synth.lpips_state(L.expected_shapes(net), seed).items()}


def _module(net, seed=7):
    return L.LPIPS(net, state_dict=_state(net, seed)).cuda()


def _pair(shape, s0=11, s1=12):
    return (torch.from_numpy(synth.synth_input(s0, shape)).cuda(), torch.from_numpy(synth.synth_input(s1, shape)).cuda())


# ---------------------------------------------------------------- conv + ReLU epilogue: bit-identical to oracle.conv2d + ReLU
# (ksz, stride, pad, Cin, Cout, H, W): Cin = 3 -> generic implicit GEMM, 5x5 Cin 64 -> vectorised implicit GEMM, 3x3 Cin % 32 == 0 ->
# halo kernel.  Each shape runs with the small-launch rule off (conv_small = 0: Cout > 64 on the 128-column blocks every full-size image
# takes) and at its default (these small launches: 64-column blocks).
@pytest.fixture
def conv_small(request):
    lib = _lib.load()
    prev = lib.femasr_conv_small_launch_blocks(request.param)
    yield request.param
    lib.femasr_conv_small_launch_blocks(prev)

CONV_SHAPES = [(11, 4, 2, 3, 64, 39, 45), (5, 1, 2, 64, 192, 9, 11), (3, 1, 1, 3, 64, 17, 23), (3, 1, 1, 64, 64, 17, 23),
               (3, 1, 1, 64, 128, 13, 21), (3, 1, 1, 192, 384, 7, 9), (3, 1, 1, 256, 256, 9, 11), (3, 1, 1, 384, 256, 7, 9),
               (3, 1, 1, 512, 512, 9, 7)]


@pytest.mark.parametrize('conv_small', [0, -1], indirect=True, ids=['bn128', 'small_launch_bn64'])
@pytest.mark.parametrize('ksz,stride,pad,cin,cout,h,w', CONV_SHAPES)
def test_conv_relu_bit_identical_to_oracle(cuda_device, conv_small, ksz, stride, pad, cin, cout, h, w):
    import gpu_utils as G
    from oracle import oracle as orc
    rng = np.random.RandomState(ksz * 1000 + cin + cout)
    x = rng.randn(2, h, w, cin).astype(np.float32)
    wt = (rng.randn(ksz, ksz, cin, cout) * np.sqrt(2.0 / (ksz * ksz * cin))).astype(np.float32)
    b = (rng.randn(cout) * 0.1).astype(np.float32)
    ref = orc.conv2d(x, wt, b, ksz, stride, pad)
    ref = np.where(ref > 0, ref, np.float32(0)).astype(np.float32)
    got = G.conv2d(x, wt, b, ksz, stride, pad, act=_lib.ACT_RELU)
    assert (ref == 0).any() and (ref > 0).any()
    assert _bits_equal(got, ref), float(np.abs(got - ref).max())
    assert not np.signbit(got).any()            # ReLU writes +0, never -0


# ---------------------------------------------------------------- tap + finalize units
def _np_pool(f, pool):
    k = 3 if pool == 1 else 2
    b, h, w, c = f.shape
    hp, wp = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if pool == 1 else (h // 2, w // 2)
    out = np.full((b, hp, wp, c), -np.inf, np.float32)
    for ky in range(k):
        for kx in range(k):
            out = np.maximum(out, f[:, ky:ky + 2 * hp:2, kx:kx + 2 * wp:2, :][:, :hp, :wp])
    return out


def _tap(f, wl, pool):
    lib = _lib.load()
    b2, h, w, c = f.shape
    tf, tw = torch.from_numpy(f).cuda(), torch.from_numpy(wl).cuda()
    nb = lib.femasr_lpips_tap_partials(h, w)
    part = torch.full((b2 // 2, nb), float('nan'), dtype=torch.float64, device='cuda')
    pooled = None
    if pool:
        hp, wp = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if pool == 1 else (h // 2, w // 2)
        pooled = torch.full((b2, hp, wp, c), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_lpips_tap(None, _lib.ptr(tf), b2, h, w, c, _lib.ptr(tw), pool, _lib.ptr(pooled), _lib.ptr(part)))
    out = torch.full((b2 // 2,), float('nan'), dtype=torch.float32, device='cuda')
    terms = torch.full((b2 // 2, 1), float('nan'), dtype=torch.float32, device='cuda')
    hw = (ctypes.c_int32 * 2)(h, w)
    _lib.check(lib.femasr_lpips_finalize(None, _lib.ptr(part), b2 // 2, 1, hw, _lib.ptr(out), _lib.ptr(terms)))
    torch.cuda.synchronize()
    return terms.cpu().numpy()[:, 0], out.cpu().numpy(), None if pooled is None else pooled.cpu().numpy()


@pytest.mark.parametrize('c,pool,h,w', [(64, 1, 23, 37), (192, 1, 15, 17), (128, 2, 21, 33), (512, 2, 9, 13), (384, 0, 11, 7),
                                        (256, 0, 70, 41)])
def test_tap_unit(cuda_device, c, pool, h, w):
    rng = np.random.RandomState(c + h)
    b = 3
    f = np.maximum(rng.randn(2 * b, h, w, c), 0).astype(np.float32)
    f[:, 2, 3, :] = 0.0                              # pixels whose features are all zero in both images
    f[0, :, :, :], f[b, :, :, :] = 0.0, 0.0         # pair 0: every pixel all zero
    wl = (rng.rand(c) / c).astype(np.float32)
    terms, out, pooled = _tap(f, wl, pool)
    if pool:
        assert _bits_equal(pooled, _np_pool(f, pool))
    ref = lpips_ref.head(torch.from_numpy(f[:b].astype(np.float64)).permute(0, 3, 1, 2),
                         torch.from_numpy(f[b:].astype(np.float64)).permute(0, 3, 1, 2), wl.astype(np.float64)).numpy()
    assert terms[0] == 0.0 and ref[0] == 0.0
    assert np.all(np.abs(terms - ref) <= 2e-6 * ref + 1e-9), (terms, ref)
    assert _bits_equal(out, terms)


@pytest.mark.parametrize('pool,h,w,pairs', [(1, 2, 9, 1), (1, 9, 2, 1), (1, 1, 1, 1), (2, 1, 8, 1), (0, 4, 4, 65536)])
def test_tap_refuses_bad_shapes_before_launch(cuda_device, pool, h, w, pairs):
    """A map too small for its max-pool (torch's floor gives no output) and more pairs than one launch takes are refused and nothing
    is written.  The feature buffer holds only the first pair's images: nothing may read past it."""
    lib = _lib.load()
    f = torch.ones((2, h, w, 64), dtype=torch.float32, device='cuda')
    wl = torch.ones(64, dtype=torch.float32, device='cuda')
    part = torch.full((4 + lib.femasr_lpips_tap_partials(h, w),), 7.0, dtype=torch.float64, device='cuda')
    pooled = torch.full((2 * 64 * 16,), 7.0, dtype=torch.float32, device='cuda')
    rc = lib.femasr_lpips_tap(None, _lib.ptr(f), 2 * pairs, h, w, 64, _lib.ptr(wl), pool, _lib.ptr(pooled), _lib.ptr(part))
    torch.cuda.synchronize()
    assert rc == -1, rc
    assert torch.all(part == 7.0) and torch.all(pooled == 7.0)


# ---------------------------------------------------------------- the metric against the fp64 restatement
@pytest.mark.parametrize('net,shape', [('alex', (1, 3, 31, 31)), ('alex', (2, 3, 64, 96)), ('alex', (3, 3, 97, 131)),
                                       ('alex', (1, 3, 256, 256)), ('vgg', (1, 3, 16, 16)), ('vgg', (2, 3, 64, 96)),
                                       ('vgg', (3, 3, 97, 131)), ('vgg', (1, 3, 128, 128))])
def test_lpips_matches_fp64_restatement(cuda_device, net, shape):
    m = _module(net)
    x0, x1 = _pair(shape)
    out, terms = m(x0, x1, per_layer=True)
    assert out.shape == (shape[0], 1, 1, 1) and out.dtype == torch.float32
    sd = {k: v.numpy() for k, v in _state(net).items()}
    rtot, rterms = lpips_ref.lpips(sd, net, x0.cpu().numpy(), x1.cpu().numpy())
    np.testing.assert_allclose(out.view(-1).cpu().numpy(), rtot, rtol=1e-4, atol=0)
    np.testing.assert_allclose(terms.cpu().numpy(), rterms, rtol=1e-4, atol=0)
    if shape[0] == 1:
        assert isinstance(m(x0, x1).item(), float)


def _compose(net, m, x0, x1):
    """The forward as a composition of the public units: scale_input, femasr_conv2d (ReLU), femasr_lpips_tap, femasr_lpips_finalize."""
    lib = _lib.load()
    B, _, H, W = x0.shape
    sd = m.state_dict()
    cur = torch.empty((2 * B, H, W, 3), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_lpips_scale_input(None, _lib.ptr(x0), _lib.ptr(x1), B, H, W, _lib.ptr(cur)))
    parts, hws, keep = [], [], []
    for k, i, cin, cout, ksz, stride, pad, tap, pool in L._CONVS[net]:
        w = sd[f'net.slice{k}.{i}.weight'].contiguous()
        packed = torch.empty(int(lib.femasr_packed_weight_floats(cout, cin, ksz, ksz)), dtype=torch.float32, device='cuda')
        _lib.check(lib.femasr_repack_oihw(None, _lib.ptr(w), cout, cin, ksz, ksz, _lib.ptr(packed)))
        bias = sd[f'net.slice{k}.{i}.bias'].contiguous()
        h, wd = cur.shape[1], cur.shape[2]
        ho, wo = (h + 2 * pad - ksz) // stride + 1, (wd + 2 * pad - ksz) // stride + 1
        out = torch.empty((2 * B, ho, wo, cout), dtype=torch.float32, device='cuda')
        a = _lib.ConvArgs()
        a.in_ = cur.data_ptr(); a.B, a.H, a.W, a.Cin = 2 * B, h, wd, cin
        a.w, a.bias = packed.data_ptr(), bias.data_ptr()
        a.Cout, a.ksz, a.stride, a.pad, a.up2, a.prologue, a.act = cout, ksz, stride, pad, 0, 0, _lib.ACT_RELU
        a.out, a.Ho, a.Wo = out.data_ptr(), ho, wo
        _lib.check(lib.femasr_conv2d(None, ctypes.byref(a)))
        keep += [packed, cur]
        cur = out
        if tap:
            t = len(parts)
            part = torch.empty((B, lib.femasr_lpips_tap_partials(ho, wo)), dtype=torch.float64, device='cuda')
            pooled = None
            if pool:
                hp, wp = ((ho - 3) // 2 + 1, (wo - 3) // 2 + 1) if pool == 1 else (ho // 2, wo // 2)
                pooled = torch.empty((2 * B, hp, wp, cout), dtype=torch.float32, device='cuda')
            wl = sd[f'lin{t}.model.1.weight'].contiguous()
            _lib.check(lib.femasr_lpips_tap(None, _lib.ptr(cur), 2 * B, ho, wo, cout, _lib.ptr(wl), pool, _lib.ptr(pooled), _lib.ptr(part)))
            parts.append(part.view(-1))
            hws += [ho, wo]
            keep.append(cur)
            if pool:
                cur = pooled
    allp = torch.cat(parts)
    out = torch.empty(B, dtype=torch.float32, device='cuda')
    terms = torch.empty((B, 5), dtype=torch.float32, device='cuda')
    _lib.check(lib.femasr_lpips_finalize(None, _lib.ptr(allp), B, 5, (ctypes.c_int32 * 10)(*hws), _lib.ptr(out), _lib.ptr(terms)))
    torch.cuda.synchronize()
    return out, terms


@pytest.mark.parametrize('net,shape', [('alex', (2, 3, 67, 95)), ('vgg', (2, 3, 37, 53))])
def test_forward_is_the_composition_of_the_units(cuda_device, net, shape):
    m = _module(net)
    x0, x1 = _pair(shape, 3, 4)
    out, terms = m(x0, x1, per_layer=True)
    cout, cterms = _compose(net, m, x0, x1)
    assert _bits_equal(terms.cpu().numpy(), cterms.cpu().numpy())
    assert _bits_equal(out.view(-1).cpu().numpy(), cout.cpu().numpy())


@pytest.mark.parametrize('net,hw', [('alex', (45, 61)), ('vgg', (33, 41))])
def test_bitwise_properties(cuda_device, net, hw):
    m = _module(net)
    x0, x1 = _pair((5, 3) + hw, 21, 22)
    assert torch.all(m(x0, x0) == 0)
    ab, t_ab = m(x0, x1, per_layer=True)
    ba, t_ba = m(x1, x0, per_layer=True)
    assert _bits_equal(ab.cpu().numpy(), ba.cpu().numpy()) and _bits_equal(t_ab.cpu().numpy(), t_ba.cpu().numpy())
    for i in range(5):          # batch invariance: pair i alone == pair i inside B = 5
        one, t_one = m(x0[i:i + 1], x1[i:i + 1], per_layer=True)
        assert _bits_equal(one.cpu().numpy(), ab[i:i + 1].cpu().numpy()) and _bits_equal(t_one.cpu().numpy(), t_ab[i:i + 1].cpu().numpy())
    again, t_again = m(x0, x1, per_layer=True)
    assert _bits_equal(again.cpu().numpy(), ab.cpu().numpy()) and _bits_equal(t_again.cpu().numpy(), t_ab.cpu().numpy())
    assert torch.all(ab > 0)


@pytest.mark.parametrize('net,hw', [('alex', (30, 64)), ('alex', (64, 30)), ('vgg', (15, 40))])
def test_below_minimum_refused_before_any_launch(cuda_device, net, hw):
    m = _module(net)
    x0, x1 = _pair((1, 3) + hw)
    with pytest.raises(_lib.FemasrError, match=str(L.MIN_SIDE[net])):
        m(x0, x1)
    lib, h = m._native(x0.device)
    out = torch.full((1,), 7.0, device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    rc = lib.femasr_lpips_forward(h, None, _lib.ptr(x0), _lib.ptr(x1), 1, hw[0], hw[1], _lib.ptr(out), None, _lib.ptr(ws), 1 << 20)
    torch.cuda.synchronize()
    assert rc == -1 and out.item() == 7.0
    nbytes = ctypes.c_size_t()
    assert lib.femasr_lpips_workspace_bytes(h, 1, hw[0], hw[1], ctypes.byref(nbytes)) == -1


def test_missing_weight_refused(cuda_device):
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.femasr_lpips_create(0, 0, ctypes.byref(h)))
    try:
        assert lib.femasr_lpips_finalize_weights(h) == -3
        assert b'net.slice1.0.weight' in lib.femasr_last_error()
    finally:
        lib.femasr_lpips_destroy(h)


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_full_size_pair(cuda_device, net):
    m = _module(net)
    x0, x1 = _pair((1, 3, 1356, 2040), 5, 6)
    out, terms = m(x0, x1, per_layer=True)
    t = terms.cpu().numpy()[0]
    tot = np.float32(t[0])
    for k in range(1, 5):
        tot = np.float32(tot + t[k])
    assert np.isfinite(out.item()) and out.item() > 0 and np.all(t > 0)
    assert _bits_equal(np.float32([out.item()]), np.float32([tot]))


# ---------------------------------------------------------------- validation and CLI surfaces
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr, 'RGB').save(path)


@pytest.mark.parametrize('mtype', ['lpips', 'lpips-vgg'])
def test_validation_reports_lpips(cuda_device, tmp_path, mtype):
    from PIL import Image
    from helpers import synth_weights
    from femasr_amd import imgproc
    from femasr_amd.data import _read
    from femasr_amd.test import test_pipeline
    net = L.METRIC_NETS[mtype]
    rng = np.random.RandomState(4)
    lq, gt, vis = tmp_path / 'lq', tmp_path / 'gt', tmp_path / 'vis'
    lq.mkdir(); gt.mkdir()
    for name, (h, w) in (('a.png', (12, 16)), ('b.png', (9, 11))):
        _png(str(lq / name), rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        _png(str(gt / name), rng.randint(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8))
    ckpt = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth_weights('x4', 11, 'trained').items()}}, str(ckpt))
    lp = tmp_path / f'{net}.pth'
    torch.save(_state(net, 9), str(lp))
    opt = dict(name='lp', model_type='FeMaSRModel', scale=4, root_path=str(tmp_path),
               datasets=dict(val=dict(name='tiny', type='PairedImageDataset', dataroot_lq=str(lq), dataroot_gt=str(gt),
                                      io_backend=dict(type='disk'))),
               network_g=dict(type='FeMaSRNet', gt_resolution=256, norm_type='gn', act_type='silu', scale_factor=4,
                              codebook_params=[[32, 1024, 512]], LQ_stage=True),
               path=dict(pretrain_network_g=str(ckpt), strict_load=False, visualization=str(vis)),
               val=dict(save_img=True, suffix='sr', metrics=dict(lp=dict(type=mtype, better='lower', pretrained_model_path=str(lp)),
                                                                 skipped=dict(type=mtype, better='lower'))))
    p = tmp_path / 'opt.yml'
    p.write_text(yaml.safe_dump(opt))
    r = test_pipeline(str(p))['tiny']
    assert r['skipped'] is None
    m = L.LPIPS(net, pretrained_model_path=str(lp)).cuda()
    want = 0.0
    for name in ('a', 'b'):
        sr_u8 = torch.from_numpy(np.asarray(Image.open(str(vis / 'tiny' / f'{name}_sr.png')))).cuda()
        sr = imgproc.u8_to_input(sr_u8)
        g = _read(str(gt / f'{name}.png')).unsqueeze(0).cuda()
        want += m(sr, g).item()
    assert r['lp'] == want / 2


def test_cli_scores_folders(cuda_device, tmp_path, capsys):
    from femasr_amd import imgproc
    from femasr_amd.lpips_folder import main
    rng = np.random.RandomState(8)
    res, gt = tmp_path / 'res', tmp_path / 'gt'
    res.mkdir(); gt.mkdir()
    imgs = {}
    for name, (h, w) in (('x1', (40, 52)), ('x2', (33, 31))):
        g, r = rng.randint(0, 256, (h, w, 3), dtype=np.uint8), rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        _png(str(gt / f'{name}.png'), g)
        _png(str(res / f'{name}_out.png'), r)
        imgs[name] = (g, r)
    lp = tmp_path / 'vgg.pth'
    torch.save({'params': {'module.' + k: v for k, v in _state('vgg', 3).items()}}, str(lp))
    main(['-r', str(res), '-g', str(gt), '-w', str(lp), '--suffix', '_out'])
    lines = capsys.readouterr().out.strip().splitlines()
    m = L.LPIPS('vgg', pretrained_model_path=str(lp)).cuda()
    vals = [m(imgproc.u8_to_input(torch.from_numpy(r).cuda()), imgproc.u8_to_input(torch.from_numpy(g).cuda())).item()
            for g, r in imgs.values()]
    assert len(lines) == 3
    for i, (name, v) in enumerate(zip(imgs, vals)):
        assert lines[i].split()[1] == name and lines[i].endswith(f'LPIPS: {v:.6f}.')
    assert lines[2] == f'Average: LPIPS: {sum(vals) / 2:.6f}'

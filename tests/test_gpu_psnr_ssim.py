"""PSNR / SSIM on the GPU against their definitions (calculate_psnr / calculate_ssim of femasr_amd.models.femasr_model, numpy / scipy on
the host), the bitwise properties of the fixed-order reductions, batch splitting, refusals, and the validation / CLI surfaces."""
import numpy as np
import pytest
import torch
import yaml

from femasr_amd import _lib
from femasr_amd import psnr_ssim as P
from femasr_amd.models import femasr_model as fm

pytestmark = pytest.mark.gpu

PSNR_TOL, SSIM_TOL = 1e-9, 1e-12


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy(), np.float64).view(np.uint64)


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _contents(h, w, seed):
    """{name: (a, b)} uint8 (h, w, 3) pairs: random, smooth bright gradients (the cancellation case), a constant image, saturated 0 / 255
    regions, identical."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = np.arange(3)[None, None, :]

    def ramp(base, sy, sx):
        return base + sy * y[..., None] * (1 + 0.1 * ch) + sx * x[..., None] - 4 * ch
    sat = rng.randint(0, 256, (h, w, 3))
    sat[: h // 2, : w // 2] = 255
    sat[h // 2:, w // 2:] = 0
    sat2 = sat.copy()
    sat2[rng.rand(h, w) < 0.2] = 255
    r = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    return {
        'random': (r, rng.randint(0, 256, (h, w, 3)).astype(np.uint8)),
        'smooth': (_u8(ramp(230, 0.3, 0.2)), _u8(ramp(226, 0.2, 0.35) + rng.randint(0, 2, (h, w, 3)))),
        'constant': (np.full((h, w, 3), 173, np.uint8), _u8(173 + rng.randint(-2, 3, (h, w, 3)))),
        'saturated': (sat.astype(np.uint8), sat2.astype(np.uint8)),
        'identical': (r, r.copy()),
    }


def _cpu(a, b, crop, ty):
    return (fm.calculate_psnr(a, b, crop_border=crop, test_y_channel=ty), fm.calculate_ssim(a, b, crop_border=crop, test_y_channel=ty))


def _cpu_mse_rgb(a, b, crop):
    a, b = a.astype(np.float64), b.astype(np.float64)
    if crop:
        a, b = a[crop:-crop, crop:-crop], b[crop:-crop, crop:-crop]
    return np.mean((a - b) ** 2)


def _check(a, b, crop, ty, p, s, m, what):
    cp, cs = _cpu(a, b, crop, ty)
    if np.isinf(cp):
        assert p == np.inf, (what, p)
    else:
        assert np.isfinite(p) and abs(p - cp) <= PSNR_TOL, (what, p, cp)
    assert abs(s - cs) <= SSIM_TOL, (what, s, cs, s - cs)
    if not ty:      # integer terms: numpy's MSE bit for bit
        cm = _cpu_mse_rgb(a, b, crop)
        assert np.float64(m).view(np.uint64) == np.float64(cm).view(np.uint64), (what, m, cm)


@pytest.mark.parametrize('ty', [True, False], ids=['y', 'rgb'])
@pytest.mark.parametrize('crop', [0, 4])
@pytest.mark.parametrize('size', ['min', (132, 68), (97, 203)])
def test_matches_the_cpu_functions(cuda_device, size, crop, ty):
    h, w = (11 + 2 * crop, 11 + 2 * crop) if size == 'min' else size
    cont = _contents(h, w, seed=h * 1000 + w + crop)
    names = list(cont)
    xa = torch.from_numpy(np.stack([cont[n][0] for n in names])).cuda()
    xb = torch.from_numpy(np.stack([cont[n][1] for n in names])).cuda()
    r = P.psnr_ssim(xa, xb, crop_border=crop, test_y_channel=ty)
    assert r.psnr.dtype == torch.float64 and r.psnr.device == xa.device and r.psnr.shape == (len(names),)
    ps, ss, ms = r.psnr.cpu().numpy(), r.ssim.cpu().numpy(), r.mse.cpu().numpy()
    for i, n in enumerate(names):
        _check(*cont[n], crop, ty, ps[i], ss[i], ms[i], n)
    assert ps[names.index('identical')] == np.inf and ss[names.index('identical')] == 1.0


def test_full_size_pair(cuda_device):
    """One 2040x1356 pair (smooth content with noise: the cancellation case at the validation size), both modes, crop 4."""
    rng = np.random.RandomState(17)
    y, x = np.mgrid[0:1356, 0:2040].astype(np.float64)
    base = 128 + 90 * np.sin(y / 300.0)[..., None] * np.cos(x / 450.0)[..., None] + np.arange(3) * 5
    a, b = _u8(base + rng.uniform(-8, 8, base.shape)), _u8(base + rng.uniform(-8, 8, base.shape))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for ty in (True, False):
        r = P.psnr_ssim(ta, tb, crop_border=4, test_y_channel=ty)
        _check(a, b, 4, ty, r.psnr.item(), r.ssim.item(), r.mse.item(), f'2040x1356 y={ty}')


# ---------------------------------------------------------------- bitwise properties
@pytest.mark.parametrize('ty', [True, False], ids=['y', 'rgb'])
@pytest.mark.parametrize('h,w,crop', [(19, 19, 4), (45, 77, 0), (70, 41, 4)])
def test_bitwise_properties(cuda_device, h, w, crop, ty):
    rng = np.random.RandomState(h + w)
    xa = torch.from_numpy(rng.randint(0, 256, (6, h, w, 3)).astype(np.uint8)).cuda()
    xb = torch.from_numpy(_u8(xa.cpu().numpy() + rng.randint(-20, 21, (6, h, w, 3)))).cuda()
    ab = P.psnr_ssim(xa, xb, crop, ty)
    ba = P.psnr_ssim(xb, xa, crop, ty)
    for u, v in zip(ab, ba):
        assert np.array_equal(_bits(u), _bits(v))                                    # symmetric
    again = P.psnr_ssim(xa, xb, crop, ty)
    for u, v in zip(ab, again):
        assert np.array_equal(_bits(u), _bits(v))                                    # run to run
    for i in range(6):                                                              # batch invariant
        one = P.psnr_ssim(xa[i], xb[i], crop, ty)
        for u, v in zip(ab, one):
            assert np.array_equal(_bits(u[i:i + 1]), _bits(v))
    # one metric alone: the same blocks, the same bits
    assert np.array_equal(_bits(P.psnr(xa, xb, crop, ty)), _bits(ab.psnr))
    assert np.array_equal(_bits(P.ssim(xa, xb, crop, ty)), _bits(ab.ssim))
    same = P.psnr_ssim(xa, xa, crop, ty)
    assert torch.all(same.ssim == 1.0) and torch.all(same.psnr == np.inf) and torch.all(same.mse == 0.0)
    assert torch.all(ab.ssim < 1.0) and torch.all(torch.isfinite(ab.psnr))


def test_batches_beyond_one_call_are_split_into_whole_pairs(cuda_device):
    n = 65535 + 40
    rng = np.random.RandomState(5)
    xa = torch.from_numpy(rng.randint(0, 256, (n, 11, 11, 3)).astype(np.uint8)).cuda()
    xb = torch.from_numpy(rng.randint(0, 256, (n, 11, 11, 3)).astype(np.uint8)).cuda()
    for ty in (True, False):
        big = P.psnr_ssim(xa, xb, 0, ty)
        part = P.psnr_ssim(xa[65500:], xb[65500:], 0, ty)          # straddles the split at 65535
        for u, v in zip(big, part):
            assert u.shape == (n,) and np.array_equal(_bits(u[65500:]), _bits(v))
        for i in (0, 65534, 65535, n - 1):
            _check(xa[i].cpu().numpy(), xb[i].cpu().numpy(), 0, ty, big.psnr[i].item(), big.ssim[i].item(), big.mse[i].item(), i)
    lib = _lib.load()
    out = torch.full((n,), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(1 << 22, dtype=torch.uint8, device='cuda')
    rc = lib.femasr_psnr_ssim(None, _lib.ptr(xa), _lib.ptr(xb), 65536, 11, 11, 0, 1, _lib.ptr(out), None, None, _lib.ptr(ws), 1 << 22)
    torch.cuda.synchronize()
    assert rc == -1 and torch.all(out == 7.0)


@pytest.mark.parametrize('h,w,crop,ssim', [(8, 40, 4, False), (40, 9, 5, False), (20, 40, 5, True), (40, 10, 0, True)])
def test_refused_before_any_launch(cuda_device, h, w, crop, ssim):
    """Shapes the library refuses leave the outputs untouched; the Python API raises."""
    lib = _lib.load()
    a = torch.zeros((2, h, w, 3), dtype=torch.uint8, device='cuda')
    outs = [torch.full((2,), 7.0, dtype=torch.float64, device='cuda') for _ in range(3)]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    ss = _lib.ptr(outs[1]) if ssim else None
    rc = lib.femasr_psnr_ssim(None, _lib.ptr(a), _lib.ptr(a), 2, h, w, crop, 0, _lib.ptr(outs[0]), ss, _lib.ptr(outs[2]), _lib.ptr(ws), 1 << 20)
    torch.cuda.synchronize()
    assert rc == -1 and all(torch.all(o == 7.0) for o in outs)
    with pytest.raises(_lib.FemasrError):
        (P.ssim if ssim else P.psnr)(a, a, crop_border=crop)
    if ssim:        # PSNR alone is defined below the SSIM window
        assert torch.all(P.psnr(a, a, crop_border=crop) == np.inf)


def test_python_refusals(cuda_device):
    a = torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='shapes differ'):
        P.psnr(a, a[:15])
    with pytest.raises(ValueError, match='uint8'):
        P.ssim(a.float(), a.float())
    with pytest.raises(ValueError, match='RGB'):
        P.psnr(a[..., :2], a[..., :2])
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        P.psnr(a, a.cpu())
    with pytest.raises(ValueError, match='one'):
        P.create_metric('psnr')(a[None], a[None])
    m = P.create_metric('ssim', crop_border=2, test_y_channel=True, color_space='ycbcr')
    assert isinstance(m(a, a), float) and m(a, a) == 1.0


# ---------------------------------------------------------------- validation and CLI surfaces
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr, 'RGB').save(path)


def test_validation_scores_on_the_gpu(cuda_device, tmp_path, monkeypatch):
    """The YAML -> validation pipeline with the CPU definitions made to raise: psnr / ssim come from the GPU and agree with the CPU
    functions evaluated on the saved PNGs.  Before the GPU metrics, validation called these functions: this test failed."""
    from PIL import Image
    from helpers import synth_weights
    from femasr_amd.test import test_pipeline
    cpu_psnr, cpu_ssim = fm.calculate_psnr, fm.calculate_ssim

    def boom(*a, **k):
        raise AssertionError('validation scored psnr / ssim on the host')
    for name in ('calculate_psnr', 'calculate_ssim'):
        monkeypatch.setattr(fm, name, boom)
    for key in ('psnr', 'ssim'):
        monkeypatch.setitem(fm._METRICS, key, boom)
    rng = np.random.RandomState(6)
    lq, gt, vis = tmp_path / 'lq', tmp_path / 'gt', tmp_path / 'vis'
    lq.mkdir(); gt.mkdir()
    for name, (h, w) in (('a.png', (12, 16)), ('b.png', (9, 11))):
        _png(str(lq / name), rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        _png(str(gt / name), rng.randint(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8))
    ckpt = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth_weights('x4', 11, 'trained').items()}}, str(ckpt))
    metrics = dict(psnr=dict(type='psnr', crop_border=4, test_y_channel=True),
                   ssim=dict(type='ssim', crop_border=4, test_y_channel=True, better='higher'),
                   psnr_rgb=dict(type='psnr', crop_border=0, color_space='rgb'),
                   ssim_rgb=dict(type='ssim', crop_border=2, test_y_channel=False),
                   niqe=dict(type='niqe', better='lower'))
    opt = dict(name='ps', model_type='FeMaSRModel', scale=4, root_path=str(tmp_path),
               datasets=dict(val=dict(name='tiny', type='PairedImageDataset', dataroot_lq=str(lq), dataroot_gt=str(gt),
                                      io_backend=dict(type='disk'))),
               network_g=dict(type='FeMaSRNet', gt_resolution=256, norm_type='gn', act_type='silu', scale_factor=4,
                              codebook_params=[[32, 1024, 512]], LQ_stage=True),
               path=dict(pretrain_network_g=str(ckpt), strict_load=False, visualization=str(vis)),
               val=dict(save_img=True, suffix='sr', metrics=metrics))
    p = tmp_path / 'opt.yml'
    p.write_text(yaml.safe_dump(opt))
    r = test_pipeline(str(p))['tiny']
    assert r['niqe'] is None
    want = dict.fromkeys(('psnr', 'ssim', 'psnr_rgb', 'ssim_rgb'), 0.0)
    for name in ('a', 'b'):
        sr = np.asarray(Image.open(str(vis / 'tiny' / f'{name}_sr.png')).convert('RGB'))
        g = np.asarray(Image.open(str(gt / f'{name}.png')).convert('RGB'))
        want['psnr'] += cpu_psnr(sr, g, crop_border=4, test_y_channel=True) / 2
        want['ssim'] += cpu_ssim(sr, g, crop_border=4, test_y_channel=True) / 2
        want['psnr_rgb'] += cpu_psnr(sr, g, crop_border=0) / 2
        want['ssim_rgb'] += cpu_ssim(sr, g, crop_border=2) / 2
    for k in ('psnr', 'psnr_rgb'):
        assert abs(r[k] - want[k]) <= PSNR_TOL, (k, r[k], want[k])
    for k in ('ssim', 'ssim_rgb'):
        assert abs(r[k] - want[k]) <= SSIM_TOL, (k, r[k], want[k])


def test_cli_scores_folders(cuda_device, tmp_path, capsys):
    from femasr_amd.psnr_ssim_folder import main
    rng = np.random.RandomState(9)
    gt, res = tmp_path / 'gt', tmp_path / 'res'
    (gt / 'sub').mkdir(parents=True); res.mkdir()
    imgs = {}
    for name, (h, w) in (('p1', (40, 52)), ('sub/p2', (33, 31)), ('p0', (24, 24))):
        g = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        r = _u8(g.astype(np.int32) + rng.randint(-30, 31, (h, w, 3)))
        _png(str(gt / f'{name}.png'), g)
        _png(str(res / f'{name.split("/")[-1]}_x4.png'), r)
        imgs[name.split('/')[-1]] = (g, r)
    order = ['p0', 'p1', 'p2']          # sorted GT paths: gt/p0.png, gt/p1.png, gt/sub/p2.png
    for ty in (False, True):
        argv = ['--gt', str(gt), '--restored', str(res), '--crop_border', '3', '--suffix', '_x4'] + (['--test_y_channel'] if ty else [])
        main(argv)
        lines = capsys.readouterr().out.strip().splitlines()
        assert lines[0] == ('Testing Y channel.' if ty else 'Testing RGB channels.') and len(lines) == 7
        ps, ss = [], []
        for i, name in enumerate(order):
            g, r = imgs[name]
            p, s = fm.calculate_psnr(g, r, crop_border=3, test_y_channel=ty), fm.calculate_ssim(g, r, crop_border=3, test_y_channel=ty)
            ps.append(p)
            ss.append(s)
            assert lines[1 + i] == f'{i + 1:3d}: {name:25}. \tPSNR: {p:.6f} dB, \tSSIM: {s:.6f}'
        assert lines[4:6] == [str(gt), str(res)]
        assert lines[6] == f'Average: PSNR: {sum(ps) / 3:.6f} dB, SSIM: {sum(ss) / 3:.6f}'

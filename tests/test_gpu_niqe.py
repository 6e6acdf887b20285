"""NIQE and imresize on the GPU against their definitions (femasr_amd.models.femasr_model, numpy fp64 on the host): bit-equal planes, equal
alpha grid positions, features to rounding, the score within the bar measured from the definition (tests/niqe_cases.py), batch / layout /
stream invariance, refusals, and the validation / CLI surfaces.  The definition's results are computed once per image and shared."""
import os

import numpy as np
import pytest
import torch
import yaml

import niqe_cases as C
from femasr_amd import _lib
from femasr_amd import niqe as N
from femasr_amd import resize as R
from femasr_amd.models import femasr_model as fm
from test_niqe_host import IMRESIZE_BAR, golden_cases

pytestmark = pytest.mark.gpu

# every sum of a block has at most 9216 fp64 terms: n eps ~ 1e-12 relative, with a margin of 100
FEATURE_TOL = 1e-10
ALPHA_COLS = [18 * s + j for s in (0, 1) for j in (0, 2, 6, 10, 14)]


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _score_close(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), (what, got)
    else:
        print(f'{what}: score {got!r}, definition {want!r}, difference {abs(got - want):.3g} (bar {C.score_bar():.3g})')
        assert abs(got - want) <= C.score_bar(), (what, got, want)


@pytest.mark.parametrize('name', list(C.SHAPES))
def test_matches_the_definition(cuda_device, name):
    img, ref, crop = C.image(name), C.reference(name), C.SHAPES[name][2]
    x = torch.from_numpy(np.array(img)).cuda()
    (feat, pos), planes = N.features(x, C.params(), crop, return_planes=True)
    assert feat.dtype == torch.float64 and feat.device == x.device and feat.shape == (1,) + ref['features'].shape
    assert pos.dtype == torch.int32 and pos.shape == (1,) + ref['positions'].shape
    for key in ('y', 'z', 'y2', 'z2'):                          # the luma, the resized plane and z at both scales: the definition's bits
        assert planes[key].shape == (1,) + ref[key].shape, key
        assert np.array_equal(_bits(planes[key][0]), _bits(ref[key])), key
    assert np.array_equal(pos[0].cpu().numpy(), ref['positions'])
    got, want = feat[0].cpu().numpy(), ref['features']
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print(f'{name}: largest feature error {err.max():.3g} (tolerance {FEATURE_TOL:.3g}), {int((~ok).sum())} NaN features')
    assert err.max() <= FEATURE_TOL
    assert np.array_equal(got[:, ALPHA_COLS], want[:, ALPHA_COLS])      # alphas are grid values: equal positions, equal bits
    score = N.niqe(x, C.params(), crop)
    assert score.shape == (1,) and score.dtype == torch.float64
    _score_close(score.item(), ref['score'], name)


def test_refused_before_any_launch(cuda_device):
    h, w, crop = C.REFUSED
    x = torch.zeros((h, w, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.FemasrError, match='no 96x96 block'):
        N.niqe(x, C.params(), crop)
    with pytest.raises(_lib.FemasrError, match='no 96x96 block'):
        N.features(torch.zeros((2, 103, 300, 3), dtype=torch.uint8, device='cuda'), C.params(), 4)
    with pytest.raises(ValueError, match='uint8'):
        N.niqe(x.float(), C.params())
    with pytest.raises(ValueError, match='RGB'):
        N.niqe(x[..., :2], C.params())
    with pytest.raises(ValueError, match='too short'):
        R.imresize(torch.zeros((2, 40), device='cuda'), 0.25)
    with pytest.raises(ValueError, match='float32 or float64'):
        R.imresize(torch.zeros((8, 8), dtype=torch.float16, device='cuda'), 0.5)


def test_batch_layout_and_stream_do_not_change_a_bit(cuda_device):
    """A batch of three images equals the three single calls bitwise (every sum depends on the block's own pixels only); a non-contiguous
    input and a call on a side stream give the same bits; so does a second run."""
    names = ('four_blocks', 'constant_block', 'tie_pixels')
    imgs = torch.from_numpy(np.stack([C.image(n) for n in names])).cuda()
    p = C.params()
    batch = N.features(imgs, p)
    for i, n in enumerate(names):
        one = N.features(imgs[i], p)
        assert np.array_equal(_bits(batch.features[i]), _bits(one.features[0])), n
        assert torch.equal(batch.positions[i], one.positions[0]), n
        assert np.array_equal(batch.positions[i].cpu().numpy(), C.reference(n)['positions'])
    again = N.features(imgs, p)
    assert np.array_equal(_bits(batch.features), _bits(again.features)) and torch.equal(batch.positions, again.positions)
    wide = torch.zeros((3, 192, 200, 4), dtype=torch.uint8, device='cuda')
    wide[:, :, :192, :3] = imgs
    view = wide[:, :, :192, :3]
    assert not view.is_contiguous()
    strided = N.features(view, p)
    assert np.array_equal(_bits(batch.features), _bits(strided.features)) and torch.equal(batch.positions, strided.positions)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = N.features(imgs, p)
        scores_side = N.niqe(imgs, p)
    side.synchronize()
    assert np.array_equal(_bits(batch.features), _bits(on_side.features)) and torch.equal(batch.positions, on_side.positions)
    scores = N.niqe(imgs, p)
    assert scores.shape == (3,) and np.array_equal(_bits(scores), _bits(scores_side))
    for i, n in enumerate(names):
        _score_close(scores[i].item(), C.reference(n)['score'], n)


def test_imresize_fp64_is_the_definition_bit_for_bit(cuda_device):
    for label, x, scale, aa, _ in golden_cases():
        want = fm.imresize(x.astype(np.float64), scale, aa)
        got = R.imresize(torch.from_numpy(x.astype(np.float64)).cuda(), scale, aa)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape, label
        assert np.array_equal(_bits(got), _bits(want)), label
    x = np.random.RandomState(3).rand(2, 3, 24, 37)              # leading dimensions are planes; a non-contiguous view
    t = torch.from_numpy(x).cuda().transpose(0, 1)
    got = R.imresize(t, 0.7, True)
    assert got.shape == (3, 2, 17, 26) and np.array_equal(_bits(got), _bits(fm.imresize(x.transpose(1, 0, 2, 3), 0.7, True)))


def test_imresize_fp32_is_within_the_host_bar_of_the_reference(cuda_device):
    worst = 0.0
    for label, x, scale, aa, want in golden_cases():
        got = R.imresize(torch.from_numpy(x).cuda(), scale, aa)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape, label
        d = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        worst = max(worst, d)
        assert d <= IMRESIZE_BAR, (label, d)
        assert np.array_equal(got.cpu().numpy(), fm.imresize(x, scale, aa).astype(np.float32)), label       # the definition rounded once
    print(f'float32 imresize against the reference fixture: largest difference {worst:.3g} (bar {IMRESIZE_BAR:.3g})')


# ---------------------------------------------------------------- validation and CLI surfaces
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr, 'RGB').save(path)


def _params_file(tmp_path):
    mu, cov, win = C.params()
    path = str(tmp_path / 'niqe_pris_params.npz')
    np.savez(path, mu_pris_param=mu[None, :], cov_pris_param=cov, gaussian_window=win)
    return path


def test_validation_scores_niqe_without_ground_truth(cuda_device, tmp_path, monkeypatch):
    """The YAML -> validation pipeline on a SingleImageDataset (no GT) with the pixel-level host definitions made to raise: niqe comes from
    the GPU and agrees with the definition evaluated on the saved PNGs.  LQ 24x48, so the x4 output is 96x192: two blocks."""
    from PIL import Image
    from helpers import synth_weights
    from femasr_amd.test import test_pipeline
    cpu_niqe = fm.calculate_niqe
    keep = {k: getattr(fm, k) for k in ('calculate_niqe', 'niqe_features', '_niqe_y', '_convolve_nearest', 'imresize', '_aggd')}

    def boom(*a, **k):
        raise AssertionError('validation scored niqe pixels on the host')
    for name in keep:
        monkeypatch.setattr(fm, name, boom)
    rng = np.random.RandomState(6)
    lq, vis = tmp_path / 'lq', tmp_path / 'vis'
    lq.mkdir()
    for name in ('a.png', 'b.png'):
        _png(str(lq / name), rng.randint(0, 256, (24, 48, 3), dtype=np.uint8))
    ckpt = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth_weights('x4', 11, 'trained').items()}}, str(ckpt))
    metrics = dict(niqe=dict(type='niqe', pretrained_model_path=_params_file(tmp_path), crop_border=0, better='lower'),
                   niqe_nofile=dict(type='niqe', better='lower'))
    opt = dict(name='nq', model_type='FeMaSRModel', scale=4, root_path=str(tmp_path),
               datasets=dict(val=dict(name='real', type='SingleImageDataset', dataroot_lq=str(lq), io_backend=dict(type='disk'))),
               network_g=dict(type='FeMaSRNet', gt_resolution=256, norm_type='gn', act_type='silu', scale_factor=4,
                              codebook_params=[[32, 1024, 512]], LQ_stage=True),
               path=dict(pretrain_network_g=str(ckpt), strict_load=False, visualization=str(vis)),
               val=dict(save_img=True, suffix='sr', metrics=metrics))
    p = tmp_path / 'opt.yml'
    p.write_text(yaml.safe_dump(opt))
    r = test_pipeline(str(p))['real']
    assert r['niqe_nofile'] is None
    for name, fn in keep.items():
        monkeypatch.setattr(fm, name, fn)
    want = 0.0
    for name in ('a', 'b'):
        sr = np.asarray(Image.open(str(vis / 'real' / f'{name}_sr.png')).convert('RGB'))
        assert sr.shape == (96, 192, 3)
        want += cpu_niqe(sr, 0, C.params()) / 2
    print(f'validation niqe {r["niqe"]!r}, definition on the saved PNGs {want!r}')
    assert np.isfinite(want) and abs(r['niqe'] - want) <= C.score_bar()


def test_cli_scores_a_folder(cuda_device, tmp_path, capsys):
    from femasr_amd.niqe_folder import main
    root = tmp_path / 'in'
    (root / 'sub').mkdir(parents=True)
    names = {'p1': C.textured(200, 200, 31), 'sub/p2': np.array(C.image('ragged_crop')), 'p0': C.textured(104, 200, 32)}      # sizes differ
    for fname, img in names.items():
        _png(str(root / f'{fname}.png'), img)
    main(['--input', str(root), '--crop_border', '4', '--params', _params_file(tmp_path)])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 5
    scores = []
    for i, fname in enumerate(('p0', 'p1', 'sub/p2')):            # sorted paths: in/p0.png, in/p1.png, in/sub/p2.png
        want = fm.calculate_niqe(names[fname], 4, C.params())
        assert np.isfinite(want)
        head, val = lines[i].rsplit(' ', 1)
        assert head == f'{i + 1:3d}: {os.path.basename(fname):25}. \tNIQE:'
        assert abs(float(val) - want) <= 1e-6 + C.score_bar()       # six printed decimals
        scores.append(float(val))
    assert lines[3] == str(root)
    assert abs(float(lines[4].replace('Average: NIQE: ', '')) - sum(scores) / 3) <= 1e-6

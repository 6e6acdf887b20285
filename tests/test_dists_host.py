"""DISTS host logic without a GPU: the float64 restatement by two routes, its properties, the weight loader's name mapping, header and
binding, the refusals of the C entries (nothing is launched), the metric split of nondist_validation and the folder pairing."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import torch

import dists_ref as R
from femasr_amd import _lib, synth
from femasr_amd import dists as D
from femasr_amd import dists_folder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_WEIGHT = -1, -3
SHAPES = [(1, 8, 8), (2, 9, 11), (3, 17, 23), (1, 33, 47)]
NEW_SYMBOLS = ['femasr_dists_create', 'femasr_dists_destroy', 'femasr_dists_set_weight', 'femasr_dists_finalize_weights',
               'femasr_dists_workspace_bytes', 'femasr_dists_forward', 'femasr_dists_features', 'femasr_dists_l2pool',
               'femasr_dists_moments_workspace_bytes', 'femasr_dists_moments', 'femasr_dists_moments_input']


def _sd(seed=5):
    return synth.dists_state(seed)


def _pair(b, h, w, s0=11, s1=12):
    return synth.synth_input(s0, (b, 3, h, w)), synth.synth_input(s1, (b, 3, h, w))


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize('b,h,w', SHAPES)
def test_two_routes_agree(b, h, w):
    sd = _sd()
    x, y = _pair(b, h, w)
    st, tt = R.dists(sd, x, y, route='torch')
    sn, tn = R.dists(sd, x, y, route='numpy')
    assert st.shape == (b,) and tt.shape == (b, 6, 2)
    assert np.abs(st - sn).max() <= 1e-12 and np.abs(tt - tn).max() <= 1e-12, (st, sn)
    assert np.all(st > 1e-3) and np.all(st < 1)
    # the single-pass form of the variance (the kernel's) against the definition's two-pass form
    fx, fy = R.features(sd, x), R.features(sd, y)
    s1, _ = R.score_from_maps(fx, fy, sd['alpha'], sd['beta'], R.moments_single_pass)
    assert np.abs(s1 - st).max() <= 1e-12


@pytest.mark.parametrize('b,h,w', SHAPES)
def test_image_against_itself_scores_zero(b, h, w):
    sd = _sd()
    x, _ = _pair(b, h, w)
    for route in ('torch', 'numpy'):
        s, _ = R.dists(sd, x, x, route=route)
        assert np.abs(s).max() <= 1e-12, s


def test_map_shapes_and_stage_magnitudes():
    sd = _sd()
    for b, h, w in SHAPES:
        maps = R.features(sd, _pair(b, h, w)[0])
        assert [(m.shape[2], m.shape[3], m.shape[1]) for m in maps] == D.map_shapes(h, w)
        assert all(0.05 < float(m.abs().max()) < 50 for m in maps[1:])       # the synthetic weights keep every stage O(1)
    assert D.map_shapes(8, 8)[-1] == (1, 1, 512) and D.map_shapes(9, 11)[2] == (5, 6, 128)
    assert D.N_CHANNELS == 1475 == sum(R.CHANNELS)
    with pytest.raises(ValueError, match='8'):
        D.map_shapes(7, 40)


def test_flat_images():
    sd = _sd()
    a = np.full((1, 3, 16, 16), 128 / 255, np.float32)
    c = np.full((1, 3, 16, 16), 200 / 255, np.float32)
    assert abs(R.dists(sd, a, a)[0][0]) <= 1e-12
    assert R.dists(sd, a, c)[0][0] > 0.05


def test_pool_restatements():
    rng = np.random.RandomState(3)
    f = torch.from_numpy(rng.randn(2, 5, 9, 6))
    a, b = R.l2pool_torch(f), R.l2pool_numpy(f)
    assert a.shape == (2, 5, 5, 3) and float((a - b).abs().max()) <= 1e-14
    assert np.allclose(R.HANN, np.outer(np.hanning(5)[1:-1], np.hanning(5)[1:-1]) / np.outer(np.hanning(5)[1:-1], np.hanning(5)[1:-1]).sum())
    # the float32 restatement of the kernel's order: within float32 rounding of the float64 pool, exact on zeros and infinities
    f32 = rng.randn(2, 9, 6, 64).astype(np.float32)
    want = R.l2pool_torch(torch.from_numpy(f32.astype(np.float64)).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    got = R.l2pool_f32(f32)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 4e-7 * np.abs(want).max()
    z = R.l2pool_f32(np.zeros((1, 3, 3, 64), np.float32))
    assert np.all(z == np.sqrt(np.float32(1e-12)))
    big = np.zeros((1, 2, 2, 64), np.float32)
    big[0, 0, 0] = 3e19
    assert np.all(np.isinf(R.l2pool_f32(big)[0, 0, 0])) and not np.isnan(R.l2pool_f32(big)).any()


# ---------------------------------------------------------------- the weight loader
def test_loader_maps_all_layouts_to_the_same_tensors(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in _sd().items()}
    want = D.expected_shapes()
    assert list(sd) == list(want) and all(tuple(sd[k].shape) == want[k] for k in want)
    # 1: one file, the DISTS module's names, nested and prefixed, with the constants of the method to ignore
    one = {'params': {'module.' + k: v for k, v in sd.items()}}
    one['params'].update({'module.mean': torch.zeros(1, 3, 1, 1), 'module.std': torch.ones(1, 3, 1, 1),
                          'module.stage2.4.filter': torch.zeros(64, 1, 3, 3)})
    torch.save(one, str(tmp_path / 'one.pth'))
    # 2: alpha / beta alone + a torchvision backbone (with classifier weights to ignore)
    torch.save({k: sd[k] for k in ('alpha', 'beta')}, str(tmp_path / 'ab.pth'))
    tv = {f'features.{k.split(".")[1]}.{k.split(".")[2]}': v for k, v in sd.items() if k.startswith('stage')}
    tv['classifier.0.weight'] = torch.zeros(4, 4)
    torch.save({'state_dict': tv}, str(tmp_path / 'tv.pth'))
    # 3: the backbone of an LPIPS-VGG file (net.sliceK.I.*; its heads are ignored)
    lp = {f'net.slice{k.split(".")[0][-1]}.{k.split(".")[1]}.{k.split(".")[2]}': v for k, v in sd.items() if k.startswith('stage')}
    lp['lin0.model.1.weight'] = torch.zeros(1, 64, 1, 1)
    torch.save(lp, str(tmp_path / 'lp.pth'))
    got = [D.load_dists_weights(str(tmp_path / 'one.pth')),
           D.load_dists_weights(str(tmp_path / 'ab.pth'), backbone_model_path=str(tmp_path / 'tv.pth')),
           D.load_dists_weights(str(tmp_path / 'ab.pth'), backbone_model_path=str(tmp_path / 'lp.pth'))]
    for g in got:
        assert list(g) == list(want)
        for k in sd:
            assert torch.equal(g[k], sd[k]), k
    m = D.DISTS(pretrained_model_path=str(tmp_path / 'one.pth'))
    assert sorted(m.state_dict()) == sorted(want)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    m2 = D.create_metric('dists', pretrained_model_path=str(tmp_path / 'ab.pth'), backbone_model_path=str(tmp_path / 'tv.pth'), as_loss=False)
    assert torch.equal(m2.alpha, sd['alpha'])


def test_loader_names_missing_and_misshaped_keys():
    sd = {k: torch.from_numpy(v) for k, v in _sd().items()}
    part = {k: v for k, v in sd.items() if k not in ('stage3.12.bias', 'beta')}
    with pytest.raises(KeyError) as e:
        D.canonical_state_dict(part)
    assert 'stage3.12.bias' in str(e.value) and 'beta' in str(e.value) and 'alpha' not in str(e.value).split('accepted')[0]
    bad = dict(sd)
    bad['stage2.5.weight'] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError, match=r'stage2\.5\.weight'):
        D.canonical_state_dict(bad)
    bad = dict(sd)
    bad['alpha'] = torch.zeros(1, 1472, 1, 1)
    with pytest.raises(ValueError, match='alpha'):
        D.canonical_state_dict(bad)


def test_module_refuses_unknown_keywords_and_warns_without_weights():
    with pytest.raises(TypeError):
        D.DISTS(pretrained_model_pth='x.pth')
    with pytest.warns(UserWarning, match='without weights'):
        D.DISTS()
    with pytest.raises(ValueError, match='pretrained_model_path'):
        D.DISTS(backbone_model_path='features.pth')
    with pytest.raises(ValueError, match='pretrained_model_path'):
        D.create_metric('dists')
    with pytest.raises(ValueError, match='unknown'):
        D.create_metric('a-dists', pretrained_model_path='x.pth')
    assert 'NOT verified' in D.__doc__


# ---------------------------------------------------------------- the C interface
def test_new_symbols_declared_bound_and_version_kept():
    assert '#include "femasr_hip_dists.h"' in open(os.path.join(ROOT, 'include', 'femasr_hip.h')).read()
    hdr = open(os.path.join(ROOT, 'include', 'femasr_hip_dists.h')).read()
    assert set(re.findall(r'^(?:int|void)\s+(femasr_[a-z0-9_]+)\s*\(', hdr, re.M)) == set(_lib.DISTS_SIGNATURES) == set(NEW_SYMBOLS)
    ct = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        m = re.search(r'^(int|void)\s+' + name + r'\s*\(([^;]*)\)\s*;', hdr, re.M | re.S)
        assert m, f'{name} is not declared in include/femasr_hip_dists.h'
        want = []
        for arg in m.group(2).replace('\n', ' ').split(','):
            arg = arg.strip()
            if '*' in arg:
                if arg.startswith('size_t *'):
                    want.append(ctypes.POINTER(ctypes.c_size_t))
                elif arg.startswith('const char *'):
                    want.append(ctypes.c_char_p)
                elif arg.startswith('const int64_t *'):
                    want.append(ctypes.POINTER(ctypes.c_int64))
                elif '**' in arg:
                    want.append(ctypes.POINTER(ctypes.c_void_p))
                else:
                    want.append(ctypes.c_void_p)
            else:
                want.append(ct[arg.rsplit(' ', 1)[0].replace('const ', '').strip()])
        res, args = _lib.DISTS_SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == 'int' else None) and list(args) == want, (name, args, want)
        assert list(getattr(lib, name).argtypes) == want
    assert lib.femasr_version() == _lib.ABI_VERSION == 107
    assert not set(_lib.DISTS_SIGNATURES) & set(_lib.SIGNATURES)


def test_the_new_size_queries_size_guarded_regions():
    queries = {n for n in _lib.DISTS_SIGNATURES if n.endswith('_bytes')}
    assert queries == {'femasr_dists_workspace_bytes', 'femasr_dists_moments_workspace_bytes'}
    with open(os.path.join(ROOT, 'tests', 'dists_utils.py')) as fh:
        asked = set(re.findall(r"\bqp\('(femasr_\w+)'", fh.read()))
    assert asked == queries


@pytest.fixture
def handle():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.femasr_dists_create(0, ctypes.byref(h)) == 0          # records the device only: no GPU is touched before set_weight
    yield lib, h
    lib.femasr_dists_destroy(h)


def test_refusals_need_no_gpu(handle):
    """Everything the entries refuse is refused before any launch - so also on a machine without a GPU.  The pointers are made up:
    a call that got past its checks would fault."""
    lib, h = handle
    n = ctypes.c_size_t(0)
    p = ctypes.c_void_p(1 << 20)            # 256-byte aligned
    big = 1 << 40
    assert lib.femasr_dists_create(0, None) == ERR_INVALID and lib.femasr_dists_create(-1, ctypes.byref(ctypes.c_void_p())) == ERR_INVALID
    # the size query: what it takes and what it refuses
    assert lib.femasr_dists_workspace_bytes(h, 1, 8, 8, ctypes.byref(n)) == 0 and n.value % 256 == 0 and n.value > 2 * 2 * 64 * 64 * 4
    assert lib.femasr_dists_workspace_bytes(h, 3, 33, 47, ctypes.byref(n)) == 0
    for b, hh, ww in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 7, 64), (64, 7, 1), (1, 8, 7), (65536, 8, 8), (1, 4096, 4096),
                      (65535, 16, 17), (2, 4096, 2048)]:
        assert lib.femasr_dists_workspace_bytes(h, b, hh, ww, ctypes.byref(n)) == ERR_INVALID, (b, hh, ww)
        assert lib.femasr_dists_forward(h, None, p, p, b, hh, ww, p, big, p, None) == ERR_INVALID, (b, hh, ww)
    assert b'2^31' in lib.femasr_last_error()
    assert lib.femasr_dists_workspace_bytes(h, 1, 4096, 4095, ctypes.byref(n)) == 0            # 2 * 4096 * 4095 * 64 < 2^31
    assert lib.femasr_dists_workspace_bytes(None, 1, 8, 8, ctypes.byref(n)) == ERR_INVALID
    assert lib.femasr_dists_workspace_bytes(h, 1, 8, 8, None) == ERR_INVALID
    # forward / features: null pointers, a short or misaligned workspace, weights that were never finalized
    assert lib.femasr_dists_workspace_bytes(h, 2, 9, 11, ctypes.byref(n)) == 0
    good = (h, None, p, p, 2, 9, 11, p, n.value, p, None)
    for i in (0, 2, 3, 7, 9):
        args = list(good)
        args[i] = None
        assert lib.femasr_dists_forward(*args) == ERR_INVALID, i
        assert lib.femasr_dists_features(*args[:10]) == ERR_INVALID, i
    assert lib.femasr_dists_forward(*good[:8], n.value - 1, p, None) == ERR_INVALID and b'workspace' in lib.femasr_last_error()
    assert lib.femasr_dists_forward(*good[:7], ctypes.c_void_p((1 << 20) + 128), n.value, p, None) == ERR_INVALID
    assert b'aligned' in lib.femasr_last_error()
    assert lib.femasr_dists_forward(*good) == ERR_INVALID and b'not finalized' in lib.femasr_last_error()
    assert lib.femasr_dists_features(*good[:10]) == ERR_INVALID and b'not finalized' in lib.femasr_last_error()
    assert lib.femasr_dists_finalize_weights(h) == ERR_WEIGHT and b'stage1.0.weight' in lib.femasr_last_error()
    assert lib.femasr_dists_finalize_weights(None) == ERR_INVALID
    assert lib.femasr_dists_set_weight(h, b'alpha', None, (ctypes.c_int64 * 4)(1, 1475, 1, 1), 4) == ERR_INVALID


def test_unit_refusals_need_no_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)
    n = ctypes.c_size_t(0)
    for args in [(None, None, 2, 8, 8, 64, p), (None, p, 2, 8, 8, 64, None), (None, p, 0, 8, 8, 64, p), (None, p, 2, 0, 8, 64, p),
                 (None, p, 2, 8, 0, 64, p), (None, p, 2, 8, 8, 3, p), (None, p, 2, 8, 8, 96, p), (None, p, 2, 8, 8, 576, p),
                 (None, p, 2, 4096, 4096, 64, p)]:
        assert lib.femasr_dists_l2pool(*args) == ERR_INVALID, args
    assert lib.femasr_dists_moments_workspace_bytes(1, 1, 1, 64, ctypes.byref(n)) == 0 and n.value == 5 * 64 * 8
    assert lib.femasr_dists_moments_workspace_bytes(1, 8, 8, 3, ctypes.byref(n)) == 0 and n.value == 256
    # the partials grow with the map's side, not with its area: at most 512 runs per pair
    assert lib.femasr_dists_moments_workspace_bytes(1, 1356, 2040, 64, ctypes.byref(n)) == 0 and n.value <= 512 * 5 * 64 * 8
    for b, h, w, c in [(0, 8, 8, 64), (1, 0, 8, 64), (1, 8, 0, 64), (65536, 8, 8, 64), (1, 8, 8, 32), (1, 8, 8, 4)]:
        assert lib.femasr_dists_moments_workspace_bytes(b, h, w, c, ctypes.byref(n)) == ERR_INVALID, (b, h, w, c)
    assert lib.femasr_dists_moments_workspace_bytes(1, 8, 8, 64, None) == ERR_INVALID
    assert lib.femasr_dists_moments_workspace_bytes(2, 17, 23, 128, ctypes.byref(n)) == 0
    good = (None, p, 2, 17, 23, 128, p, n.value, p)
    for i in (1, 6, 8):
        args = list(good)
        args[i] = None
        assert lib.femasr_dists_moments(*args) == ERR_INVALID, i
    for args in [good[:7] + (n.value - 1, p), good[:6] + (ctypes.c_void_p((1 << 20) + 8), n.value, p), good[:5] + (3, p, n.value, p),
                 good[:2] + (0, 17, 23, 128, p, n.value, p), good[:2] + (65536, 1, 1, 64, p, 1 << 40, p),
                 good[:2] + (1, 4096, 4096, 64, p, 1 << 40, p)]:
        assert lib.femasr_dists_moments(*args) == ERR_INVALID, args
    assert lib.femasr_dists_moments_workspace_bytes(2, 17, 23, 3, ctypes.byref(n)) == 0
    goodi = (None, p, p, 2, 17, 23, p, n.value, p)
    for i in (1, 2, 6, 8):
        args = list(goodi)
        args[i] = None
        assert lib.femasr_dists_moments_input(*args) == ERR_INVALID, i
    assert lib.femasr_dists_moments_input(*goodi[:7], n.value - 1, p) == ERR_INVALID
    assert lib.femasr_dists_moments_input(None, p, p, 0, 17, 23, p, n.value, p) == ERR_INVALID


# ---------------------------------------------------------------- validation's metric split and the folder CLI
def test_validation_metric_split(caplog):
    from femasr_amd.models import femasr_model as fm

    class Data(list):
        class dataset:
            opt = {'name': 'none'}
    model = fm.FeMaSRModel.__new__(fm.FeMaSRModel)
    model.opt = {'val': {'metrics': {'d': {'type': 'dists', 'better': 'lower'}, 'musiq': {'type': 'musiq'},
                                     'dw': {'type': 'dists', 'better': 'lower', 'pretrained_model_path': 'dists.pth',
                                            'backbone_model_path': 'vgg.pth'}}}}
    built = []
    model._gpu_metric = lambda name, m: built.append((name, m['type'], m['pretrained_model_path'])) or (lambda a, b: None)
    with caplog.at_level(logging.WARNING, logger='femasr_amd'):
        r = model.nondist_validation(Data(), 0, None, False)
    assert r == {'d': None, 'musiq': None, 'dw': 0.0}          # no image: the selected metric's mean of nothing
    assert built == [('dw', 'dists', 'dists.pth')]
    assert "['d', 'musiq']" in caplog.text and 'DISTS weight file' in caplog.text
    assert 'niqe_pris_params.npz' in caplog.text and 'LPIPS weight file' in caplog.text       # what the warning said before, still
    # the factory behind _gpu_metric
    seen = {}
    orig = fm.dists_metric.create_metric
    fm.dists_metric.create_metric = lambda t, **kw: seen.update(kw, type=t) or 'metric'
    try:
        m2 = fm.FeMaSRModel.__new__(fm.FeMaSRModel)
        m2.device = 'cpu'
        assert m2._gpu_metric('dw', model.opt['val']['metrics']['dw']) == 'metric'
    finally:
        fm.dists_metric.create_metric = orig
    assert seen == dict(type='dists', device='cpu', pretrained_model_path='dists.pth', backbone_model_path='vgg.pth')


def test_folder_pairing(tmp_path):
    res, gt = tmp_path / 'res', tmp_path / 'gt'
    res.mkdir(); gt.mkdir()
    for name in ('b.png', 'a.png', 'c.jpg'):
        open(str(gt / name), 'wb').close()
    got = dists_folder.pair_files(str(res), str(gt), '_out')
    assert [g[0] for g in got] == ['a', 'b', 'c']
    assert [g[1] for g in got] == [str(gt / n) for n in ('a.png', 'b.png', 'c.jpg')]
    assert [g[2] for g in got] == [str(res / n) for n in ('a_out.png', 'b_out.png', 'c_out.jpg')]
    assert dists_folder.pair_files(str(res), str(gt))[0][2] == str(res / 'a.png')
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(SystemExit, match='no images'):
        dists_folder.score_folders(str(res), str(empty), 'unused.pth')
    with pytest.raises(SystemExit) as e:
        dists_folder.main(['-r', str(res), '-g', str(gt)])                  # -w is required
    assert e.value.code == 2

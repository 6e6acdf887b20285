"""NIQE / imresize host logic without a GPU: the fp64 imresize definition against the reference's recorded outputs, the restated 7x7 order
against scipy, the luma expression against exact arithmetic, the AGGD NaN rule, the margin condition on the GPU tests' images, the score
bar those tests use, the C ABI's and Python's refusals (nothing is launched), the folder listing and the skipped metric."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import niqe_cases as C
from femasr_amd import _lib
from femasr_amd import niqe as N
from femasr_amd import niqe_folder as cli
from femasr_amd import resize as R
from femasr_amd.models import femasr_model as fm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'imresize_ref.npz')
# The fp64 definition against the reference's float32 imresize: the largest difference measured on the CPU over the fixture was 2.76e-6
# (48x48 at scale 1.5; the dyadic scales stay below 1.7e-7, the rest is the reference's float32 coordinates), times 4 because that
# rounding varies with the size.  tests/test_gpu_niqe.py holds the float32 GPU path to the same bar.
IMRESIZE_MEASURED = 2.76e-6
IMRESIZE_BAR = 4 * IMRESIZE_MEASURED
FAKE = ctypes.c_void_p(1 << 20)      # a 256-aligned non-null address: every call below must return before touching it


def golden_cases():
    """[(label, input float32, scale, antialiasing, reference output float32)]"""
    with np.load(GOLDEN) as g:
        out = []
        for i, c in enumerate(g['cases']):
            size, si, aa = str(c).split('|')
            out.append((str(c), g['in_' + size], float(g['scales'][int(si)]), bool(int(aa)), g[f'out_{i}']))
    return out


def test_imresize_definition_matches_the_reference_fixture():
    cases = golden_cases()
    assert len(cases) == 52 and {c[0].split('|')[0] for c in cases} == {'5x7', '9x11', '24x37', '48x48'}
    worst = 0.0
    for label, x, scale, aa, want in cases:
        got = fm.imresize(x, scale, aa)
        assert got.shape == want.shape and got.dtype == np.float64, label
        d = float(np.abs(got - want).max())
        print(f'{label}: {d:.3g}')
        worst = max(worst, d)
        assert d <= IMRESIZE_BAR, (label, d)
    print(f'largest difference {worst:.3g} (bar {IMRESIZE_BAR:.3g})')


def test_imresize_refuses_a_length_shorter_than_its_padding():
    with pytest.raises(ValueError, match='too short'):
        fm.imresize(np.zeros((2, 40)), 0.25)               # 8 / 0.25 = 32 taps reflect past 2 rows
    with pytest.raises(ValueError, match='too short'):
        fm.imresize_tables(3, 1, 0.125, True)
    w, idx = fm.imresize_tables(96, 48, 0.5, True)          # NIQE's second scale: 8 taps, reflected at both ends
    assert w.shape == (48, 8) and idx.dtype == np.int32 and idx.min() == 0 and idx.max() == 95
    assert list(idx[0]) == [2, 1, 0, 0, 1, 2, 3, 4] and list(idx[-1]) == [91, 92, 93, 94, 95, 95, 94, 93]


def test_the_restated_7x7_order_is_scipys_bit_for_bit():
    from scipy import ndimage
    rng = np.random.RandomState(0)
    _, _, gauss = C.params()
    asym = rng.rand(7, 7)
    planes = [rng.randint(0, 256, (40, 53)).astype(np.float64), rng.randint(0, 256, (9, 8)).astype(np.float64) ** 2,
              np.full((20, 23), 188.0), np.full((20, 23), 188.0) ** 2]
    for win in (gauss, asym):
        for x in planes:
            got, want = fm._convolve_nearest(x, win), ndimage.convolve(x, win, mode='nearest')
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_luma_expression_rounds_as_exact_arithmetic_except_on_the_194_ties():
    ties = C.tie_triples()
    assert ties.shape == (194, 3)
    assert [tuple(t) for t in ties[:3]] == [(0, 204, 68), (1, 173, 225), (2, 44, 141)]
    tie_set = np.zeros((256, 256, 256), dtype=bool)
    tie_set[ties[:, 0], ties[:, 1], ties[:, 2]] = True
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing='ij')
    for r in range(256):
        n = 65481 * r + 128553 * g + 24966 * b                    # exact: Y = n / 255000 + 16
        exact = (2 * n + 255000) // 510000 + 16                   # round(n / 255000) + 16 away from ties
        img = np.stack([np.full_like(g, r), g, b], -1).astype(np.uint8)
        y = fm._niqe_y(img)
        assert np.array_equal((n % 255000 == 127500), tie_set[r])
        assert np.array_equal(y[~tie_set[r]], exact[~tie_set[r]].astype(np.float64)), r
        assert np.all(np.abs(y[tie_set[r]] - (n[tie_set[r]] / 255000 + 16)) == 0.5)      # on a tie either neighbour, nothing else


def test_aggd_nan_rule():
    """An all-positive block has no negative side: its mean is NaN, every objective is NaN, argmin is 0: alpha 0.2, and the beta of the
    empty side is NaN (the other one is its deviation times the table's factor at position 0)."""
    rng = np.random.RandomState(1)
    p, alpha, bl, br, margin = fm._aggd(rng.rand(96, 96) + 0.1)
    assert p == 0 and alpha == 0.2 and np.isnan(bl) and br > 0 and np.isnan(margin)
    p, alpha, bl, br, margin = fm._aggd(np.zeros((48, 48)))
    assert p == 0 and alpha == 0.2 and np.isnan(bl) and np.isnan(br)
    p, alpha, bl, br, margin = fm._aggd(rng.normal(size=(96, 96)))
    assert 1500 < p < 2100 and bl > 0 and br > 0 and margin > 0       # a Gaussian: alpha near 2
    tabs = fm.aggd_tables()
    assert all(t.shape == (9801,) for t in tabs) and tabs[4][0] == 0.2 and abs(tabs[4][-1] - 10.0) < 1e-9


@pytest.mark.parametrize('name', list(C.SHAPES))
def test_margin_condition_on_the_test_images(name):
    """A condition on the inputs of tests/test_gpu_niqe.py: every alpha estimate's best grid point beats the second best by at least
    1e-9 in |r_gam - rn| (fp64 summation-order noise is about 1e-12), so equal grid positions can be demanded of the GPU."""
    ref = C.reference(name)
    m = ref['margin']
    finite = ~np.isnan(m)
    print(f'{name}: smallest margin {m[finite].min():.3g}, {int((~finite).sum())} NaN estimates, score {ref["score"]!r}')
    assert m[finite].min() >= 1e-9
    nan_rows = np.isnan(ref['features']).any(1)
    if name == 'constant_block':
        assert list(np.nonzero(nan_rows)[0]) == [0] and np.all(ref['positions'][0] == 0) and np.all(ref['features'][0, ::18] == 0.2)
        assert np.isfinite(ref['score'])
    else:
        assert finite.all() and not nan_rows.any()
    pos = ref['positions'][~nan_rows]
    assert pos.min() > 0 and pos.max() < 9800                     # the search is exercised: no alpha pinned at an end of the grid
    assert np.isnan(ref['score']) == (name == 'one_block')
    if name == 'tie_pixels':
        ties = {tuple(t) for t in C.tie_triples()}
        assert sum(tuple(px) in ties for px in C.image(name).reshape(-1, 3)) >= 50


def test_score_bar_is_measured_from_the_definition():
    bar = C.score_bar()
    print(f'score bar {bar:.3g}')
    assert 0 < bar < 1e-6


def test_calculate_niqe_is_the_pieces_and_the_tail_handles_nan_rows():
    mu, cov, win = C.params()
    ref = C.reference('ragged_crop')
    assert ref['features'].shape == (6, 36) and ref['y'].shape == (192, 288) and ref['y2'].shape == (96, 144)
    assert fm.calculate_niqe(C.image('ragged_crop'), 4, (mu, cov, win)) == ref['score']
    f = np.array(ref['features'])
    f[2, 5] = np.nan
    want_mu = np.nanmean(f, 0)
    dn = np.delete(f, 2, 0)
    inv = np.linalg.pinv((cov + np.cov(dn, rowvar=False)) / 2)
    assert fm.niqe_score_from_features(f, mu, cov) == float(np.sqrt((mu - want_mu) @ inv @ (mu - want_mu)))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.isnan(fm.niqe_score_from_features(f[:1], mu, cov))


# ---------------------------------------------------------------- refusals before any launch
@pytest.mark.parametrize('B,H,W,crop', [(0, 96, 96, 0), (65536, 96, 96, 0), (1, 95, 200, 0), (1, 200, 95, 0), (1, 103, 200, 4),
                                        (1, 96, 96, -1), (1, 8, 200, 4), (3, 16384, 16384, 0), (65535, 1 << 30, 1 << 30, 0)])
def test_abi_refuses_bad_niqe_shapes(B, H, W, crop):
    lib = _lib.load()
    n = ctypes.c_size_t(7)
    assert lib.femasr_niqe_workspace_bytes(B, H, W, crop, ctypes.byref(n)) == -1 and n.value == 7
    assert lib.femasr_niqe_features(None, FAKE, B, H, W, crop, FAKE, FAKE, FAKE, FAKE, 8, FAKE, FAKE, 8, FAKE, FAKE, FAKE, 1 << 40) == -1


def test_abi_sizes_and_refuses_bad_buffers():
    lib = _lib.load()
    n = ctypes.c_size_t()
    assert lib.femasr_niqe_workspace_bytes(2, 200, 300, 4, ctypes.byref(n)) == 0
    assert n.value == 2 * 192 * 288 * 32                           # 32 bytes per scored pixel: y, y / 255, z, and 1/2 + 1/4 + 1/4 for scale 2
    off = (ctypes.c_size_t * 4)()
    assert lib.femasr_niqe_plane_offsets(2, 200, 300, 4, ctypes.byref(off)) == 0
    assert list(off) == [0, 2 * 192 * 288 * 16, 2 * 192 * 288 * 28, 2 * 192 * 288 * 30]

    def call(ws=FAKE, ws_bytes=1 << 40, img=FAKE, taps=8):
        return lib.femasr_niqe_features(None, img, 2, 200, 300, 4, FAKE, FAKE, FAKE, FAKE, taps, FAKE, FAKE, 8, FAKE, FAKE, ws, ws_bytes)
    assert call(ws=None) == -1 and call(img=None) == -1 and call(taps=0) == -1
    assert call(ws=ctypes.c_void_p((1 << 20) + 8)) == -1           # workspace not 256-byte aligned
    assert call(ws_bytes=n.value - 1) == -4                        # FEMASR_ERR_WORKSPACE
    assert lib.femasr_imresize_workspace_bytes(3, 24, 37, 12, 19, ctypes.byref(n)) == 0 and n.value == -(-3 * 12 * 37 * 8 // 256) * 256

    def resize(N_=3, H=24, W=37, Ho=12, Wo=19, f64=1, ws_bytes=1 << 40, taps=8):
        return lib.femasr_imresize(None, FAKE, f64, N_, H, W, Ho, Wo, FAKE, FAKE, taps, FAKE, FAKE, 8, FAKE, FAKE, ws_bytes)
    assert resize(N_=0) == -1 and resize(N_=65536) == -1 and resize(Ho=0) == -1 and resize(f64=2) == -1 and resize(taps=0) == -1
    assert resize(H=1 << 16, W=1 << 15) == -1                      # a plane of 2^31 elements
    assert resize(ws_bytes=n.value - 1) == -4


def test_python_refuses_cpu_tensors_dtypes_and_shapes(tmp_path):
    p = C.params()
    a = torch.zeros((96, 96, 3), dtype=torch.uint8)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        N.niqe(a, p)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        N.features(a, p)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        R.imresize(torch.zeros(8, 8), 0.5)
    with pytest.raises(TypeError):
        N.niqe(a.numpy(), p)
    with pytest.raises(TypeError):
        R.imresize(np.zeros((8, 8)), 0.5)
    meta = torch.zeros((96, 96, 3), dtype=torch.uint8, device='meta')
    with pytest.raises(_lib.FemasrError):
        N.niqe(meta, p)
    with pytest.raises(ValueError, match='36'):
        N.niqe(a, (p[0][:35], p[1], p[2]))
    with pytest.raises(ValueError, match='unknown metric type'):
        N.create_metric('psnr')
    with pytest.raises(ValueError, match='pretrained_model_path'):
        N.create_metric('niqe')
    from femasr_amd import psnr_ssim
    with pytest.raises(ValueError, match='unknown metric type'):
        psnr_ssim.create_metric('niqe')                           # niqe has its own module


def test_params_file_round_trip(tmp_path):
    mu, cov, win = C.params()
    path = str(tmp_path / 'niqe_pris_params.npz')
    np.savez(path, mu_pris_param=mu[None, :].astype(np.float32), cov_pris_param=cov, gaussian_window=win)       # BasicSR's mu is (1, 36)
    p = N.load_pris_params(path)
    assert p.mu_pris.shape == (36,) and p.mu_pris.dtype == np.float64 and np.array_equal(p.cov_pris, cov) and np.array_equal(p.window, win)
    N.create_metric('niqe', pretrained_model_path=path, crop_border=4, better='lower')
    np.savez(path, mu_pris_param=mu, cov_pris_param=cov)
    with pytest.raises(ValueError, match='gaussian_window'):
        N.load_pris_params(path)


# ---------------------------------------------------------------- the folder CLI and the skipped metric
def test_cli_lists_recursively_and_sorted(tmp_path):
    root = str(tmp_path / 'in')
    for name in ('b.png', 'a.png', 'sub/c.png', '.hidden.png', '.cache/d.png'):
        path = os.path.join(root, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, 'wb').close()
    got = cli.list_images(root)
    assert [g[0] for g in got] == ['d', 'a', 'b', 'c']
    assert [g[1] for g in got] == sorted(os.path.join(root, n) for n in ('.cache/d.png', 'a.png', 'b.png', 'sub/c.png'))
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(SystemExit, match='no images'):
        cli.score_folder(str(empty), 'unused.npz')
    with pytest.raises(SystemExit) as e:
        cli.main(['--input', root])                               # --params is required
    assert e.value.code == 2


def test_niqe_without_a_parameter_file_stays_skipped(caplog):
    """nondist_validation's metric split, without a GPU: a niqe block without pretrained_model_path is reported as skipped (None) and the
    warning names the file it needs."""
    import logging

    class Data(list):
        class dataset:
            opt = {'name': 'none'}
    model = fm.FeMaSRModel.__new__(fm.FeMaSRModel)
    model.opt = {'val': {'metrics': {'niqe': {'type': 'niqe', 'better': 'lower'}, 'musiq': {'type': 'musiq'}}}}
    with caplog.at_level(logging.WARNING, logger='femasr_amd'):
        r = model.nondist_validation(Data(), 0, None, False)
    assert r == {'niqe': None, 'musiq': None}
    assert 'niqe_pris_params.npz' in caplog.text and "['musiq', 'niqe']" in caplog.text

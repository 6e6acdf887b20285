"""PSNR / SSIM host logic without a GPU: the C ABI's refusals (nothing is launched, so they run here), the SSIM window against the
definition, the two orders the kernels reproduce, the Python-side refusals, and the folder CLI's listing, pairing and refusal."""
import ctypes
import os

import numpy as np
import pytest
import torch

from femasr_amd import _lib
from femasr_amd import psnr_ssim as P
from femasr_amd import psnr_ssim_folder as cli
from femasr_amd.models import femasr_model as fm

FAKE = ctypes.c_void_p(1 << 20)      # a 256-aligned non-null address: every call below must return before touching it


def _ws_bytes(B, H, W, crop, ty):
    n = ctypes.c_size_t(7)
    rc = _lib.load().femasr_psnr_ssim_workspace_bytes(B, H, W, crop, ty, ctypes.byref(n))
    return rc, n.value


def _launch(B, H, W, crop, ty, psnr=True, ssim=True, mse=True, ws=FAKE, ws_bytes=1 << 40):
    lib = _lib.load()
    return lib.femasr_psnr_ssim(None, FAKE, FAKE, B, H, W, crop, ty, FAKE if psnr else None, FAKE if ssim else None, FAKE if mse else None,
                                ws, ws_bytes)


BAD_SHAPES = [  # (B, H, W, crop, test_y)
    (0, 32, 32, 0, 1),              # B < 1
    (65536, 16, 16, 0, 1),          # B > 65535 (grid.y)
    (1, 0, 32, 0, 1),               # empty image
    (1, 32, 32, -1, 1),             # negative crop
    (1, 8, 32, 4, 0),               # 2 crop == H
    (1, 32, 9, 5, 0),               # 2 crop > W
    (1, 32, 32, 0, 2),              # test_y not 0 / 1
    (3, 16384, 16384, 0, 1),        # B H W 3 >= 2^31
    (1, 26755, 26755, 0, 0),        # one image of >= 2^31 bytes
    (65535, 1 << 30, 1 << 30, 0, 1),    # B H W 3 wraps around in 64 bits
]


@pytest.mark.parametrize('B,H,W,crop,ty', BAD_SHAPES)
def test_abi_refuses_bad_shapes(B, H, W, crop, ty):
    rc, n = _ws_bytes(B, H, W, crop, ty)
    assert rc == -1 and n == 7
    assert _launch(B, H, W, crop, ty) == -1
    assert _launch(B, H, W, crop, ty, ssim=False) == -1


@pytest.mark.parametrize('H,W,crop', [(10, 40, 0), (40, 10, 0), (18, 40, 4), (40, 18, 4), (1, 1, 0)])
def test_ssim_below_its_window_is_refused_and_psnr_is_sized(H, W, crop):
    """A cropped size below 11x11 has no valid SSIM position: a launch with ssim_out set is refused, while the workspace is still sized for
    PSNR / MSE alone (that PSNR-only launch runs on the GPU: tests/test_gpu_psnr_ssim.py::test_refused_before_any_launch)."""
    rc, n = _ws_bytes(1, H, W, crop, 1)
    assert rc == 0 and n > 0 and n % 256 == 0
    assert _launch(1, H, W, crop, 1, ssim=True) == -1
    assert b'11x11' in _lib.load().femasr_last_error()


def test_abi_refuses_bad_buffers():
    rc, n = _ws_bytes(3, 64, 48, 4, 0)
    assert rc == 0
    assert _launch(3, 64, 48, 4, 0, psnr=False, ssim=False, mse=False) == -1        # nothing requested
    assert _launch(3, 64, 48, 4, 0, ws=ctypes.c_void_p((1 << 20) + 8)) == -1       # workspace not 256-byte aligned
    assert _launch(3, 64, 48, 4, 0, ws=None) == -1
    assert _launch(3, 64, 48, 4, 0, ws_bytes=n - 1) == -4                          # FEMASR_ERR_WORKSPACE
    lib = _lib.load()
    assert lib.femasr_psnr_ssim(None, None, FAKE, 3, 64, 48, 4, 0, FAKE, FAKE, FAKE, FAKE, n) == -1


def test_workspace_is_one_partial_per_block():
    """One fp64 partial per block and plane: 32 x 16 SSIM tiles of the valid map + 4096-pixel PSNR chunks of the cropped plane."""
    ho, wo, hc, wc = 1348 - 10, 2032 - 10, 1348, 2032
    blocks = -(-ho // 16) * -(-wo // 32) + -(-hc * wc // 4096)
    for B, ty, planes in ((1, 1, 1), (1, 0, 3), (16, 1, 1), (16, 0, 3)):
        assert _ws_bytes(B, 1356, 2040, 4, ty) == (0, -(-B * planes * blocks * 8 // 256) * 256)


def _numpy_g():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    return g


def test_window_is_the_definition_bit_for_bit():
    win = (ctypes.c_double * 121)()
    assert _lib.load().femasr_ssim_window(win) == 0
    got = np.frombuffer(win, dtype=np.float64).reshape(11, 11)
    want = np.outer(_numpy_g(), _numpy_g())
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _scipy_order(x, win):
    """convolve2d(x, win, 'valid') as the SSIM kernel sums it: one accumulator from 0, window row j ascending, then column k, product
    win[j][k] * x[m + 10 - j][n + 10 - k]."""
    ho, wo = x.shape[0] - 10, x.shape[1] - 10
    s = np.zeros((ho, wo))
    for j in range(11):
        for k in range(11):
            s = s + win[j, k] * x[10 - j:10 - j + ho, 10 - k:10 - k + wo]
    return s


def test_kernel_order_is_scipys_summation_order():
    """The kernel's SSIM map is _ssim_plane's bit for bit only while scipy sums in this order: if a scipy release changes it, the GPU values
    still agree to rounding, but the 1e-12 bound on one-pixel maps (tests/test_gpu_psnr_ssim.py) rests on this."""
    from scipy.signal import convolve2d
    win = np.outer(_numpy_g(), _numpy_g())
    rng = np.random.RandomState(0)
    for h, w in ((11, 11), (12, 19), (37, 23)):
        for x in (rng.randint(0, 256, (h, w)).astype(np.float64), fm._to_y(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)) ** 2):
            assert np.array_equal(_scipy_order(x, win), convolve2d(x, win, mode='valid'))


# ---------------------------------------------------------------- Python refusals (before any launch)
def test_python_refuses_cpu_tensors_dtypes_and_shapes():
    a = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        P.psnr(a, a)
    with pytest.raises(_lib.FemasrError, match='no CPU fallback'):
        P.create_metric('ssim', crop_border=4)(a, a)
    with pytest.raises(TypeError):
        P.ssim(a.numpy(), a.numpy())
    meta = torch.zeros((16, 16, 3), dtype=torch.uint8, device='meta')
    with pytest.raises(_lib.FemasrError):
        P.psnr_ssim(meta, meta)
    with pytest.raises(ValueError, match='unknown metric type'):
        P.create_metric('niqe')


def test_create_metric_takes_the_cpu_keywords():
    P.create_metric('psnr', crop_border=4, test_y_channel=True, color_space='ycbcr', better='higher')
    P.create_metric('ssim')


# ---------------------------------------------------------------- the folder CLI: listing, pairing, refusal
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'wb').close()


def test_cli_pairs_by_index_recursively_and_sorted(tmp_path):
    gt, res = str(tmp_path / 'gt'), str(tmp_path / 'res')
    for name in ('b.png', 'a.png', 'sub/c.png', '.hidden.png', '.cache/d.png'):
        _touch(os.path.join(gt, name))
    for name in ('x3.png', 'x1.png', 'deep/x2.png', 'x0.png'):
        _touch(os.path.join(res, name))
    pairs = cli.list_pairs(gt, res)
    assert [p[0] for p in pairs] == ['d', 'a', 'b', 'c']          # sorted full paths: '.cache/' < 'a.png' < 'b.png' < 'sub/'
    assert [p[1] for p in pairs] == sorted(os.path.join(gt, n) for n in ('.cache/d.png', 'a.png', 'b.png', 'sub/c.png'))
    assert [p[2] for p in pairs] == sorted(os.path.join(res, n) for n in ('x3.png', 'x1.png', 'deep/x2.png', 'x0.png'))
    with pytest.raises(SystemExit, match='pair by index'):
        cli.list_pairs(res, gt + '/sub')


def test_cli_pairs_by_suffix(tmp_path):
    gt, res = str(tmp_path / 'gt'), str(tmp_path / 'res')
    for name in ('img1.png', 'sub/img2.jpg'):
        _touch(os.path.join(gt, name))
    pairs = cli.list_pairs(gt, res, suffix='_out')
    assert pairs == [('img1', os.path.join(gt, 'img1.png'), os.path.join(res, 'img1_out.png')),
                     ('img2', os.path.join(gt, 'sub', 'img2.jpg'), os.path.join(res, 'img2_out.jpg'))]


def test_cli_refuses_correct_mean_var(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(['--gt', str(tmp_path), '--restored', str(tmp_path), '--correct_mean_var'])
    assert e.value.code == 2
    assert '--correct_mean_var is not supported' in capsys.readouterr().err


def test_cli_refuses_an_empty_folder(tmp_path):
    with pytest.raises(SystemExit, match='no images'):
        cli.score_folders(str(tmp_path), str(tmp_path))

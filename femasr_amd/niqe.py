"""NIQE of uint8 RGB images on the MI355X path: the no-reference metric of scripts/metrics/calculate_niqe.py (BasicSR's
calculate_niqe(img, crop_border, input_order='HWC', convert_to='y')), for images that have no ground truth.

    params = load_pris_params('niqe_pris_params.npz')                 BasicSR's keys mu_pris_param, cov_pris_param, gaussian_window
    niqe(img_u8, params, crop_border=0) -> (B,) float64 (host)         img_u8: uint8 (H,W,3) or (B,H,W,3) RGB on a GPU
    features(img_u8, params, crop_border=0) -> Features(features (B, n_blocks, 36) float64, positions (B, n_blocks, 10) int32), on the GPU
    create_metric('niqe', pretrained_model_path=..., crop_border=0) -> callable (sr_u8) -> float

The definition is femasr_amd.models.femasr_model's calculate_niqe (numpy, fp64).  Everything that touches pixels runs in libfemasr_hip.so
(csrc/niqe.hip, femasr_niqe_features): the rounded luma, the 7x7 local mean / deviation and z at both scales (the definition's bits), the
antialiased x0.5 imresize between them, the moments of every 96x96 block and the AGGD grid search.  The tail (nanmean, covariance, pinv,
the quadratic form; 36 numbers per block) is the definition's own host function, niqe_score_from_features, so `niqe` synchronises with the
host and returns a host tensor.  No parameter file ships with the package and none is downloaded.  There is no CPU path.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import resize

MAX_IMAGES = 65535      # images per library call (its grid.z); larger batches are split into calls of whole images
Features = namedtuple('Features', 'features positions')
Params = namedtuple('Params', 'mu_pris cov_pris window')


def load_pris_params(path):
    """Params(mu_pris (36,), cov_pris (36,36), window (7,7)) float64 from an .npz with BasicSR's keys."""
    with np.load(path) as f:
        missing = [k for k in ('mu_pris_param', 'cov_pris_param', 'gaussian_window') if k not in f.files]
        if missing:
            raise ValueError(f'{path}: not a NIQE parameter file, keys {missing} are missing (found {sorted(f.files)})')
        mu, cov, win = (np.asarray(f[k], dtype=np.float64) for k in ('mu_pris_param', 'cov_pris_param', 'gaussian_window'))
    return check_params((mu, cov, win))


def check_params(params):
    mu, cov, win = (np.array(p, dtype=np.float64) for p in params)      # (copies: the caller's arrays may be read-only)
    if mu.size != 36 or cov.shape != (36, 36) or win.shape != (7, 7):
        raise ValueError(f'niqe: expected mu_pris (36,), cov_pris (36,36) and a (7,7) window, got {mu.shape}, {cov.shape}, {win.shape}')
    return Params(mu.reshape(36), cov, np.ascontiguousarray(win))


def _images(x):
    """(B,H,W,3) contiguous uint8 view of x on a GPU; raises before any launch otherwise."""
    if not torch.is_tensor(x):
        raise TypeError(f'niqe: expected a torch tensor, got {type(x).__name__}')
    if x.device.type != 'cuda':
        raise _lib.FemasrError(f'niqe: tensor on {x.device}: it runs on a GPU only (no CPU fallback)')
    if x.dtype != torch.uint8:
        raise ValueError(f'niqe: expected uint8 images, got {x.dtype}')
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f'niqe: expected (H,W,3) or (B,H,W,3) RGB images, got {tuple(x.shape)}')
    return x.contiguous()


@torch.no_grad()
def _features(x, params, crop_border, planes):
    from .models.femasr_model import aggd_tables
    params = check_params(params)
    x = _images(x)
    B, H, W, _ = x.shape
    crop, dev = int(crop_border), x.device
    lib = _lib.load()
    step = max(1, min(MAX_IMAGES, B, ((1 << 31) - 1) // max(1, H * W * 3)))
    nbytes = ctypes.c_size_t()
    _lib.check(lib.femasr_niqe_workspace_bytes(step, H, W, crop, ctypes.byref(nbytes)))      # refuses a size without a 96x96 block
    nh, nw = (H - 2 * crop) // 96, (W - 2 * crop) // 96
    Hb, Wb = nh * 96, nw * 96
    if planes and step < B:
        raise ValueError(f'niqe: planes are returned for one library call, and {B} images of {H}x{W} need several')
    with torch.cuda.device(dev):
        window = torch.from_numpy(params.window).to(dev)
        tables = torch.from_numpy(np.concatenate(aggd_tables())).to(dev)
        wh, ih, ph = resize.device_tables(Hb, Hb // 2, 0.5, True, dev)
        ww, iw, pw = resize.device_tables(Wb, Wb // 2, 0.5, True, dev)
        feat = torch.empty((B, nh * nw, 36), dtype=torch.float64, device=dev)
        pos = torch.empty((B, nh * nw, 10), dtype=torch.int32, device=dev)
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            _lib.check(lib.femasr_niqe_features(stream, _lib.ptr(x[b0:b0 + nb]), nb, H, W, crop, _lib.ptr(window), _lib.ptr(tables),
                                                _lib.ptr(wh), _lib.ptr(ih), ph, _lib.ptr(ww), _lib.ptr(iw), pw, _lib.ptr(feat[b0:b0 + nb]),
                                                _lib.ptr(pos[b0:b0 + nb]), _lib.ptr(ws), nbytes.value))
        if not planes:
            return Features(feat, pos), None
        off = (ctypes.c_size_t * 4)()
        _lib.check(lib.femasr_niqe_plane_offsets(B, H, W, crop, ctypes.byref(off)))
        shapes = ((B, Hb, Wb), (B, Hb, Wb), (B, Hb // 2, Wb // 2), (B, Hb // 2, Wb // 2))
        out = {}
        for name, o, shp in zip(('y', 'z', 'y2', 'z2'), off, shapes):
            n = shp[0] * shp[1] * shp[2]
            out[name] = ws[o:o + 8 * n].view(torch.float64).reshape(shp).clone()
        return Features(feat, pos), out


def features(img_u8, params, crop_border=0, return_planes=False):
    """Features(features (B, n_blocks, 36) float64, positions (B, n_blocks, 10) int32) on the device: per block (in the definition's order,
    `for iw: for ih`) the 18 AGGD features of each scale, and the grid position of each of the 5 alphas per scale.  With return_planes
    also a dict of the fp64 planes y, z, y2, z2 ((B, 96 nh, 96 nw) and half that), which are the definition's bits."""
    f, planes = _features(img_u8, params, crop_border, return_planes)
    return (f, planes) if return_planes else f


def niqe(img_u8, params, crop_border=0):
    """calculate_niqe per image: (B,) float64 on the host (the tail runs there).  NaN where fewer than two blocks are free of NaN."""
    from .models.femasr_model import niqe_score_from_features
    params = check_params(params)
    feat = features(img_u8, params, crop_border).features.cpu().numpy()
    return torch.tensor([niqe_score_from_features(f, params.mu_pris, params.cov_pris) for f in feat], dtype=torch.float64)


def create_metric(metric_type, pretrained_model_path=None, crop_border=0, **_):
    """The 'niqe' metric of a validation option block: a callable (sr_u8) -> float for one (H,W,3) uint8 image on a GPU.
    `pretrained_model_path` (pyiqa's keyword) names the parameter file; other keywords (better, ...) are ignored."""
    if metric_type != 'niqe':
        raise ValueError(f"unknown metric type {metric_type!r} (known: ['niqe'])")
    if not pretrained_model_path:
        raise ValueError('niqe: pretrained_model_path (a local niqe_pris_params.npz) is required: no parameter file ships here and none '
                         'is downloaded')
    params = load_pris_params(pretrained_model_path)

    def metric(sr_u8, *_gt):
        if sr_u8.dim() != 3:
            raise ValueError(f'niqe: expected one (H,W,3) image, got {tuple(sr_u8.shape)}')
        return niqe(sr_u8, params, crop_border).item()
    return metric

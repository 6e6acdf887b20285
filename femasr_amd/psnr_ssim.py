"""PSNR and SSIM of uint8 RGB images on the MI355X path: the 'psnr' / 'ssim' metrics the reference validates with (pyiqa,
basicsr/models/femasr_model.py:29-34,259-262; options/train_FeMaSR_LQ_stage.yml: crop_border 4, test_y_channel true) and that
scripts/metrics/calculate_psnr_ssim.py prints.

    psnr(x, y, crop_border=0, test_y_channel=False) -> (B,) float64       x, y: uint8 (H,W,3) or (B,H,W,3) RGB on a GPU
    ssim(...), psnr_ssim(...) -> Scores(psnr, ssim, mse)
    create_metric('psnr' | 'ssim', crop_border=..., test_y_channel=...) -> callable (sr_u8, gt_u8) -> float

The definitions are femasr_amd.models.femasr_model's calculate_psnr / calculate_ssim (fp64, BT.601 Y not rounded); the arithmetic runs in
libfemasr_hip.so (csrc/psnr_ssim.hip, femasr_psnr_ssim).  The results agree with the CPU functions within 1e-9 dB (PSNR) and 1e-12
(SSIM); in RGB mode the MSE is numpy's and every SSIM map value scipy's, bit for bit.  There is no CPU path.
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib

MAX_PAIRS = 65535       # pairs per library call (its grid.y); larger batches are split into calls of whole pairs
Scores = namedtuple('Scores', 'psnr ssim mse')


def _pairs(x, y):
    """(B,H,W,3) contiguous uint8 views of x and y on one GPU; raises before any launch otherwise."""
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise TypeError(f'psnr / ssim: expected torch tensors, got {type(x).__name__} and {type(y).__name__}')
    if x.device.type != 'cuda' or y.device.type != 'cuda':
        raise _lib.FemasrError(f'psnr / ssim: tensors on {x.device} / {y.device}: they run on a GPU only (no CPU fallback)')
    if x.device != y.device:
        raise ValueError(f'psnr / ssim: tensors on two devices, {x.device} and {y.device}')
    if x.dtype != torch.uint8 or y.dtype != torch.uint8:
        raise ValueError(f'psnr / ssim: expected uint8 images, got {x.dtype} and {y.dtype}')
    if x.shape != y.shape:
        raise ValueError(f'psnr / ssim: shapes differ, {tuple(x.shape)} and {tuple(y.shape)}')
    if x.dim() == 3:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    if x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f'psnr / ssim: expected (H,W,3) or (B,H,W,3) RGB images, got {tuple(x.shape)}')
    return x.contiguous(), y.contiguous()


@torch.no_grad()
def _scores(x, y, crop_border, test_y_channel, want_psnr, want_ssim, want_mse):
    x, y = _pairs(x, y)
    B, H, W, _ = x.shape
    dev = x.device
    outs = [torch.empty(B, dtype=torch.float64, device=dev) if w else None for w in (want_psnr, want_ssim, want_mse)]
    lib = _lib.load()
    crop, ty = int(crop_border), int(bool(test_y_channel))
    # pairs per call: at most 65535 and fewer than 2^31 bytes per image tensor; pairs are independent and every sum is per pair, so the
    # split does not change a bit
    step = max(1, min(MAX_PAIRS, ((1 << 31) - 1) // max(1, H * W * 3)))
    nbytes = ctypes.c_size_t()
    _lib.check(lib.femasr_psnr_ssim_workspace_bytes(min(step, B), H, W, crop, ty, ctypes.byref(nbytes)))
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            _lib.check(lib.femasr_psnr_ssim(stream, _lib.ptr(x[b0:b0 + nb]), _lib.ptr(y[b0:b0 + nb]), nb, H, W, crop, ty,
                                            *[None if o is None else _lib.ptr(o[b0:b0 + nb]) for o in outs], _lib.ptr(ws), nbytes.value))
    return outs


def psnr(x, y, crop_border=0, test_y_channel=False):
    """calculate_psnr per pair: (B,) float64 on the device, +inf where the cropped images are equal."""
    return _scores(x, y, crop_border, test_y_channel, True, False, False)[0]


def ssim(x, y, crop_border=0, test_y_channel=False):
    """calculate_ssim per pair: (B,) float64 on the device.  The cropped images must be at least 11x11."""
    return _scores(x, y, crop_border, test_y_channel, False, True, False)[1]


def psnr_ssim(x, y, crop_border=0, test_y_channel=False):
    """All three per pair from one library call: Scores(psnr, ssim, mse), each (B,) float64 on the device; mse is the mean squared
    difference calculate_psnr scores (in RGB mode numpy's value bit for bit)."""
    return Scores(*_scores(x, y, crop_border, test_y_channel, True, True, True))


_FUNCS = {'psnr': psnr, 'ssim': ssim}


def create_metric(metric_type, crop_border=0, test_y_channel=False, **_):
    """The 'psnr' / 'ssim' metric of a validation option block: a callable (sr_u8, gt_u8) -> float for one (H,W,3) uint8 pair on a GPU.
    Takes the CPU functions' keywords; the others (e.g. color_space) are ignored, as calculate_psnr / calculate_ssim ignore them."""
    fn = _FUNCS.get(metric_type)
    if fn is None:
        raise ValueError(f'unknown metric type {metric_type!r} (known: {sorted(_FUNCS)})')

    def metric(sr_u8, gt_u8):
        if sr_u8.dim() != 3:
            raise ValueError(f'{metric_type}: expected one (H,W,3) image per argument, got {tuple(sr_u8.shape)}')
        return fn(sr_u8, gt_u8, crop_border, test_y_channel).item()
    return metric

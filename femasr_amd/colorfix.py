"""Wavelet colour fix (opt-in; NOT the reference's arithmetic): keep the network's detail, take everything coarser than a few pixels from
the bicubically upsampled input.

    wavelet_color_fix_f64(sr, lq, levels=5) -> float64 array        the definition (numpy, runs anywhere)
    wavelet_color_fix(sr, lq, levels=5, out=None) -> tensor          the same on the GPU (libfemasr_hip.so, csrc/colorfix.hip); no CPU path

Definition.  sr: (..., sH, sW), lq: (..., H, W) on the same value scale, s = sH / H = sW / W an integer >= 1, levels L in 1..12:
  1. up = imresize(lq, s) per plane (femasr_amd.models.femasr_model.imresize, MATLAB bicubic); no clamp
  2. d = up - sr
  3. for i = 0 .. L-1, r = 2^i, indices clamped to the plane (replicate padding), a horizontal then a vertical pass of (1/4, 1/2, 1/4):
         t[y,x]  = (d[y,cl(x-r)]/4 + d[y,x]/2) + d[y,cl(x+r)]/4
         d'[y,x] = (t[cl(y-r),x]/4 + t[y,x]/2) + t[cl(y+r),x]/4
  4. out = sr + d
By linearity this is sr - B(sr) + B(up) with B the composed blur of step 3 (`atrous_blur_f64`): the high band of the content plus the low
band of the style, with one blur chain instead of two.  B spreads over 2^L - 1 pixels to either side and reproduces constants, so a tone
offset of a whole tile disappears while detail finer than the first radii passes unchanged.

GPU arithmetic: `up` is femasr_amd.resize.imresize's float32 result (fp64 accumulation in tap order, rounded once); every later step is one
IEEE fp32 operation in the order written above, so |fp32 - definition| <= (8 L + 6) 2^-24 max(max|sr|, max|up|) and
tests/colorfix_ref.py restates it in float32 numpy bit for bit.  The uint8 form works on the planes (float)byte / 255.0f and stores
rint(clamp(out, 0, 1) * 255), half to even (tensor2img's rounding): like the uint8 blend it fixes the BYTES the canvas holds after
quantisation - it is not the quantised fp32 fix.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_LEVELS = 12
WORKSPACE_CAP = 512 << 20       # planes are worked through in groups whose workspace stays below this (one plane at least)
_TABLES = {}                    # (H, W, s, device) -> the resize tables on that device


def _check_levels(levels):
    if not isinstance(levels, (int, np.integer)) or isinstance(levels, bool) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f'color fix: levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}')
    return int(levels)


def _check_shapes(sr_shape, lq_shape):
    """(H, W, sH, sW, s) of (..., sH, sW) against (..., H, W); ValueError unless the leading axes agree and s is one integer >= 1."""
    if len(sr_shape) < 2 or len(sr_shape) != len(lq_shape) or tuple(sr_shape[:-2]) != tuple(lq_shape[:-2]):
        raise ValueError(f'color fix: sr {tuple(sr_shape)} and lq {tuple(lq_shape)} must agree in every axis but the last two')
    (sh, sw), (h, w) = sr_shape[-2:], lq_shape[-2:]
    if h < 1 or w < 1 or sh < 1 or sw < 1 or sh % h or sw % w or sh // h != sw // w:
        raise ValueError(f'color fix: sr planes of {sh}x{sw} are no integer multiple of lq planes of {h}x{w}')
    return h, w, sh, sw, sh // h


def atrous_blur_f64(d, levels):
    """Step 3 of the definition on (..., h, w) float64 planes: B(d)."""
    d = np.asarray(d, dtype=np.float64)
    h, w = d.shape[-2:]
    ys, xs = np.arange(h), np.arange(w)
    for i in range(_check_levels(levels)):
        r = 1 << i
        xm, xp = np.clip(xs - r, 0, w - 1), np.clip(xs + r, 0, w - 1)
        ym, yp = np.clip(ys - r, 0, h - 1), np.clip(ys + r, 0, h - 1)
        t = (0.25 * d[..., :, xm] + 0.5 * d) + 0.25 * d[..., :, xp]
        d = (0.25 * t[..., ym, :] + 0.5 * t) + 0.25 * t[..., yp, :]
    return d


def wavelet_color_fix_f64(sr, lq, levels=5):
    """The definition (module docstring) in numpy / float64."""
    from .models.femasr_model import imresize
    sr, lq = np.asarray(sr, dtype=np.float64), np.asarray(lq, dtype=np.float64)
    s = _check_shapes(sr.shape, lq.shape)[4]
    up = imresize(lq, s)
    return sr + atrous_blur_f64(up - sr, levels)


def _tables(h, w, s, device):
    key = (h, w, s, str(device))
    if key not in _TABLES:
        from .resize import device_tables
        if len(_TABLES) >= 8:
            _TABLES.clear()
        _TABLES[key] = device_tables(h, h * s, s, True, device) + device_tables(w, w * s, s, True, device)
    return _TABLES[key]


@torch.no_grad()
def wavelet_color_fix(sr, lq, levels=5, out=None):
    """The colour fix on the GPU.  float32: sr (B,C,sH,sW) with lq (B,C,H,W) (any equal leading axes); uint8: sr (B,sH,sW,3) with lq
    (B,H,W,3), or (sH,sW,3) with (H,W,3) - the fix of the bytes, see the module docstring.  Returns a new tensor, or `out` (a contiguous
    tensor like sr; it may be sr itself: in place).  Runs on the current stream; the workspace is bounded (WORKSPACE_CAP), planes are
    processed in groups.  ValueError on a shape / dtype mismatch, FemasrError for tensors that are not on a GPU."""
    if not torch.is_tensor(sr) or not torch.is_tensor(lq):
        raise TypeError(f'color fix: expected torch tensors, got {type(sr).__name__} and {type(lq).__name__}')
    levels = _check_levels(levels)
    if sr.dtype != lq.dtype or sr.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'color fix: sr and lq must both be float32 or both uint8, got {sr.dtype} and {lq.dtype}')
    u8 = sr.dtype == torch.uint8
    if u8:
        if sr.dim() not in (3, 4) or sr.shape[-1] != 3 or lq.shape[-1:] != sr.shape[-1:] or lq.dim() != sr.dim():
            raise ValueError(f'color fix: uint8 images are (H,W,3) or (B,H,W,3), got sr {tuple(sr.shape)} and lq {tuple(lq.shape)}')
        h, w, sh, sw, s = _check_shapes(tuple(sr.shape[:-3]) + tuple(sr.shape[-3:-1]), tuple(lq.shape[:-3]) + tuple(lq.shape[-3:-1]))
    else:
        h, w, sh, sw, s = _check_shapes(sr.shape, lq.shape)
    if sh * sw >= 1 << 31:
        raise ValueError(f'color fix: a plane of {sh}x{sw} reaches 2^31 elements')
    if out is not None and (not torch.is_tensor(out) or out.shape != sr.shape or out.dtype != sr.dtype or out.device != sr.device or
                            not out.is_contiguous()):
        raise ValueError(f'color fix: out= must be a contiguous {sr.dtype} tensor of shape {tuple(sr.shape)} on {sr.device}')
    if sr.device.type != 'cuda' or lq.device != sr.device:
        raise _lib.FemasrError(f'color fix: tensors on {sr.device} and {lq.device}: it runs on one GPU only (no CPU fallback)')
    dev = sr.device
    if out is None:
        out = torch.empty_like(sr, memory_format=torch.contiguous_format)
    planes = sr.numel() // (sh * sw)                          # (a uint8 image is three planes)
    if planes == 0:
        return out
    sr_c, lq_c = sr.contiguous(), lq.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        wh, ih, ph, ww, iw, pw = _tables(h, w, s, dev)
        per, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.femasr_color_fix_workspace_bytes(1, h, w, sh, sw, s, ctypes.byref(per)))
        group = max(1, min(planes, WORKSPACE_CAP // per.value))
        _lib.check(lib.femasr_color_fix_workspace_bytes(group, h, w, sh, sw, s, ctypes.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        fn = lib.femasr_color_fix_u8 if u8 else lib.femasr_color_fix
        _lib.check(fn(ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _lib.ptr(sr_c), _lib.ptr(lq_c), planes // 3 if u8 else planes, h, w, sh, sw, s, levels,
                      _lib.ptr(wh), _lib.ptr(ih), ph, _lib.ptr(ww), _lib.ptr(iw), pw, _lib.ptr(out), _lib.ptr(ws), nbytes.value))
    return out

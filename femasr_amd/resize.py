"""MATLAB-style bicubic `imresize` (basicsr/utils/matlab_functions.py:86, the resize that produces benchmark LQ images and NIQE's second
scale) on the MI355X path.

    imresize(x, scale, antialiasing=True) -> tensor          x: (..., H, W) float32 or float64 on a GPU; same dtype out, (..., ceil(H s), ceil(W s))

The definition is femasr_amd.models.femasr_model.imresize (numpy, fp64); its weight / index tables (imresize_tables: the reference's
formulas evaluated in fp64, the symmetric padding folded into reflected indices) are built on the host and the two passes run in
libfemasr_hip.so (csrc/niqe.hip, femasr_imresize): fp64 accumulation in tap order, so a float64 result is the definition's bit for bit and
a float32 result that value rounded once.  There is no CPU path.
"""
import ctypes
import math

import torch

from . import _lib

MAX_PLANES = 65535      # planes per library call (its grid.y)


def device_tables(in_length, out_length, scale, antialiasing, device):
    """imresize_tables on `device`: (weights (out, taps) float64, rows (out, taps) int32, taps)."""
    from .models.femasr_model import imresize_tables
    w, idx = imresize_tables(in_length, out_length, scale, antialiasing)
    return torch.from_numpy(w).to(device), torch.from_numpy(idx).to(device), w.shape[1]


@torch.no_grad()
def imresize(x, scale, antialiasing=True):
    if not torch.is_tensor(x):
        raise TypeError(f'imresize: expected a torch tensor, got {type(x).__name__}')
    if x.device.type != 'cuda':
        raise _lib.FemasrError(f'imresize: tensor on {x.device}: it runs on a GPU only (no CPU fallback)')
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'imresize: expected float32 or float64 planes, got {x.dtype}')
    if x.dim() < 2 or x.shape[-1] < 1 or x.shape[-2] < 1:
        raise ValueError(f'imresize: expected (..., H, W) planes, got {tuple(x.shape)}')
    if not scale > 0:
        raise ValueError(f'imresize: scale must be positive, got {scale}')
    H, W = x.shape[-2:]
    Ho, Wo = math.ceil(H * scale), math.ceil(W * scale)
    dev = x.device
    wh, ih, ph = device_tables(H, Ho, scale, antialiasing, dev)      # raises ValueError where the padding would leave the image
    ww, iw, pw = device_tables(W, Wo, scale, antialiasing, dev)
    planes = x.reshape(-1, H, W).contiguous()
    N = planes.shape[0]
    out = torch.empty((N, Ho, Wo), dtype=x.dtype, device=dev)
    if N == 0:
        return out.reshape(x.shape[:-2] + (Ho, Wo))
    lib = _lib.load()
    step = min(MAX_PLANES, N)
    nbytes = ctypes.c_size_t()
    _lib.check(lib.femasr_imresize_workspace_bytes(step, H, W, Ho, Wo, ctypes.byref(nbytes)))
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for n0 in range(0, N, step):
            nb = min(step, N - n0)
            _lib.check(lib.femasr_imresize(stream, _lib.ptr(planes[n0:n0 + nb]), int(x.dtype == torch.float64), nb, H, W, Ho, Wo,
                                           _lib.ptr(wh), _lib.ptr(ih), ph, _lib.ptr(ww), _lib.ptr(iw), pw, _lib.ptr(out[n0:n0 + nb]),
                                           _lib.ptr(ws), nbytes.value))
    return out.reshape(x.shape[:-2] + (Ho, Wo))

"""A final resample of the output image to any size (opt-in): the network returns x2 or x4, this turns its uint8 result into
x3, x1.5, a fixed delivery size or the input's own size - MATLAB bicubic, bytes in and bytes out, on the GPU in ONE launch.

    resample_ref(img, out_h, out_w) -> uint8                 the DEFINITION (numpy, fp64)
    target_size(h, w, net_scale, final_scale=None, final_size=None) -> (out_h, out_w)
    check_ratio(h, w, out_h, out_w)                          ResampleRatio outside MIN_RATIO .. MAX_RATIO on an axis
    prepare(h, w, out_h, out_w, device)                      every refusal about the sizes, ahead of the call (the CLI: ahead of the forward)
    resample_u8(img, out_h, out_w, out=None)                 the same bytes on the GPU (csrc/resample.hip); GPU tensors only

Definition.  img: uint8 (H,W) or (H,W,C), C in 1..4; every channel on its own (alpha is a channel like any other).
    samples  float64(byte)
    H pass   imresize_tables(H, out_h, out_h / H, antialiasing=True), then the W pass with imresize_tables(W, out_w, out_w / W, True) - the
             tables of femasr_amd.models.femasr_model.imresize, which take the lengths and the scale separately, so an exact target size and
             one ratio per axis need no new mathematics
    sums     every output is one fp64 accumulator over its taps in ascending order from 0.0, multiply and add rounded separately (the loops
             of femasr_model.imresize)
    bytes    np.rint(np.clip(v, 0, 255)): ties go to even
    refusal  where imresize_tables raises (the symmetric padding would leave the image) ResampleTooSmall; no special case is added: a
             1-pixel axis is refused even at equal size
Not done: float images, other filters.
"""
import math
from fractions import Fraction

import numpy as np

TILE = 256                          # output columns per block of the kernel at most (femasr_resample_tile(); checked at the first call)
MIN_RATIO, MAX_RATIO = Fraction(1, 8), Fraction(8)      # out / in per axis that resample_u8 takes
RATIO_LIMIT = 'the final size must lie within 1/8 .. 8 of the size it is resampled from, on each axis'


class ResampleTooSmall(ValueError):
    """An axis is too short for the bicubic tables at this ratio (imresize_tables refuses it)."""


class ResampleRatio(ValueError):
    """out / in of an axis is outside MIN_RATIO .. MAX_RATIO."""


# ---------------------------------------------------------------------------------------------------------------- definitions
def _tables(n, out):
    from .models.femasr_model import imresize_tables
    try:
        return imresize_tables(n, out, out / n, True)
    except ValueError as e:
        raise ResampleTooSmall(f'resample {n} -> {out}: {e}') from None


def _check_img(shape, dtype, what):
    if str(dtype).replace('torch.', '') != 'uint8':
        raise ValueError(f'{what}: expected uint8, got {dtype}')
    if not (len(shape) == 2 or (len(shape) == 3 and 1 <= shape[2] <= 4)) or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f'{what}: expected a non-empty (H,W) or (H,W,C) image with C in 1..4, got {tuple(shape)}')


def _check_size(out_h, out_w, what):
    for v in (out_h, out_w):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1:
            raise ValueError(f'{what}: the output size must be two integers >= 1, got {out_h!r} x {out_w!r}')
    return int(out_h), int(out_w)


def resample_values(img, out_h, out_w):
    """The definition in front of the clip and the rounding: float64 (out_h,out_w) or (out_h,out_w,C)."""
    img = np.asarray(img)
    _check_img(img.shape, img.dtype, 'resample_ref')
    out_h, out_w = _check_size(out_h, out_w, 'resample_ref')
    wh, ih = _tables(img.shape[0], out_h)
    ww, iw = _tables(img.shape[1], out_w)
    x = img.astype(np.float64).reshape(img.shape[0], img.shape[1], -1)
    out1 = np.zeros((out_h,) + x.shape[1:])
    for k in range(wh.shape[1]):
        out1 = out1 + wh[:, k][:, None, None] * x[ih[:, k]]
    out2 = np.zeros((out_h, out_w, x.shape[2]))
    for k in range(ww.shape[1]):
        out2 = out2 + ww[:, k][None, :, None] * out1[:, iw[:, k]]
    return out2.reshape((out_h, out_w) + img.shape[2:])


def resample_ref(img, out_h, out_w):
    return np.rint(np.clip(resample_values(img, out_h, out_w), 0, 255)).astype(np.uint8)


def target_size(h, w, net_scale, final_scale=None, final_size=None):
    """(out_h, out_w) of an INPUT of h x w.  final_scale: a fractions.Fraction (anything Fraction() takes exactly: an int, a Fraction, a
    string such as '1.1' or '3/2' - not a float), out = ceil(n F) in rational arithmetic (100 x 1.1 is 110); final_size: (W, H) exactly, the
    aspect ratio may change; neither: the network's own (net_scale h, net_scale w)."""
    if final_scale is not None and final_size is not None:
        raise ValueError('target_size: give final_scale or final_size, not both')
    if final_size is not None:
        out_h, out_w = _check_size(final_size[1], final_size[0], 'target_size')
        return out_h, out_w
    if final_scale is None:
        return int(net_scale) * h, int(net_scale) * w
    if isinstance(final_scale, float):
        raise ValueError(f'target_size: final_scale must be exact (a Fraction, an int or a string), got the float {final_scale!r}')
    f = Fraction(final_scale)
    if f <= 0:
        raise ValueError(f'target_size: final_scale must be positive, got {final_scale!r}')
    return math.ceil(h * f), math.ceil(w * f)


def check_ratio(h, w, out_h, out_w):
    for name, n, o in (('height', h, out_h), ('width', w, out_w)):
        if not MIN_RATIO <= Fraction(int(o), int(n)) <= MAX_RATIO:
            raise ResampleRatio(f'resample: {name} {n} -> {o} is a ratio of {o / n:.4g}: {RATIO_LIMIT}')


# ---------------------------------------------------------------------------------------------------------------- GPU
_TABLES = {}


def _device_tables(n, out, device):
    """Device copy of the imresize_tables of one axis (cached per (in, out, device)); ResampleTooSmall where the size is too small."""
    key = (n, out, str(device))
    if key not in _TABLES:
        import torch
        if len(_TABLES) >= 16:
            _TABLES.clear()
        w, idx = _tables(n, out)
        _TABLES[key] = (torch.from_numpy(w).to(device), torch.from_numpy(idx).to(device), w.shape[1])
    return _TABLES[key]


def prepare(h, w, out_h, out_w, device):
    """What resample_u8 refuses about the sizes alone, raised now - ResampleRatio, ResampleTooSmall - and the device tables made."""
    check_ratio(h, w, out_h, out_w)
    _device_tables(h, out_h, device)
    _device_tables(w, out_w, device)


def resample_u8(img, out_h, out_w, out=None):
    """resample_ref of a contiguous uint8 (H,W) or (H,W,C) GPU tensor, C in 1..4: a tensor of the same rank, ONE launch on the current
    stream; no float plane of the image, no workspace.  Equal size runs the kernel like any other.  FemasrError for a CPU tensor,
    ResampleRatio / ResampleTooSmall / ValueError for what it does not take."""
    import torch
    from . import _lib
    from .channels import _out, _stream
    if not torch.is_tensor(img):
        raise TypeError(f'resample_u8: expected a torch tensor, got {type(img).__name__}')
    _check_img(tuple(img.shape), img.dtype, 'resample_u8')
    out_h, out_w = _check_size(out_h, out_w, 'resample_u8')
    if img.device.type != 'cuda':
        raise _lib.FemasrError(f'resample_u8: tensor on {img.device}: it runs on a GPU only (no CPU fallback)')
    if not img.is_contiguous():
        raise ValueError(f'resample_u8: expected a contiguous tensor, got strides {tuple(img.stride())} for shape {tuple(img.shape)}')
    h, w = img.shape[:2]
    c = 1 if img.dim() == 2 else img.shape[2]
    check_ratio(h, w, out_h, out_w)
    out = _out(out, (out_h, out_w) + tuple(img.shape[2:]), img, 'resample_u8')
    lib = _lib.load()
    if lib.femasr_resample_tile() != TILE:
        raise _lib.FemasrError(f'resample_u8: the library tiles by {lib.femasr_resample_tile()} columns, resample.TILE says {TILE}')
    with torch.cuda.device(img.device):
        wh, ih, ph = _device_tables(h, out_h, img.device)
        ww, iw, pw = _device_tables(w, out_w, img.device)
        _lib.check(lib.femasr_resample_u8(_stream(img.device), _lib.ptr(img), h, w, c, _lib.ptr(out), out_h, out_w, _lib.ptr(wh), _lib.ptr(ih), ph,
                                          _lib.ptr(ww), _lib.ptr(iw), pw))
    return out

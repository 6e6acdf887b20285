"""Gray, gray + alpha and RGBA images through a 3-channel network (opt-in): the image is taken apart in front of the forward
and put together behind it, so the output has the input's channels.  The network, the tile driver and every option of theirs are unchanged:
they see uint8 (H,W,3) images as ever.

    split_ref(img) -> (rgb, alpha or None)             the DEFINITIONS (numpy; integers, the bicubic in fp64)
    gray_ref(rgb) -> (H,W)
    alpha_up_ref(alpha, s) -> (sH,sW)
    merge_ref(rgb_sr, alpha_sr or None, channels)
    upscale_ref(img, run, scale, alpha='bicubic')      split_ref -> run -> merge_ref on host arrays
    split_u8 / gray_u8 / alpha_bicubic_u8 / merge_u8   the same bytes on the GPU, ONE launch each (csrc/channels.hip); GPU tensors only
    upscale_u8(img_u8, run, scale, alpha='bicubic')    split_u8 -> run(rgb) -> merge_u8; `run` is the caller's rgb_u8 -> rgb_u8

Definitions.  img: uint8 (H,W) or (H,W,C), C in {1,2,3,4}; (H,W) is C = 1.
    split   C = 1, 2: the gray plane replicated into R, G, B;  C = 2, 4: the last channel is alpha
    gray    (19595 R + 38470 G + 7471 B + 32768) >> 16 - Pillow's convert('L'); a gray triple (g,g,g) gives g
    alpha   'bicubic': rint(clip(imresize(alpha as float64, s), 0, 255)), imresize the project's MATLAB bicubic
            (femasr_amd.models.femasr_model.imresize: H pass, then W pass, one accumulator per output over its taps in ascending order from
            0.0, multiply and add rounded separately); ValueError where imresize_tables refuses the size;
            'network': gray(run(alpha, alpha, alpha)) - the alpha plane takes the same forward as the colour
    merge   channels 1: gray(rgb_sr); 2: gray(rgb_sr), alpha_sr; 3: rgb_sr; 4: rgb_sr, alpha_sr
Not done: 16-bit samples; anything about the colour under fully transparent pixels (no premultiplication, no un-bleeding).
"""
import numpy as np

from .pngio import CHANNELS

ALPHA_MODES = ('bicubic', 'network')
MODES = {c: mode for c, (_, mode) in CHANNELS.items()}      # PIL's name of an image of C channels: L, LA, RGB, RGBA


# ---------------------------------------------------------------------------------------------------------------- definitions
def _channels_of(shape):
    if len(shape) == 2:
        return 1
    if len(shape) == 3 and shape[2] in MODES:
        return int(shape[2])
    raise ValueError(f'expected an (H,W) or (H,W,C) image with C in 1..4, got {tuple(shape)}')


def _check_u8(img, what):
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f'{what}: expected uint8, got {img.dtype}')
    return img


def split_ref(img):
    img = _check_u8(img, 'split_ref')
    c = _channels_of(img.shape)
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f'split_ref: empty image {img.shape}')
    px = img.reshape(img.shape[0], img.shape[1], c)
    rgb = np.ascontiguousarray(px[..., :3] if c >= 3 else np.repeat(px[..., :1], 3, axis=2))
    return rgb, (np.ascontiguousarray(px[..., c - 1]) if c in (2, 4) else None)


def gray_ref(rgb):
    rgb = _check_u8(rgb, 'gray_ref')
    if rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise ValueError(f'gray_ref: expected (...,3) RGB, got {rgb.shape}')
    v = rgb.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16).astype(np.uint8)


def _check_scale(s):
    if not isinstance(s, (int, np.integer)) or isinstance(s, bool) or s < 1:
        raise ValueError(f'scale must be an integer >= 1, got {s!r}')
    return int(s)


def alpha_up_ref(alpha, s):
    from .models.femasr_model import imresize
    alpha, s = _check_u8(alpha, 'alpha_up_ref'), _check_scale(s)
    if alpha.ndim != 2 or alpha.shape[0] < 1 or alpha.shape[1] < 1:
        raise ValueError(f'alpha_up_ref: expected an (H,W) plane, got {alpha.shape}')
    return np.rint(np.clip(imresize(alpha.astype(np.float64), s), 0, 255)).astype(np.uint8)


def _check_merge(rgb_shape, alpha_shape, channels):
    if channels not in MODES:
        raise ValueError(f'merge: channels must be 1..4, got {channels!r}')
    if len(rgb_shape) != 3 or rgb_shape[2] != 3:
        raise ValueError(f'merge: expected an (sH,sW,3) image, got {tuple(rgb_shape)}')
    if (alpha_shape is not None) != (channels in (2, 4)):
        raise ValueError(f'merge: {channels} channel(s) ' + ('need an alpha plane' if alpha_shape is None else 'take no alpha plane'))


def merge_ref(rgb_sr, alpha_sr, channels):
    rgb_sr = _check_u8(rgb_sr, 'merge_ref')
    if alpha_sr is not None:
        alpha_sr = _check_u8(alpha_sr, 'merge_ref')
    _check_merge(rgb_sr.shape, None if alpha_sr is None else alpha_sr.shape, channels)
    if alpha_sr is not None and alpha_sr.shape != rgb_sr.shape[:2]:
        raise ValueError(f'merge_ref: alpha {alpha_sr.shape} does not cover the image {rgb_sr.shape}')
    if channels == 1:
        return gray_ref(rgb_sr)
    if channels == 2:
        return np.stack([gray_ref(rgb_sr), alpha_sr], axis=2)
    if channels == 3:
        return rgb_sr
    return np.concatenate([rgb_sr, alpha_sr[..., None]], axis=2)


class AlphaTooSmall(ValueError):
    """The image is too small for the bicubic tables (imresize_tables refuses it): alpha='network' has no such limit."""


def _check_alpha_mode(alpha):
    if alpha not in ALPHA_MODES:
        raise ValueError(f'alpha must be one of {ALPHA_MODES}, got {alpha!r}')


def upscale_ref(img, run, scale, alpha='bicubic', run_alpha=None):
    """The definition of upscale_u8 on host arrays; `run`: uint8 (H,W,3) array -> uint8 (sH,sW,3) array."""
    _check_alpha_mode(alpha)
    img = _check_u8(img, 'upscale_ref')
    c = _channels_of(img.shape)
    if c == 3:
        return run(img)
    rgb, a = split_ref(img)
    a_sr = None
    if a is not None:
        a_sr = alpha_up_ref(a, scale) if alpha == 'bicubic' else gray_ref((run_alpha or run)(np.repeat(a[..., None], 3, axis=2)))
    out = merge_ref(run(rgb), a_sr, c)
    return out[..., None] if img.ndim == 3 and c == 1 else out


# ---------------------------------------------------------------------------------------------------------------- GPU
_TABLES = {}


def _tables(h, w, s, device):
    """Device copies of the two imresize_tables for scale s (cached); ValueError where the size is too small for them."""
    key = (h, w, s, str(device))
    if key not in _TABLES:
        from .resize import device_tables
        if len(_TABLES) >= 8:
            _TABLES.clear()
        _TABLES[key] = device_tables(h, h * s, s, True, device) + device_tables(w, w * s, s, True, device)
    return _TABLES[key]


def _gpu_u8(t, what, shapes):
    import torch
    from . import _lib
    if not torch.is_tensor(t):
        raise TypeError(f'{what}: expected a torch tensor, got {type(t).__name__}')
    if t.dtype != torch.uint8 or t.numel() == 0:
        raise ValueError(f'{what}: expected a non-empty uint8 tensor, got {t.dtype} {tuple(t.shape)}')
    if not shapes(tuple(t.shape)):
        raise ValueError(f'{what}: unexpected shape {tuple(t.shape)}')
    if t.device.type != 'cuda':
        raise _lib.FemasrError(f'{what}: tensor on {t.device}: it runs on a GPU only (no CPU fallback)')
    return t.contiguous()


def _out(out, shape, like, what):
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=like.device)
    if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or out.device != like.device or not out.is_contiguous():
        raise ValueError(f'{what}: out= must be a contiguous uint8 tensor of shape {tuple(shape)} on {like.device}')
    return out


def _stream(dev):
    import ctypes
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def split_u8(img):
    """split_ref of a uint8 (H,W), (H,W,C) or (B,H,W,C) GPU tensor, C in {1,2,4}: (rgb (...,H,W,3), alpha (...,H,W) or None), ONE launch on
    the current stream.  A batch needs its channel axis: a 3-D tensor is (H,W,C)."""
    import torch
    from . import _lib
    x = _gpu_u8(img, 'split_u8', lambda s: len(s) == 2 or (len(s) in (3, 4) and s[-1] in (1, 2, 4)))
    c = 1 if x.dim() == 2 else x.shape[-1]
    lead = tuple(x.shape) if x.dim() == 2 else tuple(x.shape[:-1])
    B = lead[0] if len(lead) == 3 else 1
    H, W = lead[-2:]
    rgb = torch.empty(lead + (3,), dtype=torch.uint8, device=x.device)
    alpha = torch.empty(lead, dtype=torch.uint8, device=x.device) if c != 1 else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().femasr_channels_split_u8(_stream(x.device), _lib.ptr(x), B, H, W, c, _lib.ptr(rgb), _lib.ptr(alpha)))
    return rgb, alpha


def _merge(rgb, alpha_lr, alpha_rgb, h, w, s, channels, out, what):
    import torch
    from . import _lib
    like = rgb if rgb is not None else alpha_lr
    shape = (s * h, s * w) if channels == 1 else (s * h, s * w, channels)
    out = _out(out, shape, like, what)
    for t in (alpha_lr, alpha_rgb):
        if t is not None and t.device != like.device:
            raise _lib.FemasrError(f'{what}: tensors on {like.device} and {t.device}: it runs on one GPU only')
    with torch.cuda.device(like.device):
        wh, ih, ph, ww, iw, pw = _tables(h, w, s, like.device) if alpha_lr is not None else (None, None, 0, None, None, 0)
        _lib.check(_lib.load().femasr_channels_merge_u8(_stream(like.device), _lib.ptr(rgb), _lib.ptr(alpha_lr), _lib.ptr(alpha_rgb), h, w, s, channels,
                                                        _lib.ptr(wh), _lib.ptr(ih), ph, _lib.ptr(ww), _lib.ptr(iw), pw, _lib.ptr(out)))
    return out


def _is_rgb(s):
    return len(s) == 3 and s[2] == 3


def gray_u8(rgb, out=None):
    """gray_ref of a uint8 (H,W,3) GPU tensor: (H,W), ONE launch."""
    x = _gpu_u8(rgb, 'gray_u8', _is_rgb)
    return _merge(x, None, None, x.shape[0], x.shape[1], 1, 1, out, 'gray_u8')


def alpha_bicubic_u8(alpha, s, out=None):
    """alpha_up_ref of a uint8 (H,W) GPU tensor: (sH,sW), ONE launch (the merge kernel with the alpha as its only output)."""
    s = _check_scale(s)
    a = _gpu_u8(alpha, 'alpha_bicubic_u8', lambda sh: len(sh) == 2)
    return _merge(None, a, None, a.shape[0], a.shape[1], s, 1, out, 'alpha_bicubic_u8')


def merge_u8(rgb_sr, alpha, channels, scale=None, out=None):
    """merge_ref on the GPU, ONE launch that writes the final interleaved image.  `alpha` is the alpha SOURCE (None for channels 1 and 3):
         uint8 (H,W) with `scale`: the input's alpha plane - the bicubic runs inside the kernel ('bicubic');
         uint8 (sH,sW,3):          the network's image of the alpha plane - its gray is taken inside the kernel ('network').
    No alpha plane of the output's size is made.  channels = 3 returns rgb_sr itself."""
    x = _gpu_u8(rgb_sr, 'merge_u8', _is_rgb)
    _check_merge(tuple(x.shape), None if alpha is None else tuple(alpha.shape), channels)
    sh, sw = x.shape[:2]
    if channels == 3:
        return rgb_sr
    if channels == 1:
        return _merge(x, None, None, sh, sw, 1, 1, out, 'merge_u8')
    if alpha.dim() == 3:
        a = _gpu_u8(alpha, 'merge_u8', lambda s: tuple(s) == (sh, sw, 3))
        return _merge(x, None, a, sh, sw, 1, channels, out, 'merge_u8')
    s = _check_scale(scale)
    a = _gpu_u8(alpha, 'merge_u8', lambda sp: len(sp) == 2 and (sp[0] * s, sp[1] * s) == (sh, sw))
    return _merge(x, a, None, a.shape[0], a.shape[1], s, channels, out, 'merge_u8')


def upscale_u8(img_u8, run, scale, alpha='bicubic', run_alpha=None):
    """The input's channels through a 3-channel upscaler: split_u8 -> run(rgb) -> merge_u8.
    img_u8: uint8 (H,W), (H,W,1), (H,W,2), (H,W,3) or (H,W,4) on a GPU.  run: uint8 (H,W,3) -> uint8 (scale H, scale W, 3) on the same GPU
    (FeMaSRNet.test_u8 / test_tile_u8 behind a closure: tiling, blend, self-ensemble and the arithmetic modes apply unchanged), or None on a
    rank that does not hold the result - upscale_u8 then returns None as well.  alpha = 'network' sends the alpha plane through `run_alpha`
    (default: `run`; the CLI passes the forward without the colour fix).  A 3-channel image is run(img_u8) itself: nothing else is launched."""
    _check_alpha_mode(alpha)
    scale = _check_scale(scale)
    x = _gpu_u8(img_u8, 'upscale_u8', lambda s: len(s) == 2 or (len(s) == 3 and s[2] in MODES))
    c = 1 if x.dim() == 2 else x.shape[2]
    if c == 3:
        return run(img_u8)
    h, w = x.shape[:2]
    rgb, a = split_u8(x.reshape(h, w, c))
    src = a
    if a is not None and alpha == 'bicubic':
        try:
            _tables(h, w, scale, x.device)                   # refuses a size the bicubic cannot take before the forward runs
        except ValueError as e:
            raise AlphaTooSmall(f"upscale_u8: {e}; alpha='network' takes such an image") from None
    elif a is not None:
        src = (run_alpha or run)(split_u8(a)[0])             # (H,W) -> the gray image (a, a, a)
    sr = run(rgb)
    if sr is None:
        return None
    if tuple(sr.shape) != (scale * h, scale * w, 3):
        raise ValueError(f'upscale_u8: run() returned {tuple(sr.shape)} for an input of {h}x{w} at scale {scale}')
    out = merge_u8(sr, src, c, scale if alpha == 'bicubic' else None)
    return out.reshape(scale * h, scale * w, 1) if x.dim() == 3 and c == 1 else out

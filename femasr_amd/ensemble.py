"""x8 geometric self-ensemble (opt-in; NOT the reference's arithmetic): the "+" protocol of EDSR / SwinIR / HAT - the network runs on the
eight flips and transposes of the input, each result is mapped back, the eight are averaged.

    forward_variant(x, k) / inverse_variant(y, k)       one variant, torch, host or GPU tensors
    expand_torch(x) / merge_torch(straight, transposed)  the definition in torch (host or GPU tensors; a sequential restatement)
    expand(x) / merge(straight, transposed, out=None)    the same: ONE launch each on the GPU (csrc/ensemble.hip), the torch definition on host tensors

Definition.  Images are float32 (B,C,H,W) or uint8 (B,H,W,3).  Variant k = 0..7: v = k & 1 flips rows, h = (k >> 1) & 1 flips
columns, t = (k >> 2) & 1 transposes; x_k = T^t(H^h(V^v(x))) per image and channel:
    t = 0, (H,W):  x_k[i,j] = x[v ? H-1-i : i, h ? W-1-j : j]
    t = 1, (W,H):  x_k[i,j] = x[v ? H-1-j : j, h ? W-1-i : i]
y_k = test(x_k), the unchanged forward with its mirror pad and crop: (sH,sW) for t = 0, (sW,sH) for t = 1.  The inverse:
    t = 0:  z_k[i,j] = y_k[v ? sH-1-i : i, h ? sW-1-j : j]
    t = 1:  z_k[i,j] = y_k[h ? sW-1-j : j, v ? sH-1-i : i]
float32:  out = 0.125f * (((((((z_0 + z_1) + z_2) + z_3) + z_4) + z_5) + z_6) + z_7) - fp32 adds in this order, so any sequential torch or
numpy restatement gives the same bits.
uint8:    on the BYTES the eight `test_u8` results hold after tensor2img (as `blend` and `color_fix` work for uint8): S = sum_k z_k (0..2040),
out = (S + 3 + ((S >> 3) & 1)) >> 3 = S / 8 rounded half to even.  Deliberately NOT the quantised fp32 ensemble.
test() pads bottom / right only, so the ensemble is not exactly equivariant under the eight maps: that is the definition.

Buffers are variant-major: `straight` (4,B,...) holds k = 0..3, `transposed` (4,B,...) with the two image axes swapped holds k = 4..7.
`expand` returns two views of ONE allocation, transposed right behind straight: for square images `as_batch` gives the eight variants as one
(8,B,...) tensor."""
import torch

from . import _lib

VARIANTS = 8


def _axes(t):
    """(row axis, column axis) of an image batch: float32 (..., H, W) or uint8 (..., H, W, 3)."""
    if t.dtype == torch.uint8:
        if t.dim() < 3 or t.shape[-1] != 3:
            raise ValueError(f'self-ensemble: uint8 images are (..., H, W, 3), got {tuple(t.shape)}')
        return t.dim() - 3, t.dim() - 2
    if t.dtype != torch.float32 or t.dim() < 2:
        raise ValueError(f'self-ensemble: images are float32 (..., H, W) or uint8 (..., H, W, 3), got {t.dtype} {tuple(t.shape)}')
    return t.dim() - 2, t.dim() - 1


def _check_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k < VARIANTS:
        raise ValueError(f'self-ensemble: variant must be an integer in 0..7, got {k!r}')
    return k & 1, (k >> 1) & 1, (k >> 2) & 1


def forward_variant(x, k):
    """x_k = T^t(H^h(V^v(x))): a contiguous tensor."""
    v, h, t = _check_k(k)
    r, c = _axes(x)
    dims = [a for a, on in ((r, v), (c, h)) if on]
    y = torch.flip(x, dims) if dims else x
    return (y.transpose(r, c) if t else y).contiguous()


def inverse_variant(y, k):
    """z_k = V^v(H^h(T^t(y_k))): the inverse of `forward_variant` (scale-free: it takes the result's own size)."""
    v, h, t = _check_k(k)
    r, c = _axes(y)
    z = y.transpose(r, c) if t else y
    dims = [a for a, on in ((r, v), (c, h)) if on]
    return (torch.flip(z, dims) if dims else z).contiguous()


def _batch(x):
    """(row axis, column axis) of a BATCH: float32 (B,C,H,W) or uint8 (B,H,W,3)."""
    if not torch.is_tensor(x):
        raise TypeError(f'self-ensemble: expected a torch tensor, got {type(x).__name__}')
    r, c = _axes(x)
    if x.dim() != 4:
        raise ValueError(f'self-ensemble: a batch is float32 (B,C,H,W) or uint8 (B,H,W,3), got {tuple(x.shape)}')
    return r, c


def _swapped(shape, r, c):
    s = list(shape)
    s[r], s[c] = s[c], s[r]
    return tuple(s)


def _pair(x, r, c, device=None):
    """Uninitialised (straight, transposed) for a batch like x: two views of one allocation, transposed right behind straight."""
    n = 4 * x.numel()
    buf = torch.empty(2 * n, dtype=x.dtype, device=x.device if device is None else device)
    return buf[:n].view((4,) + tuple(x.shape)), buf[n:].view((4,) + _swapped(x.shape, r, c))


def as_batch(straight, transposed):
    """The eight variants as one (8,B,...) tensor when the images are square and `transposed` lies right behind `straight` in one
    allocation (what `expand` and `result_buffers` return), else None."""
    if (straight.shape != transposed.shape or not straight.is_contiguous() or not transposed.is_contiguous() or
            straight.device != transposed.device or straight.dtype != transposed.dtype or
            straight.untyped_storage().data_ptr() != transposed.untyped_storage().data_ptr() or
            transposed.storage_offset() != straight.storage_offset() + straight.numel()):
        return None
    return torch.as_strided(straight, (8,) + tuple(straight.shape[1:]), straight.stride(), straight.storage_offset())


def result_buffers(x, scale):
    """Uninitialised (straight, transposed) for the eight results of a batch x at `scale`, laid out like `expand`'s."""
    r, c = _batch(x)
    shape = list(x.shape)
    shape[r], shape[c] = shape[r] * scale, shape[c] * scale
    return _pair(torch.empty(shape, dtype=x.dtype, device='meta'), r, c, x.device)


def expand_torch(x):
    """The definition: (straight (4,B,...) = x_0..x_3, transposed (4,B,...) = x_4..x_7)."""
    r, c = _batch(x)
    straight, transposed = _pair(x, r, c)
    for k in range(4):
        straight[k].copy_(forward_variant(x, k))
        transposed[k].copy_(forward_variant(x, 4 + k))
    return straight, transposed


def _check_pair(straight, transposed):
    if not torch.is_tensor(straight) or not torch.is_tensor(transposed):
        raise TypeError('self-ensemble: expected torch tensors')
    if straight.dim() != 5 or transposed.dim() != 5 or straight.shape[0] != 4 or straight.dtype != transposed.dtype or straight.device != transposed.device:
        raise ValueError(f'self-ensemble: expected (4,B,...) results of one dtype and device, got {tuple(straight.shape)} {straight.dtype} and '
                         f'{tuple(transposed.shape)} {transposed.dtype}')
    r, c = _axes(straight[0])
    if tuple(transposed.shape) != (4,) + _swapped(straight.shape[1:], r, c):
        raise ValueError(f'self-ensemble: transposed results of {tuple(transposed.shape)} do not belong to straight results of {tuple(straight.shape)}')
    return r, c


def _check_out(out, like):
    if out is not None and (not torch.is_tensor(out) or out.shape != like.shape or out.dtype != like.dtype or out.device != like.device or
                            not out.is_contiguous()):
        raise ValueError(f'self-ensemble: out= must be a contiguous {like.dtype} tensor of shape {tuple(like.shape)} on {like.device}')


def merge_torch(straight, transposed, out=None):
    """The definition: float32 the sequential fp32 sum of z_0..z_7 times 0.125; uint8 S / 8 of the bytes, half to even (module docstring)."""
    _check_pair(straight, transposed)
    _check_out(out, straight[0])
    z = [inverse_variant(straight[k], k) for k in range(4)] + [inverse_variant(transposed[k], 4 + k) for k in range(4)]
    if straight.dtype == torch.uint8:
        s = z[0].to(torch.int32)
        for k in range(1, VARIANTS):
            s = s + z[k].to(torch.int32)
        res = ((s + 3 + ((s >> 3) & 1)) >> 3).to(torch.uint8)
    else:
        acc = z[0] + z[1]
        for k in range(2, VARIANTS):
            acc = acc + z[k]
        res = acc * 0.125
    return res if out is None else out.copy_(res)


def _native_dims(x):
    """The (B[, C], H, W) arguments of the native calls for a batch."""
    return tuple(x.shape[:3]) if x.dtype == torch.uint8 else tuple(x.shape)


@torch.no_grad()
def expand(x):
    """(straight, transposed) of a batch - float32 (B,C,H,W) or uint8 (B,H,W,3) -, two views of one allocation.  GPU tensors: ONE
    femasr_dihedral_expand / _u8 launch on the current stream (x is read once, written eight times); host tensors: `expand_torch`."""
    r, c = _batch(x)
    if not x.is_cuda:
        return expand_torch(x)
    x = x.contiguous()
    straight, transposed = _pair(x, r, c)
    if x.numel():
        fn = _lib.load().femasr_dihedral_expand_u8 if x.dtype == torch.uint8 else _lib.load().femasr_dihedral_expand
        with torch.cuda.device(x.device):
            _lib.check(fn(torch.cuda.current_stream(x.device).cuda_stream, _lib.ptr(x), *_native_dims(x), _lib.ptr(straight), _lib.ptr(transposed)))
    return straight, transposed


@torch.no_grad()
def merge(straight, transposed, out=None):
    """The ensemble of eight results laid out like `expand`'s (straight (4,B,...), transposed (4,B,...) with the image axes swapped): a new
    tensor, or `out` (contiguous, like straight[0]).  GPU tensors: ONE femasr_dihedral_merge / _u8 launch on the current stream (eight values
    read, one written); host tensors: `merge_torch`.  uint8: the mean of the BYTES, half to even - not the quantised fp32 ensemble."""
    _check_pair(straight, transposed)
    _check_out(out, straight[0])
    if not straight.is_cuda:
        return merge_torch(straight, transposed, out)
    straight, transposed = straight.contiguous(), transposed.contiguous()
    if out is None:
        out = torch.empty_like(straight[0])
    if out.numel():
        fn = _lib.load().femasr_dihedral_merge_u8 if out.dtype == torch.uint8 else _lib.load().femasr_dihedral_merge
        with torch.cuda.device(out.device):
            _lib.check(fn(torch.cuda.current_stream(out.device).cuda_stream, _lib.ptr(straight), _lib.ptr(transposed), *_native_dims(out), _lib.ptr(out)))
    return out

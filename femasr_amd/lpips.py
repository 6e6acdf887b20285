"""LPIPS v0.1 (inference) on the MI355X path: the metric the reference validates with (`pyiqa.create_metric('lpips', ...)`,
basicsr/models/femasr_model.py:27-34,262,288-292) and that scripts/metrics/calculate_lpips.py computes with LPIPS-VGG.

    LPIPS(net='alex' | 'vgg', pretrained_model_path=..., backbone_model_path=None)(x0, x1) -> (B,1,1,1)

x0, x1: float32 (B,3,H,W) RGB in [0,1] on a GPU (scaled to [-1,1] inside, as `lpips.LPIPS(...)(x0, x1, normalize=True)` and pyiqa do).
Everything runs in libfemasr_hip.so (csrc/lpips.hip + the fp32 conv kernels with a ReLU epilogue); there is no CPU path.

Weights.  No pyiqa / lpips source is available to this project, so the checkpoint names below follow those packages' module
structure (lpips.pretrained_networks: `net.sliceK.I` with I the torchvision `features` index; lpips.LPIPS: `linK.model.1.weight`, also
reachable as `lins.K.model.1.weight`) and torchvision's `features.I`.  The whole name mapping is `_NAME_RULES` plus `METRIC_NETS`.
"""
import ctypes
import re
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib

# metric type (pyiqa's names) -> backbone
METRIC_NETS = {'lpips': 'alex', 'lpips-vgg': 'vgg'}

# (slice K, torchvision feature index I, Cin, Cout, kernel, stride, pad, tap after this conv?, pool after the tap: 0 / 1 = 3/2 / 2 = 2/2)
_CONVS = {
    'alex': (
        (1, 0, 3, 64, 11, 4, 2, True, 1),
        (2, 3, 64, 192, 5, 1, 2, True, 1),
        (3, 6, 192, 384, 3, 1, 1, True, 0),
        (4, 8, 384, 256, 3, 1, 1, True, 0),
        (5, 10, 256, 256, 3, 1, 1, True, 0),
    ),
    'vgg': (
        (1, 0, 3, 64, 3, 1, 1, False, 0), (1, 2, 64, 64, 3, 1, 1, True, 2),
        (2, 5, 64, 128, 3, 1, 1, False, 0), (2, 7, 128, 128, 3, 1, 1, True, 2),
        (3, 10, 128, 256, 3, 1, 1, False, 0), (3, 12, 256, 256, 3, 1, 1, False, 0), (3, 14, 256, 256, 3, 1, 1, True, 2),
        (4, 17, 256, 512, 3, 1, 1, False, 0), (4, 19, 512, 512, 3, 1, 1, False, 0), (4, 21, 512, 512, 3, 1, 1, True, 2),
        (5, 24, 512, 512, 3, 1, 1, False, 0), (5, 26, 512, 512, 3, 1, 1, False, 0), (5, 28, 512, 512, 3, 1, 1, True, 0),
    ),
}
TAP_CHANNELS = {net: tuple(c[3] for c in convs if c[7]) for net, convs in _CONVS.items()}
MIN_SIDE = {'alex': 31, 'vgg': 16}
_NET_ID = {'alex': 0, 'vgg': 1}


def _slice_of(net, index):
    for c in _CONVS[net]:
        if c[1] == index:
            return c[0]
    return None


# checkpoint name -> canonical name (None: not an LPIPS weight, ignored).  One table: correct it here if a checkpoint names differ.
_NAME_RULES = (
    (re.compile(r'net\.slice(\d)\.(\d+)\.(weight|bias)'), lambda net, m: f'net.slice{m[1]}.{m[2]}.{m[3]}'),      # lpips / pyiqa backbone
    (re.compile(r'features\.(\d+)\.(weight|bias)'),                                                              # torchvision backbone
     lambda net, m: None if _slice_of(net, int(m[1])) is None else f'net.slice{_slice_of(net, int(m[1]))}.{m[1]}.{m[2]}'),
    (re.compile(r'lin(\d)\.model\.1\.weight'), lambda net, m: f'lin{m[1]}.model.1.weight'),                      # lpips.LPIPS heads
    (re.compile(r'lins\.(\d)\.model\.1\.weight'), lambda net, m: f'lin{m[1]}.model.1.weight'),                   # the same, ModuleList name
)


def expected_shapes(net):
    """Canonical key -> shape of every weight the net needs."""
    out = OrderedDict()
    for k, i, cin, cout, ksz, *_ in _CONVS[net]:
        out[f'net.slice{k}.{i}.weight'] = (cout, cin, ksz, ksz)
        out[f'net.slice{k}.{i}.bias'] = (cout,)
    for t, c in enumerate(TAP_CHANNELS[net]):
        out[f'lin{t}.model.1.weight'] = (1, c, 1, 1)
    return out


def _unwrap(sd):
    """{'params' | 'state_dict': {...}} nesting (BasicSR / Lightning-style files) and a 'module.' prefix (DataParallel)."""
    while isinstance(sd, dict) and len(sd) and not any(torch.is_tensor(v) for v in sd.values()):
        for key in ('params', 'state_dict', 'params_ema'):
            if isinstance(sd.get(key), dict):
                sd = sd[key]
                break
        else:
            break
    return OrderedDict((k[7:] if k.startswith('module.') else k, v) for k, v in sd.items() if torch.is_tensor(v))


def canonical_state_dict(net, *state_dicts):
    """Map one or more checkpoint state dicts (backbone + heads in one, or split) to the canonical keys and check every shape against the
    net's channel table.  Raises KeyError naming the missing keys, ValueError naming the mis-shaped ones."""
    if net not in _CONVS:
        raise ValueError(f"net must be 'alex' or 'vgg', got {net!r}")
    want = expected_shapes(net)
    out = OrderedDict()
    for sd in state_dicts:
        for key, v in _unwrap(sd).items():
            for rx, fn in _NAME_RULES:
                m = rx.fullmatch(key)
                if m:
                    ck = fn(net, m)
                    if ck is not None and ck in want:
                        out[ck] = v.detach().to(torch.float32).cpu()
                    break
    missing = [k for k in want if k not in out]
    if missing:
        raise KeyError(f'LPIPS-{net} weights: missing {missing} (accepted layouts: net.sliceK.I.* / features.I.* for the backbone, '
                       'linK.model.1.weight / lins.K.model.1.weight for the heads)')
    bad = [f'{k}: {tuple(out[k].shape)} != {want[k]}' for k in want if tuple(out[k].shape) != want[k]]
    if bad:
        raise ValueError(f'LPIPS-{net} weights: wrong shapes {bad}')
    return OrderedDict((k, out[k]) for k in want)


def load_lpips_weights(net, pretrained_model_path, backbone_model_path=None):
    """Canonical state dict from one file holding backbone and heads, or a head file plus a backbone file."""
    sds = [torch.load(pretrained_model_path, map_location='cpu', weights_only=True)]
    if backbone_model_path is not None:
        sds.insert(0, torch.load(backbone_model_path, map_location='cpu', weights_only=True))
    return canonical_state_dict(net, *sds)


def _pool_out(n, pool):
    return (n - 3) // 2 + 1 if pool == 1 else n // 2


def tap_shapes(net, H, W):
    """[(h, w, C)] of the five taps at input (H, W) (torch's conv / max_pool2d size rules); ValueError below the net's minimum size."""
    if H < MIN_SIDE[net] or W < MIN_SIDE[net]:
        raise ValueError(f'LPIPS-{net} needs H, W >= {MIN_SIDE[net]} (a max-pool of the backbone would have no output), got {H}x{W}')
    out, y, x = [], H, W
    for _, _, _, cout, ksz, stride, pad, tap, pool in _CONVS[net]:
        y, x = (y + 2 * pad - ksz) // stride + 1, (x + 2 * pad - ksz) // stride + 1
        if tap:
            out.append((y, x, cout))
        if pool:
            y, x = _pool_out(y, pool), _pool_out(x, pool)
    return out


def max_feature_elems(net, H, W):
    """Largest NHWC tensor of ONE image inside the forward (floats)."""
    m, y, x = H * W * 3, H, W
    for _, _, _, cout, ksz, stride, pad, tap, pool in _CONVS[net]:
        y, x = (y + 2 * pad - ksz) // stride + 1, (x + 2 * pad - ksz) // stride + 1
        m = max(m, y * x * cout)
        if pool:
            y, x = _pool_out(y, pool), _pool_out(x, pool)
    return m


class _Holder(nn.Module):
    pass


class LPIPS(nn.Module):
    """Parameter holder with the canonical state-dict names; forward runs femasr_lpips_forward on the parameters' GPU."""

    def __init__(self, net='alex', pretrained_model_path=None, backbone_model_path=None, state_dict=None):
        super().__init__()
        if net not in _CONVS:
            raise ValueError(f"net must be 'alex' or 'vgg', got {net!r}")
        self.net_type = net
        backbone = _Holder()
        for k, i, cin, cout, ksz, stride, pad, _, _ in _CONVS[net]:
            if not hasattr(backbone, f'slice{k}'):
                backbone.add_module(f'slice{k}', _Holder())
            getattr(backbone, f'slice{k}').add_module(str(i), nn.Conv2d(cin, cout, ksz, stride, pad))
        self.net = backbone
        for t, c in enumerate(TAP_CHANNELS[net]):
            lin = _Holder()
            lin.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c, 1, 1, bias=False))
            self.add_module(f'lin{t}', lin)
        for p in self.parameters():
            p.requires_grad_(False)
        if pretrained_model_path is not None:
            self.load_state_dict(load_lpips_weights(net, pretrained_model_path, backbone_model_path))
        elif state_dict is not None:
            self.load_state_dict(canonical_state_dict(net, state_dict))
        elif backbone_model_path is not None:
            raise ValueError('LPIPS: backbone_model_path needs pretrained_model_path (the file with the linK heads)')
        else:       # an LPIPS with torch's random init scores nothing meaningful: say so (load_state_dict may still follow)
            warnings.warn(f'LPIPS({net!r}) built without weights (no pretrained_model_path / state_dict): its parameters are random until '
                          'load_state_dict()', stacklevel=2)
        self.eval()
        self._handle = None
        self._handle_device = None
        self._stamp = None
        self._ws = None

    # ---- native handle: repacked copies of the weights, re-pushed when a parameter changed (version counter / storage)
    def _param_stamp(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _native(self, device):
        if device.type != 'cuda':
            raise _lib.FemasrError('LPIPS (MI355X build) runs on a GPU device only; move the module to cuda. There is no CPU fallback.')
        lib = _lib.load()
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        if self._handle is None or self._handle_device != dev_index:
            self._release()
            h = ctypes.c_void_p()
            _lib.check(lib.femasr_lpips_create(_NET_ID[self.net_type], dev_index, ctypes.byref(h)))
            self._handle, self._handle_device, self._stamp = h, dev_index, None
        stamp = self._param_stamp()
        if stamp != self._stamp:
            torch.cuda.synchronize(device)
            for key, t in self.state_dict().items():
                src = t.detach().to(device=device, dtype=torch.float32).contiguous()
                shape = (ctypes.c_int64 * src.dim())(*src.shape)
                _lib.check(lib.femasr_lpips_set_weight(self._handle, key.encode(), _lib.ptr(src), shape, src.dim()))
            _lib.check(lib.femasr_lpips_finalize_weights(self._handle))
            self._stamp = stamp
        return lib, self._handle

    def _release(self):
        if getattr(self, '_handle', None) is not None:
            _lib.load().femasr_lpips_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._ws

    @torch.no_grad()
    def forward(self, x0, x1, per_layer=False):
        """(B,3,H,W) pairs in [0,1] -> (B,1,1,1) float32 (and the (B,5) tap terms with per_layer=True)."""
        if x0.shape != x1.shape or x0.dim() != 4 or x0.shape[1] != 3:
            raise ValueError(f'LPIPS: expected two (B,3,H,W) tensors of one shape, got {tuple(x0.shape)} and {tuple(x1.shape)}')
        device = self.lin0.model[1].weight.device
        if x0.device != device or x1.device != device:
            raise _lib.FemasrError(f'LPIPS: inputs on {x0.device} / {x1.device}, module on {device} (no CPU fallback)')
        lib, h = self._native(device)
        B, _, H, W = x0.shape
        x0 = x0.detach().to(torch.float32).contiguous()
        x1 = x1.detach().to(torch.float32).contiguous()
        out = torch.empty(B, dtype=torch.float32, device=device)
        terms = torch.empty((B, 5), dtype=torch.float32, device=device)
        # pairs per call: the 2-image-per-pair feature tensors stay below 2^31 elements (the library's 32-bit offsets), and at most
        # 65535 pairs (the tap launch's grid.y); pairs are independent and every sum is per pair, so the split does not change a bit
        step = max(1, min(65535, ((1 << 31) - 1) // (2 * max_feature_elems(self.net_type, H, W))))
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        for b0 in range(0, B, step):
            nb = min(step, B - b0)
            nbytes = ctypes.c_size_t()
            _lib.check(lib.femasr_lpips_workspace_bytes(h, nb, H, W, ctypes.byref(nbytes)))
            ws = self._workspace(nbytes.value, device)
            _lib.check(lib.femasr_lpips_forward(h, stream, _lib.ptr(x0[b0:b0 + nb]), _lib.ptr(x1[b0:b0 + nb]), nb, H, W,
                                                _lib.ptr(out[b0:b0 + nb]), _lib.ptr(terms[b0:b0 + nb]), _lib.ptr(ws), nbytes.value))
        out = out.view(B, 1, 1, 1)
        return (out, terms) if per_layer else out


def create_metric(metric_type, device=None, pretrained_model_path=None, backbone_model_path=None, **ignore_kwargs):
    """pyiqa.create_metric('lpips' | 'lpips-vgg', pretrained_model_path=..., ...) for the LPIPS types this build computes."""
    if metric_type not in METRIC_NETS:
        raise ValueError(f'unknown LPIPS metric type {metric_type!r} (known: {sorted(METRIC_NETS)})')
    if pretrained_model_path is None:
        raise ValueError(f"metric '{metric_type}' needs pretrained_model_path (no network access: pass the local LPIPS weight file)")
    m = LPIPS(METRIC_NETS[metric_type], pretrained_model_path=pretrained_model_path, backbone_model_path=backbone_model_path)
    return m.to(device) if device is not None else m
